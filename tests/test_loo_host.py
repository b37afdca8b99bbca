"""Leave-one-out cross-validation without a GPU: the closed form the GPU tests compare gpf_loo_batch
against (float64 NumPy, and the same formulas in np.longdouble: tests/test_loo_gpu.py and
tests/golden/make_loo_golden.py import both from here), checked against brute-force deletion of every
point and against central differences; the LOO fit (gpfit.loo.fit_loo) on an injected NumPy
evaluator; the drop-in dispatch; the C entry point's table entry.
"""
import ctypes

import numpy as np
import pytest

from test_mle_host import FIT_RECIPES, gp_sample, se_kernel

LOG_2PI = 1.8378770664093453


def _loo_from(W, K, x, y, l):
    """(mu, sd, lpd, grad) from W = Kn^-1 and the noise-free K, in the dtype of W."""
    al = W @ y
    w = np.diag(W).copy()
    q = al * al / w
    mu = y - al / w
    sd = np.sqrt(1 / w)
    lpd = np.sum(np.log(w) / 2 - q / 2) - len(y) * W.dtype.type(LOG_2PI) / 2
    c = al / w
    g = (1 + q) / w / 2
    u = W @ c
    G = (W * g[None, :]) @ W
    M = (np.outer(u, al) + np.outer(al, u) - 2 * G) * K
    grad = np.array([np.sum(M * (x[k][:, None] - x[k][None, :]) ** 2) / 2 / l[k] ** 3 for k in range(len(l))])
    return mu, sd, lpd, grad


def loo_closed_form(x, y, e, l):
    """(mu (N,), sd (N,), lpd, dlpd/dl (d,)) in float64 NumPy, fixed amplitude 1 and noise e^2:
    W = Kn^-1 (np.linalg.inv after np.linalg.cholesky has accepted Kn), alpha = W y, w = diag(W),
    mu_i = y_i - alpha_i / w_i, sd_i = sqrt(1 / w_i), lpd = sum_i [1/2 log w_i - 1/2 alpha_i^2 / w_i] - N/2 log 2 pi,
    dlpd/dl_k = 1/2 sum_ij (u_i alpha_j + u_j alpha_i - 2 G_ij) K_ij (x_ik - x_jk)^2 / l_k^3 with
    c = alpha / w, g = 1/2 (1 + alpha^2 / w) / w, u = W c, G = W diag(g) W."""
    l = np.asarray(l, dtype=np.float64).reshape(-1)
    K = se_kernel(x, l)
    Kn = K + np.diag(e ** 2)
    np.linalg.cholesky(Kn)  # LinAlgError for a matrix that is not positive definite
    return _loo_from(np.linalg.inv(Kn), K, x, y, l)


def loo_longdouble(x, y, e, l):
    """loo_closed_form's formulas in np.longdouble throughout (the kernel included), W = U^T U from a
    hand-written Cholesky factor and forward substitution (LAPACK has no long double). Returns
    longdouble arrays."""
    LD = np.longdouble
    x, y, e = (np.asarray(v, dtype=LD) for v in (x, y, e))
    l = np.asarray(l, dtype=LD).reshape(-1)
    N = len(y)
    a = x / l[:, None]
    n = np.sum(a ** 2, axis=0)
    K = np.exp(-np.maximum(n[:, None] + n[None, :] - 2 * (a.T @ a), LD(0)) / 2)
    A = K + np.diag(e ** 2)
    L = np.zeros((N, N), dtype=LD)
    for j in range(N):
        piv = A[j, j] - L[j, :j] @ L[j, :j]
        if not piv > 0:
            raise np.linalg.LinAlgError("Matrix is not positive definite")
        L[j, j] = np.sqrt(piv)
        L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    U = np.zeros((N, N), dtype=LD)  # U = L^-1, row by row
    for i in range(N):
        row = -(L[i, :i] @ U[:i, :])
        row[i] += 1
        U[i] = row / L[i, i]
    return _loo_from(U.T @ U, K, x, y, l)


def gradient_gap(g, g_ref):
    """max_k |g - g_ref| / max_k |g_ref|, the gradient's error measure of the GPU tests."""
    g_ref = np.asarray(g_ref)
    scale = np.max(np.abs(g_ref))
    return float(np.max(np.abs(np.asarray(g, dtype=g_ref.dtype) - g_ref)) / (scale if scale > 0 else 1))


def numpy_evaluator(x, y, e):
    """value_and_grad for fit_loo; a non-positive-definite point is -inf / NaN, as gpf_loo_batch's."""
    def value_and_grad(positions):
        out, grads = [], []
        for p in np.atleast_2d(positions):
            try:
                _, _, v, g = loo_closed_form(x, y, e, p)
            except np.linalg.LinAlgError:
                v, g = -np.inf, np.full(x.shape[0], np.nan)
            out.append(v)
            grads.append(g)
        return np.array(out), np.array(grads)
    return value_and_grad


def check_fit(best, info):
    """Inside the box, at least as good as the best start, and the counts add up."""
    lower, upper = info["box"]
    assert np.all(best >= lower) and np.all(best <= upper), (best, lower, upper)
    best_start = float(np.max(info["starts"][1]))
    assert info["lpd"] >= best_start, (info["lpd"], best_start)
    assert info["evals"] >= info["starts"][0].shape[0] + info["grad_evals"] > 0


# (seed, d, N, l_true, l): the shapes of the brute-force and central-difference checks (l away from the
# optimum: the error is taken relative to max |grad|, and near the optimum that is rounding noise over ~0)
SHAPES = [(3, 2, 60, (0.4, 0.7), (0.25, 0.4)), (5, 3, 200, (0.3, 0.5, 0.8), (0.28, 0.6, 0.7))]


@pytest.mark.parametrize("seed,d,N,l_true,l", SHAPES)
def test_closed_form_is_brute_force_deletion(seed, d, N, l_true, l):
    """Every point deleted in turn and predicted from the other N - 1 with np.linalg.solve."""
    x, y, e = gp_sample(seed, d, N, l_true)
    l = np.array(l)
    mu, sd, lpd, _ = loo_closed_form(x, y, e, l)
    K = se_kernel(x, l)
    Kn = K + np.diag(e ** 2)
    bmu, bsd = np.empty(N), np.empty(N)
    for i in range(N):
        keep = np.arange(N) != i
        sol = np.linalg.solve(Kn[np.ix_(keep, keep)], np.column_stack([y[keep], K[keep, i]]))
        bmu[i] = K[i, keep] @ sol[:, 0]
        bsd[i] = np.sqrt(1.0 + e[i] ** 2 - K[i, keep] @ sol[:, 1])
    blpd = np.sum(-0.5 * np.log(2 * np.pi * bsd ** 2) - 0.5 * ((y - bmu) / bsd) ** 2)
    errs = (np.max(np.abs(mu - bmu)) / np.max(np.abs(bmu)), np.max(np.abs(sd - bsd) / bsd), abs(lpd - blpd) / abs(blpd))
    print(f"[loo_host] N={N} d={d}: closed form vs deletion: mu {errs[0]:.2e}, sd {errs[1]:.2e}, lpd {errs[2]:.2e}")
    assert max(errs) < 1e-10, errs


@pytest.mark.parametrize("seed,d,N,l_true,l", SHAPES)
def test_closed_form_gradient_is_the_derivative(seed, d, N, l_true, l):
    x, y, e = gp_sample(seed, d, N, l_true)
    l = np.array(l)
    g = loo_closed_form(x, y, e, l)[3]
    fd = np.empty(d)
    for k in range(d):
        h = np.zeros(d)
        h[k] = 1e-5 * l[k]
        fd[k] = (loo_closed_form(x, y, e, l + h)[2] - loo_closed_form(x, y, e, l - h)[2]) / (2 * h[k])
    err = np.max(np.abs(fd - g)) / np.max(np.abs(g))
    print(f"[loo_host] N={N} d={d}: gradient vs central differences {err:.2e} of max |grad|")
    assert err < 1e-6, (fd, g)


def test_longdouble_form_agrees_with_float64():
    """The two references are the same formulas: they agree far inside the GPU tests' 1e-9."""
    seed, d, N, l_true, l = SHAPES[0]
    x, y, e = gp_sample(seed, d, N, l_true)
    a, b = loo_closed_form(x, y, e, l), loo_longdouble(x, y, e, l)
    assert b[3].dtype == np.longdouble
    assert np.max(np.abs(a[0] - b[0])) < 1e-11 * np.max(np.abs(a[0]))
    assert np.max(np.abs(a[1] - b[1]) / a[1]) < 1e-11
    assert abs(a[2] - b[2]) < 1e-11 * abs(a[2])
    assert gradient_gap(a[3], b[3]) < 1e-10


@pytest.mark.parametrize("seed,d,N,l_true", FIT_RECIPES)
def test_fit_loo_with_numpy_evaluator(seed, d, N, l_true):
    from gpfit.loo import fit_loo
    x, y, e = gp_sample(seed, d, N, l_true)
    ev = numpy_evaluator(x, y, e)
    best, info = fit_loo(x, y, e, num_starts=16, num_polish=1, max_points=N, seed=seed, value_and_grad=ev,
                         verbose=False)
    check_fit(best, info)
    assert "lml" not in info and set(info["polished"][0]) >= {"lpd", "start_lpd", "x", "start", "nfev", "nit", "message"}
    # the reported value is the evaluator's at the returned point
    assert abs(ev(best[None, :])[0][0] - info["lpd"]) <= 1e-9 * abs(info["lpd"])
    # seeded: the same fit again
    again, info2 = fit_loo(x, y, e, num_starts=16, num_polish=1, max_points=N, seed=seed, value_and_grad=ev,
                           verbose=False)
    np.testing.assert_array_equal(best, again)
    assert len(info["polished"]) == 1 and info2["evals"] == info["evals"]


def test_fit_loo_survives_non_pd_region():
    """Non-PD (-inf, NaN gradient) above some l: a losing point for the starts and the line search,
    never an error."""
    from gpfit.loo import fit_loo
    seed, d, N, l_true = FIT_RECIPES[0]
    x, y, e = gp_sample(seed, d, N, l_true)
    inner = numpy_evaluator(x, y, e)
    calls = {"bad": 0}

    def ev(positions):
        v, g = inner(positions)
        bad = np.any(np.atleast_2d(positions) > 0.45, axis=1)
        calls["bad"] += int(np.sum(bad))
        v[bad] = -np.inf
        g[bad] = np.nan
        return v, g

    best, info = fit_loo(x, y, e, num_starts=16, num_polish=3, max_points=N, seed=seed, value_and_grad=ev,
                         verbose=False)
    assert calls["bad"] > 0
    assert np.all(best <= 0.45) and np.isfinite(info["lpd"])
    assert info["lpd"] >= np.max(info["starts"][1])
    best2, info2 = fit_loo(x, y, e, num_starts=4, num_polish=2, max_points=N, seed=seed,
                           value_and_grad=lambda p: (np.full(len(p), -np.inf), np.full(p.shape, np.nan)),
                           verbose=False)
    assert info2["lpd"] == -np.inf and best2.shape == (d,)


def test_len_scale_opt_dispatches_loo(monkeypatch):
    """objective="loo" reaches fit_loo with the fit's keywords, and fit_loo runs on an injected
    evaluator behind it; an unknown objective still raises and names the three choices."""
    import find_len_scales as fls
    import gpfit.loo
    seed, d, N, l_true = FIT_RECIPES[2]
    x, y, e = gp_sample(seed, d, N, l_true)
    real, seen = gpfit.loo.fit_loo, {}

    def injected(xk, yk, ek, **kw):
        seen.update(kw)
        return real(xk, yk, ek, value_and_grad=numpy_evaluator(xk, yk, ek), num_polish=1, **kw)

    monkeypatch.setattr(gpfit.loo, "fit_loo", injected)
    monkeypatch.setattr(fls, "particle_swarm", lambda *a, **k: pytest.fail("the swarm ran"))
    best = fls.len_scale_opt(x, y, e, False, objective="loo", num_starts=8, max_points=N, seed=3)
    assert seen == {"num_starts": 8, "max_points": N, "seed": 3, "verbose": False}
    want, _ = real(x, y, e, value_and_grad=numpy_evaluator(x, y, e), num_polish=1, num_starts=8, max_points=N, seed=3,
                   verbose=False)
    np.testing.assert_array_equal(best, want)
    with pytest.raises(ValueError, match="unknown objective") as ei:
        fls.len_scale_opt(x, y, e, False, objective="likelihood")
    assert all(name in str(ei.value) for name in ("calibration", "marginal_likelihood", "loo"))


def test_options_yaml_accepts_loo(tmp_path, monkeypatch):
    import GP_fit
    monkeypatch.chdir(tmp_path)
    (tmp_path / "options.yaml").write_text('file_name: ["a.txt"]\nresolution: [0.1]\nlen_scale_objective: loo\n'
                                           "mle_num_starts: 24\npso_seed: 3\npso_max_points: 80\n")
    assert GP_fit._pso_overrides() == {"objective": "loo", "num_starts": 24, "seed": 3, "max_points": 80}


def test_c_entry_point_without_a_device():
    """gpf_loo_batch is in the signature table as the header declares it, and a null context is
    GPF_BAD_ARG before anything touches a device."""
    import gpfit
    from gpfit import _lib
    res, args = _lib.SIGNATURES["gpf_loo_batch"]
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
    assert res is ctypes.c_int
    assert args == [ctypes.c_void_p, dp, ctypes.c_int, dp, dp, dp, dp, ip, ip]
    lib = gpfit.load_library()
    ls, out = np.array([[0.3]]), np.zeros(1)
    bad = ctypes.c_int(7)
    rc = lib.gpf_loo_batch(None, ls.ctypes.data_as(dp), 1, out.ctypes.data_as(dp), None, None, None, None,
                           ctypes.byref(bad))
    assert rc == _lib.GPF_BAD_ARG
    assert lib.gpf_version() == _lib.ABI_VERSION == 2
