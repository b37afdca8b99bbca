"""The amplitude / noise-scale model without a GPU: the closed form the GPU tests compare
gpf_lml_hyper_batch against (float64 NumPy and the same formulas in np.longdouble;
tests/test_amplitude_gpu.py imports both from here), checked against central differences; the
closed-form best amplitude; gpfit.amplitude.fit_hyper on an injected NumPy evaluator; the options.yaml
key; the C entry point's table entry.

The closed form is built directly from Kn = a^2 K + s^2 diag(e^2) and its derivatives
dKn/da = 2 a K, dKn/ds = 2 s diag(e^2): it never forms the unit-amplitude Kt = Kn / a^2 the
library factors, so it is an independent derivation of what the device computes.
"""
import ctypes

import numpy as np
import pytest

from test_mle_host import FIT_RECIPES, gp_sample, se_kernel

LOG_2PI = 1.8378770664093453


def _hyper_from(W, logdet_half, K, x, y, e, theta):
    """(lml, grad (d + 2,)) from W = Kn^-1, sum log L_ii and the noise-free K, in the dtype of W."""
    d = len(theta) - 2
    l, a, s = theta[:d], theta[d], theta[d + 1]
    al = W @ y
    half = W.dtype.type(0.5)
    lml = -half * (y @ al) - logdet_half - half * len(y) * W.dtype.type(LOG_2PI)
    M = np.outer(al, al) - W
    MK = M * K
    g_l = [half * a * a * np.sum(MK * (x[k][:, None] - x[k][None, :]) ** 2) / l[k] ** 3 for k in range(d)]
    g_a = a * np.sum(MK)
    g_s = s * np.sum(np.diag(M) * e ** 2)
    return lml, np.array(g_l + [g_a, g_s])


def hyper_closed_form(x, y, e, theta):
    """(LML, dLML/dtheta (d + 2,)) in float64 NumPy for theta = (l_1 .. l_d, a, s),
    Kn = a^2 K(l) + s^2 diag(e^2): L = chol(Kn), W = Kn^-1 (np.linalg.inv), alpha = W y,
    LML = -1/2 y^T alpha - sum log L_ii - N/2 log(2 pi), M = alpha alpha^T - W,
    g_l_k = 1/2 sum_ij M_ij a^2 K_ij (x_ik - x_jk)^2 / l_k^3, g_a = a sum_ij (M o K)_ij,
    g_s = s sum_i M_ii e_i^2."""
    theta = np.asarray(theta, dtype=np.float64).reshape(-1)
    d = len(theta) - 2
    K = se_kernel(x, theta[:d])
    Kn = theta[d] ** 2 * K + theta[d + 1] ** 2 * np.diag(e ** 2)
    L = np.linalg.cholesky(Kn)  # LinAlgError for a matrix that is not positive definite
    return _hyper_from(np.linalg.inv(Kn), np.sum(np.log(np.diag(L))), K, x, y, e, theta)


def hyper_longdouble(x, y, e, theta):
    """hyper_closed_form's formulas in np.longdouble throughout (the kernel included), W = U^T U from a
    hand-written Cholesky factor and forward substitution (LAPACK has no long double)."""
    LD = np.longdouble
    x, y, e = (np.asarray(v, dtype=LD) for v in (x, y, e))
    theta = np.asarray(theta, dtype=LD).reshape(-1)
    d, N = len(theta) - 2, len(y)
    sc = x / theta[:d, None]
    n = np.sum(sc ** 2, axis=0)
    K = np.exp(-np.maximum(n[:, None] + n[None, :] - 2 * (sc.T @ sc), LD(0)) / 2)
    A = theta[d] ** 2 * K + theta[d + 1] ** 2 * np.diag(e ** 2)
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
    return _hyper_from(U.T @ U, np.sum(np.log(np.diag(L))), K, x, y, e, theta)


def unit_q(x, y, e, l, ratio):
    """Q = y^T Kt^-1 y of the unit-amplitude Kt = K(l) + ratio^2 diag(e^2)."""
    Kt = se_kernel(x, np.asarray(l, dtype=np.float64)) + ratio ** 2 * np.diag(e ** 2)
    return float(y @ np.linalg.solve(Kt, y))


def numpy_evaluator(x, y, e):
    """value_and_grad for fit_hyper; a non-positive-definite point is -inf / NaN, as
    gpf_lml_hyper_batch's."""
    def value_and_grad(theta):
        out, grads = [], []
        for p in np.atleast_2d(theta):
            try:
                v, g = hyper_closed_form(x, y, e, p)
            except np.linalg.LinAlgError:
                v, g = -np.inf, np.full(x.shape[0] + 2, np.nan)
            out.append(v)
            grads.append(g)
        return np.array(out), np.array(grads)
    return value_and_grad


A_GEN, S_GEN = 2.5, 2.0


def scaled_sample(seed, d, N, l_true):
    """gp_sample's data multiplied by 2.5 with its errors understated by a factor of 2, and the theta
    that generated it: (x, 2.5 y, 2.5 e / 2, (l_true, 2.5, 2))."""
    x, y, e = gp_sample(seed, d, N, l_true)
    return x, A_GEN * y, A_GEN * e / S_GEN, np.array(list(l_true) + [A_GEN, S_GEN])


def check_fit(best, info, truth_lml):
    lower, upper = info["box"]
    assert np.all(best >= lower) and np.all(best <= upper), (best, lower, upper)
    assert info["lml"] >= truth_lml, (info["lml"], truth_lml)
    assert info["lml"] >= float(np.max(info["starts"][1])) - 1e-9 * abs(info["lml"])
    assert info["evals"] >= info["starts"][0].shape[0] and info["evals"] >= info["grad_evals"] > 0


# (seed, d, N, l_true, theta): theta away from the optimum (the error is taken relative to max |grad|)
SHAPES = [(3, 2, 60, (0.4, 0.7), (0.25, 0.4, 1.7, 0.8)), (5, 3, 120, (0.3, 0.5, 0.8), (0.28, 0.6, 0.7, 0.6, 1.9))]


@pytest.mark.parametrize("seed,d,N,l_true,theta", SHAPES)
def test_closed_form_gradient_is_the_derivative(seed, d, N, l_true, theta):
    x, y, e = gp_sample(seed, d, N, l_true)
    theta = np.array(theta)
    g = hyper_closed_form(x, y, e, theta)[1]
    fd = np.empty(d + 2)
    for k in range(d + 2):
        h = np.zeros(d + 2)
        h[k] = 1e-5 * theta[k]
        fd[k] = (hyper_closed_form(x, y, e, theta + h)[0] - hyper_closed_form(x, y, e, theta - h)[0]) / (2 * h[k])
    err = np.max(np.abs(fd - g)) / np.max(np.abs(g))
    print(f"[amplitude_host] N={N} d={d}: gradient vs central differences {err:.2e} of max |grad|")
    assert err < 1e-6, (fd, g)


def test_unit_theta_is_the_length_scale_closed_form():
    """a = s = 1 is the model of every other call."""
    from test_mle_host import lml_closed_form
    seed, d, N, l_true, theta = SHAPES[0]
    x, y, e = gp_sample(seed, d, N, l_true)
    l = np.array(theta[:d])
    v, g = hyper_closed_form(x, y, e, np.append(l, [1.0, 1.0]))
    v0, g0 = lml_closed_form(x, y, e, l)
    assert abs(v - v0) < 1e-12 * abs(v0)
    assert np.max(np.abs(g[:d] - g0)) < 1e-12 * np.max(np.abs(g0))


@pytest.mark.parametrize("seed,d,N,l_true,theta", SHAPES)
def test_profiled_amplitude_zeroes_the_radial_derivative(seed, d, N, l_true, theta):
    """At fixed l and s / a the likelihood is maximal at a^2 = Q / N: there a g_a + s g_s = Q / a^2 - N = 0,
    and the value is the closed-form profile of the value at a = 1."""
    x, y, e = gp_sample(seed, d, N, l_true)
    theta = np.array(theta)
    ratio = theta[d + 1] / theta[d]
    q = unit_q(x, y, e, theta[:d], ratio)
    a = np.sqrt(q / N)
    at = np.concatenate([theta[:d], [a, ratio * a]])
    v, g = hyper_closed_form(x, y, e, at)
    radial = a * g[d] + ratio * a * g[d + 1]
    assert abs(radial) < 1e-8 * N, radial
    # away from it the radial derivative is Q / a^2 - N
    v1, g1 = hyper_closed_form(x, y, e, np.concatenate([theta[:d], [1.0, ratio]]))
    assert abs((g1[d] + ratio * g1[d + 1]) - (q - N)) < 1e-8 * max(q, N)
    assert abs(v - (v1 + 0.5 * q - 0.5 * N - 0.5 * N * np.log(q / N))) < 1e-10 * abs(v)
    for f in (0.9, 1.1):
        assert hyper_closed_form(x, y, e, np.concatenate([theta[:d], [f * a, ratio * f * a]]))[0] < v


def test_longdouble_form_agrees_with_float64():
    seed, d, N, l_true, theta = SHAPES[0]
    x, y, e = gp_sample(seed, d, N, l_true)
    (v, g), (vl, gl) = hyper_closed_form(x, y, e, theta), hyper_longdouble(x, y, e, theta)
    assert gl.dtype == np.longdouble
    assert abs(v - vl) < 1e-11 * abs(v)
    assert np.max(np.abs(g - gl)) < 1e-10 * np.max(np.abs(gl))


def test_scaled_data_is_the_unit_model():
    """lml(theta) on (y, e) = lml(l, 1, 1) on (y / a, e s / a) - N log a."""
    from gpfit.amplitude import scaled_data
    seed, d, N, l_true, theta = SHAPES[0]
    x, y, e = gp_sample(seed, d, N, l_true)
    theta = np.array(theta)
    ys, es = scaled_data(y, e, theta[d], theta[d + 1])
    np.testing.assert_array_equal(ys, y / theta[d])
    np.testing.assert_array_equal(es, e * (theta[d + 1] / theta[d]))
    v = hyper_closed_form(x, y, e, theta)[0]
    vu = hyper_closed_form(x, ys, es, np.append(theta[:d], [1.0, 1.0]))[0]
    assert abs(v - (vu - N * np.log(theta[d]))) < 1e-11 * abs(v)
    for bad in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError, match="finite and > 0"):
            scaled_data(y, e, bad, 1.0)
        with pytest.raises(ValueError, match="finite and > 0"):
            scaled_data(y, e, 1.0, bad)


@pytest.mark.parametrize("seed,d,N,l_true", FIT_RECIPES)
def test_fit_hyper_with_numpy_evaluator(seed, d, N, l_true):
    from gpfit.amplitude import fit_hyper
    x, y, e, gen = scaled_sample(seed, d, N, l_true)
    ev = numpy_evaluator(x, y, e)
    best, info = fit_hyper(x, y, e, num_starts=16, num_polish=2, max_points=N, seed=seed, value_and_grad=ev,
                           verbose=False)
    truth = hyper_closed_form(x, y, e, gen)[0]
    print(f"[amplitude_host] d={d} N={N}: fit {info['lml']:.4f} at {best}, generating theta {truth:.4f}, "
          f"best start {np.max(info['starts'][1]):.4f}, evals {info['evals']}")
    assert best.shape == (d + 2,)
    check_fit(best, info, truth)
    assert set(info) == {"lml", "evals", "grad_evals", "box", "starts", "polished"}
    assert info["starts"][0].shape == (16, d + 2) and len(info["polished"]) == 2
    # the box of the amplitude and the noise scale
    lower, upper = info["box"]
    np.testing.assert_allclose(lower[d:], [1e-3 * np.std(y), 1e-2], rtol=1e-15)
    np.testing.assert_allclose(upper[d:], [1e3 * np.std(y), 1e2], rtol=1e-15)
    # the reported value is the evaluator's at the returned point, the start values are the evaluator's
    assert abs(ev(best[None, :])[0][0] - info["lml"]) <= 1e-9 * abs(info["lml"])
    starts, vals = info["starts"]
    k = int(np.argmax(vals))
    assert abs(ev(starts[k][None, :])[0][0] - vals[k]) <= 1e-9 * abs(vals[k])
    # seeded: the same fit again
    again, info2 = fit_hyper(x, y, e, num_starts=16, num_polish=2, max_points=N, seed=seed, value_and_grad=ev,
                             verbose=False)
    np.testing.assert_array_equal(best, again)
    assert info2["evals"] == info["evals"]


def test_fit_hyper_survives_non_pd_region():
    """Non-PD (-inf, NaN gradient) above some l: a losing point for the starts and the line search,
    never an error."""
    from gpfit.amplitude import fit_hyper
    seed, d, N, l_true = FIT_RECIPES[0]
    x, y, e, _ = scaled_sample(seed, d, N, l_true)
    inner = numpy_evaluator(x, y, e)
    calls = {"bad": 0}

    def ev(theta):
        v, g = inner(theta)
        bad = np.any(np.atleast_2d(theta)[:, :d] > 0.45, axis=1)
        calls["bad"] += int(np.sum(bad))
        v[bad] = -np.inf
        g[bad] = np.nan
        return v, g

    best, info = fit_hyper(x, y, e, num_starts=16, num_polish=3, max_points=N, seed=seed, value_and_grad=ev,
                           verbose=False)
    assert calls["bad"] > 0
    assert np.all(best[:d] <= 0.45) and np.isfinite(info["lml"])
    assert info["lml"] >= np.max(info["starts"][1]) - 1e-9 * abs(info["lml"])
    # every start losing: still no error, the value says so
    best2, info2 = fit_hyper(x, y, e, num_starts=4, num_polish=2, max_points=N, seed=seed,
                             value_and_grad=lambda p: (np.full(len(p), -np.inf), np.full(p.shape, np.nan)),
                             verbose=False)
    assert info2["lml"] == -np.inf and best2.shape == (d + 2,)


def test_fit_lml_and_fit_loo_share_the_polish_stage():
    """The stage fit_hyper shares with fit_lml is the one fit_lml ran before: the recorded figures of
    tests/test_mle_host.py hold (73.44 from the best start's 68.32)."""
    from gpfit.mle import fit_lml
    from test_mle_host import numpy_evaluator as lml_evaluator
    seed, d, N, l_true = FIT_RECIPES[0]
    x, y, e = gp_sample(seed, d, N, l_true)
    _, info = fit_lml(x, y, e, num_starts=16, num_polish=1, max_points=N, seed=seed,
                      value_and_grad=lml_evaluator(x, y, e), verbose=False)
    assert abs(info["lml"] - 73.44) < 0.01 and abs(np.max(info["starts"][1]) - 68.32) < 0.01


def test_options_yaml_key_reaches_fit_hyper(tmp_path, monkeypatch):
    """len_scale_objective: marginal_likelihood_full fits with fit_hyper (the fit's keywords from the
    yaml) and predicts with GP_hyper; the swarm, len_scale_opt and GP are not called."""
    import GP_fit
    import gpfit.amplitude
    monkeypatch.chdir(tmp_path)
    (tmp_path / "options.yaml").write_text('file_name: ["a.txt"]\nresolution: [0.1]\n'
                                           "len_scale_objective: marginal_likelihood_full\n"
                                           "mle_num_starts: 24\npso_seed: 3\npso_max_points: 80\n")
    assert GP_fit._pso_overrides() == {"objective": "marginal_likelihood_full", "num_starts": 24, "seed": 3,
                                       "max_points": 80}
    seen = {}

    def fake_fit(x, y, e, **kw):
        seen["fit"] = kw
        return np.array([0.5, 2.0, 1.5]), {}

    def fake_gp(xk, yk, ek, grid, theta):
        seen["theta"] = np.array(theta)
        return np.zeros(grid.shape[1]), np.ones(grid.shape[1])

    x = np.linspace(0.0, 1.0, 5)[None, :]
    monkeypatch.setattr(gpfit.amplitude, "fit_hyper", fake_fit)
    monkeypatch.setattr(GP_fit, "GP_hyper", fake_gp)
    monkeypatch.setattr(GP_fit, "len_scale_opt", lambda *a, **k: pytest.fail("len_scale_opt ran"))
    monkeypatch.setattr(GP_fit, "GP", lambda *a, **k: pytest.fail("GP ran"))
    monkeypatch.setattr(GP_fit, "read_yaml", lambda: ([0.1], False, str(tmp_path / "out.txt"), ["x", "q", "err"],
                                                      [("a.txt", [x], [(x[0], np.ones(5))], None)], False, False))
    monkeypatch.setattr(GP_fit, "fill_convex_hull", lambda pts, res: pts)
    GP_fit.create_GP()
    assert seen["fit"] == {"num_starts": 24, "seed": 3, "max_points": 80, "verbose": False}
    np.testing.assert_array_equal(seen["theta"], [0.5, 2.0, 1.5])
    # with the marginalised prediction it is an error, not a silent choice
    (tmp_path / "options.yaml").write_text('file_name: ["a.txt"]\nresolution: [0.1]\n'
                                           "len_scale_objective: marginal_likelihood_full\nhyper_samples: 4\n")
    with pytest.raises(ValueError, match="hyper_samples"):
        GP_fit.create_GP()


def test_gp_hyper_is_in_the_drop_in_surface():
    import GP_func
    assert "GP_hyper" in GP_func.__all__
    with pytest.raises(ValueError, match="x_fit must be"):
        GP_func.GP_hyper(np.zeros((2, 3)), np.zeros(3), np.ones(3), np.zeros((1, 4)), np.ones(4))


def test_c_entry_point_without_a_device():
    """gpf_lml_hyper_batch is in the signature table as the header declares it, and a null context is
    GPF_BAD_ARG before anything touches a device."""
    import gpfit
    from gpfit import _lib
    res, args = _lib.SIGNATURES["gpf_lml_hyper_batch"]
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
    assert res is ctypes.c_int
    assert args == [ctypes.c_void_p, dp, ctypes.c_int, dp, dp, dp, ip, ip]
    lib = gpfit.load_library()
    th, out = np.array([[0.3, 1.0, 1.0]]), np.zeros(1)
    bad = ctypes.c_int(7)
    rc = lib.gpf_lml_hyper_batch(None, th.ctypes.data_as(dp), 1, out.ctypes.data_as(dp), None, None, None,
                                 ctypes.byref(bad))
    assert rc == _lib.GPF_BAD_ARG
    assert lib.gpf_version() == _lib.ABI_VERSION == 2
