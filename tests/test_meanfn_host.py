"""The marginalised polynomial mean without a GPU: the basis, the closed form the GPU tests compare
gpf_lml_mean_batch against (gpfit.meanfn.mean_closed_form, float64 NumPy straight from Kn by Rasmussen &
Williams eq. 2.45) checked against the same formulas in np.longdouble (``mean_longdouble``, which
tests/test_meanfn_gpu.py imports), against a literal evaluation of eq. 2.45 with determinants and
against central differences; the closed-form best amplitude; gpfit.meanfn.fit_mean on an injected NumPy
evaluator; the options.yaml key; the bindings' argument checks and the C entry points' table entries.
"""
import ctypes

import numpy as np
import pytest

from test_mle_host import FIT_RECIPES, gp_sample, se_kernel

LOG_2PI = 1.8378770664093453


def mean_longdouble(x, y, e, H, theta):
    """gpfit.meanfn.reml_from's formulas in np.longdouble throughout (the kernel included), W = U^T U from
    a hand-written Cholesky factor and forward substitution as tests/test_amplitude_host.py's
    hyper_longdouble: (lml, grad (d + 2,), beta (m,), Q')."""
    from gpfit.meanfn import reml_from
    LD = np.longdouble
    x, y, e, H = (np.asarray(v, dtype=LD) for v in (x, y, e, np.atleast_2d(H)))
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
    U = np.zeros((N, N), dtype=LD)
    for i in range(N):
        row = -(L[i, :i] @ U[:i, :])
        row[i] += 1
        U[i] = row / L[i, i]
    out = reml_from(U.T @ U, np.sum(np.log(np.diag(L))), K, x, y, e, H, theta)
    assert out[1].dtype == LD
    return out


def gaps(got, ref):
    """The distances the GPU tests use: value and Q' |.| / max(|ref|, 1), gradient and beta the largest
    component error over the largest reference component."""
    v, g, b, q = got
    rv, rg, rb, rq = (np.asarray(r, dtype=np.float64) for r in ref)
    return (abs(v - rv) / max(abs(rv), 1.0), np.max(np.abs(g - rg)) / np.max(np.abs(rg)),
            np.max(np.abs(b - rb)) / max(np.max(np.abs(rb)), 1.0), abs(q - rq) / max(abs(rq), 1.0))


def trend_sample(seed, d, N, l_true):
    """gp_sample's data times 2.5 plus the mean 5 + 3 u_1 (u the first coordinate mapped to [-1, 1] by the
    training box), errors understated by a factor of 2: (x, y, e, generating theta, generating beta in the
    linear basis)."""
    from gpfit.meanfn import basis
    x, y, e = gp_sample(seed, d, N, l_true)
    H, _ = basis(x, "linear")
    beta = np.zeros(1 + d)
    beta[0], beta[1] = 5.0, 3.0
    return x, 2.5 * y + H.T @ beta, 2.5 * e / 2.0, np.array(list(l_true) + [2.5, 2.0]), beta


# (seed, d, N, l_true, kind, theta): theta away from the optimum
SHAPES = [(3, 2, 60, (0.4, 0.7), "quadratic", (0.25, 0.4, 1.7, 0.8)),
          (5, 3, 120, (0.3, 0.5, 0.8), "linear", (0.28, 0.6, 0.7, 0.6, 1.9)),
          (7, 1, 40, (0.3,), "constant", (0.2, 1.3, 1.1))]


def _shape(seed, d, N, l_true, kind):
    from gpfit.meanfn import basis
    x, y, e = gp_sample(seed, d, N, l_true)
    y = y + 5.0 + 2.0 * x[0]
    return x, y, e, basis(x, kind)[0]


def test_basis_shapes_box_round_trip_and_row_limit():
    from gpfit.meanfn import basis, basis_rows
    rng = np.random.default_rng(0)
    x = rng.uniform(2.0, 7.0, size=(3, 50))
    for kind, m in (("constant", 1), ("linear", 4), ("quadratic", 10)):
        H, box = basis(x, kind)
        assert H.shape == (m, 50) and basis_rows(kind, 3) == m
        np.testing.assert_array_equal(H[0], np.ones(50))
        assert np.linalg.matrix_rank(H) == m
    H, (lo, hi) = basis(x, "quadratic")
    np.testing.assert_array_equal(lo, x.min(axis=1))
    np.testing.assert_array_equal(hi, x.max(axis=1))
    assert np.min(H[1:4]) == -1.0 and np.max(H[1:4]) == 1.0
    np.testing.assert_allclose(H[4], H[1] ** 2, rtol=0, atol=0)
    np.testing.assert_array_equal(H[5], H[1] * H[2])
    # the query points use the training box: the same points give the same rows, others extrapolate
    H2, box2 = basis(x[:, :7], "quadratic", (lo, hi))
    np.testing.assert_array_equal(H2, H[:, :7])
    np.testing.assert_array_equal(box2[0], lo)
    far, _ = basis(np.full((3, 1), 12.0), "linear", (lo, hi))
    assert np.all(far[1:] > 1.0)
    # a coordinate without spread maps to 0
    flat = x.copy()
    flat[1] = 3.0
    np.testing.assert_array_equal(basis(flat, "linear")[0][2], np.zeros(50))
    # 1 + 7 + 28 = 36 rows
    with pytest.raises(ValueError, match="more than 32"):
        basis(rng.uniform(size=(7, 40)), "quadratic")
    assert basis(rng.uniform(size=(6, 40)), "quadratic")[0].shape == (28, 40)
    with pytest.raises(ValueError, match="kind"):
        basis(x, "cubic")
    with pytest.raises(ValueError, match="box"):
        basis(x, "linear", (lo[:2], hi[:2]))


@pytest.mark.parametrize("seed,d,N,l_true,kind,theta", SHAPES)
def test_closed_form_against_longdouble_and_eq_2_45(seed, d, N, l_true, kind, theta):
    from gpfit.meanfn import mean_closed_form
    x, y, e, H = _shape(seed, d, N, l_true, kind)
    theta = np.array(theta)
    got = mean_closed_form(x, y, e, H, theta)
    gv, gg, gb, gq = gaps(got, mean_longdouble(x, y, e, H, theta))
    print(f"[meanfn_host] N={N} d={d} {kind}: float64 vs longdouble value {gv:.2e} grad {gg:.2e} beta {gb:.2e} Q' {gq:.2e}")
    assert max(gv, gg, gb, gq) < 1e-10
    # eq. 2.45 literally: -1/2 y^T Ky^-1 y + 1/2 y^T C y - 1/2 log|Ky| - 1/2 log|A| - (n - m)/2 log 2 pi
    m = H.shape[0]
    Kn = theta[d] ** 2 * se_kernel(x, theta[:d]) + theta[d + 1] ** 2 * np.diag(e ** 2)
    Ki = np.linalg.inv(Kn)
    A = H @ Ki @ H.T
    C = Ki @ H.T @ np.linalg.inv(A) @ H @ Ki
    direct = (-0.5 * y @ Ki @ y + 0.5 * y @ C @ y - 0.5 * np.linalg.slogdet(Kn)[1] - 0.5 * np.linalg.slogdet(A)[1]
              - 0.5 * (N - m) * LOG_2PI)
    assert abs(got[0] - direct) < 1e-11 * max(abs(direct), 1.0)
    np.testing.assert_allclose(got[2], np.linalg.solve(A, H @ Ki @ y), rtol=1e-9)
    # Q' is y^T Pt y of the unit-amplitude matrix
    Kt = Kn / theta[d] ** 2
    Kti = np.linalg.inv(Kt)
    Pt = Kti - Kti @ H.T @ np.linalg.inv(H @ Kti @ H.T) @ H @ Kti
    assert abs(got[3] - y @ Pt @ y) < 1e-10 * abs(got[3])


@pytest.mark.parametrize("seed,d,N,l_true,kind,theta", SHAPES)
def test_closed_form_gradient_is_the_derivative(seed, d, N, l_true, kind, theta):
    from gpfit.meanfn import mean_closed_form
    x, y, e, H = _shape(seed, d, N, l_true, kind)
    theta = np.array(theta)
    g = mean_closed_form(x, y, e, H, theta)[1]
    fd = np.empty(d + 2)
    for k in range(d + 2):
        h = np.zeros(d + 2)
        h[k] = 1e-5 * theta[k]
        fd[k] = (mean_closed_form(x, y, e, H, theta + h)[0] - mean_closed_form(x, y, e, H, theta - h)[0]) / (2 * h[k])
    err = np.max(np.abs(fd - g)) / np.max(np.abs(g))
    print(f"[meanfn_host] N={N} d={d} {kind}: gradient vs central differences {err:.2e} of max |grad|")
    assert err < 1e-6, (fd, g)


@pytest.mark.parametrize("seed,d,N,l_true,kind,theta", SHAPES)
def test_profiled_amplitude_zeroes_the_radial_derivative(seed, d, N, l_true, kind, theta):
    """At fixed l and s / a the restricted likelihood is maximal at a^2 = Q' / (N - m)."""
    from gpfit.meanfn import mean_closed_form
    x, y, e, H = _shape(seed, d, N, l_true, kind)
    theta = np.array(theta)
    m, ratio = H.shape[0], theta[d + 1] / theta[d]
    v1, g1, b1, q = mean_closed_form(x, y, e, H, np.concatenate([theta[:d], [1.0, ratio]]))
    a = np.sqrt(q / (N - m))
    v, g, b, q2 = mean_closed_form(x, y, e, H, np.concatenate([theta[:d], [a, ratio * a]]))
    assert abs(a * g[d] + ratio * a * g[d + 1]) < 1e-8 * N
    assert abs(q2 - q) < 1e-10 * q                      # Q' and beta do not depend on a at fixed s / a
    np.testing.assert_allclose(b, b1, rtol=1e-9, atol=1e-12)
    assert abs((g1[d] + ratio * g1[d + 1]) - (q - (N - m))) < 1e-8 * max(q, N)
    assert abs(v - (v1 + 0.5 * q - 0.5 * (N - m) - 0.5 * (N - m) * np.log(q / (N - m)))) < 1e-10 * abs(v)
    for f in (0.9, 1.1):
        assert mean_closed_form(x, y, e, H, np.concatenate([theta[:d], [f * a, ratio * f * a]]))[0] < v


def test_value_is_invariant_under_what_the_basis_spans():
    """y + H^T c changes beta by c and nothing else. (A modest c: the closed form works from Kn^-1 y, which
    holds |c|^2 eps cond(Kn) of y^T P y and is 5e-8 off at an offset of 1000 on this shape; the device
    forms the residual instead, and tests/test_meanfn_gpu.py shifts by 1000 there.)"""
    from gpfit.meanfn import mean_closed_form
    seed, d, N, l_true, kind, theta = SHAPES[1]
    x, y, e, H = _shape(seed, d, N, l_true, kind)
    c = np.array([10.0, -4.0, 0.7, 0.5])
    v, g, b, q = mean_closed_form(x, y, e, H, theta)
    v2, g2, b2, q2 = mean_closed_form(x, y + H.T @ c, e, H, theta)
    assert abs(v2 - v) < 1e-9 * max(abs(v), 1.0)
    assert np.max(np.abs(g2 - g)) < 1e-9 * np.max(np.abs(g))
    np.testing.assert_allclose(b2 - b, c, rtol=1e-9)


def test_predict_closed_form_is_the_vague_prior_limit():
    """Eq. 2.41-2.42 against an ordinary GP with the kernel Kn + b H^T H as b grows."""
    from gpfit.meanfn import basis, predict_mean_closed_form
    seed, d, N, l_true, kind, theta = SHAPES[0]
    x, y, e, H = _shape(seed, d, N, l_true, "linear")
    theta = np.array(theta)
    _, box = basis(x, "linear")
    xf = np.random.default_rng(1).uniform(-0.3, 1.3, size=(d, 25))
    hf = basis(xf, "linear", box)[0]
    mu, sd, beta, bcov = predict_mean_closed_form(x, y, e, H, theta, xf, hf)
    a, s, b = theta[d], theta[d + 1], 1e6
    aa, bb = x / theta[:d, None], xf / theta[:d, None]
    ks = a * a * np.exp(-0.5 * np.maximum(np.sum(aa ** 2, 0)[:, None] + np.sum(bb ** 2, 0)[None, :] - 2 * aa.T @ bb, 0))
    Kb = a * a * se_kernel(x, theta[:d]) + s * s * np.diag(e ** 2) + b * H.T @ H
    kb = ks + b * H.T @ hf
    sol = np.linalg.solve(Kb, kb)
    np.testing.assert_allclose(mu, sol.T @ y, rtol=1e-5)
    np.testing.assert_allclose(sd ** 2, a * a + b * np.sum(hf * hf, 0) - np.sum(kb * sol, 0), rtol=1e-4)
    assert bcov.shape == (d + 1, d + 1) and np.all(np.linalg.eigvalsh(bcov) > 0)


def numpy_evaluator():
    """value_and_grad for fit_mean: bound to the prepared points and basis by the fit
    (value_and_grad.bind); a non-positive-definite point is -inf / NaN, as gpf_lml_mean_batch's."""
    from gpfit.meanfn import mean_closed_form
    data = {}

    def value_and_grad(theta):
        out, grads = [], []
        for p in np.atleast_2d(theta):
            try:
                v, g = mean_closed_form(data["x"], data["y"], data["e"], data["H"], p)[:2]
            except np.linalg.LinAlgError:
                v, g = -np.inf, np.full(len(p), np.nan)
            out.append(v)
            grads.append(g)
        return np.array(out), np.array(grads)

    value_and_grad.bind = lambda x, y, e, H: data.update(x=x, y=y, e=e, H=H)
    return value_and_grad


def test_fit_mean_with_numpy_evaluator():
    from gpfit.amplitude import fit_hyper
    from gpfit.meanfn import basis, fit_mean, mean_closed_form
    from test_amplitude_host import numpy_evaluator as hyper_evaluator
    seed, d, N, l_true = FIT_RECIPES[0]
    x, y, e, gen, beta_gen = trend_sample(seed, d, N, l_true)
    ev = numpy_evaluator()
    best, info = fit_mean(x, y, e, kind="linear", num_starts=16, num_polish=2, max_points=N, seed=seed,
                          value_and_grad=ev, verbose=False)
    H = basis(x, "linear")[0]
    truth = mean_closed_form(x, y, e, H, gen)[0]
    print(f"[meanfn_host] fit {info['lml']:.4f} at {best}, generating theta {truth:.4f}, beta {info['beta']}, "
          f"evals {info['evals']}")
    assert best.shape == (d + 2,)
    assert set(info) == {"lml", "evals", "grad_evals", "box", "starts", "polished", "beta"}
    lower, upper = info["box"]
    assert np.all(best >= lower) and np.all(best <= upper)
    assert info["lml"] >= truth, (info["lml"], truth)
    assert info["lml"] >= float(np.max(info["starts"][1])) - 1e-9 * abs(info["lml"])
    assert abs(ev(best[None, :])[0][0] - info["lml"]) <= 1e-9 * abs(info["lml"])
    # the start values are the evaluator's at the starts (the closed-form amplitude a^2 = Q' / (N - m))
    starts, vals = info["starts"]
    k = int(np.argmax(vals))
    assert abs(ev(starts[k][None, :])[0][0] - vals[k]) <= 1e-9 * abs(vals[k])
    # beta near the generating coefficients: every component within 4 of its own standard deviations,
    # sqrt(diag cov(beta)) at the fitted theta (the GP part of the data has prior sd 2.5 and length scales
    # of a third of the box, so the level is known to about 1.5: the yardstick is the model's own)
    from gpfit.meanfn import predict_mean_closed_form
    bcov = predict_mean_closed_form(x, y, e, H, best, x[:, :1], H[:, :1])[3]
    assert info["beta"].shape == (3,)
    sd_beta = np.sqrt(np.diag(bcov))
    print(f"[meanfn_host] beta - generating {info['beta'] - beta_gen}, sd {sd_beta}")
    assert np.all(np.abs(info["beta"] - beta_gen) < 4.0 * sd_beta), (info["beta"], beta_gen, sd_beta)
    assert np.all(sd_beta < 2.5)  # (and the data do say something about them)
    # the zero-mean fit of the same data explains the level with a larger amplitude
    zero, _ = fit_hyper(x, y, e, num_starts=16, num_polish=2, max_points=N, seed=seed,
                        value_and_grad=hyper_evaluator(x, y, e), verbose=False)
    assert zero[d] > best[d]
    # seeded: the same fit again; full=False pins a = s = 1
    again, _ = fit_mean(x, y, e, kind="linear", num_starts=16, num_polish=2, max_points=N, seed=seed,
                        value_and_grad=numpy_evaluator(), verbose=False)
    np.testing.assert_array_equal(best, again)
    pinned, pinfo = fit_mean(x, y, e, kind="constant", full=False, num_starts=8, num_polish=1, max_points=N, seed=seed,
                             value_and_grad=numpy_evaluator(), verbose=False)
    np.testing.assert_array_equal(pinned[d:], [1.0, 1.0])
    assert pinfo["starts"][0].shape == (8, d + 2) and np.isfinite(pinfo["lml"]) and pinfo["beta"].shape == (1,)
    with pytest.raises(ValueError, match="more than 32"):
        fit_mean(np.zeros((7, 50)), np.zeros(50), np.ones(50), kind="quadratic", value_and_grad=ev)


def _run_gp_fit(tmp_path, monkeypatch, extra, seen):
    import GP_fit
    monkeypatch.chdir(tmp_path)
    (tmp_path / "options.yaml").write_text('file_name: ["a.txt"]\nresolution: [0.1]\n' + extra)
    x = np.linspace(0.0, 1.0, 5)[None, :]

    def fake_hyper(xk, yk, ek, grid, theta):
        seen["predict"] = "GP_hyper"
        return np.linspace(1.0, 2.0, grid.shape[1]), np.full(grid.shape[1], 0.25)

    def fake_mean(xk, yk, ek, grid, theta, kind):
        seen["predict"], seen["kind"] = "GP_mean", kind
        return np.linspace(1.0, 2.0, grid.shape[1]), np.full(grid.shape[1], 0.5)

    monkeypatch.setattr(GP_fit, "GP_hyper", fake_hyper)
    monkeypatch.setattr(GP_fit, "GP_mean", fake_mean)
    monkeypatch.setattr(GP_fit, "len_scale_opt", lambda *a, **k: pytest.fail("len_scale_opt ran"))
    monkeypatch.setattr(GP_fit, "GP", lambda *a, **k: pytest.fail("GP ran"))
    monkeypatch.setattr(GP_fit, "read_yaml", lambda: ([0.1], False, str(tmp_path / "out.txt"), ["x", "q", "err"],
                                                      [("a.txt", [x], [(x[0], np.ones(5))], None)], False, False))
    monkeypatch.setattr(GP_fit, "fill_convex_hull", lambda pts, res: pts)
    GP_fit.create_GP()
    return (tmp_path / "out.txt").read_bytes()


def test_options_yaml_key(tmp_path, monkeypatch):
    """mean_function: linear with marginal_likelihood_full fits with fit_mean and predicts with GP_mean;
    without the key the run is the one before (fit_hyper, GP_hyper, the same bytes written); with any
    other objective the key is a ValueError that says so."""
    import GP_fit
    import gpfit.amplitude
    import gpfit.meanfn
    seen = {}

    def fake_hyper_fit(x, y, e, **kw):
        seen["fit"], seen["fit_kw"] = "fit_hyper", kw
        return np.array([0.5, 2.0, 1.5]), {}

    def fake_mean_fit(x, y, e, **kw):
        seen["fit"], seen["fit_kw"] = "fit_mean", kw
        return np.array([0.5, 2.0, 1.5]), {"beta": np.zeros(2)}

    monkeypatch.setattr(gpfit.amplitude, "fit_hyper", fake_hyper_fit)
    monkeypatch.setattr(gpfit.meanfn, "fit_mean", fake_mean_fit)
    base = "len_scale_objective: marginal_likelihood_full\nmle_num_starts: 24\npso_seed: 3\npso_max_points: 80\n"
    without = _run_gp_fit(tmp_path, monkeypatch, base, seen)
    assert seen == {"fit": "fit_hyper", "fit_kw": {"num_starts": 24, "seed": 3, "max_points": 80, "verbose": False},
                    "predict": "GP_hyper"}
    assert GP_fit._mean_function() is None
    assert GP_fit._pso_overrides() == {"objective": "marginal_likelihood_full", "num_starts": 24, "seed": 3,
                                       "max_points": 80}
    # byte-identical to what the same run wrote before the key existed: the frame GP_hyper's values give
    import pandas as pd
    want = pd.DataFrame({"x": np.linspace(0.0, 1.0, 5), "a": np.linspace(1.0, 2.0, 5), "a_unc": np.full(5, 0.25)})
    assert without == want.to_csv(index=False).encode()
    seen.clear()
    with_key = _run_gp_fit(tmp_path, monkeypatch, base + "mean_function: linear\n", seen)
    assert seen == {"fit": "fit_mean", "fit_kw": {"kind": "linear", "num_starts": 24, "seed": 3, "max_points": 80,
                                                  "verbose": False}, "predict": "GP_mean", "kind": "linear"}
    assert with_key != without
    for objective in ("", "len_scale_objective: marginal_likelihood\n", "len_scale_objective: loo\n",
                      "len_scale_objective: calibration\n"):
        with pytest.raises(ValueError, match="valid only with len_scale_objective: marginal_likelihood_full"):
            _run_gp_fit(tmp_path, monkeypatch, objective + "mean_function: constant\n", seen)
    with pytest.raises(ValueError, match="constant, linear or quadratic"):
        _run_gp_fit(tmp_path, monkeypatch, base + "mean_function: cubic\n", seen)


def test_gp_mean_is_in_the_drop_in_surface():
    import GP_func
    assert "GP_mean" in GP_func.__all__
    with pytest.raises(ValueError, match="x_fit must be"):
        GP_func.GP_mean(np.zeros((2, 3)), np.zeros(3), np.ones(3), np.zeros((1, 4)), np.ones(4))
    from gpfit.meanfn import predict_mean
    with pytest.raises(ValueError, match="theta must be"):
        predict_mean(np.zeros((2, 3)), np.zeros(3), np.ones(3), np.zeros((2, 4)), np.ones(3))


def _bare_context(N, d, m):
    """A Context whose library handle is never touched: the shape checks must raise before it is."""
    from gpfit._lib import Context

    class NoLibrary:
        def __getattr__(self, name):
            raise AssertionError(f"the library was called ({name})")

    c = Context.__new__(Context)
    c.lib, c._h, c.N, c.d, c.m = NoLibrary(), None, N, d, m
    return c


def test_binding_argument_checks_do_not_touch_a_device():
    c = _bare_context(50, 2, 0)
    rng = np.random.default_rng(0)
    H = rng.standard_normal((3, 50))
    for bad, msg in ((H[:, :49], r"H must be \(m, 50\)"), (rng.standard_normal((33, 50)), "1 to 32 rows"),
                     (np.empty((0, 50)), "1 to 32 rows"), (np.vstack([H, H[:1] + H[1:2]]), "rank-deficient"),
                     (np.where(np.arange(50) == 3, np.nan, H), "finite")):
        with pytest.raises(ValueError, match=msg):
            c.set_basis(bad)
    with pytest.raises(ValueError, match="fewer rows than there are points"):
        _bare_context(3, 2, 0).set_basis(rng.standard_normal((3, 3)))
    with pytest.raises(ValueError, match="set_data first"):
        _bare_context(0, 0, 0).set_basis(H)
    with pytest.raises(ValueError, match="no basis for this data"):
        c.lml_mean_batch(np.ones((2, 4)))
    with pytest.raises(ValueError, match="no basis for this data"):
        c.predict_mean(np.ones(2), np.zeros((2, 5)), np.zeros((3, 5)))
    c = _bare_context(50, 2, 3)
    with pytest.raises(ValueError, match=r"theta must be \(P, 4\)"):
        c.lml_mean_batch(np.ones((2, 3)))
    with pytest.raises(ValueError, match=r"x_fit must be \(2, M\)"):
        c.predict_mean(np.ones(2), np.zeros((3, 5)), np.zeros((3, 5)))
    with pytest.raises(ValueError, match=r"h_fit must be \(3, 5\)"):
        c.predict_mean(np.ones(2), np.zeros((2, 5)), np.zeros((2, 5)))
    with pytest.raises(ValueError, match="h_fit must be finite"):
        c.predict_mean(np.ones(2), np.zeros((2, 5)), np.full((3, 5), np.inf))


def test_c_entry_points_without_a_device():
    """The three new symbols are exported with the header's signatures, and a null context is GPF_BAD_ARG
    before anything touches a device."""
    import gpfit
    from gpfit import _lib
    dp, ip, vp = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int), ctypes.c_void_p
    assert _lib.SIGNATURES["gpf_set_basis"] == (ctypes.c_int, [vp, dp, ctypes.c_int])
    assert _lib.SIGNATURES["gpf_lml_mean_batch"] == (ctypes.c_int, [vp, dp, ctypes.c_int, dp, dp, dp, dp, ip, ip])
    assert _lib.SIGNATURES["gpf_predict_mean"] == (ctypes.c_int, [vp, dp, dp, dp, ctypes.c_int64, ctypes.c_int64,
                                                                  dp, dp, dp, dp])
    lib = gpfit.load_library()
    th, out = np.array([[0.3, 1.0, 1.0]]), np.zeros(1)
    bad = ctypes.c_int(7)
    assert lib.gpf_set_basis(None, out.ctypes.data_as(dp), 1) == _lib.GPF_BAD_ARG
    assert lib.gpf_lml_mean_batch(None, th.ctypes.data_as(dp), 1, out.ctypes.data_as(dp), None, None, None, None,
                                  ctypes.byref(bad)) == _lib.GPF_BAD_ARG
    assert lib.gpf_predict_mean(None, th.ctypes.data_as(dp), out.ctypes.data_as(dp), out.ctypes.data_as(dp), 1, 1,
                                out.ctypes.data_as(dp), out.ctypes.data_as(dp), None, None) == _lib.GPF_BAD_ARG
    assert lib.gpf_version() == _lib.ABI_VERSION == 2
    assert {"fit_mean", "predict_mean", "basis", "mean_closed_form", "predict_mean_closed_form"} <= set(dir(gpfit.meanfn))
