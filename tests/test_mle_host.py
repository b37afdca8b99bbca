"""The maximum-marginal-likelihood driver (gpfit.mle.fit_lml) and its drop-in surface, without a GPU:
the fit runs on an injected NumPy evaluator, the closed form the GPU tests compare gpf_lml_batch
against (tests/test_lml_grad_gpu.py imports it from here).
"""
import numpy as np
import pytest


def se_kernel(x, l):
    """kernel_func(x, x, l) (GP_func.py:49-65): noise-free ARD squared-exponential, x (d, N)."""
    a = x / np.asarray(l, dtype=np.float64)[:, None]
    n = np.sum(a ** 2, axis=0)
    r2 = np.maximum(n[:, None] + n[None, :] - 2.0 * (a.T @ a), 0.0)
    return np.exp(-0.5 * r2)


def lml_closed_form(x, y, e, l):
    """(LML, dLML/dl) in float64 NumPy, fixed amplitude 1 and noise e^2:
    LML = -1/2 y^T alpha - sum log L_ii - N/2 log(2 pi), W = Kn^-1 (np.linalg.inv), L = chol(Kn),
    dLML/dl_k = 1/2 sum_ij (alpha_i alpha_j - W_ij) K_ij (x_ik - x_jk)^2 / l_k^3."""
    l = np.asarray(l, dtype=np.float64).reshape(-1)
    K = se_kernel(x, l)
    Kn = K + np.diag(e ** 2)
    L = np.linalg.cholesky(Kn)
    W = np.linalg.inv(Kn)
    al = W @ y
    lml = -0.5 * (y @ al) - np.sum(np.log(np.diag(L))) - 0.5 * len(y) * np.log(2.0 * np.pi)
    M = (np.outer(al, al) - W) * K
    g = np.array([0.5 * np.sum(M * (x[k][:, None] - x[k][None, :]) ** 2) / l[k] ** 3 for k in range(len(l))])
    return lml, g


def numpy_evaluator(x, y, e):
    """value_and_grad for fit_lml; a non-positive-definite point is -inf / NaN, as gpf_lml_batch's."""
    def value_and_grad(positions):
        out, grads = [], []
        for p in np.atleast_2d(positions):
            try:
                v, g = lml_closed_form(x, y, e, p)
            except np.linalg.LinAlgError:
                v, g = -np.inf, np.full(x.shape[0], np.nan)
            out.append(v)
            grads.append(g)
        return np.array(out), np.array(grads)
    return value_and_grad


# (seed, d, N, l_true): tests/test_lml_grad_gpu.py runs the first on the GPU
FIT_RECIPES = [(0, 2, 150, (0.3, 0.6)), (1, 3, 200, (0.25, 0.5, 0.9)), (2, 1, 100, (0.2,))]


def gp_sample(seed, d, N, l_true):
    """y = chol(K + 1e-10 I) randn + e randn at x ~ U(0,1)^d, e ~ U(0.05, 0.2), default_rng(seed)."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(size=(d, N))
    e = rng.uniform(0.05, 0.2, size=N)
    K = se_kernel(x, np.array(l_true))
    f = np.linalg.cholesky(K + 1e-10 * np.eye(N)) @ rng.standard_normal(N)
    y = f + e * rng.standard_normal(N)
    return x, y, e


def check_fit(best, info, truth_lml):
    lower, upper = info["box"]
    assert np.all(best >= lower) and np.all(best <= upper), (best, lower, upper)
    best_start = float(np.max(info["starts"][1]))
    assert info["lml"] >= truth_lml, (info["lml"], truth_lml)
    assert info["lml"] >= best_start, (info["lml"], best_start)
    assert info["evals"] >= info["starts"][0].shape[0] + info["grad_evals"] > 0


@pytest.mark.parametrize("seed,d,N,l_true", FIT_RECIPES)
def test_fit_lml_with_numpy_evaluator(seed, d, N, l_true):
    from gpfit.mle import fit_lml
    x, y, e = gp_sample(seed, d, N, l_true)
    ev = numpy_evaluator(x, y, e)
    best, info = fit_lml(x, y, e, num_starts=16, num_polish=1, max_points=N, seed=seed, value_and_grad=ev,
                         verbose=False)
    truth = lml_closed_form(x, y, e, l_true)[0]
    check_fit(best, info, truth)
    # the reported value is the evaluator's at the returned point
    assert abs(ev(best[None, :])[0][0] - info["lml"]) <= 1e-9 * abs(info["lml"])
    # seeded: the same fit again
    again, info2 = fit_lml(x, y, e, num_starts=16, num_polish=1, max_points=N, seed=seed, value_and_grad=ev,
                           verbose=False)
    np.testing.assert_array_equal(best, again)
    assert len(info["polished"]) == 1 and info2["evals"] == info["evals"]


def test_fit_lml_recorded_values():
    """The figures the GPU end-to-end case was specified with (seed 0, d = 2, N = 150): fit 73.44,
    truth 72.06, best start 68.32."""
    from gpfit.mle import fit_lml
    seed, d, N, l_true = FIT_RECIPES[0]
    x, y, e = gp_sample(seed, d, N, l_true)
    best, info = fit_lml(x, y, e, num_starts=16, num_polish=1, max_points=N, seed=seed,
                         value_and_grad=numpy_evaluator(x, y, e), verbose=False)
    assert abs(info["lml"] - 73.44) < 0.01
    assert abs(lml_closed_form(x, y, e, l_true)[0] - 72.06) < 0.01
    assert abs(np.max(info["starts"][1]) - 68.32) < 0.01


def test_closed_form_gradient_is_the_derivative():
    x, y, e = gp_sample(3, 2, 60, (0.4, 0.7))
    l = np.array([0.35, 0.55])
    _, g = lml_closed_form(x, y, e, l)
    for k in range(2):
        h = np.zeros(2)
        h[k] = 1e-5
        fd = (lml_closed_form(x, y, e, l + h)[0] - lml_closed_form(x, y, e, l - h)[0]) / 2e-5
        assert abs(fd - g[k]) <= 1e-6 * max(1.0, abs(g[k])), (k, fd, g[k])


def test_fit_lml_survives_non_pd_region():
    """An evaluator that reports non-PD (-inf, NaN gradient) above some l: a losing point for the
    starts and for the line search, never an error; the fit stays in the good region."""
    from gpfit.mle import fit_lml
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

    best, info = fit_lml(x, y, e, num_starts=16, num_polish=3, max_points=N, seed=seed, value_and_grad=ev,
                         verbose=False)
    assert calls["bad"] > 0
    assert np.all(best <= 0.45) and np.isfinite(info["lml"])
    assert info["lml"] >= np.max(info["starts"][1])
    # every start losing: still no error, the value says so
    best2, info2 = fit_lml(x, y, e, num_starts=4, num_polish=2, max_points=N, seed=seed,
                           value_and_grad=lambda p: (np.full(len(p), -np.inf), np.full(p.shape, np.nan)),
                           verbose=False)
    assert info2["lml"] == -np.inf and best2.shape == (d,)


def test_fit_lml_box_lower_bound_is_positive():
    """The reference's lower bound is the smallest positive gap between coordinates and can be 0
    (a constant coordinate has none): the fit's box starts at max(lower, 1e-3 upper)."""
    from gpfit.mle import fit_lml
    from gpfit.swarm import search_bounds
    x, y, e = gp_sample(4, 2, 40, (0.3, 0.6))
    x[1, :20] = np.round(x[1, :20], 1)  # repeated values: tiny or zero gaps are not the issue here
    lo, hi = search_bounds(x)
    _, info = fit_lml(x, y, e, num_starts=4, num_polish=1, max_points=40, seed=0,
                      value_and_grad=numpy_evaluator(x, y, e), verbose=False)
    lower, upper = info["box"]
    np.testing.assert_array_equal(upper, hi)
    np.testing.assert_array_equal(lower, np.maximum(lo, 1e-3 * hi))
    assert np.all(lower > 0)


def test_len_scale_opt_objective_dispatch(monkeypatch):
    import find_len_scales as fls
    import gpfit.mle
    seen = {}

    def fake_fit(x, y, e, **kw):
        seen["fit"] = kw
        return np.array([0.5]), {}

    def fake_swarm(x, y, e, progress, **kw):
        seen["swarm"] = kw
        return np.array([0.25]), {}

    monkeypatch.setattr(gpfit.mle, "fit_lml", fake_fit)
    monkeypatch.setattr(fls, "particle_swarm", fake_swarm)
    x, y, e = np.zeros((1, 3)), np.zeros(3), np.ones(3)
    assert fls.len_scale_opt(x, y, e, False)[0] == 0.25
    # the default objective reaches the swarm with exactly the arguments it always got
    assert seen["swarm"] == {"num_particles": 40, "max_iter": 500, "max_points": 100, "init_positions": None,
                             "seed": None}
    assert "fit" not in seen
    assert fls.len_scale_opt(x, y, e, False, objective="calibration", seed=4)[0] == 0.25
    assert seen["swarm"]["seed"] == 4 and "fit" not in seen
    assert fls.len_scale_opt(x, y, e, False, objective="marginal_likelihood", num_starts=12, max_points=50,
                             seed=7)[0] == 0.5
    assert seen["fit"] == {"num_starts": 12, "max_points": 50, "seed": 7, "verbose": False}
    with pytest.raises(ValueError, match="unknown objective"):
        fls.len_scale_opt(x, y, e, False, objective="likelihood")


@pytest.mark.parametrize("extra,want", [
    ("", {}),
    ("pso_seed: 3\npso_max_points: 80\n", {"seed": 3, "max_points": 80}),
    ("len_scale_objective: marginal_likelihood\nmle_num_starts: 24\npso_seed: 3\npso_max_points: 80\n",
     {"objective": "marginal_likelihood", "num_starts": 24, "seed": 3, "max_points": 80}),
    ("len_scale_objective: calibration\n", {"objective": "calibration"}),
])
def test_options_yaml_keys_reach_len_scale_opt(tmp_path, monkeypatch, extra, want):
    import GP_fit
    monkeypatch.chdir(tmp_path)
    (tmp_path / "options.yaml").write_text('file_name: ["a.txt"]\nresolution: [0.1]\n' + extra)
    seen = []

    def fake_opt(x, y, e, progress, **kw):
        seen.append(kw)
        return np.array([0.5])

    x = np.linspace(0.0, 1.0, 5)[None, :]
    monkeypatch.setattr(GP_fit, "len_scale_opt", fake_opt)
    monkeypatch.setattr(GP_fit, "read_yaml", lambda: ([0.1], False, str(tmp_path / "out.txt"), ["x", "q", "err"],
                                                      [("a.txt", [x], [(x[0], np.ones(5))], None)], False, False))
    monkeypatch.setattr(GP_fit, "fill_convex_hull", lambda pts, res: pts)
    monkeypatch.setattr(GP_fit, "GP", lambda xk, yk, ek, grid, ls: (np.zeros(grid.shape[1]), np.ones(grid.shape[1])))
    GP_fit.create_GP()
    assert seen == [want]
