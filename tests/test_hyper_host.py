"""Host side of the length-scale marginalisation (gpfit.hyper: mixture_from, sample_hyper with an
injected evaluator, argument checks), the options.yaml key and the binding of gpf_predict_batch. No
GPU needed."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent


def _components(p, m, seed=0):
    rng = np.random.default_rng(seed)
    return rng.normal(size=(p, m)), rng.uniform(0.05, 1.5, size=(p, m)), rng.uniform(0.1, 2.0, size=p)


# ---- mixture_from ----

def test_mixture_of_one_returns_its_input():
    from gpfit.hyper import mixture_from
    mu, sd, _ = _components(1, 9)
    mix_mu, mix_sd = mixture_from(mu, sd)
    np.testing.assert_array_equal(mix_mu, mu[0])
    np.testing.assert_allclose(mix_sd, sd[0], rtol=2e-16, atol=0.0)   # sqrt(sd * sd): one rounding each way
    mix_mu, mix_sd = mixture_from(mu, sd, [3.0])
    np.testing.assert_array_equal(mix_mu, mu[0])


def test_mixture_of_identical_components_is_the_component():
    from gpfit.hyper import mixture_from
    mu, sd, w = _components(1, 9, seed=1)
    mix_mu, mix_sd = mixture_from(np.repeat(mu, 4, axis=0), np.repeat(sd, 4, axis=0), [0.5, 0.25, 0.125, 0.125])
    np.testing.assert_allclose(mix_mu, mu[0], rtol=1e-15, atol=0.0)
    np.testing.assert_allclose(mix_sd, sd[0], rtol=1e-15, atol=0.0)


def test_mixture_against_longdouble():
    from gpfit.hyper import mixture_from
    mu, sd, w = _components(7, 33, seed=2)
    w[3] = 0.0
    mix_mu, mix_sd = mixture_from(mu, sd, w)
    lw = (w.astype(np.longdouble) / np.sum(w.astype(np.longdouble)))[:, None]
    lmu, lsd = mu.astype(np.longdouble), sd.astype(np.longdouble)
    ref_mu = np.sum(lw * lmu, axis=0)
    ref_sd = np.sqrt(np.sum(lw * (lsd * lsd + (lmu - ref_mu[None, :]) ** 2), axis=0))
    assert np.max(np.abs(mix_mu - ref_mu)) < 1e-13
    assert np.max(np.abs(mix_sd - ref_sd)) < 1e-13
    # the law of total variance: never below the mean within-component variance
    assert np.all(mix_sd ** 2 >= np.sum(np.asarray(lw, dtype=np.float64) * sd ** 2, axis=0) - 1e-13)


def test_mixture_argument_errors():
    from gpfit.hyper import mixture_from
    mu, sd, _ = _components(3, 5)
    with pytest.raises(ValueError):
        mixture_from(mu, sd, [1.0, -1.0, 1.0])
    with pytest.raises(ValueError):
        mixture_from(mu, sd, [0.0, 0.0, 0.0])
    with pytest.raises(ValueError):
        mixture_from(mu, sd, [1.0, 1.0])
    with pytest.raises(ValueError):
        mixture_from(mu, sd, [1.0, np.inf, 1.0])
    with pytest.raises(ValueError):
        mixture_from(mu, sd[:2])
    with pytest.raises(ValueError):
        mixture_from(mu[0], sd[0])


# ---- sample_hyper with an injected evaluator ----

H_TRUE = np.array([[40.0, 12.0], [12.0, 25.0]])


def _data(n=30, d=2, seed=3):
    rng = np.random.default_rng(seed)
    x = rng.uniform(size=(d, n))
    return x, np.sin(3 * x[0]), np.full(n, 0.1)


def _quadratic(t_star, calls=None):
    """An exact quadratic log-density in t = log l: F = -1/2 (t - t*)^T H (t - t*); the evaluator returns
    the gradient in l, dF/dl = (dF/dt) / l, as gpf_lml_batch does."""
    def value_and_grad(positions):
        if calls is not None:
            calls.append(positions.shape[0])
        dt = np.log(positions) - t_star[None, :]
        return -0.5 * np.einsum("ki,ij,kj->k", dt, H_TRUE, dt), -(dt @ H_TRUE) / positions
    return value_and_grad


def _box_centre(x):
    from gpfit.mle import LOWER_FRACTION
    from gpfit.swarm import search_bounds
    lower, upper = search_bounds(x)
    lower = np.maximum(lower, LOWER_FRACTION * upper)
    return lower, upper, 0.5 * (np.log(lower) + np.log(upper))


def test_sample_hyper_recovers_the_hessian_of_a_quadratic():
    """Central differences are exact on a quadratic, so only the rounding of the gradients remains:
    |H - H_true| < 100 eps max|g| / h with g the gradients (in t) at the 2d difference points. The
    quadratic is centred away from best_l, where the gradient is of order |H| and its rounding is what
    limits the difference quotient (at the centre itself g is of order |H| h, and the rounding of
    t = log(exp(t)) inside any evaluator that takes l, about eps |t| |H| / h, would exceed the formula)."""
    from gpfit.hyper import HESSIAN_STEP, sample_hyper
    x, y, e = _data()
    lower, upper, t_star = _box_centre(x)
    centre = t_star + np.array([0.7, -0.4])
    quad, calls, gmax = _quadratic(centre), [], []

    def evaluator(positions):
        calls.append(positions.shape[0])
        lml, g = quad(positions)
        if len(calls) == 1:
            gmax.append(np.max(np.abs(g * positions)))
        return lml, g

    ls, w, info = sample_hyper(x, y, e, best_l=np.exp(t_star), n_samples=16, seed=4, value_and_grad=evaluator)
    err = np.max(np.abs(info["hessian"] - H_TRUE))
    bound = 100 * np.finfo(float).eps * gmax[0] / HESSIAN_STEP
    print(f"[hyper] Hessian of a quadratic: max error {err:.3e}, bound {bound:.3e} (max|g| {gmax[0]:.3e})")
    assert err < bound, (err, bound)
    np.testing.assert_array_equal(info["hessian"], info["hessian"].T)
    assert calls == [4, 16], "the 2d difference points in one batched call, the K proposals in another"
    assert info["evals"] == 20
    np.testing.assert_allclose(info["cov"], 1.5 ** 2 * np.linalg.inv(H_TRUE), rtol=1e-6)
    assert ls.shape == (16, 2) and w.shape == (16,)
    assert abs(np.sum(w) - 1.0) < 1e-12 and np.all(w >= 0.0)
    assert 1.0 <= info["ess"] <= 16.0
    np.testing.assert_array_equal(info["best_l"], np.exp(t_star))


def test_uninflated_proposal_of_a_quadratic_has_uniform_weights():
    from gpfit.hyper import sample_hyper
    x, y, e = _data()
    _, _, t_star = _box_centre(x)
    ls, w, info = sample_hyper(x, y, e, best_l=np.exp(t_star), n_samples=24, inflate=1.0, seed=5,
                               value_and_grad=_quadratic(t_star))
    assert np.max(np.abs(w * 24 - 1.0)) < 1e-6
    assert info["ess"] == pytest.approx(24.0, rel=1e-6)


def test_same_seed_same_samples_inside_the_box():
    from gpfit.hyper import sample_hyper
    x, y, e = _data()
    lower, upper, t_star = _box_centre(x)
    # a centre near the box's corner: many proposals fall outside and are redrawn
    t_corner = np.log(upper) - 0.05
    a = sample_hyper(x, y, e, best_l=np.exp(t_corner), n_samples=64, seed=6, value_and_grad=_quadratic(t_corner))
    b = sample_hyper(x, y, e, best_l=np.exp(t_corner), n_samples=64, seed=6, value_and_grad=_quadratic(t_corner))
    c = sample_hyper(x, y, e, best_l=np.exp(t_corner), n_samples=64, seed=7, value_and_grad=_quadratic(t_corner))
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])
    assert not np.array_equal(a[0], c[0])
    for ls in (a[0], c[0]):
        assert np.all(ls >= lower) and np.all(ls <= upper)


def test_flat_direction_gets_the_box_wide_proposal():
    """A log-density that ignores every length scale: the Hessian is 0, its eigenvalues are floored so
    that the proposal's standard deviation is the box's smallest width, and the weights stay finite."""
    from gpfit.hyper import sample_hyper
    x, y, e = _data()
    lower, upper, t_star = _box_centre(x)

    def flat(positions):
        return np.zeros(positions.shape[0]), np.zeros_like(positions)

    ls, w, info = sample_hyper(x, y, e, best_l=np.exp(t_star), n_samples=32, inflate=1.0, seed=8, value_and_grad=flat)
    width = np.min(np.log(upper) - np.log(lower))
    np.testing.assert_allclose(info["cov"], width ** 2 * np.eye(2), rtol=1e-12)
    assert np.all(np.isfinite(w)) and abs(np.sum(w) - 1.0) < 1e-12


def _lml_closed_form(x, y, e):
    """NumPy closed-form LML and its gradient in l (d = 1), a non-positive-definite point as -inf / NaN."""
    def value_and_grad(positions):
        lml, grad = np.empty(positions.shape[0]), np.empty_like(positions)
        d2 = (x[0][:, None] - x[0][None, :]) ** 2
        for i, (l,) in enumerate(positions):
            K = np.exp(-0.5 * d2 / l ** 2)
            try:
                L = np.linalg.cholesky(K + np.diag(e ** 2))
            except np.linalg.LinAlgError:
                lml[i], grad[i] = -np.inf, np.nan
                continue
            alpha = np.linalg.solve(L.T, np.linalg.solve(L, y))
            W = np.linalg.solve(L.T, np.linalg.solve(L, np.eye(len(y))))
            lml[i] = -0.5 * y @ alpha - np.sum(np.log(np.diag(L))) - 0.5 * len(y) * np.log(2 * np.pi)
            grad[i, 0] = 0.5 * np.sum((np.outer(alpha, alpha) - W) * K * d2 / l ** 3)
        return lml, grad
    return value_and_grad


def test_sample_hyper_on_a_real_marginal_likelihood():
    from gpfit.hyper import sample_hyper
    rng = np.random.default_rng(9)
    x = np.sort(rng.uniform(size=(1, 40)), axis=1)
    y = np.sin(5 * x[0]) + 0.1 * rng.standard_normal(40)
    e = np.full(40, 0.1)
    ls, w, info = sample_hyper(x, y, e, n_samples=12, seed=10, value_and_grad=_lml_closed_form(x, y, e))
    assert ls.shape == (12, 1) and np.all(ls > 0.0)
    assert np.all(np.isfinite(w)) and np.all(w >= 0.0) and abs(np.sum(w) - 1.0) < 1e-12
    assert 1.0 <= info["ess"] <= 12.0
    assert info["hessian"][0, 0] > 0.0, "fit_lml's optimum is a maximum of the LML"
    assert info["evals"] > 14   # fit_lml's evaluations, the 2 difference points and the 12 proposals
    lo, hi = info["box"]
    assert np.all(ls >= lo) and np.all(ls <= hi)


def test_non_pd_samples_get_weight_zero():
    from gpfit.hyper import sample_hyper
    x, y, e = _data()
    _, _, t_star = _box_centre(x)
    quad = _quadratic(t_star)

    def evaluator(positions):
        lml, g = quad(positions)
        if positions.shape[0] == 10:
            lml = lml.copy()
            lml[[2, 7]] = -np.inf
        return lml, g

    ls, w, info = sample_hyper(x, y, e, best_l=np.exp(t_star), n_samples=10, seed=11, value_and_grad=evaluator)
    assert w[2] == 0.0 and w[7] == 0.0 and abs(np.sum(w) - 1.0) < 1e-12
    assert np.all(np.isfinite(w))


def test_sample_hyper_argument_errors():
    from gpfit.hyper import sample_hyper
    x, y, e = _data()
    _, _, t_star = _box_centre(x)
    q = _quadratic(t_star)
    with pytest.raises(ValueError):
        sample_hyper(x, y, e, best_l=np.exp(t_star), n_samples=0, value_and_grad=q)
    with pytest.raises(ValueError):
        sample_hyper(x, y, e, best_l=np.exp(t_star), inflate=0.0, value_and_grad=q)
    with pytest.raises(ValueError):
        sample_hyper(x, y, e, best_l=[0.5], value_and_grad=q)
    with pytest.raises(ValueError):
        sample_hyper(x, y, e, best_l=[0.5, -0.5], value_and_grad=q)


def test_predict_marginal_argument_errors():
    """Everything predict_marginal rejects is rejected before a device is touched."""
    from gpfit.hyper import predict_marginal
    x, y, e = _data(n=6)
    q = np.zeros((2, 4))
    ls = np.full((3, 2), 0.3)
    with pytest.raises(ValueError):
        predict_marginal(x, y, e, q, ls=ls, method="serial")
    with pytest.raises(ValueError):
        predict_marginal(x, y, e, np.zeros((3, 4)), ls=ls)
    with pytest.raises(ValueError):
        predict_marginal(x, y, e, q, ls=np.full((3, 1), 0.3))
    with pytest.raises(ValueError):
        predict_marginal(x, y, e, q, ls=-ls)
    with pytest.raises(ValueError):
        predict_marginal(x, y, e, q, ls=ls, weights=[1.0, -1.0, 1.0])
    with pytest.raises(ValueError):
        predict_marginal(x, y, e, q, ls=ls, weights=[0.0, 0.0, 0.0])
    with pytest.raises(ValueError):
        predict_marginal(x, y, e, q, ls=ls, weights=[1.0, 1.0])
    with pytest.raises(ValueError):
        predict_marginal(x, y, e, q, ls=ls, chunk=-1)
    with pytest.raises(ValueError):
        predict_marginal(x, y, e, q, ls=ls, n_samples=4)
    with pytest.raises(ValueError):
        predict_marginal(x, y, e, q, weights=[1.0])


# ---- options.yaml ----

@pytest.mark.parametrize("extra,want", [("", None), ("pso_seed: 3\n", None), ("hyper_samples: 16\n", 16)])
def test_options_yaml_hyper_samples_selects_the_path(tmp_path, monkeypatch, extra, want):
    """Without the key create_GP predicts with GP() exactly as before; with it, through the marginal route."""
    import GP_fit
    monkeypatch.chdir(tmp_path)
    (tmp_path / "options.yaml").write_text('file_name: ["a.txt"]\nresolution: [0.1]\n' + extra)
    assert GP_fit._hyper_samples() == want
    assert "hyper_samples" not in GP_fit._pso_overrides()
    seen = {"opt": [], "gp": 0, "marginal": []}

    def fake_opt(xk, yk, ek, progress, **kw):
        seen["opt"].append(kw)
        return np.array([0.5])

    def fake_gp(xk, yk, ek, grid, ls):
        seen["gp"] += 1
        return np.zeros(grid.shape[1]), np.ones(grid.shape[1])

    def fake_marginal(xk, yk, ek, grid, ls, k, pso):
        seen["marginal"].append((k, dict(pso)))
        return np.zeros(grid.shape[1]), np.full(grid.shape[1], 2.0)

    x = np.linspace(0.0, 1.0, 5)[None, :]
    monkeypatch.setattr(GP_fit, "len_scale_opt", fake_opt)
    monkeypatch.setattr(GP_fit, "read_yaml", lambda: ([0.1], False, str(tmp_path / "out.txt"), ["x", "q", "err"],
                                                      [("a.txt", [x], [(x[0], np.ones(5))], None)], False, False))
    monkeypatch.setattr(GP_fit, "fill_convex_hull", lambda pts, res: pts)
    monkeypatch.setattr(GP_fit, "GP", fake_gp)
    monkeypatch.setattr(GP_fit, "_marginal", fake_marginal)
    merged, _ = GP_fit.create_GP()
    assert all("hyper_samples" not in kw for kw in seen["opt"]), "the key must not reach len_scale_opt"
    if want is None:
        assert seen["gp"] == 1 and seen["marginal"] == []
        assert list(merged["a_unc"]) == [1.0] * 5
    else:
        assert seen["gp"] == 0 and [k for k, _ in seen["marginal"]] == [want]
        assert list(merged["a_unc"]) == [2.0] * 5


@pytest.mark.parametrize("bad", ["0", "-3", "2.5", "true", '"many"'])
def test_options_yaml_hyper_samples_must_be_a_positive_integer(tmp_path, bad):
    import GP_fit
    (tmp_path / "options.yaml").write_text(f"hyper_samples: {bad}\n")
    with pytest.raises(ValueError):
        GP_fit._hyper_samples(tmp_path / "options.yaml")


def test_gp_fit_docstring_lists_the_key():
    import GP_fit
    assert "hyper_samples" in GP_fit.__doc__


# ---- binding ----

def test_predict_batch_is_declared_and_bound():
    import gpfit._lib as L
    header = (ROOT / "include" / "gpfit.h").read_text()
    assert re.search(r"\bint\s+gpf_predict_batch\s*\(", header)
    assert "gpf_predict_batch" in L.SIGNATURES
    res, args = L.SIGNATURES["gpf_predict_batch"]
    assert res is ctypes.c_int and len(args) == 12
    assert callable(L.Context.predict_batch)
    import GP_func
    assert callable(GP_func.GP_marginal)


def test_memory_plan_of_predict_batch():
    """gpf_predict_batch's planner on given byte counts (the library's own function, host only)."""
    from gpfit._lib import predict_batch_plan
    per, col = 268e6, (4096 + 2 * 32 + 3) * 8.0      # N=4096: a particle's workspace, a particle's query column
    keep = 2048 * 1048576.0
    # roomy device: every particle in one chunk; chunk=0 stays within the kept-buffer limit, an explicit chunk is taken
    plan = predict_batch_plan(250e9, 0.0, 0, per, col, 1e6, 64, 10112)
    assert plan == {"pc": 64, "cq": 896, "regrow": False}
    assert 1e6 + 64 * col * plan["cq"] <= keep < 1e6 + 64 * col * (plan["cq"] + 128)
    assert predict_batch_plan(250e9, 0.0, 0, per, col, 1e6, 64, 10112, chunk=16384) == {"pc": 64, "cq": 10112, "regrow": False}
    assert predict_batch_plan(250e9, 0.0, 0, per, col, 1e6, 64, 10112, chunk=1000)["cq"] == 1024
    # fewer slots held than wanted: ensure_work regrows by itself, nothing to give back
    assert predict_batch_plan(250e9, 0.0, 2, per, col, 1e6, 8, 1024) == {"pc": 8, "cq": 1024, "regrow": False}
    # the buffers do not fit half of the memory at the full chunk: the query chunk is halved first
    plan = predict_batch_plan(64 * per / 0.85 + 3e9, 0.0, 0, per, col, 1e6, 64, 10112, chunk=16384)
    assert plan["pc"] == 64 and plan["cq"] < 10112 and 1e6 + 64 * col * plan["cq"] <= 0.5 * (64 * per / 0.85 + 3e9 - 64 * per)
    # an earlier batch left a workspace of 64 slots of 4 GB and 50 MB free: the buffers of 4 particles do not fit
    # beside it, so the workspace is given back and regrown to 4 slots
    big, bcol = 4e9, (16384 + 2 * 128 + 3) * 8.0
    plan = predict_batch_plan(50e6, 0.0, 64, big, bcol, 1e5, 4, 1024)
    assert plan == {"pc": 4, "cq": 1024, "regrow": True}
    # ... and kept when they do fit beside it
    assert predict_batch_plan(5e9, 0.0, 64, big, bcol, 1e5, 4, 1024) == {"pc": 4, "cq": 1024, "regrow": False}
    # the call's own kept buffers count as available
    assert predict_batch_plan(50e6, 5e9, 64, big, bcol, 1e5, 4, 1024)["regrow"] is False
    # one particle at chunk 128 fits nowhere
    with pytest.raises(ValueError):
        predict_batch_plan(1e6, 0.0, 0, 1e9, bcol, 1e5, 4, 1024)
    with pytest.raises(ValueError):
        predict_batch_plan(250e9, 0.0, 0, per, col, 1e6, 0, 1024)


def test_null_context_is_bad_arg_without_a_device():
    import gpfit._lib as L
    lib = L.load_library()
    assert lib.gpf_predict_batch(None, None, 0, None, None, 0, 0, None, None, None, None, None) == L.GPF_BAD_ARG
    assert lib.gpf_predict_batch(None, None, 3, None, None, 5, 0, None, None, None, None, None) == L.GPF_BAD_ARG


def test_no_cpu_fallback_without_device():
    """With no GPU visible the marginal routes raise like every other entry point; with one visible the
    open succeeds and there is nothing to fall back from."""
    import gpfit._lib as L
    lib = L.load_library()
    h = ctypes.c_void_p()
    if lib.gpf_open(0, ctypes.byref(h)) == 0:
        lib.gpf_close(h)
        return
    import GP_func
    from gpfit.hyper import predict_marginal
    x, y, e = _data(n=6)
    with pytest.raises(L.GPFitError):
        predict_marginal(x, y, e, np.zeros((2, 4)), ls=np.full((3, 2), 0.3))
    with pytest.raises(L.GPFitError):
        predict_marginal(x, y, e, np.zeros((2, 4)), ls=np.full((3, 2), 0.3), method="loop")
    with pytest.raises(L.GPFitError):
        GP_func.GP_marginal(x, y, e, np.zeros((2, 4)), np.full((3, 2), 0.3))
