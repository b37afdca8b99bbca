"""gpf_lml_hyper_batch (the log marginal likelihood under Kn = a^2 K(l) + s^2 diag(e^2) and its gradient
in (l, a, s)) against the float64 NumPy closed form of tests/test_amplitude_host.py, which is built
from Kn directly and never forms the unit-amplitude matrix the device factors.

Recipe: tests/test_lml_grad_gpu.py's, then a ~ U(0.5, 3), rho ~ U(0.7, 1.5), s = a rho from the same rng.
Tolerance 1e-9 (the project's LML tolerance): value |got - want| / max(|want|, 1); gradient the largest
component error over the largest reference component, per particle, over all d + 2 components. On this
recipe the float64 closed form is within 2.5e-12 (value) and 9.2e-13 (gradient) of the same formulas in
np.longdouble (N = 129 and 300 at d = 2, N = 200 at d = 3, five particles each), so 1e-9 leaves the
orders of margin the length-scale test has. The measured
maxima are printed (run with -s) and sit in the assert messages.
"""
import numpy as np
import pytest

from test_amplitude_host import hyper_closed_form, scaled_sample, unit_q
from test_lml_grad_gpu import _recipe
from test_mle_host import FIT_RECIPES

pytestmark = pytest.mark.gpu

TOL = 1e-9


@pytest.fixture(scope="module")
def ctx():
    import gpfit
    c = gpfit.Context(0)
    yield c
    c.close()


def _recipe_hyper(N, d, P=5):
    """_recipe's draws in _recipe's order, then a and rho from the same generator: (x, y, e, theta (P, d + 2))."""
    rng = np.random.default_rng(N)
    x = rng.uniform(size=(d, N))
    y = np.sin(3 * x[0]) + (x[1] if d > 1 else 0.0) + 0.1 * rng.standard_normal(N)
    e = rng.uniform(0.05, 0.2, size=N)
    ls = rng.uniform(0.05, 0.8, size=(P, d))
    a = rng.uniform(0.5, 3.0, size=P)
    rho = rng.uniform(0.7, 1.5, size=P)
    x0, y0, e0, ls0 = _recipe(N, d, P)
    assert np.array_equal(x, x0) and np.array_equal(y, y0) and np.array_equal(e, e0) and np.array_equal(ls, ls0)
    return x, y, e, np.column_stack([ls, a, a * rho])


_REF = {}


def _reference(key, x, y, e, theta):
    """The closed form of every particle, computed once per case and shared."""
    if key not in _REF:
        vals, grads = zip(*(hyper_closed_form(x, y, e, p) for p in theta))
        v, g = np.array(vals), np.array(grads)
        v.setflags(write=False)
        g.setflags(write=False)
        _REF[key] = (v, g)
    return _REF[key]


def _errors(lml, grad, want, gwant):
    ev = np.abs(lml - want) / np.maximum(np.abs(want), 1.0)
    scale = np.max(np.abs(gwant), axis=1)
    eg = np.max(np.abs(grad - gwant), axis=1) / np.where(scale > 0, scale, 1.0)
    return ev, eg


def _check(tag, lml, grad, want, gwant, rows=None):
    rows = list(range(len(want)) if rows is None else rows)
    ev, eg = _errors(lml, grad, want, gwant)
    ev, eg = ev[rows], eg[rows]
    print(f"[amplitude] {tag}: max value err {np.max(ev):.3e}, max gradient err {np.max(eg):.3e} (tol {TOL:.0e})")
    assert np.max(ev) < TOL, f"{tag}: value errors {ev}"
    assert np.max(eg) < TOL, f"{tag}: gradient errors {eg}"


@pytest.mark.parametrize("N", [1, 2, 127, 128, 129, 257, 300])
def test_tile_boundaries_vs_closed_form(ctx, N):
    x, y, e, th = _recipe_hyper(N, 2)
    want, gwant = _reference(("tb", N), x, y, e, th)
    ctx.set_data(x, y, e)
    lml, grad, q = ctx.lml_hyper_batch(th, want_q=True)
    assert grad.shape == (5, 4)
    if N == 1:
        np.testing.assert_array_equal(grad[:, :2], np.zeros((5, 2)))
    _check(f"N={N} d=2", lml, grad, want, gwant)
    # Q = y^T Kt^-1 y of the unit-amplitude Kt = K + (s / a)^2 diag(e^2)
    qref = np.array([unit_q(x, y, e, p[:2], p[3] / p[2]) for p in th])
    err = np.max(np.abs(q - qref) / np.maximum(np.abs(qref), 1.0))
    print(f"[amplitude] N={N} d=2: max Q err {err:.3e}")
    assert err < TOL, err


@pytest.mark.parametrize("d", [1, 3, 4])
def test_dimensions_vs_closed_form(ctx, d):
    x, y, e, th = _recipe_hyper(200, d)
    want, gwant = _reference(("dim", d), x, y, e, th)
    ctx.set_data(x, y, e)
    lml, grad = ctx.lml_hyper_batch(th)
    _check(f"N=200 d={d}", lml, grad, want, gwant)


def _case3():
    x, y, e, th = _recipe_hyper(1100, 3, P=6)
    assert len({tuple(p) for p in th}) == 6 and len(set(th[:, 3])) == 6 and len(set(th[:, 4] / th[:, 3])) == 6
    return x, y, e, th, _reference(("big", 1100), x, y, e, th)


def test_nine_block_columns_ragged(ctx):
    x, y, e, th, (want, gwant) = _case3()
    ctx.set_data(x, y, e)
    lml, grad = ctx.lml_hyper_batch(th)
    _check("N=1100 d=3 P=6", lml, grad, want, gwant)


def test_chunked_batch(monkeypatch):
    """6 particles through a workspace capped at 4 per chunk (a fresh context: the cap is read when the
    workspace is sized): the second chunk's particles must get their own noise factors, amplitudes and
    length scales. The same tolerances against the closed form, row by row."""
    import gpfit
    x, y, e, th, (want, gwant) = _case3()
    monkeypatch.setenv("GPF_MAX_CHUNK", "4")
    c = gpfit.Context(0)
    try:
        c.set_data(x, y, e)
        lml, grad = c.lml_hyper_batch(th)
    finally:
        c.close()
    _check("N=1100 d=3 P=6, chunks of 4", lml, grad, want, gwant)


def test_persistent_factorisation(ctx, monkeypatch):
    """GPF_PERSIST=1: k_build_cov builds the diagonal blocks, k_factor every other tile."""
    import gpfit
    x, y, e, th = _recipe_hyper(300, 2)
    want, gwant = _reference(("tb", 300), x, y, e, th)
    monkeypatch.setenv("GPF_PERSIST", "1")
    assert gpfit.plan_check(5, 3)["persistent"] == 1
    ctx.set_data(x, y, e)
    lml, grad = ctx.lml_hyper_batch(th)
    _check("N=300 d=2 GPF_PERSIST=1", lml, grad, want, gwant)


def test_unit_amplitude_is_lml_batch_bitwise_repeats_and_value_only(ctx):
    x, y, e, th = _recipe_hyper(300, 2)
    ctx.set_data(x, y, e)
    ls = np.ascontiguousarray(th[:, :2])
    base, gbase = ctx.lml_batch(ls)
    unit = np.column_stack([ls, np.ones(5), np.ones(5)])
    lml, grad = ctx.lml_hyper_batch(unit)
    np.testing.assert_array_equal(lml, base)
    np.testing.assert_array_equal(grad[:, :2], gbase)
    assert np.all(np.isfinite(grad[:, 2:]))
    lml, grad, q = ctx.lml_hyper_batch(th, want_q=True)
    lml2, grad2, q2 = ctx.lml_hyper_batch(th, want_q=True)
    np.testing.assert_array_equal(lml, lml2)
    np.testing.assert_array_equal(grad, grad2)
    np.testing.assert_array_equal(q, q2)
    only, none, qo = ctx.lml_hyper_batch(th, grad=False, want_q=True)
    assert none is None
    np.testing.assert_array_equal(only, lml)
    np.testing.assert_array_equal(qo, q)
    assert len(ctx.lml_hyper_batch(th, grad=False)) == 2


def test_scaling_identity(ctx):
    """The model with (a, s) on (x, y, e) is the unit model on (x, y / a, e s / a): lml(theta) is
    lml_batch(l) there minus N log a, and predict_hyper is a times predict there, bit for bit."""
    from gpfit.amplitude import predict_hyper, scaled_data
    N = 300
    x, y, e, th = _recipe_hyper(N, 2)
    ctx.set_data(x, y, e)
    lml, _ = ctx.lml_hyper_batch(th, grad=False)
    xf = np.random.default_rng(7).uniform(size=(2, 40))
    worst = 0.0
    for p, row in enumerate(th):
        a, s = row[2], row[3]
        ys, es = scaled_data(y, e, a, s)
        ctx.set_data(x, ys, es)
        want = ctx.lml_batch(row[None, :2], grad=False)[0][0] - N * np.log(a)
        worst = max(worst, abs(lml[p] - want) / max(abs(want), 1.0))
        mu, sd = ctx.predict(row[:2], xf)
        mh, sh = predict_hyper(x, y, e, xf, row, ctx=ctx)
        np.testing.assert_array_equal(mh, a * mu)
        np.testing.assert_array_equal(sh, a * sd)
    print(f"[amplitude] N={N}: lml(theta) vs lml_batch on the scaled data - N log a: {worst:.3e}")
    assert worst < TOL, worst


@pytest.mark.parametrize("N", [200, 300])
def test_neighbours_untouched(N):
    """eval_batch, lml_batch, then lml_hyper_batch with noise factors != 1 on a larger batch (the
    workspace grows), then eval_batch and lml_batch again: bitwise the same scores, LML and gradient
    (N = 200: the replayed-graph path)."""
    import gpfit
    from oracle import ref_cpu
    x, y, e, th = _recipe_hyper(N, 2, P=12)
    ls = np.ascontiguousarray(th[:, :2])
    assert np.all(np.abs((th[:, 3] / th[:, 2]) ** 2 - 1.0) > 1e-3)
    s, ex = ref_cpu.sigma_grid()
    c = gpfit.Context(0)
    try:
        c.set_data(x, y, e)
        c.set_grid(s, ex, np.full(2, 1e-3), np.full(2, 2.0))
        first = c.eval_batch(ls[:5])
        assert np.all(np.isfinite(first)) and np.all(first < 1e13)
        lml, grad = c.lml_batch(ls[:5])
        hl, hg = c.lml_hyper_batch(th)
        assert np.all(np.isfinite(hl)) and np.all(np.isfinite(hg))
        np.testing.assert_array_equal(c.eval_batch(ls[:5]), first)
        lml2, grad2 = c.lml_batch(ls[:5])
        np.testing.assert_array_equal(lml2, lml)
        np.testing.assert_array_equal(grad2, grad)
        # and without a regrow in between
        c.lml_hyper_batch(th[:5])
        np.testing.assert_array_equal(c.eval_batch(ls[:5]), first)
        np.testing.assert_array_equal(c.lml_batch(ls[:5])[0], lml)
    finally:
        c.close()


def test_non_pd_particle_does_not_spoil_the_batch(ctx):
    """One singular particle among good ones (the clustered points of the existing non-PD tests:
    l = 0.2 fails inside the cluster, l in [0.011, 0.02] is well conditioned; zero noise, so the noise
    scale cannot rescue it)."""
    from test_gpu import _cluster_data
    N, c0, P, bad = 1024, 400, 6, 3
    x, y, e = _cluster_data(N, c0)
    rng = np.random.default_rng(P)
    a = rng.uniform(0.5, 3.0, size=P)
    good = np.column_stack([rng.uniform(0.011, 0.02, size=P), a, a * rng.uniform(0.7, 1.5, size=P)])
    want, gwant = _reference(("cluster", N), x, y, e, good)
    ctx.set_data(x, y, e)
    clean, gclean = ctx.lml_hyper_batch(good)
    _check("cluster N=1024, clean batch", clean, gclean, want, gwant)
    Q = good.copy()
    Q[bad, 0] = 0.2
    lml, grad, q = ctx.lml_hyper_batch(Q, strict=False, want_q=True)
    others = [p for p in range(P) if p != bad]
    assert lml[bad] == -np.inf and np.all(np.isnan(grad[bad])) and np.isnan(q[bad])
    assert np.all(np.isfinite(lml[others])) and np.all(np.isfinite(grad[others])) and np.all(np.isfinite(q[others]))
    _check("cluster N=1024, one non-PD row", lml, grad, want, gwant, rows=others)
    with pytest.raises(np.linalg.LinAlgError, match="Matrix is not positive definite") as ei:
        ctx.lml_hyper_batch(Q)
    assert ei.value.particle == bad
    after, gafter = ctx.lml_hyper_batch(good)
    _check("cluster N=1024, clean batch after the failure", after, gafter, want, gwant)


def test_non_pd_particle_in_a_later_chunk(monkeypatch):
    """The singular particle in the second chunk (P = 6 through a workspace capped at 4: row 5 is slot 1
    of its chunk): its status, -inf, NaN gradient row (all d + 2 components) and NaN Q land at its index in
    the batch, not at its slot. The same clustered points at N = 300, the cluster in the second tile."""
    import gpfit
    from test_gpu import _cluster_data
    N, c0, P, bad = 300, 144, 6, 5
    x, y, e = _cluster_data(N, c0)
    rng = np.random.default_rng(P)
    a = rng.uniform(0.5, 3.0, size=P)
    good = np.column_stack([rng.uniform(0.011, 0.02, size=P), a, a * rng.uniform(0.7, 1.5, size=P)])
    want, gwant = _reference(("cluster", N), x, y, e, good)
    Q = good.copy()
    Q[bad, 0] = 0.2
    others = [p for p in range(P) if p != bad]
    monkeypatch.setenv("GPF_MAX_CHUNK", "4")
    c = gpfit.Context(0)
    try:
        c.set_data(x, y, e)
        lml, grad, q = c.lml_hyper_batch(Q, strict=False, want_q=True)
        assert lml[bad] == -np.inf and np.all(np.isnan(grad[bad])) and np.isnan(q[bad])
        assert np.all(np.isfinite(lml[others])) and np.all(np.isfinite(grad[others])) and np.all(np.isfinite(q[others]))
        _check("cluster N=300, non-PD row 5 in chunk 2", lml, grad, want, gwant, rows=others)
        with pytest.raises(np.linalg.LinAlgError, match="Matrix is not positive definite") as ei:
            c.lml_hyper_batch(Q)
        assert ei.value.particle == bad
        after, gafter = c.lml_hyper_batch(good)
        _check("cluster N=300, clean batch after the failure", after, gafter, want, gwant)
    finally:
        c.close()


def test_bad_arguments():
    import gpfit
    c = gpfit.Context(0)
    try:
        with pytest.raises(ValueError, match="gpf_set_data"):
            c.lml_hyper_batch(np.array([[0.3, 0.3, 1.0, 1.0]]))
        x, y, e, th = _recipe_hyper(50, 2)
        c.set_data(x, y, e)
        for col in (1, 2, 3):  # a length scale, a, s
            for v in (0.0, -1.0, np.nan, np.inf):
                Q = th.copy()
                Q[2, col] = v
                with pytest.raises(ValueError, match="finite and > 0"):
                    c.lml_hyper_batch(Q)
        for a, s in ((1e-200, 1e200), (1e200, 1e-200)):  # (s / a)^2 overflows, underflows to 0
            Q = th.copy()
            Q[1, 2:] = a, s
            with pytest.raises(ValueError, match="finite and > 0"):
                c.lml_hyper_batch(Q)
        with pytest.raises(ValueError, match=r"theta must be \(P, 4\)"):
            c.lml_hyper_batch(th[:, :3])
        assert c.lml_hyper_batch(np.empty((0, 4)))[0].shape == (0,)
        # no grid, no box: set_data alone is enough
        want, gwant = _reference(("args", 50), x, y, e, th)
        lml, grad = c.lml_hyper_batch(th)
        _check("N=50 d=2, no grid", lml, grad, want, gwant)
    finally:
        c.close()


def test_fit_hyper_end_to_end(ctx):
    """fit_hyper on the device: tests/test_mle_host.py's first recipe (seed 0, d = 2, N = 150) multiplied
    by 2.5 with its errors understated by a factor of 2. The device value at the result is the closed
    form's, and no lower than at the theta that generated the data."""
    from gpfit.amplitude import fit_hyper
    seed, d, N, l_true = FIT_RECIPES[0]
    x, y, e, gen = scaled_sample(seed, d, N, l_true)
    best, info = fit_hyper(x, y, e, num_starts=16, num_polish=1, max_points=N, seed=0, ctx=ctx, verbose=False)
    at_best = ctx.lml_hyper_batch(best[None, :], grad=False)[0][0]
    truth = ctx.lml_hyper_batch(gen[None, :], grad=False)[0][0]
    print(f"[amplitude] fit {info['lml']:.4f} at {best}, generating theta {truth:.4f}, "
          f"best start {np.max(info['starts'][1]):.4f}, evals {info['evals']}, grad evals {info['grad_evals']}")
    ref = hyper_closed_form(x, y, e, best)[0]
    assert abs(at_best - ref) < TOL * max(abs(ref), 1.0), (at_best, ref)
    assert abs(truth - hyper_closed_form(x, y, e, gen)[0]) < TOL * max(abs(truth), 1.0)
    assert abs(info["lml"] - at_best) < TOL * max(abs(at_best), 1.0)
    assert info["lml"] >= truth, (info["lml"], truth)
    lower, upper = info["box"]
    assert np.all(best >= lower) and np.all(best <= upper)
    assert info["grad_evals"] < info["evals"]  # the starts were scored without the gradient pass
