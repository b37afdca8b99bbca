"""gpf_lml_batch (batched log marginal likelihood and its length-scale gradient, k_lml_grad) against
the float64 NumPy closed form (np.linalg.inv / np.linalg.cholesky, tests/test_mle_host.py).

Tolerances: value |got - want| / |want| < 1e-9 (the existing LML test's), gradient
max_k |g - g_ref| / max_k |g_ref| < 1e-9 per particle. On the recipe below at N <= 300 the float64
closed form differs from the same formula in np.longdouble by <= 1.2e-12 (gradient) and <= 1.6e-12
(value), cond(Kn) <= 9e4: 1e-9 leaves about three orders for a different summation order. The
measured maxima are printed (run with -s) and sit in the assert messages.
"""
import numpy as np
import pytest

from test_mle_host import FIT_RECIPES, check_fit, gp_sample, lml_closed_form

pytestmark = pytest.mark.gpu

TOL = 1e-9


@pytest.fixture(scope="module")
def ctx():
    import gpfit
    c = gpfit.Context(0)
    yield c
    c.close()


def _recipe(N, d, P=5):
    """The data of test_tile_boundaries_vs_oracle: default_rng(N), x ~ U(0,1)^d,
    y = sin(3 x0) + x1 + 0.1 randn (d = 1: sin(3 x0) + 0.1 randn), e ~ U(0.05, 0.2), l ~ U(0.05, 0.8)."""
    rng = np.random.default_rng(N)
    x = rng.uniform(size=(d, N))
    y = np.sin(3 * x[0]) + (x[1] if d > 1 else 0.0) + 0.1 * rng.standard_normal(N)
    e = rng.uniform(0.05, 0.2, size=N)
    ls = rng.uniform(0.05, 0.8, size=(P, d))
    return x, y, e, ls


_REF = {}


def _reference(key, x, y, e, ls):
    """The closed form of every particle, computed once per case and shared."""
    if key not in _REF:
        vals, grads = zip(*(lml_closed_form(x, y, e, p) for p in ls))
        v, g = np.array(vals), np.array(grads)
        v.setflags(write=False)
        g.setflags(write=False)
        _REF[key] = (v, g)
    return _REF[key]


def _errors(lml, grad, want, gwant):
    ev = np.abs(lml - want) / np.abs(want)
    scale = np.max(np.abs(gwant), axis=1)
    eg = np.max(np.abs(grad - gwant), axis=1) / np.where(scale > 0, scale, 1.0)
    return ev, eg


def _check(tag, lml, grad, want, gwant, rows=None):
    rows = range(len(want)) if rows is None else rows
    ev, eg = _errors(lml, grad, want, gwant)
    ev, eg = ev[list(rows)], eg[list(rows)]
    print(f"[lml_grad] {tag}: max value err {np.max(ev):.3e}, max gradient err {np.max(eg):.3e} (tol {TOL:.0e})")
    assert np.max(ev) < TOL, f"{tag}: value errors {ev}"
    assert np.max(eg) < TOL, f"{tag}: gradient errors {eg}"


@pytest.mark.parametrize("N", [1, 2, 127, 128, 129, 257, 300])
def test_tile_boundaries_vs_closed_form(ctx, N):
    x, y, e, ls = _recipe(N, 2)
    want, gwant = _reference(("tb", N), x, y, e, ls)
    ctx.set_data(x, y, e)
    lml, grad = ctx.lml_batch(ls)
    if N == 1:
        np.testing.assert_array_equal(grad, np.zeros((5, 2)))
        assert np.all(gwant == 0)
    _check(f"N={N} d=2", lml, grad, want, gwant)


@pytest.mark.parametrize("d", [1, 3, 4])
def test_dimensions_vs_closed_form(ctx, d):
    x, y, e, ls = _recipe(200, d)
    want, gwant = _reference(("dim", d), x, y, e, ls)
    ctx.set_data(x, y, e)
    lml, grad = ctx.lml_batch(ls)
    _check(f"N=200 d={d}", lml, grad, want, gwant)


def _case3():
    x, y, e, ls = _recipe(1100, 3, P=6)
    assert len({tuple(p) for p in ls}) == 6  # distinct rows: a row mix-up shows
    return x, y, e, ls, _reference(("big", 1100), x, y, e, ls)


def test_nine_block_columns_ragged(ctx):
    x, y, e, ls, (want, gwant) = _case3()
    ctx.set_data(x, y, e)
    lml, grad = ctx.lml_batch(ls)
    _check("N=1100 d=3 P=6", lml, grad, want, gwant)


def test_chunked_batch(monkeypatch):
    """6 particles through a workspace capped at 4 per chunk (a fresh context: the cap is read when
    the workspace is sized): the same tolerances against the closed form, row by row."""
    import gpfit
    x, y, e, ls, (want, gwant) = _case3()
    monkeypatch.setenv("GPF_MAX_CHUNK", "4")
    c = gpfit.Context(0)
    try:
        c.set_data(x, y, e)
        lml, grad = c.lml_batch(ls)
    finally:
        c.close()
    _check("N=1100 d=3 P=6, chunks of 4", lml, grad, want, gwant)


def test_repeats_value_only_and_single_particle(ctx):
    x, y, e, ls = _recipe(300, 2)
    ctx.set_data(x, y, e)
    lml, grad = ctx.lml_batch(ls)
    lml2, grad2 = ctx.lml_batch(ls)
    np.testing.assert_array_equal(lml, lml2)
    np.testing.assert_array_equal(grad, grad2)
    only, none = ctx.lml_batch(ls, grad=False)
    assert none is None
    np.testing.assert_array_equal(only, lml)
    single = np.array([ctx.log_marginal_likelihood(p) for p in ls])
    err = np.max(np.abs(lml - single) / np.abs(single))
    print(f"[lml_grad] lml_batch vs log_marginal_likelihood: {err:.3e}")
    assert err < TOL, err


def test_non_pd_particle_does_not_spoil_the_batch(ctx):
    """One singular particle among good ones (the clustered points of the existing non-PD tests:
    l = 0.2 fails inside the cluster, l in [0.011, 0.02] is well conditioned)."""
    from test_gpu import _cluster_data
    N, c0, P, bad = 1024, 400, 6, 3
    x, y, e = _cluster_data(N, c0)
    rng = np.random.default_rng(P)
    good = rng.uniform(0.011, 0.02, size=(P, 1))
    want, gwant = _reference(("cluster", N), x, y, e, good)
    ctx.set_data(x, y, e)
    clean, gclean = ctx.lml_batch(good)
    _check("cluster N=1024, clean batch", clean, gclean, want, gwant)
    Q = good.copy()
    Q[bad, 0] = 0.2
    lml, grad = ctx.lml_batch(Q, strict=False)
    others = [p for p in range(P) if p != bad]
    assert lml[bad] == -np.inf and np.all(np.isnan(grad[bad]))
    assert np.all(np.isfinite(lml[others])) and np.all(np.isfinite(grad[others]))
    _check("cluster N=1024, one non-PD row", lml, grad, want, gwant, rows=others)
    with pytest.raises(np.linalg.LinAlgError, match="Matrix is not positive definite") as ei:
        ctx.lml_batch(Q)
    assert ei.value.particle == bad
    after, gafter = ctx.lml_batch(good)
    _check("cluster N=1024, clean batch after the failure", after, gafter, want, gwant)


def test_non_pd_particle_in_a_later_chunk(monkeypatch):
    """The singular particle in the second chunk (P = 6 through a workspace capped at 4: row 5 is slot 1
    of its chunk): its status, -inf and NaN row land at its index in the batch, not at its slot. The same
    clustered points at N = 300, the cluster in the second tile."""
    import gpfit
    from test_gpu import _cluster_data
    N, c0, P, bad = 300, 144, 6, 5
    x, y, e = _cluster_data(N, c0)
    good = np.random.default_rng(P).uniform(0.011, 0.02, size=(P, 1))
    want, gwant = _reference(("cluster", N), x, y, e, good)
    Q = good.copy()
    Q[bad, 0] = 0.2
    others = [p for p in range(P) if p != bad]
    monkeypatch.setenv("GPF_MAX_CHUNK", "4")
    c = gpfit.Context(0)
    try:
        c.set_data(x, y, e)
        lml, grad = c.lml_batch(Q, strict=False)
        assert lml[bad] == -np.inf and np.all(np.isnan(grad[bad]))
        assert np.all(np.isfinite(lml[others])) and np.all(np.isfinite(grad[others]))
        _check("cluster N=300, non-PD row 5 in chunk 2", lml, grad, want, gwant, rows=others)
        with pytest.raises(np.linalg.LinAlgError, match="Matrix is not positive definite") as ei:
            c.lml_batch(Q)
        assert ei.value.particle == bad
        after, gafter = c.lml_batch(good)
        _check("cluster N=300, clean batch after the failure", after, gafter, want, gwant)
    finally:
        c.close()


def test_bad_arguments():
    import gpfit
    c = gpfit.Context(0)
    try:
        with pytest.raises(ValueError, match="gpf_set_data"):
            c.lml_batch(np.array([[0.3, 0.3]]))
        x, y, e, ls = _recipe(50, 2)
        c.set_data(x, y, e)
        for v in (0.0, -0.1, np.nan, np.inf):
            Q = ls.copy()
            Q[2, 1] = v
            with pytest.raises(ValueError, match="finite and > 0"):
                c.lml_batch(Q)
        # no grid, no box: set_data alone is enough
        want, gwant = _reference(("args", 50), x, y, e, ls)
        lml, grad = c.lml_batch(ls)
        _check("N=50 d=2, no grid", lml, grad, want, gwant)
    finally:
        c.close()


@pytest.mark.parametrize("N", [200, 300])
def test_evaluation_path_untouched(N):
    """eval_batch, then lml_batch of a larger batch (the workspace grows), then eval_batch again:
    bitwise the same scores (N = 200: the replayed-graph path)."""
    import gpfit
    from oracle import ref_cpu
    x, y, e, ls = _recipe(N, 2, P=12)
    s, ex = ref_cpu.sigma_grid()
    c = gpfit.Context(0)
    try:
        c.set_data(x, y, e)
        c.set_grid(s, ex, np.full(2, 1e-3), np.full(2, 2.0))
        first = c.eval_batch(ls[:5])
        assert np.all(np.isfinite(first)) and np.all(first < 1e13)
        lml, grad = c.lml_batch(ls)
        assert np.all(np.isfinite(lml)) and np.all(np.isfinite(grad))
        np.testing.assert_array_equal(c.eval_batch(ls[:5]), first)
    finally:
        c.close()


def test_fit_lml_end_to_end(ctx):
    """fit_lml on the device (seed 0, d = 2, N = 150, l_true = (0.3, 0.6)); with the NumPy evaluator
    the fit reaches 73.44, above the truth's 72.06 and the best start's 68.32
    (tests/test_mle_host.py). max_points = N: those figures are for all 150 points, not a subsample."""
    from gpfit.mle import fit_lml
    seed, d, N, l_true = FIT_RECIPES[0]
    x, y, e = gp_sample(seed, d, N, l_true)
    best, info = fit_lml(x, y, e, num_starts=16, num_polish=1, max_points=N, seed=0, ctx=ctx, verbose=False)
    truth = ctx.lml_batch(np.array([l_true]), grad=False)[0][0]
    print(f"[lml_grad] fit {info['lml']:.4f} at {best}, truth {truth:.4f}, "
          f"best start {np.max(info['starts'][1]):.4f}, evals {info['evals']}")
    check_fit(best, info, truth)
    assert abs(truth - lml_closed_form(x, y, e, l_true)[0]) < TOL * abs(truth)
