"""gpf_loo_batch (batched leave-one-out predictions, their log predictive density and its length-scale
gradient: k_loo_points, k_loo_w, k_loo_scale_mirror, k_loo_u, k_loo_grad) against the closed form of
tests/test_loo_host.py evaluated in np.longdouble.

Tolerances. lpd relative, mu relative to max |mu| and sd relative: each < 1e-9, the project's bound
(the float64 closed form is within 4.4e-12 of the longdouble one on this recipe). The gradient is
worse conditioned than the LML's: the float64 closed form itself is up to 7.8e-10 from the longdouble
one (N = 300, d = 2), so per particle
    max_k |g - g_ref| / max_k |g_ref| < max(1e-9, 10 gap64),
gap64 being the float64 closed form's error against longdouble for that particle: the device may be
ten times less accurate than NumPy's float64 evaluation of the same formula, with 1e-9 as the floor.
The longdouble reference is computed once per case here for N <= 300 and read from
tests/golden/loo_longdouble.npz (tests/golden/make_loo_golden.py) at N = 1100.
At N = 1 the reference mean is exactly 0 and "relative to max |mu|" has no scale: there the mean is
held to 1e-9 |y| (it is y - alpha / w with alpha / w = y up to rounding).
The measured maxima are printed (run with -s) and sit in the assert messages.
"""
import numpy as np
import pytest

from conftest import data_sha256, load_golden
from test_lml_grad_gpu import _recipe
from test_loo_host import check_fit, gradient_gap, loo_closed_form, loo_longdouble
from test_mle_host import FIT_RECIPES, gp_sample

pytestmark = pytest.mark.gpu

TOL = 1e-9


@pytest.fixture(scope="module")
def ctx():
    import gpfit
    c = gpfit.Context(0)
    yield c
    c.close()


_REF = {}


def _reference(key, x, y, e, ls):
    """(mu, sd, lpd, grad, gap64) of every particle in longdouble rounded to float64, computed once
    per case and shared; gap64 is the float64 closed form's gradient error against it."""
    if key not in _REF:
        rows = []
        for p in ls:
            m, s, v, g = loo_longdouble(x, y, e, p)
            gap = gradient_gap(loo_closed_form(x, y, e, p)[3], g)
            rows.append((m.astype(np.float64), s.astype(np.float64), np.float64(v), g.astype(np.float64), gap))
        ref = tuple(np.array(col) for col in zip(*rows))
        for a in ref:
            a.setflags(write=False)
        _REF[key] = ref
    return _REF[key]


def _golden_reference():
    x, y, e, ls = _recipe(1100, 3, P=6)
    assert len({tuple(p) for p in ls}) == 6  # distinct rows: a row mix-up shows
    z = load_golden("loo_longdouble.npz")
    assert data_sha256(x, y, e, ls) == str(z["sha256"]), "regenerated inputs differ from the fixture's"
    np.testing.assert_array_equal(z["ls"], ls)
    return x, y, e, ls, (z["mu"], z["sd"], z["lpd"], z["grad"], z["gap64"])


def _check(tag, got, ref, rows=None):
    lpd, grad, mu, sd = got
    rmu, rsd, rlpd, rgrad, gap = ref
    rows = list(range(len(rlpd)) if rows is None else rows)
    ev = (np.abs(lpd - rlpd) / np.abs(rlpd))[rows]
    em = (np.max(np.abs(mu - rmu), axis=1) / np.max(np.abs(rmu), axis=1))[rows]
    es = np.max(np.abs(sd - rsd) / rsd, axis=1)[rows]
    eg = np.array([gradient_gap(grad[p], rgrad[p]) for p in rows])
    tg = np.maximum(TOL, 10.0 * gap[rows])
    print(f"[loo] {tag}: max err lpd {np.max(ev):.3e}, mu {np.max(em):.3e}, sd {np.max(es):.3e} (tol {TOL:.0e}); "
          f"gradient {np.max(eg):.3e} (float64 closed form {np.max(gap[rows]):.3e}, worst err / tol {np.max(eg / tg):.3f})")
    assert np.max(ev) < TOL, f"{tag}: lpd errors {ev}"
    assert np.max(em) < TOL, f"{tag}: mu errors {em}"
    assert np.max(es) < TOL, f"{tag}: sd errors {es}"
    assert np.all(eg < tg), f"{tag}: gradient errors {eg}, tolerances {tg}"


def _loo(c, ls, **kw):
    return c.loo_batch(ls, grad=True, points=True, **kw)


@pytest.mark.parametrize("N", [1, 2, 127, 128, 129, 257, 300])
def test_tile_boundaries(ctx, N):
    x, y, e, ls = _recipe(N, 2)
    ctx.set_data(x, y, e)
    got = _loo(ctx, ls)
    assert got[0].shape == (5,) and got[1].shape == (5, 2) and got[2].shape == got[3].shape == (5, N)
    if N == 1:
        lpd, grad, mu, sd = got
        np.testing.assert_array_equal(grad, np.zeros((5, 2)))
        assert np.max(np.abs(mu)) < TOL * abs(y[0]), mu
        want_sd = np.sqrt(1.0 + e[0] ** 2)
        assert np.max(np.abs(sd - want_sd)) < TOL * want_sd, sd
        want = -0.5 * np.log(2 * np.pi * want_sd ** 2) - 0.5 * (y[0] / want_sd) ** 2
        print(f"[loo] N=1: |mu| {np.max(np.abs(mu)):.3e}, sd err {np.max(np.abs(sd - want_sd)):.3e}")
        assert np.max(np.abs(lpd - want)) < TOL * abs(want), lpd
        return
    _check(f"N={N} d=2", got, _reference(("tb", N), x, y, e, ls))


@pytest.mark.parametrize("d", [1, 3, 4])
def test_dimensions(ctx, d):
    x, y, e, ls = _recipe(200, d)
    ctx.set_data(x, y, e)
    _check(f"N=200 d={d}", _loo(ctx, ls), _reference(("dim", d), x, y, e, ls))


@pytest.mark.parametrize("d", [17, 32])
def test_run_time_dimensions(ctx, d):
    """The run-time-d epilogue and the LDS layout at DMAX, on test_dimension_gpu.py's recipe."""
    from test_dimension_gpu import recipe
    x, y, e, ls = recipe(200, d, 3)
    ctx.set_data(x, y, e)
    got = _loo(ctx, ls)
    assert got[1].shape == (3, d)
    _check(f"N=200 d={d}", got, _reference(("rtd", d), x, y, e, ls))


def test_nine_block_columns_ragged(ctx):
    x, y, e, ls, ref = _golden_reference()
    ctx.set_data(x, y, e)
    _check("N=1100 d=3 P=6", _loo(ctx, ls), ref)


def test_chunked_batch(monkeypatch):
    """6 particles through a workspace capped at 4 per chunk (a fresh context: the cap is read when
    the workspace is sized)."""
    import gpfit
    x, y, e, ls, ref = _golden_reference()
    monkeypatch.setenv("GPF_MAX_CHUNK", "4")
    c = gpfit.Context(0)
    try:
        c.set_data(x, y, e)
        got = _loo(c, ls)
    finally:
        c.close()
    _check("N=1100 d=3 P=6, chunks of 4", got, ref)


def test_single_particle(ctx):
    """P = 1: the single-particle split factorisation feeds the same kernels (its schedule differs from
    the batch's in the last bits, so the bound is the closed-form tolerance, not equality)."""
    x, y, e, ls = _recipe(300, 2)
    ref = _reference(("tb", 300), x, y, e, ls)
    ctx.set_data(x, y, e)
    for p in (0, 3):
        got = _loo(ctx, ls[p:p + 1])
        _check(f"N=300 d=2 P=1 (row {p})", got, tuple(a[p:p + 1] for a in ref))


def test_value_only_and_repeats_are_bitwise(ctx):
    x, y, e, ls = _recipe(300, 2)
    ctx.set_data(x, y, e)
    full = _loo(ctx, ls)
    again = _loo(ctx, ls)
    for a, b in zip(full, again):
        np.testing.assert_array_equal(a, b)
    lpd, none, mu, sd = ctx.loo_batch(ls, grad=False, points=True)
    assert none is None
    np.testing.assert_array_equal(lpd, full[0])
    np.testing.assert_array_equal(mu, full[2])
    np.testing.assert_array_equal(sd, full[3])
    two = ctx.loo_batch(ls, grad=False)
    assert len(two) == 2 and two[1] is None
    np.testing.assert_array_equal(two[0], full[0])


def _cluster_at_origin(N, c0, nc=20, spacing=0.01):
    """test_gpu._cluster_data's construction (d = 1, unit-spaced points, a cluster of nc points spaced
    `spacing` at rows c0.., zero noise) with the cluster at the origin and the other points at 10 + i.
    There the cluster sits at x = -50, and |a|^2 + |b|^2 - 2ab at a = x / l ~ 4500 rounds K's entries
    at the 1e-9 level: the float64 closed form is then 3e-8 (sd) from the longdouble one whatever the
    solver, and a 1e-9 check against longdouble would measure the kernel's rounding, not the LOO
    kernels. At the origin a <= 19 and the float64 closed form is within 3e-11 of longdouble for
    l <= 0.017 (1.8e-9 at l = 0.02, where the cluster block's conditioning shows: the good particles
    stay below 0.016)."""
    x = np.arange(N, dtype=float) + 10.0
    x[c0:c0 + nc] = spacing * np.arange(nc)
    x = x[None, :]
    y = np.sin(x[0]) + 0.01 * np.arange(N) / N
    return x, y, np.zeros(N)


def test_non_pd_particle_does_not_spoil_the_batch(ctx):
    """One singular particle among good ones, on the near-duplicate zero-noise points of the existing
    non-PD tests (l = 0.2 fails inside the cluster, l in [0.011, 0.016] is well conditioned), at
    N = 300 with the cluster in the second tile so that the longdouble reference stays quick."""
    N, c0, P, bad = 300, 144, 6, 3
    x, y, e = _cluster_at_origin(N, c0)
    good = np.random.default_rng(P).uniform(0.011, 0.016, size=(P, 1))
    ref = _reference(("cluster", N), x, y, e, good)
    ctx.set_data(x, y, e)
    _check("cluster N=300, clean batch", _loo(ctx, good), ref)
    Q = good.copy()
    Q[bad, 0] = 0.2
    with pytest.raises(np.linalg.LinAlgError):
        loo_closed_form(x, y, e, Q[bad])
    got = _loo(ctx, Q, strict=False)
    lpd, grad, mu, sd = got
    others = [p for p in range(P) if p != bad]
    assert lpd[bad] == -np.inf and np.all(np.isnan(grad[bad])) and np.all(np.isnan(mu[bad])) and np.all(np.isnan(sd[bad]))
    assert all(np.all(np.isfinite(a[others])) for a in got)
    _check("cluster N=300, one non-PD row", got, ref, rows=others)
    with pytest.raises(np.linalg.LinAlgError, match="Matrix is not positive definite") as ei:
        _loo(ctx, Q)
    assert ei.value.particle == bad
    _check("cluster N=300, clean batch after the failure", _loo(ctx, good), ref)


def test_non_pd_particle_in_a_later_chunk(monkeypatch):
    """The singular particle in the second chunk (P = 6 through a workspace capped at 4: row 5 is slot 1
    of its chunk): its status, -inf and NaN rows (gradient, mu, sd) land at its index in the batch, not
    at its slot. The data and particles of the test above (and its reference)."""
    import gpfit
    N, c0, P, bad = 300, 144, 6, 5
    x, y, e = _cluster_at_origin(N, c0)
    good = np.random.default_rng(P).uniform(0.011, 0.016, size=(P, 1))
    ref = _reference(("cluster", N), x, y, e, good)
    Q = good.copy()
    Q[bad, 0] = 0.2
    others = [p for p in range(P) if p != bad]
    monkeypatch.setenv("GPF_MAX_CHUNK", "4")
    c = gpfit.Context(0)
    try:
        c.set_data(x, y, e)
        got = _loo(c, Q, strict=False)
        lpd, grad, mu, sd = got
        assert lpd[bad] == -np.inf and np.all(np.isnan(grad[bad])) and np.all(np.isnan(mu[bad])) and np.all(np.isnan(sd[bad]))
        assert all(np.all(np.isfinite(a[others])) for a in got)
        _check("cluster N=300, non-PD row 5 in chunk 2", got, ref, rows=others)
        with pytest.raises(np.linalg.LinAlgError, match="Matrix is not positive definite") as ei:
            _loo(c, Q)
        assert ei.value.particle == bad
        _check("cluster N=300, clean batch after the failure", _loo(c, good), ref)
    finally:
        c.close()


def test_bad_arguments():
    import gpfit
    c = gpfit.Context(0)
    try:
        with pytest.raises(ValueError, match="gpf_set_data"):
            c.loo_batch(np.array([[0.3, 0.3]]))
        x, y, e, ls = _recipe(50, 2)
        c.set_data(x, y, e)
        for v in (0.0, -0.1, np.nan, np.inf):
            Q = ls.copy()
            Q[2, 1] = v
            with pytest.raises(ValueError, match="finite and > 0"):
                c.loo_batch(Q)
        with pytest.raises(ValueError, match="positions must be"):
            c.loo_batch(np.ones((2, 3)))
        lpd, grad = c.loo_batch(np.empty((0, 2)))
        assert lpd.shape == (0,) and grad.shape == (0, 2)
    finally:
        c.close()


def test_other_calls_keep_their_bits():
    """lml_batch (value and gradient), eval_batch and predict on one context, before and after a
    loo_batch with the gradient: bitwise equal."""
    import gpfit
    from oracle import ref_cpu
    x, y, e, ls = _recipe(300, 2, P=6)
    s, ex = ref_cpu.sigma_grid()
    xf = np.random.default_rng(7).uniform(size=(2, 150))
    c = gpfit.Context(0)

    def calls():
        return [*c.lml_batch(ls), c.eval_batch(ls), *c.predict(ls[1], xf)]

    try:
        c.set_data(x, y, e)
        c.set_grid(s, ex, np.full(2, 1e-3), np.full(2, 2.0))
        before = calls()
        got = c.loo_batch(ls, grad=True)
        assert np.all(np.isfinite(got[0])) and np.all(np.isfinite(got[1]))
        after = calls()
        assert len(before) == len(after) == 5
        for a, b in zip(before, after):
            assert np.all(np.isfinite(a))
            np.testing.assert_array_equal(a, b)
    finally:
        c.close()


def test_fit_loo_end_to_end(ctx):
    """fit_loo on the device (seed 0, d = 2, N = 150, l_true = (0.3, 0.6)); max_points = N: all 150
    points, not a subsample."""
    from gpfit.loo import fit_loo, loo_predict
    seed, d, N, l_true = FIT_RECIPES[0]
    x, y, e = gp_sample(seed, d, N, l_true)
    best, info = fit_loo(x, y, e, num_starts=16, num_polish=1, max_points=N, seed=0, ctx=ctx, verbose=False)
    print(f"[loo] fit {info['lpd']:.4f} at {best}, best start {np.max(info['starts'][1]):.4f}, evals {info['evals']}")
    check_fit(best, info)
    want = loo_closed_form(x, y, e, best)
    assert abs(info["lpd"] - want[2]) < TOL * abs(want[2])
    again, info2 = fit_loo(x, y, e, num_starts=16, num_polish=1, max_points=N, seed=0, ctx=ctx, verbose=False)
    np.testing.assert_array_equal(best, again)
    assert info2["evals"] == info["evals"]
    mu, sd, rep = loo_predict(x, y, e, best, ctx=ctx)
    assert np.max(np.abs(mu - want[0])) < TOL * np.max(np.abs(want[0])) and np.max(np.abs(sd - want[1]) / want[1]) < TOL
    assert abs(rep["lpd"] - info["lpd"]) < TOL * abs(want[2])
    np.testing.assert_array_equal(rep["pulls"], (y - mu) / sd)
    assert 0.0 <= rep["coverage"][0] <= rep["coverage"][1] <= 1.0
