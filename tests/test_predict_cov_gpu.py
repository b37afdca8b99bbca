"""gpf_predict_cov (joint posterior covariance Sigma = K_ss - V^T V and mean at the query points;
k_predict_v, k_post_cov, k_mirror_lower) against the float64 NumPy closed form written below.

Tolerances: max |Sigma - Sigma_ref| < 1e-9 absolute (the prior variance is 1, so absolute equals
relative to the prior scale) and max |mu - mu_ref| / max(1, max |mu_ref|) < 1e-9: the project's
bound for the LML value and gradient. On this recipe the float64 closed form differs from the same
formula in 80-bit np.longdouble by at most 1.4e-13 (Sigma) and 1.3e-12 (mu), cond(Kn) <= 8.6e4
(measured on the CPU for the five tile-boundary cases), so 1e-9 leaves about four orders for a
different summation order. The measured maxima are printed (run with -s) and sit in the assert
messages; on one MI355X: Sigma within 5.3e-14, mu within 2.1e-13, the clipped diagonal within 3.2e-15
of predict()'s variance (profiles/predict_cov/pytest_gpu.log).
"""
import numpy as np
import pytest

from test_lml_grad_gpu import _recipe

pytestmark = pytest.mark.gpu

TOL = 1e-9


@pytest.fixture(scope="module")
def ctx():
    import gpfit
    c = gpfit.Context(0)
    yield c
    c.close()


def _kernel(a, b, l):
    """kernel_func (GP_func.py:49-65) in float64 NumPy."""
    a, b = a / l[:, None], b / l[:, None]
    r2 = (np.sum(a * a, axis=0)[:, None] + np.sum(b * b, axis=0)[None, :]) - 2.0 * (a.T @ b)
    return np.exp(-0.5 * np.maximum(r2, 0.0))


def _case(N, d, M):
    """Data and length scales of tests/test_lml_grad_gpu.py::_recipe(N, d); queries U(-0.1, 1.1)^d from
    default_rng(1000 + M), the first min(N, M) // 4 on training points, the last two a duplicate pair."""
    x, y, e, ls = _recipe(N, d)
    q = np.random.default_rng(1000 + M).uniform(-0.1, 1.1, (d, M))
    k = min(N, M) // 4
    q[:, :k] = x[:, :k]
    if M > 2:
        q[:, -1] = q[:, -2]
    return x, y, e, ls, q


_REF = {}


def _reference(N, d, M, row):
    """(mu, Sigma) of the closed form for length-scale row `row`, computed once per case and shared."""
    key = (N, d, M, row)
    if key not in _REF:
        x, y, e, ls, q = _case(N, d, M)
        l = ls[row]
        Kn = _kernel(x, x, l) + np.diag(e ** 2)
        Ks = _kernel(x, q, l)
        L = np.linalg.cholesky(Kn)
        v = np.linalg.solve(L, Ks)
        Kss = _kernel(q, q, l)
        np.fill_diagonal(Kss, 1.0)
        cov = Kss - v.T @ v
        mu = Ks.T @ np.linalg.solve(Kn, y)
        mu.setflags(write=False)
        cov.setflags(write=False)
        _REF[key] = (mu, cov)
    return _REF[key]


def _check_case(ctx, N, d, M, rows=(0, 1, 2)):
    x, y, e, ls, q = _case(N, d, M)
    ctx.set_data(x, y, e)
    for row in rows:
        tag = f"N={N} d={d} M={M} ls row {row}"
        mu_ref, cov_ref = _reference(N, d, M, row)
        mu, cov = ctx.predict_cov(ls[row], q)
        assert mu.shape == (M,) and cov.shape == (M, M)
        mu_p, sd_p = ctx.predict(ls[row], q)
        ec = np.max(np.abs(cov - cov_ref))
        em = np.max(np.abs(mu - mu_ref)) / max(1.0, np.max(np.abs(mu_ref)))
        ev = np.max(np.abs(np.clip(np.diag(cov), 1e-12, None) - sd_p ** 2))
        print(f"[predict_cov] {tag}: max cov err {ec:.3e}, mu err {em:.3e}, |clip(diag) - sd^2| {ev:.3e}, "
              f"min diag {np.min(np.diag(cov)):.3e} (tol {TOL:.0e})")
        assert ec < TOL, f"{tag}: max |cov - cov_ref| = {ec:.3e}"
        assert em < TOL, f"{tag}: mu error {em:.3e}"
        np.testing.assert_array_equal(cov, cov.T, err_msg=f"{tag}: cov is not exactly symmetric")
        np.testing.assert_array_equal(mu, mu_p, err_msg=f"{tag}: mu is not bitwise predict()'s")
        assert ev < TOL, f"{tag}: |clip(diag cov, 1e-12) - sd_predict^2| = {ev:.3e}"
        if M > 2:
            er = np.max(np.abs(cov[-1] - cov[-2]))
            emd = abs(mu[-1] - mu[-2])
            print(f"[predict_cov] {tag}: duplicate pair: rows differ by {er:.3e}, means by {emd:.3e}")
            assert er < TOL, f"{tag}: rows of the duplicate pair differ by {er:.3e}"
            assert emd < TOL, f"{tag}: means of the duplicate pair differ by {emd:.3e}"


@pytest.mark.parametrize("N,d,M", [(1, 2, 129), (129, 2, 1), (128, 1, 128), (300, 2, 257), (257, 3, 300)])
def test_tile_boundaries_vs_closed_form(ctx, N, d, M):
    _check_case(ctx, N, d, M)


def test_deep_and_ragged(ctx):
    """Nine depth tiles, two ragged column tiles."""
    _check_case(ctx, 1100, 3, 130)


def test_repeatability_and_buffer_reuse(ctx):
    """predict and predict_cov interleaved on one context, with batches of other sizes in between:
    each keeps its own bits."""
    from oracle import ref_cpu
    x, y, e, ls, q300 = _case(300, 2, 300)
    q129 = _case(300, 2, 129)[4]
    s, ex = ref_cpu.sigma_grid()
    ctx.set_data(x, y, e)
    ctx.set_grid(s, ex, np.full(2, 1e-3), np.full(2, 2.0))
    p1 = ctx.predict(ls[0], q300)
    c1 = ctx.predict_cov(ls[0], q129)
    p2 = ctx.predict(ls[0], q300)
    c2 = ctx.predict_cov(ls[0], q129)
    for a, b in zip(p1 + c1, p2 + c2):
        np.testing.assert_array_equal(a, b)
    assert np.all(np.isfinite(ctx.eval_batch(ls)))
    assert np.all(np.isfinite(ctx.eval_batch(ls[:2])))
    c3 = ctx.predict_cov(ls[0], q129)
    np.testing.assert_array_equal(c3[0], c1[0])
    np.testing.assert_array_equal(c3[1], c1[1])
    # a wider call in between regrows the kept buffers; the narrower one still gives the same bits
    ctx.predict_cov(ls[0], q300)
    c4 = ctx.predict_cov(ls[0], q129)
    np.testing.assert_array_equal(c4[0], c1[0])
    np.testing.assert_array_equal(c4[1], c1[1])
    np.testing.assert_array_equal(ctx.predict(ls[0], q300)[0], p1[0])


def test_not_positive_definite_leaves_outputs_untouched(ctx):
    """The first two training points identical with e = 0, d = 1 (one coordinate: the builder's
    |a|^2 + |b|^2 - 2 a.b is then exactly 0, so K's leading 2x2 block is exactly [[1, 1], [1, 1]] and
    the second pivot exactly 0 under any summation order). LinAlgError, the caller's buffers
    untouched, and the next call is clean."""
    import ctypes
    import gpfit._lib as L
    x, y, e, ls, q = _case(128, 1, 128)
    xb, eb = x.copy(), e.copy()
    xb[:, 1] = xb[:, 0]
    eb[:2] = 0.0
    with pytest.raises(np.linalg.LinAlgError):
        np.linalg.cholesky(_kernel(xb, xb, ls[0]) + np.diag(eb ** 2))
    ctx.set_data(xb, y, eb)
    with pytest.raises(np.linalg.LinAlgError, match="Matrix is not positive definite"):
        ctx.predict_cov(ls[0], q)
    M = q.shape[1]
    mu, cov = np.full(M, -7.25), np.full((M, M), -7.25)
    l0, qc = np.ascontiguousarray(ls[0]), np.ascontiguousarray(q)
    dp = ctypes.POINTER(ctypes.c_double)
    rc = ctx.lib.gpf_predict_cov(ctx._h, l0.ctypes.data_as(dp), qc.ctypes.data_as(dp), M, mu.ctypes.data_as(dp),
                                 cov.ctypes.data_as(dp))
    assert rc == L.GPF_NOT_PD
    assert np.all(mu == -7.25) and np.all(cov == -7.25)
    _check_case(ctx, 128, 1, 128, rows=(0,))


def test_arguments():
    import gpfit
    c = gpfit.Context(0)
    try:
        x, y, e, ls, q = _case(129, 2, 5)
        with pytest.raises(ValueError, match="gpf_set_data"):
            c.predict_cov(ls[0], q)
        c.set_data(x, y, e)
        mu, cov = c.predict_cov(ls[0], np.empty((2, 0)))
        assert mu.shape == (0,) and cov.shape == (0, 0)
        for v in (-0.1, 0.0, np.nan, np.inf):
            l = ls[0].copy()
            l[1] = v
            with pytest.raises(ValueError, match="finite and > 0"):
                c.predict_cov(l, q)
        mu, cov = c.predict_cov(ls[0], q)  # the context is clean after the refusals
        np.testing.assert_array_equal(mu, c.predict(ls[0], q)[0])
        np.testing.assert_array_equal(cov, cov.T)
    finally:
        c.close()


def test_draws_plumbing():
    """GP_func.GP_draws: shape, the same bits on a second call, and equal to draws_from on GP_cov's
    (mu, cov) with the same normals."""
    import GP_func
    from gpfit.posterior import draws_from
    x, y, e, ls, q = _case(300, 2, 64)
    d1 = GP_func.GP_draws(x, y, e, q, ls[0], 3, seed=11)
    d2 = GP_func.GP_draws(x, y, e, q, ls[0], 3, seed=11)
    assert d1.shape == (3, 64) and np.all(np.isfinite(d1))
    np.testing.assert_array_equal(d1, d2)
    z = np.random.default_rng(11).standard_normal((3, 64))
    mu, cov = GP_func.GP_cov(x, y, e, q, ls[0])
    d3, info = draws_from(mu, cov, z=z)
    np.testing.assert_array_equal(d1, d3)
    assert info["jitter"] <= 1e-6
    assert not np.array_equal(d1, GP_func.GP_draws(x, y, e, q, ls[0], 3, seed=12))
