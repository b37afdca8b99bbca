"""gpf_predict_linear (R linear functionals of the latent posterior over M query points, the query
axis folded away on the device: k_lin_nn, k_lin_tn, k_lin_reduce behind k_cross_cov, with k_predict_v
and k_mirror_lower) against the float64 NumPy closed form written below.

Tolerances: max |cov - ref| / s < 1e-9 with s = max diag(A K_ss A^T), the prior scale of the
functionals (1.0-2.0 for these weights); the same bound for the prior term A K_ss A^T alone; and
max |mean - ref| / max(1, max |ref|) < 1e-9: the project's bound for the LML, its gradient and
predict_cov. On this recipe the float64 closed form differs from the same formula in np.longdouble by
at most 2.6e-14 (cov / s) and 4.1e-13 (mean), measured on the CPU for (N, d, M, R) = (300, 2, 700, 6),
(257, 3, 300, 130), (129, 2, 1, 1) and (1100, 3, 1500, 6), length-scale rows 0-2, where the smallest
posterior variance is 2e-5: 1e-9 leaves about four orders for a different summation order. The
measured maxima are printed (run with -s) and sit in the assert messages; one MI355X's are in
profiles/predict_linear/pytest_gpu.log.
"""
import ctypes

import numpy as np
import pytest

from test_predict_cov_gpu import _case, _kernel   # _case: the data of test_lml_grad_gpu._recipe(N, d) and the queries

pytestmark = pytest.mark.gpu

TOL = 1e-9


@pytest.fixture(scope="module")
def ctx():
    import gpfit
    c = gpfit.Context(0)
    yield c
    c.close()


def _weights(M, R):
    """The first R rows that exist of: the mean of all points; the mean of the first M // 2; the last
    point alone; q0 - q1; then random subsets (default_rng(7), probability 0.3 plus one forced member)
    with U(0.5, 1.5) weights normalised to sum 1."""
    rows = [np.full(M, 1.0 / M)]
    if M // 2 >= 1:
        r = np.zeros(M)
        r[:M // 2] = 1.0 / (M // 2)
        rows.append(r)
    r = np.zeros(M)
    r[-1] = 1.0
    rows.append(r)
    if M >= 2:
        r = np.zeros(M)
        r[0], r[1] = 1.0, -1.0
        rows.append(r)
    rng = np.random.default_rng(7)
    while len(rows) < R:
        member = rng.random(M) < 0.3
        member[rng.integers(M)] = True
        r = rng.uniform(0.5, 1.5, M) * member
        rows.append(r / r.sum())
    assert len(rows) >= R
    return np.ascontiguousarray(np.stack(rows[:R]))


_REF = {}


def _reference(N, d, M, R, row):
    """(mean, cov, prior) of the closed form for length-scale row `row`, computed once per case and shared."""
    key = (N, d, M, R, row)
    if key not in _REF:
        x, y, e, ls, q = _case(N, d, M)
        A = _weights(M, R)
        l = ls[row]
        Kn = _kernel(x, x, l) + np.diag(e ** 2)
        L = np.linalg.cholesky(Kn)
        V = np.linalg.solve(L, _kernel(x, q, l) @ A.T)
        Kss = _kernel(q, q, l)
        np.fill_diagonal(Kss, 1.0)
        prior = A @ Kss @ A.T
        cov = prior - V.T @ V
        mean = V.T @ np.linalg.solve(L, y)
        for a in (mean, cov, prior):
            a.setflags(write=False)
        _REF[key] = (mean, cov, prior)
    return _REF[key]


def _errors(got, ref):
    (mean, cov, prior), (mean_r, cov_r, prior_r) = got, ref
    s = np.max(np.diag(prior_r))
    return (np.max(np.abs(cov - cov_r)) / s, np.max(np.abs(prior - prior_r)) / s,
            np.max(np.abs(mean - mean_r)) / max(1.0, np.max(np.abs(mean_r))), s)


def _check_case(ctx, N, d, M, R, chunk=0, rows=(0, 1, 2)):
    x, y, e, ls, q = _case(N, d, M)
    A = _weights(M, R)
    ctx.set_data(x, y, e)
    out = []
    for row in rows:
        tag = f"N={N} d={d} M={M} R={R} chunk={chunk} ls row {row}"
        got = ctx.predict_linear(ls[row], q, A, chunk=chunk, want_prior=True)
        assert got[0].shape == (R,) and got[1].shape == (R, R) and got[2].shape == (R, R)
        ec, ep, em, s = _errors(got, _reference(N, d, M, R, row))
        print(f"[predict_linear] {tag}: cov err / s {ec:.3e}, prior err / s {ep:.3e}, mean err {em:.3e}, s {s:.3f}, "
              f"min diag cov {np.min(np.diag(got[1])):.3e} (tol {TOL:.0e})")
        assert ec < TOL, f"{tag}: max |cov - ref| / s = {ec:.3e}"
        assert ep < TOL, f"{tag}: max |prior - ref| / s = {ep:.3e}"
        assert em < TOL, f"{tag}: mean error {em:.3e}"
        np.testing.assert_array_equal(got[1], got[1].T, err_msg=f"{tag}: cov is not exactly symmetric")
        np.testing.assert_array_equal(got[2], got[2].T, err_msg=f"{tag}: prior is not exactly symmetric")
        out.append(got)
    return out


@pytest.mark.parametrize("N,d,M,R", [(129, 2, 1, 1), (1, 2, 129, 2), (128, 1, 128, 128), (300, 2, 700, 6),
                                     (257, 3, 300, 130)])
def test_tile_boundaries_vs_closed_form(ctx, N, d, M, R):
    _check_case(ctx, N, d, M, R)


def test_chunking(ctx):
    """chunk=128: six passes, the last ragged, and 36 block pairs; chunk=256: three; each against the
    closed form, and the spread between the chunkings (they may differ in the last bits)."""
    c0 = _check_case(ctx, 300, 2, 700, 6, chunk=0)
    c128 = _check_case(ctx, 300, 2, 700, 6, chunk=128)
    c256 = _check_case(ctx, 300, 2, 700, 6, chunk=256)
    for row in range(3):
        sp = [max(np.max(np.abs(a[row][k] - b[row][k])) for a, b in ((c0, c128), (c0, c256), (c128, c256))) for k in range(3)]
        print(f"[predict_linear] chunkings 0 / 128 / 256, ls row {row}: spread mean {sp[0]:.3e}, cov {sp[1]:.3e}, "
              f"prior {sp[2]:.3e}")
    # a chunk that is no multiple of the tile is rounded up to one: the bits of chunk=128
    x, y, e, ls, q = _case(300, 2, 700)
    got = ctx.predict_linear(ls[0], q, _weights(700, 6), chunk=100, want_prior=True)
    for a, b in zip(got, c128[0]):
        np.testing.assert_array_equal(a, b)


def test_deep(ctx):
    """Nine depth tiles of the factor, three chunks of query points."""
    _check_case(ctx, 1100, 3, 1500, 6, chunk=512)


def test_against_dense_route_on_device(ctx):
    from gpfit.linear import functionals_from
    N, d, M, R = 257, 3, 300, 6
    x, y, e, ls, q = _case(N, d, M)
    A = _weights(M, R)
    ctx.set_data(x, y, e)
    for row in range(3):
        mean, cov, prior = ctx.predict_linear(ls[row], q, A, want_prior=True)
        mean_d, cov_d = functionals_from(*ctx.predict_cov(ls[row], q), A)
        s = np.max(np.diag(_reference(N, d, M, R, row)[2]))
        ec = np.max(np.abs(cov - cov_d)) / s
        em = np.max(np.abs(mean - mean_d)) / max(1.0, np.max(np.abs(mean_d)))
        print(f"[predict_linear] vs dense route N={N} d={d} M={M} R={R} ls row {row}: cov {ec:.3e}, mean {em:.3e}")
        assert ec < TOL, f"ls row {row}: max |cov - dense| / s = {ec:.3e}"
        assert em < TOL, f"ls row {row}: mean vs dense {em:.3e}"
    # identity weights: the functionals are the points themselves
    N, d, M = 300, 2, 130
    x, y, e, ls, q = _case(N, d, M)
    ctx.set_data(x, y, e)
    for row in range(3):
        mean, cov, prior = ctx.predict_linear(ls[row], q, np.eye(M), want_prior=True)
        mu, sig = ctx.predict_cov(ls[row], q)
        ec, em = np.max(np.abs(cov - sig)), np.max(np.abs(mean - mu)) / max(1.0, np.max(np.abs(mu)))
        print(f"[predict_linear] identity weights N={N} d={d} M={M} ls row {row}: cov {ec:.3e}, mean {em:.3e}")
        assert ec < TOL, f"ls row {row}: max |cov - predict_cov's| = {ec:.3e}"
        assert em < TOL, f"ls row {row}: mean vs predict_cov's {em:.3e}"
        np.testing.assert_array_equal(np.diag(prior), np.ones(M))


def test_repeatability_and_non_interference(ctx):
    """predict, predict_cov and predict_linear interleaved on one context, with calls of other sizes in
    between: each keeps its own bits."""
    x, y, e, ls, q = _case(300, 2, 300)
    q129 = _case(300, 2, 129)[4]
    A, A129 = _weights(300, 6), _weights(129, 5)
    ctx.set_data(x, y, e)
    p1 = ctx.predict(ls[0], q)
    l1 = ctx.predict_linear(ls[0], q, A, chunk=128, want_prior=True)
    c1 = ctx.predict_cov(ls[0], q129)
    l2 = ctx.predict_linear(ls[0], q, A, chunk=128, want_prior=True)
    p2 = ctx.predict(ls[0], q)
    c2 = ctx.predict_cov(ls[0], q129)
    for a, b in zip(p1 + c1 + l1, p2 + c2 + l2):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(l1[1], l1[1].T)
    np.testing.assert_array_equal(l1[2], l1[2].T)
    # a wider call and a narrower one in between: the kept buffers regrow or are wider than needed
    ctx.predict_linear(ls[1], _case(300, 2, 700)[4], _weights(700, 130))
    n1 = ctx.predict_linear(ls[0], q129, A129, want_prior=True)
    l3 = ctx.predict_linear(ls[0], q, A, chunk=128, want_prior=True)
    for a, b in zip(l1, l3):
        np.testing.assert_array_equal(a, b)
    for a, b in zip(n1, ctx.predict_linear(ls[0], q129, A129, want_prior=True)):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(ctx.predict_cov(ls[0], q129)[1], c1[1])
    np.testing.assert_array_equal(ctx.predict(ls[0], q)[0], p1[0])
    # without the prior the mean and the covariance are the same bits
    for a, b in zip(ctx.predict_linear(ls[0], q, A, chunk=128), l1[:2]):
        np.testing.assert_array_equal(a, b)


def test_not_positive_definite_leaves_outputs_untouched(ctx):
    """test_predict_cov_gpu's construction: the first two training points identical with e = 0, d = 1,
    so the second pivot is exactly 0. LinAlgError, the caller's buffers untouched, the next call clean."""
    import gpfit._lib as L
    x, y, e, ls, q = _case(128, 1, 128)
    A = _weights(128, 6)
    xb, eb = x.copy(), e.copy()
    xb[:, 1] = xb[:, 0]
    eb[:2] = 0.0
    with pytest.raises(np.linalg.LinAlgError):
        np.linalg.cholesky(_kernel(xb, xb, ls[0]) + np.diag(eb ** 2))
    ctx.set_data(xb, y, eb)
    with pytest.raises(np.linalg.LinAlgError, match="Matrix is not positive definite"):
        ctx.predict_linear(ls[0], q, A)
    mean, cov, prior = np.full(6, -7.25), np.full((6, 6), -7.25), np.full((6, 6), -7.25)
    l0, qc = np.ascontiguousarray(ls[0]), np.ascontiguousarray(q)
    dp = ctypes.POINTER(ctypes.c_double)
    rc = ctx.lib.gpf_predict_linear(ctx._h, l0.ctypes.data_as(dp), qc.ctypes.data_as(dp), 128, A.ctypes.data_as(dp), 6, 0,
                                    mean.ctypes.data_as(dp), cov.ctypes.data_as(dp), prior.ctypes.data_as(dp))
    assert rc == L.GPF_NOT_PD
    assert np.all(mean == -7.25) and np.all(cov == -7.25) and np.all(prior == -7.25)
    _check_case(ctx, 128, 1, 128, 6, rows=(0,))


def test_contract():
    import gpfit
    import gpfit._lib as L
    c = gpfit.Context(0)
    try:
        x, y, e, ls, q = _case(129, 2, 5)
        A = _weights(5, 4)
        with pytest.raises(ValueError, match="gpf_set_data"):
            c.predict_linear(ls[0], q, A)
        c.set_data(x, y, e)
        mean, cov = c.predict_linear(ls[0], np.empty((2, 0)), np.empty((3, 0)))   # M == 0
        assert mean.shape == (3,) and cov.shape == (3, 3)
        mean, cov, prior = c.predict_linear(ls[0], q, np.empty((0, 5)), want_prior=True)   # R == 0
        assert mean.shape == (0,) and cov.shape == (0, 0) and prior.shape == (0, 0)
        for v in (np.nan, np.inf, -np.inf):
            bad = A.copy()
            bad[3, 4] = v
            with pytest.raises(ValueError, match="finite"):
                c.predict_linear(ls[0], q, bad)
        with pytest.raises(ValueError, match=">= 0"):
            c.predict_linear(ls[0], q, A, chunk=-1)
        with pytest.raises(ValueError, match="weights must be"):
            c.predict_linear(ls[0], q, A[:, :4])
        for v in (-0.1, 0.0, np.nan, np.inf):
            l = ls[0].copy()
            l[1] = v
            with pytest.raises(ValueError, match="finite and > 0"):
                c.predict_linear(l, q, A)
        # R < 0 cannot come from an array's shape: the C entry point itself, outputs untouched
        dp = ctypes.POINTER(ctypes.c_double)
        l0, qc = np.ascontiguousarray(ls[0]), np.ascontiguousarray(q)
        mean, cov = np.full(4, -7.25), np.full((4, 4), -7.25)
        for m, r, ch in ((5, -1, 0), (-1, 4, 0), (5, 4, -128)):
            rc = c.lib.gpf_predict_linear(c._h, l0.ctypes.data_as(dp), qc.ctypes.data_as(dp), m, A.ctypes.data_as(dp), r, ch,
                                          mean.ctypes.data_as(dp), cov.ctypes.data_as(dp), None)
            assert rc == L.GPF_BAD_ARG, (m, r, ch)
        rc = c.lib.gpf_predict_linear(c._h, l0.ctypes.data_as(dp), qc.ctypes.data_as(dp), 5, A.ctypes.data_as(dp), 4, 0,
                                      mean.ctypes.data_as(dp), None, None)
        assert rc == L.GPF_BAD_ARG
        assert c.lib.gpf_predict_linear(None, None, None, 0, None, 0, 0, None, None, None) == L.GPF_BAD_ARG
        assert np.all(mean == -7.25) and np.all(cov == -7.25)
        # the context is clean after the refusals
        mean, cov = c.predict_linear(ls[0], q, A)
        mu, sig = c.predict_cov(ls[0], q)
        assert np.max(np.abs(mean - A @ mu)) < TOL and np.max(np.abs(cov - A @ sig @ A.T)) < TOL
    finally:
        c.close()


def test_gp_func_and_region_weights():
    """GP_func.GP_linear with region_weights' boxes: the stream and the dense route of
    gpfit.linear.predict_linear agree, and the variance of a region's mean is below its prior's."""
    import GP_func
    from gpfit.linear import predict_linear, region_weights
    x, y, e, ls, q = _case(300, 2, 300)
    W = region_weights(q, [[(-0.1, 1.1), (-0.1, 1.1)], [(0.0, 0.5), (0.0, 0.5)], [(0.5, 1.1), (0.2, 0.9)]])
    mean, cov = GP_func.GP_linear(x, y, e, q, ls[0], W)
    ms, cs, info = predict_linear(x, y, e, q, ls[0], W, method="stream")
    md, cd, info_d = predict_linear(x, y, e, q, ls[0], W, method="dense")
    assert info["method"] == "stream" and info_d["method"] == "dense"
    np.testing.assert_array_equal(mean, ms)
    np.testing.assert_array_equal(cov, cs)
    s = np.max(np.diag(info["prior"]))
    ec, em = np.max(np.abs(cs - cd)) / s, np.max(np.abs(ms - md)) / max(1.0, np.max(np.abs(md)))
    print(f"[predict_linear] GP_linear regions: stream vs dense cov {ec:.3e}, mean {em:.3e}")
    assert ec < TOL and em < TOL, (ec, em)
    assert np.all(np.diag(cs) < np.diag(info["prior"]))
