"""gpf_predict_conditioned (the latent posterior at M query points conditioned on R measured linear
functionals: gpf_predict_linear's pipeline, then k_con_tn, k_con_h, the dense Cholesky of H, k_dc_inv_*,
k_con_g and per chunk k_predict_vsq, k_con_tn, k_lin_nn, k_con_out) against the float64 NumPy closed form
written below.

Inputs: data and queries of test_predict_cov_gpu._case, weights of test_predict_linear_gpu._weights,
s_r = 0.02 + 0.03 (r mod 5), b = A (sin 3 q0 + q1) + s randn from default_rng(99 + R) (no q1 term at d = 1).

Tolerances: max |mu' - ref| / max(1, max |ref|) < 1e-9, max |var' - ref| < 1e-9 absolute (the prior
variance is 1) and |chi2 - ref| / max(1, ref) < 1e-9: the project's standing bound. On the cases below
(the deep one included), length-scale rows 0-2, the float64 closed form as written here differs from the
same formula in np.longdouble by at most 2.0e-12 (mean), 1.9e-13 (variance) and 1.5e-12 (chi2), so 1e-9
leaves about three orders for a different summation order; cond(H) is between 1 and 606; the smallest
conditioned variance is 1.1e-4 (2.0e-4 without the deep case), so the 1e-12 clip never acts; and the
conditioning moves the mean by up to 1.45 and the variance by up to 0.84, so a kernel that does nothing
cannot pass (measured on the CPU). The measured
maxima are printed (run with -s) and sit in the assert messages; on one MI355X: the mean within 3.8e-13,
the variance within 5.1e-14, chi2 within 2.8e-12, a point functional against predict() on the augmented
data set within 4.3e-14 (profiles/predict_conditioned/pytest_gpu.log).
"""
import ctypes

import numpy as np
import pytest

from test_predict_cov_gpu import _case, _kernel, _reference as _posterior_reference
from test_predict_linear_gpu import _weights

pytestmark = pytest.mark.gpu

TOL = 1e-9


@pytest.fixture(scope="module")
def ctx():
    import gpfit
    c = gpfit.Context(0)
    yield c
    c.close()


def _measurements(q, A):
    """(b, s) of the recipe above for the queries q (d, M) and the weights A (R, M)."""
    R = A.shape[0]
    s = 0.02 + 0.03 * (np.arange(R) % 5)
    f = np.sin(3.0 * q[0]) + (q[1] if q.shape[0] > 1 else 0.0)
    return A @ f + s * np.random.default_rng(99 + R).standard_normal(R), s


_REF = {}


def _reference(N, d, M, R, row):
    """(mu', var', chi2, mu, var) of the closed form for length-scale row `row`, computed once per case
    and shared (the unconditioned posterior is test_predict_cov_gpu's reference)."""
    key = (N, d, M, R, row)
    if key not in _REF:
        q = _case(N, d, M)[4]
        A = _weights(M, R)
        b, s = _measurements(q, A)
        mu, cov = _posterior_reference(N, d, M, row)
        C = cov @ A.T
        Lh = np.linalg.cholesky(A @ C + np.diag(s * s))
        E = np.linalg.solve(Lh, C.T).T
        g = np.linalg.solve(Lh, b - A @ mu)
        out = (mu + E @ g, np.diag(cov) - np.sum(E * E, axis=1), float(g @ g), mu, np.diag(cov).copy())
        for a in out:
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _REF[key] = out
    return _REF[key]


def _check_case(ctx, N, d, M, R, chunk=0, rows=(0, 1, 2)):
    x, y, e, ls, q = _case(N, d, M)
    A = _weights(M, R)
    b, s = _measurements(q, A)
    ctx.set_data(x, y, e)
    out = []
    for row in rows:
        tag = f"N={N} d={d} M={M} R={R} chunk={chunk} ls row {row}"
        mu_r, var_r, chi_r, mu0, var0 = _reference(N, d, M, R, row)
        mu, sd, info = ctx.predict_conditioned(ls[row], q, A, b, s, chunk=chunk)
        assert mu.shape == (M,) and sd.shape == (M,)
        em = np.max(np.abs(mu - mu_r)) / max(1.0, np.max(np.abs(mu_r)))
        ev = np.max(np.abs(sd * sd - var_r))
        ec = abs(info["chi2"] - chi_r) / max(1.0, chi_r)
        print(f"[predict_conditioned] {tag}: mean err {em:.3e}, var err {ev:.3e}, chi2 err {ec:.3e} (chi2 {chi_r:.3f}), "
              f"min var' {np.min(var_r):.3e}, moved mean {np.max(np.abs(mu_r - mu0)):.3f}, "
              f"var {np.max(np.abs(var_r - var0)):.3f} (tol {TOL:.0e})")
        assert em < TOL, f"{tag}: max |mu' - ref| / max(1, max |ref|) = {em:.3e}"
        assert ev < TOL, f"{tag}: max |var' - ref| = {ev:.3e}"
        assert ec < TOL, f"{tag}: |chi2 - ref| / max(1, ref) = {ec:.3e}"
        out.append((mu, sd, info["chi2"]))
    return out


@pytest.mark.parametrize("N,d,M,R", [(129, 2, 1, 1), (1, 2, 129, 2), (128, 1, 128, 128), (300, 2, 700, 6),
                                     (257, 3, 300, 130), (200, 2, 400, 300)])
def test_tile_boundaries_vs_closed_form(ctx, N, d, M, R):
    """(257, 3, 300, 130): two block rows of the inverse; (200, 2, 400, 300): three, so the sum inside
    the inverse is exercised."""
    _check_case(ctx, N, d, M, R)


def test_chunking(ctx):
    """chunk=128: six passes, the last ragged; chunk=256: three; each against the closed form, and the
    spread between the chunkings (they may differ in the last bits)."""
    c0 = _check_case(ctx, 300, 2, 700, 6, chunk=0)
    c128 = _check_case(ctx, 300, 2, 700, 6, chunk=128)
    c256 = _check_case(ctx, 300, 2, 700, 6, chunk=256)
    for row in range(3):
        sp = [max(np.max(np.abs(a[row][k] - b[row][k])) for a, b in ((c0, c128), (c0, c256), (c128, c256))) for k in range(3)]
        print(f"[predict_conditioned] chunkings 0 / 128 / 256, ls row {row}: spread mean {sp[0]:.3e}, sd {sp[1]:.3e}, "
              f"chi2 {sp[2]:.3e}")
    # a chunk that is no multiple of the tile is rounded up to one: the bits of chunk=128
    x, y, e, ls, q = _case(300, 2, 700)
    A = _weights(700, 6)
    b, s = _measurements(q, A)
    mu, sd, info = ctx.predict_conditioned(ls[0], q, A, b, s, chunk=100)
    np.testing.assert_array_equal(mu, c128[0][0])
    np.testing.assert_array_equal(sd, c128[0][1])
    assert info["chi2"] == c128[0][2]


def test_deep(ctx):
    """Nine depth tiles of the factor, three chunks of query points."""
    _check_case(ctx, 1100, 3, 1500, 6, chunk=512)


def test_augmentation_on_device(ctx):
    """Conditioning on one point functional (q_j, b, s) equals adding the training point (q_j, b, s):
    predict() on the 201-point data set, at all M = 300 queries."""
    N, d, M, j = 200, 2, 300, 100
    x, y, e, ls, q = _case(N, d, M)
    assert np.min(np.sum((x - q[:, j:j + 1]) ** 2, axis=0)) > 1e-6  # not a training point
    bj, sj = 0.4, 0.1
    A = np.zeros((1, M))
    A[0, j] = 1.0
    for row in range(3):
        ctx.set_data(x, y, e)
        mu, sd, info = ctx.predict_conditioned(ls[row], q, A, [bj], [sj])
        mu0, sd0 = ctx.predict(ls[row], q)
        ctx.set_data(np.hstack([x, q[:, j:j + 1]]), np.append(y, bj), np.append(e, sj))
        mu_a, sd_a = ctx.predict(ls[row], q)
        em = np.max(np.abs(mu - mu_a)) / max(1.0, np.max(np.abs(mu_a)))
        es = np.max(np.abs(sd - sd_a))
        print(f"[predict_conditioned] augmentation N={N}+1 M={M} ls row {row}: mean {em:.3e}, sd {es:.3e}, "
              f"moved mean {np.max(np.abs(mu - mu0)):.3e}, sd {np.max(np.abs(sd - sd0)):.3e}")
        assert em < TOL, f"ls row {row}: mean vs the augmented data set {em:.3e}"
        assert es < TOL, f"ls row {row}: sd vs the augmented data set {es:.3e}"
        # the comparison can tell the conditioned posterior from the plain one: both moved by far more than TOL
        assert np.max(np.abs(mu - mu0)) > 1e3 * TOL and np.max(np.abs(sd - sd0)) > 1e3 * TOL


def test_exact_constraint(ctx):
    """R = 1, s = 0, a single point functional: the point takes the value, with no variance left (the
    clip puts sd's floor at 1e-6)."""
    N, d, M, j = 200, 2, 300, 100
    x, y, e, ls, q = _case(N, d, M)
    ctx.set_data(x, y, e)
    A = np.zeros((1, M))
    A[0, j] = 1.0
    for row in range(3):
        mu, sd, info = ctx.predict_conditioned(ls[row], q, A, [0.4], [0.0])
        print(f"[predict_conditioned] exact constraint ls row {row}: |mu'[j] - b| {abs(mu[j] - 0.4):.3e}, sd'[j] {sd[j]:.3e}")
        assert abs(mu[j] - 0.4) < TOL, f"ls row {row}: mu'[j] - b = {mu[j] - 0.4:.3e}"
        assert sd[j] < 2e-6, f"ls row {row}: sd'[j] = {sd[j]:.3e}"


def test_functionals_are_bitwise_predict_linear(ctx):
    for (N, d, M, R, chunk) in ((300, 2, 700, 6, 0), (300, 2, 700, 6, 128), (257, 3, 300, 130, 256)):
        x, y, e, ls, q = _case(N, d, M)
        A = _weights(M, R)
        b, s = _measurements(q, A)
        ctx.set_data(x, y, e)
        info = ctx.predict_conditioned(ls[0], q, A, b, s, chunk=chunk, want_functionals=True)[2]
        mean, cov = ctx.predict_linear(ls[0], q, A, chunk=chunk)
        np.testing.assert_array_equal(info["fmean"], mean)
        np.testing.assert_array_equal(info["fcov"], cov)


def test_repeatability_and_non_interference(ctx):
    """predict, predict_linear, predict_cov before and after conditioned calls (of other sizes too) on one
    context: each keeps its own bits, and a repeated conditioned call gives the same bits."""
    x, y, e, ls, q = _case(300, 2, 300)
    q129 = _case(300, 2, 129)[4]
    A = _weights(300, 6)
    b, s = _measurements(q, A)
    ctx.set_data(x, y, e)
    p1 = ctx.predict(ls[0], q)
    l1 = ctx.predict_linear(ls[0], q, A, chunk=128, want_prior=True)
    c1 = ctx.predict_cov(ls[0], q129)
    n1 = ctx.predict_conditioned(ls[0], q, A, b, s, chunk=128, want_functionals=True)
    # a wider conditioned call in between: the kept buffers regrow, then are wider than needed
    q7, A7 = _case(300, 2, 700)[4], _weights(700, 130)
    ctx.predict_conditioned(ls[1], q7, A7, *_measurements(q7, A7))
    n2 = ctx.predict_conditioned(ls[0], q, A, b, s, chunk=128, want_functionals=True)
    p2 = ctx.predict(ls[0], q)
    l2 = ctx.predict_linear(ls[0], q, A, chunk=128, want_prior=True)
    c2 = ctx.predict_cov(ls[0], q129)
    for a, b_ in zip(p1 + l1 + c1, p2 + l2 + c2):
        np.testing.assert_array_equal(a, b_)
    np.testing.assert_array_equal(n1[0], n2[0])
    np.testing.assert_array_equal(n1[1], n2[1])
    assert n1[2]["chi2"] == n2[2]["chi2"]
    np.testing.assert_array_equal(n1[2]["fmean"], n2[2]["fmean"])
    np.testing.assert_array_equal(n1[2]["fcov"], n2[2]["fcov"])


def test_errors_and_contract(ctx):
    import gpfit._lib as L
    N, d, M = 129, 2, 140
    x, y, e, ls, q = _case(N, d, M)
    A = _weights(M, 4)
    b, s = _measurements(q, A)
    ctx.set_data(x, y, e)
    with pytest.raises(ValueError, match="R > 1024"):
        ctx.predict_conditioned(ls[0], q, np.zeros((1025, M)), np.zeros(1025), np.ones(1025))
    neg = s.copy()
    neg[2] = -0.1
    with pytest.raises(ValueError, match=">= 0"):
        ctx.predict_conditioned(ls[0], q, A, b, neg)
    nanb = b.copy()
    nanb[1] = np.nan
    with pytest.raises(ValueError, match="finite"):
        ctx.predict_conditioned(ls[0], q, A, nanb, s)
    # two identical functionals with zero error, the value at a query so far from the data that its
    # cross-covariance underflows to 0 and its posterior variance is the prior's 1.0 exactly: H is
    # [[1, 1], [1, 1]] and its second pivot exactly 0. LinAlgError, the caller's buffers untouched, the
    # last-error text names H, and the next call is clean
    dup = np.zeros((2, M))
    dup[:, 100] = 1.0
    qfar = q.copy()
    qfar[:, 100] = 50.0
    with pytest.raises(np.linalg.LinAlgError):
        ctx.predict_conditioned(ls[0], qfar, dup, [0.3, 0.3], [0.0, 0.0])
    dp = ctypes.POINTER(ctypes.c_double)
    l0, qc = np.ascontiguousarray(ls[0]), np.ascontiguousarray(qfar)
    b2, s2 = np.array([0.3, 0.3]), np.zeros(2)
    mu, sd, fm, fc = np.full(M, -7.25), np.full(M, -7.25), np.full(2, -7.25), np.full((2, 2), -7.25)
    chi = ctypes.c_double(-7.25)

    def call(m, r):
        return ctx.lib.gpf_predict_conditioned(ctx._h, l0.ctypes.data_as(dp), qc.ctypes.data_as(dp), m, dup.ctypes.data_as(dp),
                                               r, b2.ctypes.data_as(dp), s2.ctypes.data_as(dp), 0, mu.ctypes.data_as(dp),
                                               sd.ctypes.data_as(dp), fm.ctypes.data_as(dp), fc.ctypes.data_as(dp),
                                               ctypes.byref(chi))

    def untouched():
        return (np.all(mu == -7.25) and np.all(sd == -7.25) and np.all(fm == -7.25) and np.all(fc == -7.25)
                and chi.value == -7.25)

    assert call(M, 2) == L.GPF_NOT_PD
    assert untouched()
    assert b"H = A Sigma A^T" in ctx.lib.gpf_last_error(ctx._h)
    # M == 0 and R == 0 write nothing
    assert call(0, 2) == L.GPF_OK and call(M, 0) == L.GPF_OK
    assert untouched()
    assert call(-1, 2) == L.GPF_BAD_ARG and call(M, -1) == L.GPF_BAD_ARG
    assert untouched()
    mu0, sd0, info = ctx.predict_conditioned(ls[0], q, np.empty((0, M)), [], [])   # R == 0: the plain prediction
    for a, b_ in zip((mu0, sd0), ctx.predict(ls[0], q)):
        np.testing.assert_array_equal(a, b_)
    _check_case(ctx, 300, 2, 700, 6, rows=(0,))


def test_not_positive_definite_training_covariance(ctx):
    """test_predict_cov_gpu's construction: the first two training points identical with e = 0, d = 1.
    LinAlgError, the last-error text names the training covariance."""
    x, y, e, ls, q = _case(128, 1, 128)
    A = _weights(128, 6)
    b, s = _measurements(q, A)
    xb, eb = x.copy(), e.copy()
    xb[:, 1] = xb[:, 0]
    eb[:2] = 0.0
    ctx.set_data(xb, y, eb)
    with pytest.raises(np.linalg.LinAlgError):
        ctx.predict_conditioned(ls[0], q, A, b, s)
    assert b"training points" in ctx.lib.gpf_last_error(ctx._h)
    _check_case(ctx, 128, 1, 128, 128, rows=(0,))


def test_routes_agree(ctx):
    """method="stream" and method="dense" of gpfit.conditioned.predict_conditioned, and GP_func.GP_conditioned."""
    import GP_func
    from gpfit.conditioned import predict_conditioned
    x, y, e, ls, q = _case(300, 2, 700)
    A = _weights(700, 6)
    b, s = _measurements(q, A)
    ms, ss, info_s = predict_conditioned(x, y, e, q, ls[0], A, b, s, method="stream", ctx=ctx)
    md, sdd, info_d = predict_conditioned(x, y, e, q, ls[0], A, b, s, method="dense", ctx=ctx)
    assert info_s["method"] == "stream" and info_d["method"] == "dense"
    em = np.max(np.abs(ms - md)) / max(1.0, np.max(np.abs(md)))
    ev = np.max(np.abs(ss * ss - sdd * sdd))
    ec = abs(info_s["chi2"] - info_d["chi2"]) / max(1.0, info_d["chi2"])
    print(f"[predict_conditioned] stream vs dense N=300 d=2 M=700 R=6: mean {em:.3e}, var {ev:.3e}, chi2 {ec:.3e}")
    assert em < TOL and ev < TOL and ec < TOL, (em, ev, ec)
    mu, sd = GP_func.GP_conditioned(x, y, e, q, ls[0], A, b, s)
    assert np.max(np.abs(mu - md)) / max(1.0, np.max(np.abs(md))) < TOL and np.max(np.abs(sd * sd - sdd * sdd)) < TOL
