"""gpf_posterior_draws (Context.posterior_draws, sample_posterior(method="device")): joint posterior
draws with Sigma, its factor and the product mu + z L^T on the device (gpf_densechol.hip: the dense
factorisation and k_draws), against gpf_predict_cov's (mu, Sigma) and the host path.

Bounds, u = 2^-53 (derived, not tuned):
  factor   max |L L^T - (Sigma + jitter I)| <= 8 M u sqrt(cond_2(Sigma + jitter I)) max diag (the
           reconstruction bound of tests/test_dense_chol_gpu.py);
  product  |draws - (mu + z L^T)| <= 4 (M + 1) u (|z| |L|^T) + 4 u |mu| elementwise: a dot product of
           length M and one addition in either summation order;
  host     |draws - draws_host| <= 8 M u cond_2 max |z| max |L_np| on a case with cond_2 <= 1e7: the
           factor bound of tests/test_dense_chol_gpu.py times the row sum of |z|.
The measured maxima are printed (run with -s) and kept in profiles/posterior_draws/pytest_gpu.log.
"""
import ctypes

import numpy as np
import pytest

from test_predict_cov_gpu import _case, _kernel

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


@pytest.fixture(scope="module")
def ctx():
    import gpfit
    c = gpfit.Context(0)
    yield c
    c.close()


def _recon_bound(a_j):
    return 8.0 * a_j.shape[0] * U * np.sqrt(np.linalg.cond(a_j, 2)) * np.max(np.diag(a_j))


@pytest.mark.parametrize("N,d,M,S", [(1, 2, 129, 1), (129, 2, 1, 3), (128, 1, 128, 128), (300, 2, 257, 5), (257, 3, 300, 130)])
def test_parity_with_predict_cov(ctx, N, d, M, S):
    from gpfit.posterior import JITTERS
    x, y, e, ls, q = _case(N, d, M)
    z = np.random.default_rng(500 + S).standard_normal((S, M))
    ctx.set_data(x, y, e)
    mu_c, cov = ctx.predict_cov(ls[0], q)
    mu, draws, info = ctx.posterior_draws(ls[0], q, z, want_chol=True)
    L = info["chol"]
    assert mu.shape == (M,) and draws.shape == (S, M) and L.shape == (M, M)
    assert info["jitter"] in JITTERS and info["tries"] == JITTERS.index(info["jitter"]) + 1
    np.testing.assert_array_equal(mu, mu_c, err_msg="mu is not bitwise predict_cov()'s")
    assert np.all(np.triu(L, 1) == 0.0)
    a_j = cov + info["jitter"] * np.eye(M)
    e_r, b_r = np.max(np.abs(L @ L.T - a_j)), _recon_bound(a_j)
    want = mu + z @ L.T
    bound = 4.0 * (M + 1) * U * (np.abs(z) @ np.abs(L).T) + 4.0 * U * np.abs(mu)
    diff = np.abs(draws - want)
    print(f"[posterior_draws] N={N} d={d} M={M} S={S}: jitter {info['jitter']:.0e}, max |L L^T - (Sigma + jitter I)| = "
          f"{e_r:.3e} (bound {b_r:.3e}), max |draws - (mu + z L^T)| = {np.max(diff):.3e}, largest ratio to its bound "
          f"{np.max(diff / bound):.3e}")
    assert e_r <= b_r
    assert np.all(diff <= bound)


def _well_conditioned():
    """150 training points and 300 queries in [0, 3]^2, l = (0.15, 0.2): cond_2(Sigma + 1e-12 I) = 1.7e6
    with this seed (the queries' nearest pairs decide it: seeds 43-52 give 4e5 to 8e7)."""
    rng = np.random.default_rng(46)
    x = rng.uniform(0.0, 3.0, size=(2, 150))
    y = np.sin(2.0 * x[0]) + np.cos(x[1]) + 0.1 * rng.standard_normal(150)
    q = rng.uniform(0.0, 3.0, size=(2, 300))
    return x, y, np.full(150, 0.1), np.array([0.15, 0.2]), q


_HOST = {}


def _host_reference():
    """(z, draws, info, bound) of the host path on the well-conditioned case, shared and read-only."""
    if not _HOST:
        import gpfit
        from gpfit.posterior import draws_from
        x, y, e, l, q = _well_conditioned()
        c = gpfit.Context(0)
        try:
            c.set_data(x, y, e)
            mu, cov = c.predict_cov(l, q)
        finally:
            c.close()
        a_j = cov + 1e-12 * np.eye(300)
        cond = np.linalg.cond(a_j, 2)
        assert cond <= 1e7, f"the case is not well-conditioned: cond_2 = {cond:.3e}"  # a condition on the input
        z = np.random.default_rng(77).standard_normal((7, 300))
        draws, info = draws_from(mu, cov, z=z)
        bound = 8.0 * 300 * U * cond * np.max(np.abs(z)) * np.max(np.abs(np.linalg.cholesky(a_j)))
        for a in (z, draws):
            a.setflags(write=False)
        _HOST.update(z=z, draws=draws, info=info, bound=bound, cond=cond)
    return _HOST


def test_against_the_host_path(ctx):
    x, y, e, l, q = _well_conditioned()
    ref = _host_reference()
    ctx.set_data(x, y, e)
    mu, draws, info = ctx.posterior_draws(l, q, ref["z"])
    err = np.max(np.abs(draws - ref["draws"]))
    print(f"[posterior_draws] host path: cond_2 {ref['cond']:.3e}, max |draws - draws_host| = {err:.3e} (bound {ref['bound']:.3e})")
    assert info["jitter"] == ref["info"]["jitter"] == 1e-12 and info["tries"] == 1
    assert err <= ref["bound"]


def test_methods_agree_for_a_seed(ctx):
    import GP_func
    from gpfit.posterior import sample_posterior
    x, y, e, l, q = _well_conditioned()
    bound = _host_reference()["bound"] / np.max(np.abs(_host_reference()["z"]))
    dh, ih = sample_posterior(x, y, e, q, l, 4, seed=5, ctx=ctx, method="host")
    dd, idv = sample_posterior(x, y, e, q, l, 4, seed=5, ctx=ctx, method="device")
    zmax = np.max(np.abs(np.random.default_rng(5).standard_normal((4, 300))))
    err = np.max(np.abs(dd - dh))
    print(f"[posterior_draws] methods, seed 5: max |device - host| = {err:.3e} (bound {bound * zmax:.3e})")
    assert idv["jitter"] == ih["jitter"] and idv["tries"] == ih["tries"]
    assert sorted(idv) == ["jitter", "mu", "tries"]
    np.testing.assert_array_equal(idv["mu"], ih["mu"])
    assert dd.shape == (4, 300) and err <= bound * zmax
    g = GP_func.GP_draws(x, y, e, q, l, 4, seed=5, method="device")
    np.testing.assert_array_equal(g, dd)
    np.testing.assert_array_equal(GP_func.GP_draws(x, y, e, q, l, 4, seed=5), dh)


def test_not_positive_definite_training_matrix_leaves_outputs_untouched(ctx):
    """The recipe of tests/test_predict_cov_gpu.py::test_not_positive_definite_leaves_outputs_untouched."""
    import gpfit._lib as lib
    x, y, e, ls, q = _case(128, 1, 128)
    xb, eb = x.copy(), e.copy()
    xb[:, 1] = xb[:, 0]
    eb[:2] = 0.0
    with pytest.raises(np.linalg.LinAlgError):
        np.linalg.cholesky(_kernel(xb, xb, ls[0]) + np.diag(eb ** 2))
    M, S = q.shape[1], 3
    z = np.random.default_rng(1).standard_normal((S, M))
    ctx.set_data(xb, y, eb)
    mu, draws = np.full(M, -7.25), np.full((S, M), -7.25)
    with pytest.raises(np.linalg.LinAlgError, match="Matrix is not positive definite"):
        ctx.posterior_draws(ls[0], q, z, out=(mu, draws))
    assert np.all(mu == -7.25) and np.all(draws == -7.25)
    chol = np.full((M, M), -7.25)
    jit, tries = ctypes.c_double(-1.0), ctypes.c_int(-1)
    jj, l0, qc = np.array(lib.JITTERS), np.ascontiguousarray(ls[0]), np.ascontiguousarray(q)
    dp = ctypes.POINTER(ctypes.c_double)
    rc = ctx.lib.gpf_posterior_draws(ctx._h, l0.ctypes.data_as(dp), qc.ctypes.data_as(dp), M, z.ctypes.data_as(dp), S,
                                     jj.ctypes.data_as(dp), 4, mu.ctypes.data_as(dp), draws.ctypes.data_as(dp),
                                     chol.ctypes.data_as(dp), ctypes.byref(jit), ctypes.byref(tries))
    assert rc == lib.GPF_NOT_PD
    assert np.all(mu == -7.25) and np.all(draws == -7.25) and np.all(chol == -7.25) and jit.value == -1.0
    ctx.set_data(x, y, e)  # the next call is clean
    mu2, d2, _ = ctx.posterior_draws(ls[0], q, z)
    np.testing.assert_array_equal(mu2, ctx.predict_cov(ls[0], q)[0])
    assert np.all(np.isfinite(d2))


def test_repeatability_and_buffer_reuse(ctx):
    """predict, predict_cov and posterior_draws interleaved on one context, with wider calls in
    between: each keeps its own bits."""
    x, y, e, ls, q300 = _case(300, 2, 300)
    q129 = _case(300, 2, 129)[4]
    z129 = np.random.default_rng(2).standard_normal((5, 129))
    z300 = np.random.default_rng(3).standard_normal((130, 300))
    ctx.set_data(x, y, e)
    p1 = ctx.predict(ls[0], q300)
    c1 = ctx.predict_cov(ls[0], q129)
    d1 = ctx.posterior_draws(ls[0], q129, z129, want_chol=True)
    p2 = ctx.predict(ls[0], q300)
    d2 = ctx.posterior_draws(ls[0], q129, z129, want_chol=True)
    c2 = ctx.predict_cov(ls[0], q129)
    for a, b in zip(p1 + c1 + d1[:2], p2 + c2 + d2[:2]):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(d1[2]["chol"], d2[2]["chol"])
    assert d1[2]["jitter"] == d2[2]["jitter"]
    # a wider and taller call in between regrows the kept buffers; the narrower one keeps its bits
    ctx.posterior_draws(ls[0], q300, z300)
    d3 = ctx.posterior_draws(ls[0], q129, z129)
    np.testing.assert_array_equal(d3[0], d1[0])
    np.testing.assert_array_equal(d3[1], d1[1])
    np.testing.assert_array_equal(ctx.predict_cov(ls[0], q129)[1], c1[1])
    np.testing.assert_array_equal(ctx.predict(ls[0], q300)[0], p1[0])


def test_arguments(ctx):
    import gpfit
    x, y, e, ls, q = _case(129, 2, 129)
    z = np.zeros((2, 129))
    ctx.set_data(x, y, e)
    with pytest.raises(ValueError, match="z must be"):
        ctx.posterior_draws(ls[0], q, z[:, :-1])
    with pytest.raises(ValueError, match="jitters"):
        ctx.posterior_draws(ls[0], q, z, jitters=(1e-10, 1e-12))
    with pytest.raises(ValueError, match="finite and > 0"):
        ctx.posterior_draws(np.array([0.3, -1.0]), q, z)
    mu, draws, info = ctx.posterior_draws(ls[0], q[:, :0], np.zeros((2, 0)))
    assert mu.shape == (0,) and draws.shape == (2, 0)
    mu, draws, info = ctx.posterior_draws(ls[0], q, np.zeros((0, 129)))
    assert draws.shape == (0, 129)
    # all-zero normals: every draw is the mean, exactly
    mu, draws, _ = ctx.posterior_draws(ls[0], q, z)
    np.testing.assert_array_equal(draws, np.broadcast_to(mu, (2, 129)))
    c = gpfit.Context(0)
    try:
        with pytest.raises(ValueError, match="set_data"):
            c.posterior_draws(ls[0], q, z)
    finally:
        c.close()
