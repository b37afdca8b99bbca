"""gpf_chol_dense (Context.chol_dense): the dense blocked Cholesky factorisation of gpf_densechol.hip
(k_dc_init, k_dc_diag, k_dc_finish, k_dc_trail) and its jitter ladder against numpy.linalg.cholesky.

Bounds, u = 2^-53 (derived, not tuned):
  factor        max |L - L_np| <= 8 n u cond_2(A) max |L_np|: both factors are backward stable, and the
                Cholesky factor's sensitivity to a relative perturbation of A is bounded by cond_2(A)
                (Sun 1991), n u being the size of either backward error;
  reconstruction  max |L L^T - (A + jitter I)| <= 8 n u sqrt(cond_2(A + jitter I)) max diag: the
                finishes multiply by U_JJ = L_JJ^-1 instead of solving, which carries cond(L_JJ) <=
                cond(L) = sqrt(cond(A)).
cond_2 comes from NumPy inside the test. The measured maxima are printed (run with -s); on one
MI355X (profiles/posterior_draws/pytest_gpu.log): factor within 1.5e-15 of NumPy's at n = 641 (bound
4.3e-12), reconstruction of the ill-conditioned posterior (cond 5.5e10) within 2.1e-15 (bound
9.4e-10), the ladder cases (cond 1.1e8 at jitter 1e-8) within 4.3e-12 of NumPy's factor (bound
2.3e-5) and 1.0e-15 in the reconstruction (bound 1.8e-9).
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


@pytest.fixture(scope="module")
def ctx():
    import gpfit
    c = gpfit.Context(0)
    yield c
    c.close()


_MATS = {}


def _spd(n, neg=False):
    """A = Q diag(linspace(0.1, 1, n)) Q^T, symmetrised, Q from the QR factorisation of a seeded normal
    matrix; neg: the smallest eigenvalue set to -1e-9. Built once per (n, neg), read-only."""
    if (n, neg) not in _MATS:
        q, _ = np.linalg.qr(np.random.default_rng(7000 + n).standard_normal((n, n)))
        w = np.linspace(0.1, 1.0, n)
        if neg:
            w[0] = -1e-9
        a = (q * w) @ q.T
        a = 0.5 * (a + a.T)
        a.setflags(write=False)
        _MATS[(n, neg)] = a
    return _MATS[(n, neg)]


def _factor_bound(a_j, l_np):
    n = a_j.shape[0]
    return 8.0 * n * U * np.linalg.cond(a_j, 2) * np.max(np.abs(l_np))


def _recon_bound(a_j):
    n = a_j.shape[0]
    return 8.0 * n * U * np.sqrt(np.linalg.cond(a_j, 2)) * np.max(np.diag(a_j))


@pytest.mark.parametrize("n", [1, 127, 128, 129, 257, 300, 641])
def test_tile_boundaries_vs_numpy(ctx, n):
    a = _spd(n)
    l_np = np.linalg.cholesky(a)
    L, info = ctx.chol_dense(a, jitters=(0.0,))
    assert L.shape == (n, n)
    err, bound = np.max(np.abs(L - l_np)), _factor_bound(a, l_np)
    print(f"[chol_dense] n={n}: max |L - L_np| = {err:.3e} (bound {bound:.3e}), cond {np.linalg.cond(a, 2):.3g}")
    assert info == {"jitter": 0.0, "tries": 1}
    assert np.all(np.triu(L, 1) == 0.0), "the upper triangle is not exactly zero"
    assert err <= bound, f"n={n}: max |L - L_np| = {err:.3e} > {bound:.3e}"


def _posterior_case():
    rng = np.random.default_rng(42)
    x = rng.uniform(size=(2, 150))
    y = np.sin(3.0 * x[0]) + np.cos(2.0 * x[1]) + 0.1 * rng.standard_normal(150)
    q = rng.uniform(size=(2, 300))
    return x, y, np.full(150, 0.1), np.array([0.3, 0.4]), q


def test_reconstruction_of_an_ill_conditioned_posterior(ctx):
    """Sigma of 300 queries among 150 training points, e = 0.1, l = (0.3, 0.4): cond(Sigma + 1e-12 I) is
    about 6e10 and NumPy factorises it at the first jitter."""
    from gpfit.posterior import JITTERS
    x, y, e, l, q = _posterior_case()
    ctx.set_data(x, y, e)
    _, cov = ctx.predict_cov(l, q)
    np.linalg.cholesky(cov + JITTERS[0] * np.eye(300))  # (a condition on the input)
    L, info = ctx.chol_dense(cov)
    assert info["jitter"] in JITTERS and 1 <= info["tries"] <= len(JITTERS)
    a_j = cov + info["jitter"] * np.eye(300)
    err, bound = np.max(np.abs(L @ L.T - a_j)), _recon_bound(a_j)
    print(f"[chol_dense] posterior M=300: jitter {info['jitter']:.0e} after {info['tries']} tries, cond "
          f"{np.linalg.cond(a_j, 2):.3e}, max |L L^T - (Sigma + jitter I)| = {err:.3e} (bound {bound:.3e})")
    assert np.all(np.triu(L, 1) == 0.0)
    assert err <= bound


@pytest.mark.parametrize("n", [130, 300])
def test_ladder(ctx, n):
    """Smallest eigenvalue -1e-9: indefinite at jitter 1e-12 and 1e-10 (by 9e-10, far above the
    rounding of either factorisation), positive definite at 1e-8."""
    import gpfit._lib as lib
    from gpfit.posterior import JITTERS
    a, eye = _spd(n, neg=True), np.eye(n)
    for j in JITTERS[:2]:  # (conditions on the input)
        with pytest.raises(np.linalg.LinAlgError):
            np.linalg.cholesky(a + j * eye)
    a_j = a + 1e-8 * eye
    l_np = np.linalg.cholesky(a_j)
    L, info = ctx.chol_dense(a)
    assert info == {"jitter": 1e-8, "tries": 3}
    e_f, b_f = np.max(np.abs(L - l_np)), _factor_bound(a_j, l_np)
    e_r, b_r = np.max(np.abs(L @ L.T - a_j)), _recon_bound(a_j)
    print(f"[chol_dense] ladder n={n}: max |L - L_np| = {e_f:.3e} (bound {b_f:.3e}), max |L L^T - (A + 1e-8 I)| = "
          f"{e_r:.3e} (bound {b_r:.3e})")
    assert e_f <= b_f and e_r <= b_r
    assert np.all(np.triu(L, 1) == 0.0)
    # a ladder that ends too early: LinAlgError, and the caller's buffer is not written
    with pytest.raises(np.linalg.LinAlgError, match="not positive definite") as ei:
        ctx.chol_dense(a, jitters=JITTERS[:2])
    assert ei.value.tries == 2
    out = np.full((n, n), -7.25)
    jit, tries = ctypes.c_double(-1.0), ctypes.c_int(-1)
    jj, ac = np.array(JITTERS[:2]), np.ascontiguousarray(a)
    dp = ctypes.POINTER(ctypes.c_double)
    rc = ctx.lib.gpf_chol_dense(ctx._h, ac.ctypes.data_as(dp), n, jj.ctypes.data_as(dp), 2, out.ctypes.data_as(dp),
                                ctypes.byref(jit), ctypes.byref(tries))
    assert rc == lib.GPF_NOT_PD and tries.value == 2 and jit.value == -1.0
    assert np.all(out == -7.25)
    np.testing.assert_array_equal(ctx.chol_dense(a)[0], L)  # the context is clean afterwards


def test_repeatability_and_buffer_reuse(ctx):
    a = _spd(129)
    l1, i1 = ctx.chol_dense(a, jitters=(0.0,))
    l2, i2 = ctx.chol_dense(a, jitters=(0.0,))
    np.testing.assert_array_equal(l1, l2)
    assert i1 == i2
    ctx.chol_dense(_spd(300), jitters=(0.0,))  # leaves wider buffers behind
    l3, _ = ctx.chol_dense(a, jitters=(0.0,))
    np.testing.assert_array_equal(l1, l3)


def test_arguments(ctx):
    import gpfit._lib as lib
    with pytest.raises(ValueError, match="square"):
        ctx.chol_dense(np.zeros((3, 4)))
    with pytest.raises(ValueError, match="jitters"):
        ctx.chol_dense(np.eye(3), jitters=())
    L, info = ctx.chol_dense(np.zeros((0, 0)))
    assert L.shape == (0, 0) and info["tries"] == 0
    dp = ctypes.POINTER(ctypes.c_double)
    a, out, bad = np.eye(3), np.full((3, 3), -7.25), np.array([float("nan")])
    jit, tries = ctypes.c_double(-1.0), ctypes.c_int(-1)
    for n, jp, nj in ((-1, bad, 1), (3, bad, 1), (3, bad, 0), (3, None, 1)):
        rc = ctx.lib.gpf_chol_dense(ctx._h, a.ctypes.data_as(dp), n, None if jp is None else jp.ctypes.data_as(dp), nj,
                                    out.ctypes.data_as(dp), ctypes.byref(jit), ctypes.byref(tries))
        assert rc == lib.GPF_BAD_ARG
    assert np.all(out == -7.25)
    # only the lower triangle is read
    b = _spd(129).copy()
    want = ctx.chol_dense(b, jitters=(0.0,))[0]
    b[np.triu_indices(129, 1)] = 123.0
    np.testing.assert_array_equal(ctx.chol_dense(b, jitters=(0.0,))[0], want)
