"""gpf_predict_batch (prediction at P length-scale samples in one batched call and their mixture;
k_predict_vsq_batch, k_predict_mix, k_predict_mix_out) against the float64 NumPy closed form written
below, against predict() bit for bit at P = 1, and against gpfit.hyper.mixture_from.

Tolerances. Per particle max |mu - mu_ref| / max(1, max |mu_ref|) < 1e-9 and max |sd^2 - var_ref| < 1e-9:
the project's bound for every prediction call (its headroom over the closed form's own float64 error
is documented in test_predict_cov_gpu.py). The mixture against mixture_from on the same call's
per-particle outputs: 1e-12 max(1, |ref|) — West's update is O(P) roundings of 1.1e-16 with P <= 8,
and the two-pass yardstick is the same. The measured maxima are printed (run with -s) and sit in the
assert messages (profiles/predict_batch/pytest_gpu.log).
"""
import ctypes

import numpy as np
import pytest

from test_predict_cov_gpu import _case, _kernel

pytestmark = pytest.mark.gpu

TOL = 1e-9
MIX_TOL = 1e-12


@pytest.fixture(scope="module")
def ctx():
    import gpfit
    c = gpfit.Context(0)
    yield c
    c.close()


_REF = {}


def _reference(N, d, M, row):
    """(mu, var) of the closed form for length-scale row `row`: Kn = K + diag(e^2), mu = K_s^T Kn^-1 y,
    var = clip(1 - colsum((L^-1 K_s)^2), 1e-12); computed once per case and shared."""
    key = (N, d, M, row)
    if key not in _REF:
        x, y, e, ls, q = _case(N, d, M)
        l = ls[row]
        Kn = _kernel(x, x, l) + np.diag(e ** 2)
        Ks = _kernel(x, q, l)
        L = np.linalg.cholesky(Kn)
        v = np.linalg.solve(L, Ks)
        mu = Ks.T @ np.linalg.solve(Kn, y)
        var = np.clip(1.0 - np.sum(v * v, axis=0), 1e-12, None)
        mu.setflags(write=False)
        var.setflags(write=False)
        _REF[key] = (mu, var)
    return _REF[key]


@pytest.mark.parametrize("N,d,M,P", [(129, 2, 1, 1), (1, 2, 129, 2), (128, 1, 128, 3), (300, 2, 700, 3), (257, 3, 300, 3),
                                     (1100, 3, 130, 2)])
def test_tile_boundaries_vs_closed_form(ctx, N, d, M, P):
    """Ragged and exact tiles on both axes, one and several row tiles, and nine depth tiles."""
    x, y, e, ls, q = _case(N, d, M)
    ctx.set_data(x, y, e)
    mix_mu, mix_sd, info = ctx.predict_batch(ls[:P], q, want_each=True)
    assert mix_mu.shape == (M,) and mix_sd.shape == (M,)
    assert info["mu"].shape == (P, M) and info["sd"].shape == (P, M)
    for p in range(P):
        mu_ref, var_ref = _reference(N, d, M, p)
        em = np.max(np.abs(info["mu"][p] - mu_ref)) / max(1.0, np.max(np.abs(mu_ref)))
        ev = np.max(np.abs(info["sd"][p] ** 2 - var_ref))
        print(f"[predict_batch] N={N} d={d} M={M} P={P} particle {p}: mu err {em:.3e}, var err {ev:.3e} (tol {TOL:.0e})")
        assert em < TOL, f"N={N} d={d} M={M} particle {p}: mu error {em:.3e}"
        assert ev < TOL, f"N={N} d={d} M={M} particle {p}: max |sd^2 - var_ref| = {ev:.3e}"
    assert np.all(np.isfinite(mix_mu)) and np.all(mix_sd > 0.0)


@pytest.mark.parametrize("N,d,M", [(300, 2, 700), (129, 2, 1)])
def test_one_particle_is_bitwise_predict(ctx, N, d, M):
    x, y, e, ls, q = _case(N, d, M)
    ctx.set_data(x, y, e)
    for row in (0, 1):
        mu, sd = ctx.predict(ls[row], q)
        mix_mu, mix_sd, info = ctx.predict_batch(ls[row:row + 1], q, want_each=True)
        np.testing.assert_array_equal(info["mu"][0], mu, err_msg=f"row {row}: mu_p is not bitwise predict()'s")
        np.testing.assert_array_equal(info["sd"][0], sd, err_msg=f"row {row}: sd_p is not bitwise predict()'s")
        np.testing.assert_array_equal(mix_mu, mu, err_msg=f"row {row}: mix_mu is not bitwise predict()'s")
        np.testing.assert_array_equal(mix_sd, sd, err_msg=f"row {row}: mix_sd is not bitwise predict()'s")


@pytest.mark.parametrize("weights", [None, [0.5, 0.0, 3.0, 1.25, 0.25]], ids=["equal", "unequal"])
def test_mixture_vs_two_pass(ctx, weights):
    """Equal weights, and unequal ones with one zero and a sum of 5."""
    from gpfit.hyper import mixture_from
    N, d, M = 300, 2, 700
    x, y, e, ls, q = _case(N, d, M)
    ctx.set_data(x, y, e)
    mix_mu, mix_sd, info = ctx.predict_batch(ls, q, weights=weights, want_each=True)
    ref_mu, ref_sd = mixture_from(info["mu"], info["sd"], weights)
    em = np.max(np.abs(mix_mu - ref_mu) / np.maximum(1.0, np.abs(ref_mu)))
    es = np.max(np.abs(mix_sd - ref_sd) / np.maximum(1.0, np.abs(ref_sd)))
    print(f"[predict_batch] mixture P=5 weights {weights}: mix_mu err {em:.3e}, mix_sd err {es:.3e} (tol {MIX_TOL:.0e})")
    assert em < MIX_TOL, f"mix_mu differs from mixture_from by {em:.3e}"
    assert es < MIX_TOL, f"mix_sd differs from mixture_from by {es:.3e}"
    w = np.full(5, 0.2) if weights is None else np.asarray(weights) / np.sum(weights)
    within = np.sum(w[:, None] * info["sd"] ** 2, axis=0)
    assert np.all(mix_sd ** 2 >= within - 1e-12), "the mixture's variance is below the mean within-component variance"
    # the spread of the means must show: these length scales differ by up to 16x
    assert np.max(mix_sd ** 2 - within) > 1e-6


def test_query_chunking_is_bitwise(ctx):
    N, d, M = 300, 2, 700
    x, y, e, ls, q = _case(N, d, M)
    ctx.set_data(x, y, e)
    w = [0.5, 0.0, 3.0, 1.25, 0.25]
    mu0, sd0, i0 = ctx.predict_batch(ls, q, weights=w, want_each=True)
    for chunk in (128, 256):
        mu, sd, i1 = ctx.predict_batch(ls, q, weights=w, chunk=chunk, want_each=True)
        np.testing.assert_array_equal(mu, mu0, err_msg=f"chunk={chunk}: mix_mu")
        np.testing.assert_array_equal(sd, sd0, err_msg=f"chunk={chunk}: mix_sd")
        np.testing.assert_array_equal(i1["mu"], i0["mu"], err_msg=f"chunk={chunk}: mu_PM")
        np.testing.assert_array_equal(i1["sd"], i0["sd"], err_msg=f"chunk={chunk}: sd_PM")


def test_particle_chunking_carries_the_state(ctx, monkeypatch):
    """GPF_MAX_CHUNK=2 with P=5: three particle chunks (2, 2, 1); the mixture state must carry across."""
    N, d, M = 300, 2, 700
    x, y, e, ls, q = _case(N, d, M)
    ctx.set_data(x, y, e)
    w = [0.5, 0.0, 3.0, 1.25, 0.25]
    mu0, sd0, i0 = ctx.predict_batch(ls, q, weights=w, want_each=True)
    monkeypatch.setenv("GPF_MAX_CHUNK", "2")
    mu, sd, i1 = ctx.predict_batch(ls, q, weights=w, want_each=True)
    monkeypatch.delenv("GPF_MAX_CHUNK")
    errs = [np.max(np.abs(a - b)) for a, b in ((mu, mu0), (sd, sd0), (i1["mu"], i0["mu"]), (i1["sd"], i0["sd"]))]
    print(f"[predict_batch] GPF_MAX_CHUNK=2 vs one chunk, P=5: max diffs mix_mu {errs[0]:.3e}, mix_sd {errs[1]:.3e}, "
          f"mu_PM {errs[2]:.3e}, sd_PM {errs[3]:.3e} (tol {TOL:.0e})")
    assert max(errs) < TOL, f"particle chunks disagree: {errs}"
    # the chunks really ran: one k_predict_vsq_batch launch and one K_s entry per particle chunk and query
    # chunk in the profile's slots [15..17] and [18..20]
    ctx.set_profiling(True)
    try:
        for env, chunk, launches in ((None, 0, 1), ("2", 0, 3), ("2", 256, 9)):
            if env is not None:
                monkeypatch.setenv("GPF_MAX_CHUNK", env)
            ctx.reset_profile()
            ctx.predict_batch(ls, q, weights=w, chunk=chunk)
            prof = ctx.profile()
            monkeypatch.delenv("GPF_MAX_CHUNK", raising=False)
            assert prof["predict_launches"] == launches and prof["predict_cov_launches"] == launches, (env, chunk, prof)
            assert prof["predict_flops"] > 0 and prof["predict_cov_bytes"] > 0
    finally:
        ctx.set_profiling(False)


def test_both_dispatch_orders_give_the_same_bits(ctx, monkeypatch):
    """k_predict_vsq_batch under GPF_PREDBATCH_ORDER=0 (grid (nqt, nt, pc)) and =1 (grid (nqt, pc, nt)), each
    set explicitly (the default picks one by the pass's width, and picks order 1 at every shape of this
    file), at three row tiles x six column tiles x five particles: bitwise each other, and at P = 1
    both bitwise predict()."""
    N, d, M = 300, 2, 700
    x, y, e, ls, q = _case(N, d, M)
    ctx.set_data(x, y, e)
    w = [0.5, 0.0, 3.0, 1.25, 0.25]
    mu_p, sd_p = ctx.predict(ls[1], q)
    out, one = {}, {}
    for order in ("0", "1"):
        monkeypatch.setenv("GPF_PREDBATCH_ORDER", order)
        out[order] = ctx.predict_batch(ls, q, weights=w, want_each=True)
        one[order] = ctx.predict_batch(ls[1:2], q, want_each=True)
    monkeypatch.delenv("GPF_PREDBATCH_ORDER")
    np.testing.assert_array_equal(out["0"][2]["mu"], out["1"][2]["mu"])
    np.testing.assert_array_equal(out["0"][2]["sd"], out["1"][2]["sd"])
    np.testing.assert_array_equal(out["0"][0], out["1"][0])
    np.testing.assert_array_equal(out["0"][1], out["1"][1])
    for order in ("0", "1"):
        np.testing.assert_array_equal(one[order][2]["mu"][0], mu_p, err_msg=f"order {order}: mu_p is not predict()'s")
        np.testing.assert_array_equal(one[order][2]["sd"][0], sd_p, err_msg=f"order {order}: sd_p is not predict()'s")
        np.testing.assert_array_equal(one[order][0], mu_p, err_msg=f"order {order}: mix_mu is not predict()'s")
        np.testing.assert_array_equal(one[order][1], sd_p, err_msg=f"order {order}: mix_sd is not predict()'s")
    # order 0 against the closed form as well: a wrong decode there must not hide behind order 1
    monkeypatch.setenv("GPF_PREDBATCH_ORDER", "0")
    _, _, info = ctx.predict_batch(ls[:3], q, want_each=True)
    monkeypatch.delenv("GPF_PREDBATCH_ORDER")
    for p in range(3):
        mu_ref, var_ref = _reference(N, d, M, p)
        assert np.max(np.abs(info["mu"][p] - mu_ref)) / max(1.0, np.max(np.abs(mu_ref))) < TOL
        assert np.max(np.abs(info["sd"][p] ** 2 - var_ref)) < TOL


@pytest.mark.parametrize("d", [1, 2, 3, 5, 9, 32])
def test_cross_cov_batch_is_bitwise_cross_cov(ctx, monkeypatch, d):
    """k_cross_cov_batch (a copy of k_cross_cov's body with the particle on a grid axis) against k_cross_cov
    itself, launched once per particle (GPF_PREDBATCH_KS=0, an internal switch kept for this test): every
    instantiation — d = 1, 2, 3 templated, d = 5, 9 and 32 the run-time one (at 32 with 76,032 bytes of
    dynamic LDS; tests/test_dimension_gpu.py repeats 9 and 32 with length scales that keep K_s of order 1,
    which these do not) — with three particles, so that the
    offsets of particles 1 and 2 are pinned too; and at P = 1 bitwise predict(), which uses k_cross_cov."""
    N, M = 257, 300
    x, y, e, ls, q = _case(N, d, M)
    ctx.set_data(x, y, e)
    out = {}
    for ks in ("0", "1"):
        monkeypatch.setenv("GPF_PREDBATCH_KS", ks)
        out[ks] = ctx.predict_batch(ls[:3], q, want_each=True)
    monkeypatch.delenv("GPF_PREDBATCH_KS")
    np.testing.assert_array_equal(out["0"][2]["mu"], out["1"][2]["mu"])
    np.testing.assert_array_equal(out["0"][2]["sd"], out["1"][2]["sd"])
    np.testing.assert_array_equal(out["0"][0], out["1"][0])
    np.testing.assert_array_equal(out["0"][1], out["1"][1])
    mu_p, sd_p = ctx.predict(ls[2], q)
    mix_mu, mix_sd, _ = ctx.predict_batch(ls[2:3], q)
    np.testing.assert_array_equal(mix_mu, mu_p)
    np.testing.assert_array_equal(mix_sd, sd_p)


def test_repeatability_and_buffer_separation(ctx):
    N, d, M = 300, 2, 257
    x, y, e, ls, q = _case(N, d, M)
    _, _, _, _, q_wide = _case(N, d, 700)
    ctx.set_data(x, y, e)
    mu_p, sd_p = ctx.predict(ls[0], q)
    mu_c, cov_c = ctx.predict_cov(ls[1], q)
    lml, grad = ctx.lml_batch(ls)
    a = ctx.predict_batch(ls[:3], q, want_each=True)
    b = ctx.predict_batch(ls[:3], q, want_each=True)
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])
    np.testing.assert_array_equal(a[2]["mu"], b[2]["mu"])
    np.testing.assert_array_equal(a[2]["sd"], b[2]["sd"])

    def others_keep_their_bits(tag):
        m2, s2 = ctx.predict(ls[0], q)
        np.testing.assert_array_equal(m2, mu_p, err_msg=f"{tag}: predict mu")
        np.testing.assert_array_equal(s2, sd_p, err_msg=f"{tag}: predict sd")
        m3, c3 = ctx.predict_cov(ls[1], q)
        np.testing.assert_array_equal(m3, mu_c, err_msg=f"{tag}: predict_cov mu")
        np.testing.assert_array_equal(c3, cov_c, err_msg=f"{tag}: predict_cov cov")
        l2, g2 = ctx.lml_batch(ls)
        np.testing.assert_array_equal(l2, lml, err_msg=f"{tag}: lml_batch value")
        np.testing.assert_array_equal(g2, grad, err_msg=f"{tag}: lml_batch gradient")

    others_keep_their_bits("after predict_batch")
    ctx.predict_batch(ls, q_wide, want_each=True)   # wider and more particles: the buffers regrow
    others_keep_their_bits("after a wider predict_batch")
    c = ctx.predict_batch(ls[:3], q, want_each=True)
    np.testing.assert_array_equal(c[0], a[0])
    np.testing.assert_array_equal(c[1], a[1])


def test_eval_batch_keeps_its_bits(ctx):
    """ctx.eval_batch (the swarm's objective, replayed as a captured graph at this size) before and after
    predict_batch calls that grow their buffers."""
    from oracle import ref_cpu
    N, d, M = 129, 2, 257
    x, y, e, ls, q = _case(N, d, M)
    _, _, _, _, q_wide = _case(N, d, 700)
    ctx.set_data(x, y, e)
    lo, hi = ref_cpu.search_bounds(x)
    s, ex = ref_cpu.sigma_grid()
    ctx.set_grid(s, ex, lo, hi)
    pos = np.clip(ls, lo * 1.01 + 1e-3, hi * 0.99)
    before = ctx.eval_batch(pos)
    ctx.predict_batch(ls[:3], q)
    np.testing.assert_array_equal(ctx.eval_batch(pos), before)
    ctx.predict_batch(ls, q_wide, want_each=True)
    np.testing.assert_array_equal(ctx.eval_batch(pos), before)


def _bad_case():
    """d = 1, N = 128: x[0] = 0 and x[1] = 1e-9 without noise. At l = 1 the leading 2 x 2 block of K is
    exactly [[1, 1], [1, 1]] (exp(-5e-19) rounds to 1): the second pivot is 0. At l = 1e-6 it factorises."""
    rng = np.random.default_rng(128)
    x = np.sort(rng.uniform(0.01, 1.0, size=(1, 128)), axis=1)
    x[0, 0], x[0, 1] = 0.0, 1e-9
    y = np.sin(3 * x[0]) + 0.1 * rng.standard_normal(128)
    e = np.full(128, 0.1)
    e[:2] = 0.0
    q = rng.uniform(0.0, 1.0, size=(1, 130))
    pos = np.array([[1e-6], [1.0], [1e-6]])
    return x, y, e, q, pos


def test_one_bad_particle(ctx):
    x, y, e, q, pos = _bad_case()
    K = _kernel(x, x, pos[1]) + np.diag(e ** 2)
    assert K[0, 0] == 1.0 and K[0, 1] == 1.0 and K[1, 1] == 1.0
    with pytest.raises(np.linalg.LinAlgError):
        np.linalg.cholesky(K)
    np.linalg.cholesky(_kernel(x, x, pos[0]) + np.diag(e ** 2))
    ctx.set_data(x, y, e)
    with pytest.raises(np.linalg.LinAlgError) as err:
        ctx.predict_batch(pos, q)
    assert err.value.particle == 1
    # through the raw C-ABI: the return code, *bad_idx and the untouched mixture outputs
    from gpfit._lib import GPF_NOT_PD, _ptr
    M = q.shape[1]
    mix_mu, mix_sd = np.full(M, -7.25), np.full(M, -7.25)
    bad = ctypes.c_int(-5)
    rc = ctx.lib.gpf_predict_batch(ctx._h, _ptr(pos), 3, None, _ptr(np.ascontiguousarray(q)), M, 0, _ptr(mix_mu), _ptr(mix_sd),
                                   None, None, ctypes.byref(bad))
    assert rc == GPF_NOT_PD and bad.value == 1
    assert np.all(mix_mu == -7.25) and np.all(mix_sd == -7.25)
    # the next call is clean, and equals the good particles' own predictions
    good = pos[[0, 2]]
    mu, sd, info = ctx.predict_batch(good, q, want_each=True)
    m0, s0 = ctx.predict(pos[0], q)
    scale = max(1.0, np.max(np.abs(m0)))
    for got, want in ((info["mu"][0], m0), (info["mu"][1], m0), (mu, m0)):
        assert np.max(np.abs(got - want)) / scale < TOL
    for got in (info["sd"][0], info["sd"][1], sd):
        assert np.max(np.abs(got ** 2 - s0 ** 2)) < TOL


def test_bad_arguments(ctx):
    x, y, e, ls, q = _case(129, 2, 130)
    ctx.set_data(x, y, e)
    with pytest.raises(ValueError):
        ctx.predict_batch(ls, q, weights=[1.0, 1.0])
    with pytest.raises(ValueError):
        ctx.predict_batch(ls, q, weights=[1.0, -1.0, 1.0, 1.0, 1.0])
    with pytest.raises(ValueError):
        ctx.predict_batch(ls, q, weights=np.zeros(5))
    with pytest.raises(ValueError):
        ctx.predict_batch(ls, q, weights=[1.0, np.nan, 1.0, 1.0, 1.0])
    with pytest.raises(ValueError):
        ctx.predict_batch(-ls, q)
    with pytest.raises(ValueError):
        ctx.predict_batch(ls, q, chunk=-1)
    with pytest.raises(ValueError):
        ctx.predict_batch(ls[:, :1], q)
    with pytest.raises(ValueError):
        ctx.predict_batch(ls[:0], q)                  # P = 0: a mixture of nothing
    mu, sd, _ = ctx.predict_batch(ls, q[:, :0])       # M = 0
    assert mu.shape == (0,) and sd.shape == (0,)


def test_predict_marginal_end_to_end(ctx):
    """Samples drawn from the device's marginal likelihood (N = 150 > 100: the KMeans subsample, the
    fit, the Hessian and the scoring all run), then the batched route against the loop."""
    from gpfit.hyper import predict_marginal
    N, d, M = 150, 2, 200
    x, y, e, _, q = _case(N, d, M)
    mu_b, sd_b, ib = predict_marginal(x, y, e, q, method="batch", ctx=ctx, n_samples=8, seed=0)
    mu_l, sd_l, il = predict_marginal(x, y, e, q, method="loop", ctx=ctx, n_samples=8, seed=0)
    np.testing.assert_array_equal(ib["ls"], il["ls"])
    np.testing.assert_array_equal(ib["weights"], il["weights"])
    em = np.max(np.abs(mu_b - mu_l)) / max(1.0, np.max(np.abs(mu_l)))
    es = np.max(np.abs(sd_b - sd_l))
    print(f"[predict_batch] predict_marginal N={N} M={M} K=8: batch vs loop mu {em:.3e}, sd {es:.3e}, ess {ib['ess']:.2f}")
    assert em < TOL and es < TOL
    assert ib["ls"].shape == (8, d) and abs(np.sum(ib["weights"]) - 1.0) < 1e-12
    assert 1.0 <= ib["ess"] <= 8.0
    assert ib["sample"]["ess"] == pytest.approx(ib["ess"], rel=1e-12)
