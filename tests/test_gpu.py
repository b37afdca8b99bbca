"""Parity of the HIP path (through the C-ABI) with the reference and the oracle.

Tolerances (BASELINE.json north_star): predictive mean / sd within 1e-6
relative; the objective ("log-lik eval") within 1e-8 relative.
"""
import os

import numpy as np
import pytest

from oracle import ref_cpu

pytestmark = pytest.mark.gpu

RTOL_MU_SD = 1e-6
RTOL_LOSS = 1e-8


def _fx(x):
    return np.asfortranarray(x)


@pytest.fixture(scope="module")
def ctx():
    import gpfit
    c = gpfit.Context(0)
    yield c
    c.close()


def _blas_threads():
    """The oracle's dense LAPACK at N >= 4096 with the box's CPU share (conftest pins one BLAS
    thread for the reference-identical small cases; threads change only the rounding)."""
    from threadpoolctl import threadpool_limits
    return threadpool_limits(limits=min(16, os.cpu_count() or 1), user_api="blas")


def _rel(a, b, floor=1e-3):
    return np.max(np.abs(a - b) / np.maximum(np.abs(b), floor))


def test_mfma_f64_fragment_layout(ctx):
    rng = np.random.default_rng(0)
    a = rng.integers(-8, 8, size=(16, 4)).astype(np.float64)
    b = rng.integers(-8, 8, size=(4, 16)).astype(np.float64)  # asymmetric
    np.testing.assert_array_equal(ctx.selftest_mfma(a, b), a @ b)


def test_objective_testfiles_vs_reference(ctx, f2):
    s, ex = f2["sigma_vals"], f2["expected"]
    for i in range(int(f2["ncases"])):
        x, y, e = f2[f"c{i}_x"], f2[f"c{i}_y"], f2[f"c{i}_e"]
        lo, hi, P = f2[f"c{i}_lo"], f2[f"c{i}_hi"], f2[f"c{i}_P"]
        ctx.set_data(x, y, e)
        ctx.set_grid(s, ex, lo, hi)
        loss, mu, sd = ctx.eval_batch(P, want_mu_sd=True)
        want = f2[f"c{i}_loss"]
        assert np.all((want == 1e13) == (loss == 1e13))
        assert _rel(loss, want) < RTOL_LOSS, str(f2[f"c{i}_tag"])
        mu8, sd8 = f2[f"c{i}_mu8"], f2[f"c{i}_sd8"]
        ok = np.isfinite(mu8[:, 0])
        if ok.any():
            assert _rel(mu[:8][ok], mu8[ok]) < RTOL_MU_SD
            assert _rel(sd[:8][ok], sd8[ok]) < RTOL_MU_SD


def test_objective_synthetic_vs_reference(ctx, f3):
    s, ex = f3["sigma_vals"], f3["expected"]
    for i in range(int(f3["ncases"])):
        x, y, e = f3[f"c{i}_x"], f3[f"c{i}_y"], f3[f"c{i}_e"]
        lo, hi, P = f3[f"c{i}_lo"], f3[f"c{i}_hi"], f3[f"c{i}_P"]
        ctx.set_data(x, y, e)
        ctx.set_grid(s, ex, lo, hi)
        loss, mu, sd = ctx.eval_batch(P, want_mu_sd=True)
        assert _rel(loss, f3[f"c{i}_loss"]) < RTOL_LOSS, f3[f"c{i}_meta"]
        assert _rel(mu[0], f3[f"c{i}_mu0"]) < RTOL_MU_SD
        assert _rel(sd[0], f3[f"c{i}_sd0"]) < RTOL_MU_SD


@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 127, 128, 129, 200, 255, 256, 257, 300])
def test_tile_boundaries_vs_oracle(ctx, N):
    rng = np.random.default_rng(N)
    d = 2
    x = rng.uniform(size=(d, N))
    y = np.sin(3 * x[0]) + x[1] + 0.1 * rng.standard_normal(N)
    e = rng.uniform(0.05, 0.2, size=N)
    s, ex = ref_cpu.sigma_grid()
    lo, hi = np.full(d, 1e-3), np.full(d, 2.0)
    P = rng.uniform(0.05, 0.8, size=(5, d))
    ctx.set_data(x, y, e)
    ctx.set_grid(s, ex, lo, hi)
    loss, mu, sd = ctx.eval_batch(P, want_mu_sd=True)
    for k in range(5):
        m, sg = ref_cpu.GP(x, y, e, x, P[k], batch_size=N)
        assert _rel(mu[k], m) < RTOL_MU_SD and _rel(sd[k], sg) < RTOL_MU_SD
        want = ref_cpu.evaluate_loss(P[k], x, y, e, s, ex, lo, hi)
        assert abs(loss[k] - want) / abs(want) < RTOL_LOSS


def test_gp_predict_vs_reference_and_committed_outputs(ctx, f1):
    import GP_func
    for i in range(int(f1["ncases"])):
        x, y, e, ls = f1[f"c{i}_x"], f1[f"c{i}_y"], f1[f"c{i}_e"], f1[f"c{i}_ls"]
        xfit = f1[f"c{i}_xfit"]
        mu, sd = GP_func.GP(_fx(x), y, e, xfit, ls)
        assert _rel(mu, f1[f"c{i}_mu"]) < RTOL_MU_SD
        assert _rel(sd, f1[f"c{i}_sd"]) < RTOL_MU_SD
        n = int(f1[f"c{i}_ntrain"])
        assert _rel(mu[n:], f1[f"c{i}_committed_mu"]) < RTOL_MU_SD
        assert _rel(sd[n:], f1[f"c{i}_committed_sd"]) < RTOL_MU_SD
        mu7, sd7 = GP_func.GP(_fx(x), y, e, xfit, ls, batch_size=7)
        np.testing.assert_array_equal(mu7, mu)
        np.testing.assert_array_equal(sd7, sd)


def test_kernel_func_vs_oracle(ctx):
    import GP_func
    rng = np.random.default_rng(3)
    x1, x2 = rng.uniform(size=(3, 70)), rng.uniform(size=(3, 131))
    l = np.array([0.2, 0.5, 1.3])
    got = GP_func.kernel_func(x1, x2, l)
    want = ref_cpu.kernel_func(x1, x2, l)
    assert got.shape == (70, 131)
    np.testing.assert_allclose(got, want, rtol=1e-13, atol=1e-15)


def test_find_len_scales_dropin_scalar_api(ctx, f2):
    import find_len_scales as fls
    s, ex = fls.sigma_to_percent(f2["sigma_vals"]), None
    np.testing.assert_array_equal(s, f2["expected"])
    x, y, e = _fx(f2["c0_x"]), f2["c0_y"], f2["c0_e"]
    lo, hi, P = f2["c0_lo"], f2["c0_hi"], f2["c0_P"]
    args = (P[0], x, y, e, f2["sigma_vals"], f2["expected"], lo, hi)
    v = fls.evaluate_loss_helper(args)
    assert abs(v - f2["c0_loss"][0]) / f2["c0_loss"][0] < RTOL_LOSS
    assert fls.wass_loss(*args) == -v
    assert fls.evaluate_loss(P[-9], x, y, e, f2["sigma_vals"], f2["expected"], lo, hi) == f2["c0_loss"][-9]


@pytest.mark.parametrize("k", [0, 1, 2])
def test_pso_trajectory_replay_every_eval_on_gpu(ctx, f4, k, capsys):
    """Replay the reference's full 500-iteration PSO trajectory (driven by the
    reference scores through the drop-in driver, bit-for-bit) and score every
    one of its ~20k particle positions on the GPU as well: each must agree to
    1e-8 relative, sentinels exactly — except threshold ties, where a pull lies
    within 1e-9 of |pull| = 1 and one coverage count legitimately flips (the
    swarm converges onto such edges); those are counted separately and must
    stay rare."""
    from gpfit.swarm import particle_swarm
    x, y, e = _fx(f4[f"c{k}_x"]), f4[f"c{k}_y"], f4[f"c{k}_e"]
    stats = {"n": 0, "ties": 0, "worst_nontie": 0.0}

    def tee(args):
        ref = np.array([ref_cpu.evaluate_loss_helper(a) for a in args])
        _, xk, yk, ek, s, ex, lo, hi = args[0]
        ctx.set_data(xk, yk, ek)
        ctx.set_grid(s, ex, lo, hi)
        got = ctx.eval_batch(np.stack([a[0] for a in args]))
        assert np.array_equal(got == 1e13, ref == 1e13)
        for i in np.nonzero((ref < 1e13) & (np.abs(got - ref) > RTOL_LOSS * np.abs(ref)))[0]:
            if pull_at_threshold(args[i][0], xk, yk, ek, s):
                stats["ties"] += 1
            else:
                stats["worst_nontie"] = max(stats["worst_nontie"], abs(got[i] - ref[i]) / abs(ref[i]))
        stats["n"] += len(args)
        return ref

    best, _ = particle_swarm(x, y, e, True, init_positions=f4[f"c{k}_init"], seed=int(f4[f"c{k}_seed"]),
                             evaluator=tee)
    capsys.readouterr()
    assert np.array_equal(best, f4[f"c{k}_best"])
    assert stats["n"] >= 40 * 501
    assert stats["worst_nontie"] < RTOL_LOSS, stats
    assert stats["ties"] <= 0.05 * stats["n"], stats  # late iterations sit on a cell edge


def assert_loss_or_ties(got, want, mu_ref, sd_ref, y, s, tol=1e-9, what=""):
    """The objective within RTOL_LOSS of the reference's, or the difference fully explained by
    threshold ties: reference pulls (mu - y) / max(sd * s_k, 1e-12) within `tol` of |pull| = 1
    (find_len_scales.py:162-163), where one coverage count can flip between two correct fp64
    evaluations. A flip at grid point k moves measured_k by 1/N and the trapezoid (:166) by at
    most its weight w_k / N, so |got - want| may not exceed the sum of those over the tied
    pulls (plus RTOL_LOSS)."""
    if abs(got - want) <= RTOL_LOSS * abs(want):
        return
    N = y.shape[0]
    pulls = (mu_ref[:, None] - y[:, None]) / np.maximum(sd_ref[:, None] * s[None, :], 1e-12)
    near = np.abs(np.abs(pulls) - 1.0) < tol
    w = np.full(s.shape, s[1] - s[0])  # trapezoid weights of the uniform grid (:66)
    w[0] = w[-1] = w[0] / 2
    bound = float(np.sum(near * w[None, :]) / N)
    assert near.any() and abs(got - want) <= bound * 1.001 + RTOL_LOSS * abs(want), \
        (what, got, want, int(near.sum()), bound)


def pull_at_threshold(ls, x, y, e, s, tol=1e-9):
    """A coverage count can flip between two correct fp64 evaluations only if some
    reference pull (mu - y) / max(sd * s_k, 1e-12) sits within rounding of |pull| = 1
    (find_len_scales.py:162-163)."""
    mu, sd = ref_cpu.GP(x, y, e, x, ls, batch_size=x.shape[1])
    pulls = (mu[:, None] - y[:, None]) / np.maximum(sd[:, None] * s[None, :], 1e-12)
    return float(np.min(np.abs(np.abs(pulls) - 1.0))) < tol


@pytest.mark.parametrize("k", [0, 1])
def test_pso_on_gpu_end_to_end(ctx, f4, k, capsys):
    """The GPU-driven PSO itself (len_scale_opt drop-in). Its trajectory can part
    from the reference's once a 1e-12-level score difference flips a stall
    counter (the loss is piecewise constant in l), so this checks the outcome:
    the optimum it reports is as good as the reference's (within 1%) and its
    reported score is the objective at its reported position, up to a coverage
    tie: the swarm converges onto edges of the piecewise-constant loss, where a
    pull sits within rounding of |pull| = 1 and two correct fp64 evaluations
    may count it differently (pull_at_threshold)."""
    import find_len_scales as fls
    x, y, e = _fx(f4[f"c{k}_x"]), f4[f"c{k}_y"], f4[f"c{k}_e"]
    best = fls.len_scale_opt(x, y, e, True, init_positions=f4[f"c{k}_init"], seed=int(f4[f"c{k}_seed"]))
    out = capsys.readouterr().out.splitlines()
    ref_score = float(str(f4[f"c{k}_log"]).splitlines()[-2])
    got_score = float(out[-2])
    assert got_score <= ref_score * 1.01
    lo, hi = ref_cpu.search_bounds(x)
    s, ex = ref_cpu.sigma_grid()
    ref_at_best = ref_cpu.evaluate_loss(best, x, y, e, s, ex, lo, hi)
    if abs(ref_at_best - got_score) > 1e-8 * got_score:
        assert pull_at_threshold(best, x, y, e, s), (ref_at_best, got_score)


@pytest.mark.parametrize("n,d,k,dup", [(1024, 3, 100, 0), (4096, 3, 100, 0), (16384, 4, 100, 0), (600, 2, 100, 400),
                                       (3000, 5, 37, 0), (3000, 7, 37, 0), (2000, 32, 50, 0)])
def test_kmeans_fit_on_gpu_matches_sklearn(ctx, n, d, k, dup):
    """The KMeans subsample's fit with the Lloyd E/M-steps on the GPU (gpf_kmeans_step,
    gpfit.kmeans): labels equal to sklearn's KMeans(k, n_init='auto', random_state=0).fit (the
    reference's call, find_len_scales.py:27-31), centres within 1e-12; duplicate points (empty
    clusters relocated) included; d = 7 and 32 run k_km_assign's run-time-d path."""
    from sklearn.cluster import KMeans
    from gpfit.kmeans import kmeans_fit
    rng = np.random.default_rng(n + d + k + dup)
    X = rng.uniform(size=(n, d))
    if dup:
        X[-dup:] = X[:8][rng.integers(0, 8, size=dup)]
    with _blas_threads():
        km = KMeans(n_clusters=k, n_init="auto", random_state=0).fit(X)
    labels, centres = kmeans_fit(ctx, X, k)
    assert np.array_equal(labels, km.labels_)
    np.testing.assert_allclose(centres, km.cluster_centers_, rtol=0, atol=1e-12)


def test_kmeans_step_buffers_follow_k_and_d(ctx):
    """gpf_kmeans_step keeps its centre buffers between calls: a call with more dimensions at the
    same or a smaller k, or more clusters, must resize them (a d-only change once overran them). The
    sequence goes on through d = 7, 9 and 32 (k_km_assign's run-time-d path; 6 and 8 are templated), d
    rising and falling on the live context."""
    rng = np.random.default_rng(5)
    for n, d, k in ((500, 2, 50), (700, 5, 50), (400, 3, 120), (300, 4, 10), (400, 32, 100), (600, 6, 40),
                    (500, 9, 64), (600, 7, 40), (500, 8, 64)):
        X = rng.uniform(size=(n, d))
        C = X[rng.choice(n, k, replace=False)]
        ctx.kmeans_set(X)
        labels, sums, counts, dist = ctx.kmeans_step(C, update=True, want_dist=True)
        d2 = np.einsum("ij,ij->i", C, C)[None, :] - 2.0 * (X @ C.T)
        assert np.array_equal(labels, np.argmin(d2, axis=1))
        assert np.array_equal(counts, np.bincount(labels, minlength=k).astype(float))
        ref = np.zeros((k, d))
        np.add.at(ref, labels, X)
        np.testing.assert_allclose(sums, ref, rtol=1e-13, atol=1e-13)
        np.testing.assert_allclose(dist, np.sum((X - C[labels]) ** 2, axis=1), rtol=1e-13, atol=1e-15)


def test_kmeans_subsample_on_gpu_keeps_reference_points(ctx):
    """F10 (the points the reference's len_scale_opt keeps at N = 300..4096, d = 2..4) through
    prepare() with a GPU context, the product path of the drop-in's len_scale_opt: the same points
    in the same order, and the same search box."""
    from conftest import fixture_data, load_golden
    from gpfit.swarm import prepare
    f = load_golden("f10_kmeans.npz")
    for i in range(int(f["ncases"])):
        x, y, e = fixture_data(f[f"c{i}_meta"], f[f"c{i}_data_sha256"])
        xs, ys, es, lo, hi, _, _ = prepare(np.asfortranarray(x), y, e, max_points=100, verbose=False, ctx=ctx)
        idx = f[f"c{i}_idx"]
        assert np.array_equal(xs, x[:, idx]) and np.array_equal(ys, y[idx]) and np.array_equal(es, e[idx])
        assert np.array_equal(lo, f[f"c{i}_lo"]) and np.array_equal(hi, f[f"c{i}_hi"])


def test_not_positive_definite_raises_like_numpy(ctx):
    x = np.array([[0.0, 1.0, 1.0, 2.0]])  # duplicate point, zero noise: K singular exactly
    y, e = np.array([0.1, 0.2, 0.2, 0.3]), np.zeros(4)
    with pytest.raises(np.linalg.LinAlgError):
        ref_cpu.GP(x, y, e, x, np.array([1.0]))
    ctx.set_data(x, y, e)
    s, ex = ref_cpu.sigma_grid()
    ctx.set_grid(s, ex, np.array([0.5]), np.array([2.0]))
    with pytest.raises(np.linalg.LinAlgError, match="not positive definite"):
        ctx.eval_batch(np.array([[1.0], [1.5]]))
    import GP_func
    with pytest.raises(np.linalg.LinAlgError):
        GP_func.GP(x, y, e, x, np.array([1.0]))


def test_predict_not_positive_definite_leaves_outputs_untouched(ctx):
    """test_predict_cov_gpu.py's recipe for gpf_predict: N = 128, d = 1, M = 128, the first two training
    points identical with e = 0 (K's leading 2x2 block is exactly [[1, 1], [1, 1]] and the second
    pivot exactly 0). GPF_NOT_PD from the raw entry point, the caller's buffers untouched, and the next
    call on the good data is within the module's tolerance of the oracle."""
    import ctypes
    import gpfit._lib as L
    from test_predict_cov_gpu import _case
    x, y, e, ls, q = _case(128, 1, 128)
    xb, eb = x.copy(), e.copy()
    xb[:, 1] = xb[:, 0]
    eb[:2] = 0.0
    with pytest.raises(np.linalg.LinAlgError):
        ref_cpu.GP(xb, y, eb, q, ls[0])
    ctx.set_data(xb, y, eb)
    with pytest.raises(np.linalg.LinAlgError, match="Matrix is not positive definite"):
        ctx.predict(ls[0], q)
    M = q.shape[1]
    mu, sd = np.full(M, -7.25), np.full(M, -7.25)
    l0, qc = np.ascontiguousarray(ls[0]), np.ascontiguousarray(q)
    dp = ctypes.POINTER(ctypes.c_double)
    rc = ctx.lib.gpf_predict(ctx._h, l0.ctypes.data_as(dp), qc.ctypes.data_as(dp), M, 10000, mu.ctypes.data_as(dp),
                             sd.ctypes.data_as(dp))
    assert rc == L.GPF_NOT_PD
    assert np.all(mu == -7.25) and np.all(sd == -7.25)
    ctx.set_data(x, y, e)
    mu, sd = ctx.predict(ls[0], q)
    m0, s0 = ref_cpu.GP(x, y, e, q, ls[0])
    assert _rel(mu, m0) < RTOL_MU_SD and _rel(sd, s0) < RTOL_MU_SD


def _cluster_data(N, c0, nc=20, spacing=0.01, dup=False):
    """d = 1 points where K's first failing pivot sits past row 384 for a chosen particle only:
    x_i = i (unit spacing), except a cluster of nc points spaced `spacing` at rows c0.. 50 below the
    rest; zero noise. For l in [0.011, 0.02] every pair outside the cluster is uncorrelated (K = I
    there) and the cluster's Gaussian block is well conditioned (LAPACK's smallest pivot 0.0073 at
    l = 0.02); at l = 0.2 the cluster block is numerically rank ~4, and dpotrf fails inside it
    (row c0 + 5: info 406 at N=1024 / c0=400, 1006 at N=4096 / c0=1000). The search box is
    (0.01, N + 49), so every particle reaches the GPU."""
    x = np.arange(N, dtype=float)
    x[c0:c0 + nc] = -50.0 + spacing * np.arange(nc)  # (near the origin: the reference's |a|^2 + |b|^2 - 2ab
    # form, GP_func.py:59-62, would lose the cluster's distances to cancellation at large coordinates)
    if dup:  # row c0 + 31 repeats row c0 + 30: K's 2x2 block there is exactly [[1, 1], [1, 1]] and every
        # other entry of those rows underflows to exactly 0 for l <= 0.02, so the pivot of row c0 + 31 is
        # exactly 0 under any summation order — for every particle
        x[c0 + 31] = x[c0 + 30]
    x = x[None, :]
    y = np.sin(x[0]) + 0.01 * np.arange(N) / N
    return x, y, np.zeros(N)


def _cluster_K(x, l):
    return ref_cpu.kernel_func(x, x, np.array([l]))  # the reference's K (zero noise)


@pytest.mark.parametrize("sched", ["C_two_groups", "D_share", "E_persistent", "B_early_diag"])
def test_not_pd_past_block3_on_timed_schedules(ctx, monkeypatch, sched):
    """The reference's LinAlgError contract (GP_func.py:22 -> numpy.linalg.cholesky, propagated
    out of the pool at find_len_scales.py:103) on every timed schedule, with the failing pivot in
    block column J >= 3 and only one live particle singular: C's two concurrent
    groups with the fused diagonal factor (N=4096, 64 particles, failure in block 7; the bad
    particle in either group), D's 32-particle share, E's persistent k_factor (GPF_PERSIST=1), B's
    early-diagonal launches with the look-ahead and the reordered dispatch (N=1024, 32 particles,
    block 3). The error is numpy's, `particle` is the bad row, and the batch that follows is bitwise
    the clean batch run before it (no state survives a failed factorisation). LAPACK itself is
    checked on the same matrices: it fails for the bad particle and not for the good ones."""
    N, c0, P, env, bads = {"C_two_groups": (4096, 1000, 64, {}, (37, 5)),
                           "D_share": (4096, 1000, 32, {}, (17,)),
                           "E_persistent": (4096, 1000, 16, {"GPF_PERSIST": "1"}, (11,)),
                           "B_early_diag": (1024, 400, 32, {}, (20, 0))}[sched]
    x, y, e = _cluster_data(N, c0)
    import scipy.linalg as sl
    info = sl.lapack.dpotrf(_cluster_K(x, 0.2), lower=1)[1]  # LAPACK: the 1-based failing row
    assert c0 < info <= c0 + 20 and (info - 1) // 128 >= 3, info
    assert sl.lapack.dpotrf(_cluster_K(x, 0.02), lower=1)[1] == 0
    s, ex = ref_cpu.sigma_grid()
    lo, hi = ref_cpu.search_bounds(x)
    assert lo[0] < 0.011 and hi[0] > 0.2
    ctx.set_data(x, y, e)
    ctx.set_grid(s, ex, lo, hi)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    rng = np.random.default_rng(P)
    good = rng.uniform(0.011, 0.02, size=(P, 1))
    clean = ctx.eval_batch(good)
    assert np.all(np.isfinite(clean)) and np.all(clean < 1e13)
    for k in bads:
        Q = good.copy()
        Q[k, 0] = 0.2
        with pytest.raises(np.linalg.LinAlgError, match="Matrix is not positive definite") as ei:
            ctx.eval_batch(Q)
        assert ei.value.particle == k, (sched, k, ei.value.particle)
        np.testing.assert_array_equal(ctx.eval_batch(good), clean)
    # an exactly zero pivot (duplicate point, zero noise; the r5b tree's failure was this contract at
    # N = 4, where the pivot's rounding decides) in block >= 3 for every particle: the first live
    # particle is reported (row 0 is a sentinel and never reaches the GPU)
    xd, yd, ed = _cluster_data(N, c0, dup=True)
    assert sl.lapack.dpotrf(_cluster_K(xd, 0.02), lower=1)[1] == c0 + 32
    ctx.set_data(xd, yd, ed)
    Q = good.copy()
    Q[0, 0] = 2.0 * hi[0]
    with pytest.raises(np.linalg.LinAlgError, match="Matrix is not positive definite") as ei:
        ctx.eval_batch(Q)
    assert ei.value.particle == 1, (sched, ei.value.particle)
    ctx.set_data(x, y, e)
    np.testing.assert_array_equal(ctx.eval_batch(good), clean)


def test_not_pd_past_block3_in_prediction(ctx):
    """GP_func.GP (GP_fit.py:32 -> GP_func.py:22) through gpf_predict's single-particle schedule
    (the all-tile split with the flat finish and the early diagonal factor) at N=4096, failing
    pivot in block 7: raises numpy's error; a good length scale right after predicts normally, and
    within 1e-6 of the oracle (the reference op sequence)."""
    import GP_func
    N, c0 = 4096, 1000
    x, y, e = _cluster_data(N, c0)
    xf = x[:, c0 - 8:c0 + 24] + 0.004  # queries beside the last plain points and between cluster points
    with pytest.raises(np.linalg.LinAlgError, match="Matrix is not positive definite"):
        GP_func.GP(x, y, e, xf, np.array([0.2]))
    mu, sd = GP_func.GP(x, y, e, xf, np.array([0.015]))
    with _blas_threads():
        m0, s0 = ref_cpu.GP(x, y, e, xf, np.array([0.015]))
    assert _rel(mu, m0) < RTOL_MU_SD and _rel(sd, s0) < RTOL_MU_SD


@pytest.mark.parametrize("N,d,P,groups,paired", [(4096, 3, 64, None, True), (4096, 3, 32, None, True),
                                                  (3900, 2, 16, None, True), (512, 2, 8, None, True),
                                                  (2048, 4, 24, "1", True), (2049, 3, 40, "2", False)])
def test_paired_block_columns_bitwise(ctx, monkeypatch, N, d, P, groups, paired):
    """Paired block columns (gpf::pair_decode; r6): the lead launch J runs block column J+1's GEMMs
    over the columns < J beside the tiles that stream the same panels, the follow launch J+1 finishes
    from those partials. Every element sees the same MFMAs in the same order (a chain split at a
    chunk boundary with an exact store and reload), so scores, mean and sd are bitwise those of the
    unpaired launches: C (64 particles, two groups), D's share, an odd block-column count (nt = 31),
    the smallest paired nt (4), one group of 24, and 40 particles in two groups of 20 (not multiples
    of 8: unpaired, same results). Deterministic over two runs."""
    rng = np.random.default_rng(N + P)
    x = rng.uniform(size=(d, N))
    y = np.sum(np.sin(2 * np.pi * x), axis=0) + 0.1 * rng.standard_normal(N)
    e = rng.uniform(0.05, 0.2, size=N)
    s, ex = ref_cpu.sigma_grid()
    lo, hi = ref_cpu.search_bounds(x)
    ctx.set_data(x, y, e)
    ctx.set_grid(s, ex, lo, hi)
    Q = rng.uniform(0.1, 0.5, size=(P, d))
    monkeypatch.setenv("GPF_PERSIST", "0")
    monkeypatch.setenv("GPF_EARLY_DIAG", "0")  # (pairs run with the fused diagonal factor, unsplit)
    monkeypatch.setenv("GPF_SPLIT_K", "1")
    if groups:
        monkeypatch.setenv("GPF_GROUPS", groups)
    out = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("GPF_PAIR", mode)
        out[mode] = ctx.eval_batch(Q, want_mu_sd=True)
    again = ctx.eval_batch(Q, want_mu_sd=True)
    for a, b, c in zip(out["0"], out["1"], again):
        np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(b, c)
    import gpfit
    st = gpfit.plan_check(P, (N + 127) // 128)
    assert (st["lead_launches"] > 0) == paired, st
    if N <= 2049:
        mo, so = ref_cpu.GP_train_identity(x, y, e, Q[0])
        assert _rel(out["1"][1][0], mo) < RTOL_MU_SD and _rel(out["1"][2][0], so) < RTOL_MU_SD


@pytest.mark.parametrize("N,d,P,pb,first,frm", [(1024, 2, 32, "1", "1", "1"), (2049, 3, 12, "2", "0", "1"),
                                                (700, 4, 5, "3", "1", "2"), (1024, 2, 64, "1", "1", "-2"),
                                                (1024, 2, 32, "1", "1", "-2"), (2049, 3, 24, "1", "1", "-3")])
def test_all_tile_lookahead_pieces(ctx, monkeypatch, N, d, P, pb, first, frm):
    """All-tile look-ahead in pieces (GPF_LA_ALL; gpf::lall_decode, r6): launch J runs every GEMM of
    launch J+1 over the columns final before it, in pieces of <= 2 blocks, and launch J+1 sums them.
    Against the launches without it (GPF_LA_ALL=0): the partial sums round differently from one MFMA
    chain, so mean/sd within 1e-10 and the objective within 1e-10 or explained by threshold ties;
    deterministic over two runs; and against the oracle's identity form. Shapes: config B (32
    particles, nt = 8), nt = 17, nt = 6, and 64 particles (two groups, the piece buffer's parities
    per group)."""
    rng = np.random.default_rng(N * 7 + P)
    x = rng.uniform(size=(d, N))
    y = np.sum(np.sin(2 * np.pi * x), axis=0) + 0.1 * rng.standard_normal(N)
    e = rng.uniform(0.05, 0.2, size=N)
    s, ex = ref_cpu.sigma_grid()
    lo, hi = ref_cpu.search_bounds(x)
    ctx.set_data(x, y, e)
    ctx.set_grid(s, ex, lo, hi)
    Q = rng.uniform(0.1, 0.5, size=(P, d))
    monkeypatch.setenv("GPF_EARLY_DIAG", "1")
    monkeypatch.setenv("GPF_PERSIST", "0")
    monkeypatch.setenv("GPF_SPLIT_K", "1")
    monkeypatch.setenv("GPF_LA_ALL", "1")
    monkeypatch.setenv("GPF_LA_ALL_PB", pb)  # piece size in blocks
    monkeypatch.setenv("GPF_LA_ALL_FIRST", first)  # pieces ahead of the tiles
    monkeypatch.setenv("GPF_LA_ALL_FROM", frm)  # the first producing launch (negative: from nt)
    import gpfit
    st = gpfit.plan_check(P, (N + 127) // 128)
    g, gm, gs = ctx.eval_batch(Q, want_mu_sd=True)
    again = ctx.eval_batch(Q, want_mu_sd=True)
    for a, b in zip((g, gm, gs), again):
        np.testing.assert_array_equal(a, b)
    monkeypatch.setenv("GPF_LA_ALL", "0")
    w, wm, ws = ctx.eval_batch(Q, want_mu_sd=True)
    assert st["workgroups"] > gpfit.plan_check(P, (N + 127) // 128)["workgroups"]  # the pieces ran
    assert _rel(gm, wm) < 1e-10 and _rel(gs, ws) < 1e-10, (_rel(gm, wm), _rel(gs, ws))
    for k in range(P):
        if abs(g[k] - w[k]) > 1e-10 * abs(w[k]):
            assert_loss_or_ties(g[k], w[k], wm[k], ws[k], y, s, what=k)
    mo, so = ref_cpu.GP_train_identity(x, y, e, Q[0])
    assert _rel(gm[0], mo) < RTOL_MU_SD and _rel(gs[0], so) < RTOL_MU_SD


def test_scratch_buffers_across_schedules_on_one_context(monkeypatch):
    """Every scratch buffer of the factorisation (Scratch::grow, sized by plan_factor) on one live
    context, across grow / reuse / a larger chunk, at the smallest shape that uses them all (nt = 4:
    the floor of pairs, pieces and the split): the paired columns' partials and start words at 8 then
    16 particles (regrown, the start words re-zeroed on the stream), the piece buffer (its knobs set on
    top of the first steps', which keep the launches unsplit) and, with the pieces from launch 2 on, the
    critical-tile look-ahead buffer that feeds that launch, the split buffers of a single particle, then
    8 particles again. Each step's losses are bitwise those of the same call on a fresh context."""
    import gpfit
    N, d = 512, 2
    rng = np.random.default_rng(512)
    x = rng.uniform(size=(d, N))
    y = np.sum(np.sin(2 * np.pi * x), axis=0) + 0.1 * rng.standard_normal(N)
    e = rng.uniform(0.05, 0.2, size=N)
    s, ex = ref_cpu.sigma_grid()
    lo, hi = ref_cpu.search_bounds(x)
    Q = rng.uniform(0.1, 0.5, size=(16, d))
    pairs = {"GPF_PERSIST": "0", "GPF_EARLY_DIAG": "0", "GPF_SPLIT_K": "1", "GPF_PAIR": "1"}
    pieces = dict(pairs, GPF_EARLY_DIAG="1", GPF_LA_ALL="1", GPF_LA_ALL_FROM="1")
    pieces2 = dict(pieces, GPF_LA_ALL_FROM="2")
    steps = [(8, pairs), (16, pairs), (16, pieces), (16, pieces2), (1, {}), (8, {})]
    knobs = sorted(pieces)

    def fresh():
        c = gpfit.Context(0)
        c.set_data(x, y, e)
        c.set_grid(s, ex, lo, hi)
        return c

    live = fresh()
    try:
        for i, (P, kv) in enumerate(steps):
            for k in knobs:
                monkeypatch.delenv(k, raising=False)
            for k, v in kv.items():
                monkeypatch.setenv(k, v)
            st = gpfit.plan_check(P, 4)
            assert (st["lead_launches"] > 0) == (kv is pairs) and (st["split_tiles"] > 0) == (not kv), (i, st)
            if kv in (pieces, pieces2):  # unsplit early-diagonal launches with piece workgroups beside the tiles
                assert st["diag_workgroups"] == 4 * P and st["split_tiles"] == 0, (i, st)
                assert st["workgroups"] > st["whole_tiles"] + st["diag_workgroups"] + st["syrk_workgroups"], (i, st)
            got = live.eval_batch(Q[:P])
            ref = fresh()
            try:
                want = ref.eval_batch(Q[:P])
            finally:
                ref.close()
            np.testing.assert_array_equal(got, want, err_msg=f"step {i}: {P} particles, {kv}")
            assert np.all(np.isfinite(got)) and np.all(got < 1e13)
    finally:
        live.close()


def test_sentinels_never_reach_gpu_and_mix_with_live_particles(ctx, f2):
    x, y, e = f2["c0_x"], f2["c0_y"], f2["c0_e"]
    lo, hi = f2["c0_lo"], f2["c0_hi"]
    ctx.set_data(x, y, e)
    ctx.set_grid(f2["sigma_vals"], f2["expected"], lo, hi)
    P = np.stack([lo, hi, (lo + hi) / 2, lo - 1, np.array([lo[0], (lo[1] + hi[1]) / 2])])
    ctx.reset_profile()
    ctx.set_profiling(True)
    loss = ctx.eval_batch(P)
    prof = ctx.profile()
    ctx.set_profiling(False)
    assert loss[0] == loss[1] == loss[3] == loss[4] == 1e13
    assert loss[2] < 1e13
    assert prof["evals"] == 1


def test_chunked_batches_equal_single_batch(f3, monkeypatch):
    import gpfit
    i = 4
    x, y, e = f3[f"c{i}_x"], f3[f"c{i}_y"], f3[f"c{i}_e"]
    s, ex, lo, hi, P = f3["sigma_vals"], f3["expected"], f3[f"c{i}_lo"], f3[f"c{i}_hi"], f3[f"c{i}_P"]
    a = gpfit.Context(0)
    a.set_data(x, y, e); a.set_grid(s, ex, lo, hi)
    full = a.eval_batch(P)
    a.close()
    monkeypatch.setenv("GPF_MAX_CHUNK", "3")
    b = gpfit.Context(0)
    b.set_data(x, y, e); b.set_grid(s, ex, lo, hi)
    chunked = b.eval_batch(P)
    b.close()
    np.testing.assert_array_equal(full, chunked)


@pytest.mark.parametrize("N,d,M", [(1500, 2, 20000), (4096, 3, 3000)])
def test_predict_chunking_bitwise(ctx, N, d, M):
    """gpf_predict with the queries in one chunk and in chunks of 16384 (the reference's
    batch_size only bounds its own memory, GP_func.py:28-30): the same kernels per query column,
    so mu and sd bitwise equal; mu = sum_t V_t^T z_t (no alpha) against the oracle's GP() on a
    sample of the queries."""
    rng = np.random.default_rng(N + M)
    x = rng.uniform(size=(d, N))
    y = np.sin(5 * x[0]) * np.cos(2 * x[-1]) + 0.1 * rng.standard_normal(N)
    e = rng.uniform(0.05, 0.2, size=N)
    xf = rng.uniform(-0.1, 1.1, size=(d, M))
    ls = rng.uniform(0.1, 0.4, size=d)
    ctx.set_data(x, y, e)
    a = ctx.predict(ls, xf, batch_size=M)
    b = ctx.predict(ls, xf, batch_size=1000)
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])
    k = np.linspace(0, M - 1, 64).astype(int)
    with _blas_threads():
        m0, s0 = ref_cpu.GP(x, y, e, xf[:, k], ls, batch_size=10000)
    assert _rel(a[0][k], m0) < RTOL_MU_SD and _rel(a[1][k], s0) < RTOL_MU_SD


def test_predict_ill_conditioned_vs_reference(ctx):
    """The prediction's mean is formed as sum_t V_t^T z_t, not the reference's K_s^T alpha
    (GP_func.py:36): on an ill-conditioned K (small noise, clustered training points, long length
    scale) the two summation orders still agree with the reference's GP() to 1e-6."""
    rng = np.random.default_rng(77)
    N, d = 600, 2
    x = np.concatenate([rng.uniform(0.0, 0.3, size=(d, N // 2)), 0.3 + 0.002 * rng.standard_normal((d, N // 2))], axis=1)
    y = np.sin(4 * x[0]) + x[1] ** 2 + 0.01 * rng.standard_normal(N)
    e = np.full(N, 0.01)
    ls = np.array([0.45, 0.5])
    xf = rng.uniform(-0.05, 0.4, size=(d, 3000))
    ctx.set_data(x, y, e)
    mu, sd = ctx.predict(ls, xf)
    m0, s0 = ref_cpu.GP(x, y, e, xf, ls, batch_size=10000)
    assert _rel(mu, m0) < RTOL_MU_SD and _rel(sd, s0) < RTOL_MU_SD


@pytest.mark.parametrize("keep_mb", [None, "0"])
def test_predict_buffer_reuse_across_calls(monkeypatch, keep_mb):
    """gpf_predict keeps its query-chunk buffers in the context between calls (grow-only): a
    call after a larger one runs with a smaller leading dimension inside the bigger buffers, a
    call after set_data with another N reallocates. Every result equals that of a fresh context
    bit for bit. With GPF_PREDICT_KEEP_MB=0 (buffers larger than the bound are freed at the end
    of each call, so a huge batch cannot pin HBM) the results are the same."""
    import gpfit
    if keep_mb is not None:
        monkeypatch.setenv("GPF_PREDICT_KEEP_MB", keep_mb)
    rng = np.random.default_rng(17)
    datasets = []
    for N, d in ((300, 2), (700, 3)):
        x = rng.uniform(size=(d, N))
        y = np.sin(4 * x[0]) + 0.1 * rng.standard_normal(N)
        datasets.append((x, y, rng.uniform(0.05, 0.2, size=N), rng.uniform(0.1, 0.5, size=d)))
    calls = [(0, 200), (0, 3000), (0, 130), (1, 1000), (1, 64), (0, 500)]
    a = gpfit.Context(0)
    kept = []
    cur = None
    for k, m in calls:
        x, y, e, ls = datasets[k]
        if cur != k:
            a.set_data(x, y, e)
            cur = k
        xf = rng.uniform(size=(x.shape[0], m))
        kept.append((k, xf, a.predict(ls, xf)))
    a.close()
    for k, xf, (mu, sd) in kept:
        x, y, e, ls = datasets[k]
        b = gpfit.Context(0)
        b.set_data(x, y, e)
        mu0, sd0 = b.predict(ls, xf)
        b.close()
        np.testing.assert_array_equal(mu, mu0)
        np.testing.assert_array_equal(sd, sd0)


def test_graph_replay_equals_plain_launches(f2, monkeypatch):
    """Small batches (N <= 256) replay a captured HIP graph padded to all P slots; the scores
    equal the plain launch path bit for bit, across changing sentinel patterns and reuse."""
    import gpfit
    x, y, e = _fx(f2["c0_x"]), f2["c0_y"], f2["c0_e"]
    lo, hi = ref_cpu.search_bounds(x)
    s, ex = ref_cpu.sigma_grid()
    rng = np.random.default_rng(11)
    batches = []
    for _ in range(4):
        pos = lo + (hi - lo) * rng.uniform(-0.2, 1.2, size=(40, x.shape[0]))  # some land outside: sentinels
        batches.append(pos)
    a = gpfit.Context(0)
    a.set_data(x, y, e); a.set_grid(s, ex, lo, hi)
    with_graph = [a.eval_batch(p) for p in batches]
    a.close()
    monkeypatch.setenv("GPF_NO_GRAPH", "1")
    b = gpfit.Context(0)
    b.set_data(x, y, e); b.set_grid(s, ex, lo, hi)
    plain = [b.eval_batch(p) for p in batches]
    b.close()
    for g, q in zip(with_graph, plain):
        np.testing.assert_array_equal(g, q)
    assert any((g == 1e13).any() for g in with_graph) and any((g < 1e13).any() for g in with_graph)


def test_log_marginal_likelihood_vs_oracle(ctx, f3):
    for i in [0, 4]:
        x, y, e, P = f3[f"c{i}_x"], f3[f"c{i}_y"], f3[f"c{i}_e"], f3[f"c{i}_P"]
        ctx.set_data(x, y, e)
        got = ctx.log_marginal_likelihood(P[0])
        want = ref_cpu.log_marginal_likelihood(x, y, e, P[0])
        assert abs(got - want) / abs(want) < 1e-9


def test_bad_dimension_is_value_error(ctx):
    with pytest.raises(ValueError):
        ctx.set_data(np.zeros((40, 5)), np.zeros(5), np.ones(5))


@pytest.mark.parametrize("N,d", [(4096, 3)])
def test_headline_size_vs_oracle_identity(ctx, N, d):
    """BASELINE config C size: every particle's mean/sd against the oracle's identity form,
    its objective against the oracle's scoring of those (1e-8, or threshold ties), and
    permutation invariance (size independent)."""
    rng = np.random.default_rng(1)
    x = rng.uniform(0, 1, size=(d, N))
    y = np.sum(np.sin(2 * np.pi * x), axis=0) + 0.1 * rng.standard_normal(N)
    e = np.full(N, 0.1)
    lo, hi = ref_cpu.search_bounds(x)
    s, ex = ref_cpu.sigma_grid()
    P = rng.uniform(0.05, 0.6, size=(3, d))
    ctx.set_data(x, y, e)
    ctx.set_grid(s, ex, lo, hi)
    loss, mu, sd = ctx.eval_batch(P, want_mu_sd=True)
    with _blas_threads():
        for k in range(3):
            m0, s0 = ref_cpu.GP_train_identity(x, y, e, P[k])
            assert _rel(mu[k], m0) < RTOL_MU_SD and _rel(sd[k], s0) < RTOL_MU_SD
            w = ref_cpu.coverage_loss(m0, s0, y, s, ex) + 0.01 * ref_cpu.proximity_penalty(P[k], lo, hi)
            assert_loss_or_ties(loss[k], w, m0, s0, y, s, what=k)
    perm = rng.permutation(N)
    ctx.set_data(x[:, perm], y[perm], e[perm])
    lp = ctx.eval_batch(P)
    for k in range(3):
        assert_loss_or_ties(lp[k], loss[k], mu[k][perm], sd[k][perm], y[perm], s, what=k)


def test_large_hetero_vs_oracle_identity(ctx):
    """Config E's regime (d=4, heteroscedastic noise) at N=8192: 64 block columns, every
    k_step path (fused K tiles, streamed dense and triangular runs, fused diagonals) at a
    depth the N<=4096 cases do not reach. Every particle's mean/sd against the oracle's
    identity form, objective at 1e-8 or threshold ties."""
    N, d = 8192, 4
    rng = np.random.default_rng(7)
    x = rng.uniform(0, 1, size=(d, N))
    y = np.sum(np.sin(2 * np.pi * x), axis=0) + 0.1 * rng.standard_normal(N)
    e = rng.uniform(0.05, 0.2, size=N)
    lo, hi = ref_cpu.search_bounds(x)
    s, ex = ref_cpu.sigma_grid()
    P = rng.uniform(0.1, 0.5, size=(2, d))
    ctx.set_data(x, y, e)
    ctx.set_grid(s, ex, lo, hi)
    loss, mu, sd = ctx.eval_batch(P, want_mu_sd=True)
    with _blas_threads():
        for k in range(2):
            m1, s1 = ref_cpu.GP_train_identity(x, y, e, P[k])
            assert _rel(mu[k], m1) < RTOL_MU_SD and _rel(sd[k], s1) < RTOL_MU_SD
            w = ref_cpu.coverage_loss(m1, s1, y, s, ex) + 0.01 * ref_cpu.proximity_penalty(P[k], lo, hi)
            assert_loss_or_ties(loss[k], w, m1, s1, y, s, what=k)


@pytest.mark.parametrize("split", [2, 7])
def test_split_k_matches_unsplit_and_oracle(ctx, monkeypatch, split):
    """Split-K launches (gpf::split_part: partial GEMMs summed by the last workgroup to arrive)
    against the unsplit path and the oracle. GPF_SPLIT_K forces the split factor."""
    N, d = 1000, 3
    rng = np.random.default_rng(11)
    x = rng.uniform(size=(d, N))
    y = np.sin(4 * x[0]) + x[1] * x[2] + 0.1 * rng.standard_normal(N)
    e = rng.uniform(0.05, 0.2, size=N)
    s, ex = ref_cpu.sigma_grid()
    lo, hi = ref_cpu.search_bounds(x)
    P = rng.uniform(0.1, 0.5, size=(4, d))
    ctx.set_data(x, y, e)
    ctx.set_grid(s, ex, lo, hi)
    monkeypatch.setenv("GPF_SPLIT_K", "1")
    l1, m1, s1 = ctx.eval_batch(P, want_mu_sd=True)
    monkeypatch.setenv("GPF_SPLIT_K", str(split))
    l2, m2, s2 = ctx.eval_batch(P, want_mu_sd=True)
    l3, m3, s3 = ctx.eval_batch(P, want_mu_sd=True)
    np.testing.assert_array_equal(m2, m3)  # deterministic: partials summed in slot order
    assert _rel(m2, m1) < 1e-10 and _rel(s2, s1) < 1e-10
    assert _rel(l2, l1) < RTOL_LOSS
    mo, so = ref_cpu.GP_train_identity(x, y, e, P[2])
    assert _rel(m2[2], mo) < RTOL_MU_SD and _rel(s2[2], so) < RTOL_MU_SD


@pytest.mark.parametrize("N,d", [(700, 2), (1920, 3)])
def test_all_tile_split_live_counts(ctx, monkeypatch, N, d):
    """The all-tile split with its flat finish (gpf::flat_piece) forced on a multi-particle batch
    (GPF_SPLIT_K=2; by default it runs for launches of <= 64 tiles only) across changing
    live-particle counts (sentinels never run; buffers grow between batches): more workgroups than
    CUs (at least 4 pieces per tile), deterministic, and within 1e-10 of the unsplit path.
    (r5: replaces the critical-tile split's test; that split was removed.)"""
    rng = np.random.default_rng(N + d)
    x = rng.uniform(size=(d, N))
    y = np.sin(3 * x[0]) + 0.1 * rng.standard_normal(N)
    e = rng.uniform(0.05, 0.2, size=N)
    s, ex = ref_cpu.sigma_grid()
    lo, hi = ref_cpu.search_bounds(x)
    ctx.set_data(x, y, e)
    ctx.set_grid(s, ex, lo, hi)
    P = rng.uniform(0.1, 0.5, size=(24, d))
    masks = [np.arange(24) % 3 == 0, np.zeros(24, bool), np.arange(24) % 5 == 1, np.arange(24) % 3 == 0]
    got = []
    for m in masks:
        Q = P.copy()
        Q[m, 0] = hi[0] + 1.0  # sentinels: outside the box
        monkeypatch.setenv("GPF_SPLIT_K", "2")
        g, gm, gs = ctx.eval_batch(Q, want_mu_sd=True)
        np.testing.assert_array_equal(g, ctx.eval_batch(Q))  # deterministic
        monkeypatch.setenv("GPF_SPLIT_K", "1")
        w, wm, ws = ctx.eval_batch(Q, want_mu_sd=True)
        monkeypatch.delenv("GPF_SPLIT_K", raising=False)
        assert np.all(g[m] == 1e13)
        live = ~m
        assert _rel(gm[live], wm[live]) < 1e-10 and _rel(gs[live], ws[live]) < 1e-10
        # the objective within 1e-10 of the unsplit path like mean/sd (no blanket 1e-8),
        # unless a pull of the unsplit run sits at |pull| = 1, where the two correct fp64 runs may
        # count one coverage point differently (assert_loss_or_ties bounds that difference)
        for k in np.flatnonzero(live):
            if abs(g[k] - w[k]) > 1e-10 * abs(w[k]):
                assert_loss_or_ties(g[k], w[k], wm[k], ws[k], y, s, what=k)
        got.append(g)
    np.testing.assert_array_equal(got[0], got[3])


@pytest.mark.parametrize("N", [2048, 4096])
def test_single_particle_split_factor_tight(ctx, monkeypatch, N):
    """The single-particle factorisation (the prediction's schedule: the all-tile split with the
    flat finish, every tile cut into >= 4 pieces, deep launches up to nt = 32) against the unsplit
    launches (GPF_SPLIT_K=1), factor by factor (the flat finish had no tight independent
    check). The split sums each tile's partial products in slot order instead of one MFMA chain, so
    the two differ by rounding only: L, U = L^-1, z and alpha within 1e-11 of their largest entry
    (normwise; their condition grows with N/e^2, ~1e5 here). The split run is repeated three
    times and must be bitwise deterministic — a race in the finish (e.g. an LDS hand-over area
    overwritten) shows up as a mismatch here."""
    rng = np.random.default_rng(N)
    d = 3
    x = rng.uniform(size=(d, N))
    y = np.sum(np.sin(2 * np.pi * x), axis=0) + 0.1 * rng.standard_normal(N)
    e = rng.uniform(0.05, 0.2, size=N)
    s, ex = ref_cpu.sigma_grid()
    lo, hi = ref_cpu.search_bounds(x)
    ctx.set_data(x, y, e)
    ctx.set_grid(s, ex, lo, hi)
    ls = np.array([0.3, 0.25, 0.4])
    monkeypatch.delenv("GPF_SPLIT_K", raising=False)
    runs = [ctx.debug_factor(ls) for _ in range(3)]
    for r in runs[1:]:
        for a, b in zip(runs[0], r):
            np.testing.assert_array_equal(np.tril(a) if a.ndim == 2 else a, np.tril(b) if b.ndim == 2 else b)
    monkeypatch.setenv("GPF_SPLIT_K", "1")
    ref = ctx.debug_factor(ls)
    monkeypatch.delenv("GPF_SPLIT_K")
    for name, a, b in zip(("L", "U", "z", "alpha"), runs[0], ref):
        a, b = (np.tril(a)[:N, :N], np.tril(b)[:N, :N]) if a.ndim == 2 else (a[:N], b[:N])
        err = np.max(np.abs(a - b)) / np.max(np.abs(b))  # normwise: small entries carry absolute rounding
        print(f"N={N} {name}: max |split - unsplit| / max |unsplit| = {err:.2e}")
        assert err < 1e-11, (name, err)


@pytest.mark.parametrize("N,d,hetero,seed", [(130, 1, False, 1), (383, 5, True, 2), (512, 2, True, 3),
                                             (777, 3, False, 4), (1500, 4, True, 5), (2049, 2, False, 6)])
def test_random_configs_vs_oracle(ctx, N, d, hetero, seed):
    """Sweep of sizes off the tile grid, dimensionalities 1..5 and both noise models: every
    particle's mean/sd against the oracle (the reference op sequence up to N=777, the identity
    form above) and the objective against the oracle's scoring of those."""
    rng = np.random.default_rng(100 + seed)
    x = rng.uniform(0, 1, size=(d, N))
    y = np.sum(np.cos(3 * x), axis=0) + 0.05 * rng.standard_normal(N)
    e = rng.uniform(0.05, 0.2, size=N) if hetero else np.full(N, 0.1)
    s, ex = ref_cpu.sigma_grid()
    lo, hi = ref_cpu.search_bounds(x)
    P = rng.uniform(0.08, 0.6, size=(3, d))
    ctx.set_data(x, y, e)
    ctx.set_grid(s, ex, lo, hi)
    loss, mu, sd = ctx.eval_batch(P, want_mu_sd=True)
    for k in range(3):
        if N <= 777:
            m0, s0 = ref_cpu.GP(x, y, e, x, P[k], batch_size=N)
        else:
            m0, s0 = ref_cpu.GP_train_identity(x, y, e, P[k])
        assert _rel(mu[k], m0) < RTOL_MU_SD and _rel(sd[k], s0) < RTOL_MU_SD
        w = ref_cpu.coverage_loss(m0, s0, y, s, ex) + 0.01 * ref_cpu.proximity_penalty(P[k], lo, hi)
        assert_loss_or_ties(loss[k], w, m0, s0, y, s, what=k)


def _reference_share(ctx, monkeypatch, fx, P, slots, rounds=2):
    """Score P (with the fixture's particles at `slots`) on the default schedule, twice; then without
    the look-ahead pieces (GPF_LA_ALL=0: within 1e-10), and that bitwise against the persistent
    factorisation (GPF_PERSIST=1) and the per-block-column launches with one particle group
    (GPF_PERSIST=0, GPF_GROUPS=1); returns (loss, mu, sd) of the default run."""
    from conftest import fixture_data
    x, y, e = fixture_data(fx["meta"], fx["data_sha256"])
    ctx.set_data(x, y, e)
    ctx.set_grid(fx["sigma_vals"], fx["expected"], fx["lo"], fx["hi"])
    monkeypatch.delenv("GPF_GROUPS", raising=False)
    monkeypatch.delenv("GPF_PERSIST", raising=False)
    runs = [ctx.eval_batch(P, want_mu_sd=True) for _ in range(rounds)]
    for a, b in zip(runs[0], runs[1]):
        np.testing.assert_array_equal(a, b)  # deterministic
    # (r6) the early-diagonal launches' look-ahead pieces (config B's last launch) sum partials, which
    # rounds differently from one MFMA chain: the bitwise schedule comparisons run without them, and
    # the default run is within 1e-10 of that (the objective also, or explained by threshold ties)
    monkeypatch.setenv("GPF_LA_ALL", "0")
    base = ctx.eval_batch(P, want_mu_sd=True)
    assert _rel(runs[0][1], base[1]) < 1e-10 and _rel(runs[0][2], base[2]) < 1e-10
    for k in range(P.shape[0]):
        if abs(runs[0][0][k] - base[0][k]) > 1e-10 * abs(base[0][k]):
            assert_loss_or_ties(runs[0][0][k], base[0][k], base[1][k], base[2][k], y, fx["sigma_vals"], what=k)
    for persist, groups in (("1", None), ("0", "1")):
        monkeypatch.setenv("GPF_PERSIST", persist)
        if groups:
            monkeypatch.setenv("GPF_GROUPS", groups)
        other = ctx.eval_batch(P, want_mu_sd=True)
        for a, b in zip(base, other):
            np.testing.assert_array_equal(a, b)  # the schedule changes, not the arithmetic
    monkeypatch.delenv("GPF_GROUPS", raising=False)
    monkeypatch.delenv("GPF_PERSIST", raising=False)
    monkeypatch.delenv("GPF_LA_ALL", raising=False)
    loss, mu, sd = runs[0]
    for j, k in enumerate(slots):
        assert _rel(mu[k], fx["mu"][j]) < RTOL_MU_SD, j
        assert _rel(sd[k], fx["sd"][j]) < RTOL_MU_SD, j
        assert_loss_or_ties(loss[k], fx["loss"][j], fx["mu"][j], fx["sd"][j], y, fx["sigma_vals"], what=j)
    return x, y, e, loss, mu, sd


def test_configD_share_two_groups_vs_reference(ctx, monkeypatch):
    """Config D's per-GPU share (N=4096 d=3, 32 particles) on its default schedule: two particle
    groups on concurrent streams (gpfit.plan_check). The 4 particles of F8 (the reference's own
    evaluate_loss and the GP() mu/sd inside it, make_golden_big.py) sit among 28 others: mu/sd
    at 1e-6, objective at 1e-8 or threshold ties; deterministic; bitwise equal to the persistent
    factorisation and to one group; 4 of the others against the oracle's identity form."""
    import gpfit
    from conftest import load_golden
    assert gpfit.plan_check(32, 32)["groups"] == 2
    fx = load_golden("f8_configC.npz")
    rng = np.random.default_rng(404)
    P = rng.uniform(0.05, 0.6, size=(32, 3))
    slots = [0, 9, 18, 31]
    P[slots] = fx["P"]
    x, y, e, loss, mu, sd = _reference_share(ctx, monkeypatch, fx, P, slots)
    s, ex, lo, hi = fx["sigma_vals"], fx["expected"], fx["lo"], fx["hi"]
    with _blas_threads():
        for k in (1, 8, 16, 30):
            m0, s0 = ref_cpu.GP_train_identity(x, y, e, P[k])
            assert _rel(mu[k], m0) < RTOL_MU_SD and _rel(sd[k], s0) < RTOL_MU_SD
            w = ref_cpu.coverage_loss(m0, s0, y, s, ex) + 0.01 * ref_cpu.proximity_penalty(P[k], lo, hi)
            assert_loss_or_ties(loss[k], w, m0, s0, y, s, what=k)


def test_configC_full_swarm_vs_reference(ctx, monkeypatch):
    """BASELINE config C exactly as bench.py times it: N=4096 d=3, one 64-particle batch on the
    default schedule (two particle groups of 32 on concurrent streams, 992 workgroups per
    launch, two slot rounds). The 4 particles of F8 (the reference's evaluate_loss and the GP()
    mu/sd inside it, make_golden_big.py) sit among 60 others, two in each group: mu/sd at 1e-6,
    objective at 1e-8 or threshold ties; deterministic; bitwise equal to the persistent
    factorisation (4 different work queues) and to one group; 4 further particles against the
    oracle's identity form."""
    import gpfit
    from conftest import load_golden
    plan = gpfit.plan_check(64, 32)
    assert plan["groups"] == 2 and plan["diag_workgroups"] == 0  # the slot-bound fused schedule
    fx = load_golden("f8_configC.npz")
    rng = np.random.default_rng(6464)
    P = rng.uniform(0.05, 0.6, size=(64, 3))
    slots = [0, 21, 40, 63]  # launch groups [0, 32) and [32, 64); persistent queues p mod 8 = 0, 5, 0, 7
    P[slots] = fx["P"]
    x, y, e, loss, mu, sd = _reference_share(ctx, monkeypatch, fx, P, slots)
    s, ex, lo, hi = fx["sigma_vals"], fx["expected"], fx["lo"], fx["hi"]
    with _blas_threads():
        for k in (7, 31, 32, 55):
            m0, s0 = ref_cpu.GP_train_identity(x, y, e, P[k])
            assert _rel(mu[k], m0) < RTOL_MU_SD and _rel(sd[k], s0) < RTOL_MU_SD
            w = ref_cpu.coverage_loss(m0, s0, y, s, ex) + 0.01 * ref_cpu.proximity_penalty(P[k], lo, hi)
            assert_loss_or_ties(loss[k], w, m0, s0, y, s, what=k)


def test_configB_schedule_vs_reference(ctx, monkeypatch):
    """BASELINE config B exactly as bench.py times it: N=1024 d=2 with §8d's seed 0, one
    32-particle batch on B's default schedule (the early diagonal factor: launch J starts with
    one diagonal workgroup per particle that publishes block J through a flag; one group). The 8
    particles of F11 (the reference's evaluate_loss and its GP() mu/sd on exactly this data,
    make_golden_big.py) sit among 24 others: mu/sd at 1e-6, objective at 1e-8 or threshold ties;
    deterministic across runs; and the 24 others against the oracle's identity form."""
    import gpfit
    from conftest import load_golden
    plan = gpfit.plan_check(32, 8)
    assert plan["diag_workgroups"] == 32 * 8 and plan["groups"] == 1 and plan["S"] == 1
    fx = load_golden("f11_configB.npz")
    rng = np.random.default_rng(1024)
    P = rng.uniform(0.05, 0.6, size=(32, 2))
    slots = [0, 3, 8, 13, 17, 22, 27, 31]
    P[slots] = fx["P"]
    x, y, e, loss, mu, sd = _reference_share(ctx, monkeypatch, fx, P, slots, rounds=3)
    s, ex, lo, hi = fx["sigma_vals"], fx["expected"], fx["lo"], fx["hi"]
    for k in (k for k in range(32) if k not in slots):
        m0, s0 = ref_cpu.GP_train_identity(x, y, e, P[k])
        assert _rel(mu[k], m0) < RTOL_MU_SD and _rel(sd[k], s0) < RTOL_MU_SD, k
        w = ref_cpu.coverage_loss(m0, s0, y, s, ex) + 0.01 * ref_cpu.proximity_penalty(P[k], lo, hi)
        assert_loss_or_ties(loss[k], w, m0, s0, y, s, what=k)


def _config_e_fixture():
    """F9 and F9b (two more reference-scored particles on the same data) as one fixture."""
    from conftest import load_golden
    a = load_golden("f9_configE.npz")
    fx = {k: a[k] for k in a.files}
    b = load_golden("f9b_configE.npz")
    assert str(b["data_sha256"]) == str(fx["data_sha256"])
    for k in ("P", "loss", "mu", "sd"):
        fx[k] = np.concatenate([fx[k], b[k]])
    return fx


def test_configE_share_two_groups_vs_reference(ctx, monkeypatch):
    """Config E's per-GPU share (N=16384 d=4 heteroscedastic, 16 particles, 128 block columns)
    on its default schedule (the persistent factorisation). The 4 particles of F9 + F9b (the
    reference's evaluate_loss at this size, make_golden_big.py) among 12 others: mu/sd at 1e-6,
    objective at 1e-8 or threshold ties; deterministic; bitwise equal to the per-block-column
    launches (two groups and one); and 2 of the 12 others against the oracle's identity form
    (dpotrf + dtrtri on the host)."""
    import gpfit
    assert gpfit.plan_check(16, 128)["persistent"] == 1
    fx = _config_e_fixture()
    rng = np.random.default_rng(1604)
    P = rng.uniform(0.05, 0.6, size=(16, 4))
    slots = [3, 6, 12, 15]
    P[slots] = fx["P"]
    x, y, e, loss, mu, sd = _reference_share(ctx, monkeypatch, fx, P, slots)
    s, ex, lo, hi = fx["sigma_vals"], fx["expected"], fx["lo"], fx["hi"]
    with _blas_threads():
        for k in (0, 9):
            m0, s0 = ref_cpu.GP_train_identity_tri(x, y, e, P[k])
            assert _rel(mu[k], m0) < RTOL_MU_SD and _rel(sd[k], s0) < RTOL_MU_SD, k
            w = ref_cpu.coverage_loss(m0, s0, y, s, ex) + 0.01 * ref_cpu.proximity_penalty(P[k], lo, hi)
            assert_loss_or_ties(loss[k], w, m0, s0, y, s, what=k)


@pytest.mark.parametrize("N,d,P", [(1000, 3, 24), (2048, 2, 13), (1536, 4, 3), (4096, 3, 64)])
def test_persistent_factor_bitwise(ctx, monkeypatch, N, d, P):
    """The persistent factorisation (gpf::k_factor: one launch, items taken from per-XCD work
    queues in dependency order, hand-offs through per-particle counters) runs the arithmetic of
    the per-block-column launches: scores, mean and sd bitwise equal to GPF_PERSIST=0, for queue
    counts 8 (P = 24, 64), 8 with uneven queues (P = 13) and 3 (P = 3); one particle against the
    oracle's identity form; the host-side plan check decodes the same queues. (The launches
    compared against are unsplit: split-K pieces would sum in another order.)"""
    import gpfit
    rng = np.random.default_rng(N + 31 * P + d)
    x = rng.uniform(size=(d, N))
    y = np.sin(3 * x[0]) + x[-1] ** 2 + 0.1 * rng.standard_normal(N)
    e = rng.uniform(0.05, 0.2, size=N)
    s, ex = ref_cpu.sigma_grid()
    lo, hi = ref_cpu.search_bounds(x)
    ctx.set_data(x, y, e)
    ctx.set_grid(s, ex, lo, hi)
    Q = rng.uniform(0.08, 0.5, size=(P, d))
    monkeypatch.setenv("GPF_PERSIST", "1")
    assert gpfit.plan_check(P, -(-N // 128))["persistent"] == 1
    on = ctx.eval_batch(Q, want_mu_sd=True)
    again = ctx.eval_batch(Q, want_mu_sd=True)
    monkeypatch.setenv("GPF_PERSIST", "0")
    monkeypatch.setenv("GPF_SPLIT_K", "1")  # (few-tile launches would otherwise sum split-K pieces: other rounding)
    monkeypatch.setenv("GPF_LA_ALL", "0")  # (likewise the early-diagonal launches' look-ahead pieces, r6)
    off = ctx.eval_batch(Q, want_mu_sd=True)
    monkeypatch.delenv("GPF_PERSIST")
    monkeypatch.delenv("GPF_SPLIT_K")
    monkeypatch.delenv("GPF_LA_ALL")
    for a, b, c in zip(on, again, off):
        np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(a, c)
    if N <= 2048:
        mo, so = ref_cpu.GP_train_identity(x, y, e, Q[-1])
        assert _rel(on[1][-1], mo) < RTOL_MU_SD and _rel(on[2][-1], so) < RTOL_MU_SD


def test_persistent_timeout_reported_then_correct(ctx, monkeypatch):
    """A hand-off wait of the persistent factorisation that times out (GPF_WAIT_SPINS=0) sets the
    abort word, every other wait gives up, the launch drains and the host reports the timeout;
    the next batch (k_build_cov resets the counters, the queue heads and the abort word) is
    bitwise equal to a clean run."""
    N, d = 2048, 3
    rng = np.random.default_rng(2718)
    x = rng.uniform(size=(d, N))
    y = np.cos(5 * x[1]) + 0.1 * rng.standard_normal(N)
    e = np.full(N, 0.1)
    s, ex = ref_cpu.sigma_grid()
    lo, hi = ref_cpu.search_bounds(x)
    ctx.set_data(x, y, e)
    ctx.set_grid(s, ex, lo, hi)
    Q = rng.uniform(0.1, 0.5, size=(48, d))
    monkeypatch.setenv("GPF_PERSIST", "1")
    want = ctx.eval_batch(Q)
    monkeypatch.setenv("GPF_WAIT_SPINS", "0")
    with pytest.raises(RuntimeError, match="timed out"):
        ctx.eval_batch(Q)
    monkeypatch.delenv("GPF_WAIT_SPINS")
    np.testing.assert_array_equal(ctx.eval_batch(Q), want)
    monkeypatch.delenv("GPF_PERSIST")


@pytest.mark.parametrize("N,d,P", [(1024, 2, 12), (2048, 3, 32)])
def test_critical_tile_lookahead_bitwise(ctx, monkeypatch, N, d, P):
    """The critical-tile look-ahead (gpf::la_item: launch J's SYRK workgroups run the first 7/16 of
    the next critical tile's GEMM, launch J+1 continues from the stored partial; on by default for
    early-diagonal launches without split) runs the same MFMAs in the same order as the unsplit
    tile: scores, mean and sd bitwise equal with it off (GPF_LOOKAHEAD=0), on one particle group
    (N=1024, 12 particles) and on two concurrent groups (N=2048, 32 particles: 2 x 16, each with
    its own look-ahead partials), and the two-group schedule bitwise equal to one group."""
    import gpfit
    rng = np.random.default_rng(N + P + 7)
    x = rng.uniform(size=(d, N))
    y = np.cos(4 * x[0]) + x[-1] + 0.1 * rng.standard_normal(N)
    e = rng.uniform(0.05, 0.2, size=N)
    s, ex = ref_cpu.sigma_grid()
    lo, hi = ref_cpu.search_bounds(x)
    ctx.set_data(x, y, e)
    ctx.set_grid(s, ex, lo, hi)
    Q = rng.uniform(0.1, 0.5, size=(P, d))
    st = gpfit.plan_check(P, -(-N // 128))
    assert st["diag_workgroups"] > 0 and st["S"] == 1  # the early-diagonal, unsplit schedule
    on = ctx.eval_batch(Q, want_mu_sd=True)
    monkeypatch.setenv("GPF_LOOKAHEAD", "0")
    off = ctx.eval_batch(Q, want_mu_sd=True)
    monkeypatch.delenv("GPF_LOOKAHEAD")
    for a, b in zip(on, off):
        np.testing.assert_array_equal(a, b)
    if P >= 16:
        monkeypatch.setenv("GPF_GROUPS", "1")
        one = ctx.eval_batch(Q, want_mu_sd=True)
        monkeypatch.delenv("GPF_GROUPS")
        for a, b in zip(on, one):
            np.testing.assert_array_equal(a, b)
    mo, so = ref_cpu.GP_train_identity(x, y, e, Q[0])
    assert _rel(on[1][0], mo) < RTOL_MU_SD and _rel(on[2][0], so) < RTOL_MU_SD


@pytest.mark.gpu
@pytest.mark.parametrize("N,d,P", [(1024, 2, 32), (2048, 3, 20), (1500, 2, 7)])
def test_reordered_dispatch_bitwise(ctx, monkeypatch, N, d, P):
    """The reordered dispatch of early-diagonal launches with SYRK workgroups (r4, gpf::step_decode
    ro: the light U tiles first, then the diagonal workgroups, the other tiles, the SYRK workgroups
    last, so that the diagonal factors do not share their CUs) only changes which workgroup runs
    where: scores, mean and sd bitwise equal with it off (GPF_REORDER=0), config B's shape included."""
    import gpfit
    rng = np.random.default_rng(N + 3 * P)
    x = rng.uniform(size=(d, N))
    y = np.sin(3 * x[0]) + x[-1] ** 2 + 0.1 * rng.standard_normal(N)
    e = rng.uniform(0.05, 0.2, size=N)
    s, ex = ref_cpu.sigma_grid()
    lo, hi = ref_cpu.search_bounds(x)
    ctx.set_data(x, y, e)
    ctx.set_grid(s, ex, lo, hi)
    Q = rng.uniform(0.1, 0.5, size=(P, d))
    st = gpfit.plan_check(P, -(-N // 128))
    assert st["diag_workgroups"] > 0 and st["syrk_workgroups"] > 0 and st["S"] == 1
    on = ctx.eval_batch(Q, want_mu_sd=True)
    monkeypatch.setenv("GPF_REORDER", "0")
    off = ctx.eval_batch(Q, want_mu_sd=True)
    monkeypatch.delenv("GPF_REORDER")
    for a, b in zip(on, off):
        np.testing.assert_array_equal(a, b)
    mo, so = ref_cpu.GP_train_identity(x, y, e, Q[-1])
    assert _rel(on[1][-1], mo) < RTOL_MU_SD and _rel(on[2][-1], so) < RTOL_MU_SD


@pytest.mark.gpu
def test_lookahead_partials_survive_late_critical_tile(ctx, monkeypatch):
    """the look-ahead partial of launch J is double-buffered by launch parity
    (gpf::la_slot), so a critical tile dispatched after its own launch's look-ahead has already
    written cannot seed from the next tile's partial. GPF_LA_DELAY_TEST=1 makes every seeded
    critical tile wait ~0.3 ms before it loads the partial (after the SYRK workgroup of the same
    launch has stored its own): scores, mean and sd stay bitwise equal (config B's schedule)."""
    import gpfit
    N, d, P = 1024, 2, 32
    rng = np.random.default_rng(4242)
    x = rng.uniform(size=(d, N))
    y = np.sin(6 * x[0]) * x[1] + 0.1 * rng.standard_normal(N)
    e = np.full(N, 0.1)
    s, ex = ref_cpu.sigma_grid()
    lo, hi = ref_cpu.search_bounds(x)
    ctx.set_data(x, y, e)
    ctx.set_grid(s, ex, lo, hi)
    Q = rng.uniform(0.1, 0.5, size=(P, d))
    assert gpfit.plan_check(P, N // 128)["syrk_workgroups"] > 0
    want = ctx.eval_batch(Q, want_mu_sd=True)
    monkeypatch.setenv("GPF_LA_DELAY_TEST", "1")
    late = ctx.eval_batch(Q, want_mu_sd=True)
    monkeypatch.delenv("GPF_LA_DELAY_TEST")
    for a, b in zip(want, late):
        np.testing.assert_array_equal(a, b)


@pytest.mark.gpu
def test_split_handoff_timeout_then_correct(ctx, monkeypatch):
    """a timed-out split-K hand-off (single-particle factorisation: every tile
    split, the binary reduction tree of gpf::split_part) is reported, and the next factorisation is
    correct: run_factor re-zeroes the tickets and ready flags a timed-out pair leaves set."""
    N, d = 2048, 2
    rng = np.random.default_rng(78)
    x = rng.uniform(size=(d, N))
    y = np.sin(4 * x[0]) + 0.1 * rng.standard_normal(N)
    e = np.full(N, 0.1)
    ctx.set_data(x, y, e)
    xf = rng.uniform(size=(d, 700))
    ls = np.array([0.3, 0.4])
    want = ctx.predict(ls, xf)
    monkeypatch.setenv("GPF_WAIT_SPINS", "0")
    with pytest.raises(RuntimeError, match="timed out"):
        ctx.predict(ls, xf)
    monkeypatch.delenv("GPF_WAIT_SPINS")
    for _ in range(2):
        got = ctx.predict(ls, xf)
        np.testing.assert_array_equal(got[0], want[0])
        np.testing.assert_array_equal(got[1], want[1])


@pytest.mark.parametrize("N,d,P", [(1000, 2, 12), (2049, 3, 5), (4096, 3, 1)])
def test_early_diagonal_factor_matches_fused(ctx, monkeypatch, N, d, P):
    """The early diagonal factor (k_step<SPLIT, 1>: block J factored by extra workgroups at the
    start of launch J and handed to the tiles through a flag) against the fused factor at the end
    of the previous launch's critical tile: the same arithmetic, so bitwise equal scores, mean
    and sd, on the unsplit paths (N=1000, 2049). The all-tile split (one particle:
    the prediction path) always runs the early factor (its flat finish waits for the diagonal
    block inside the launch), so there GPF_EARLY_DIAG=0 must change nothing: the factor itself
    bitwise equal. The deferred diagonal update (one
    SYRK workgroup per particle and launch applies the earlier terms to the next diagonal block,
    the critical tile the last one; GPF_DEFER_SYRK=0 restores the per-tile look-ahead) runs the
    same MFMAs per element in the same order: bitwise equal to the look-ahead, with either
    diagonal factor."""
    rng = np.random.default_rng(N + P)
    x = rng.uniform(size=(d, N))
    y = np.sin(5 * x[0]) + 0.1 * rng.standard_normal(N)
    e = rng.uniform(0.05, 0.2, size=N)
    s, ex = ref_cpu.sigma_grid()
    lo, hi = ref_cpu.search_bounds(x)
    ctx.set_data(x, y, e)
    ctx.set_grid(s, ex, lo, hi)
    Q = rng.uniform(0.1, 0.5, size=(P, d))
    # (r6: the early-diagonal launches' look-ahead pieces sum partials, which rounds differently from one
    # MFMA chain; this bitwise comparison runs without them — test_all_tile_lookahead_pieces checks them)
    monkeypatch.setenv("GPF_LA_ALL", "0")
    out = {}
    for mode, ed, defer in (("fused", "0", "1"), ("fused_lookahead", "0", "0"), ("ed", "1", "1"),
                            ("ed_lookahead", "1", "0")):
        monkeypatch.setenv("GPF_EARLY_DIAG", ed)
        monkeypatch.setenv("GPF_DEFER_SYRK", defer)
        out[mode] = ctx.eval_batch(Q, want_mu_sd=True)
        if P == 1:
            out[mode + "f"] = ctx.debug_factor(Q[0])
    for k in ("GPF_EARLY_DIAG", "GPF_DEFER_SYRK"):
        monkeypatch.delenv(k)
    for other in ("fused_lookahead", "ed", "ed_lookahead"):
        for a, b in zip(out["fused"], out[other]):
            np.testing.assert_array_equal(a, b)
        if P == 1:
            for a, b in zip(out["fusedf"], out[other + "f"]):
                np.testing.assert_array_equal(np.tril(a) if a.ndim == 2 else a, np.tril(b) if b.ndim == 2 else b)
    if N <= 2049:
        mo, so = ref_cpu.GP_train_identity(x, y, e, Q[0])
        assert _rel(out["fused"][1][0], mo) < RTOL_MU_SD and _rel(out["fused"][2][0], so) < RTOL_MU_SD


def test_handoff_timeout_is_reported(ctx, monkeypatch):
    """The bounded spin of the in-launch hand-offs (gpf::wait_diag): with the bound forced to zero
    polls (GPF_WAIT_SPINS=0) a tile that finds the diagonal block (or the SYRK workgroup's update)
    not yet published gives up, skips the work that would read it, and the host reports the
    timeout as a device error instead of scoring garbage; the next batch with the normal bound is
    correct again."""
    N, d = 1024, 2
    rng = np.random.default_rng(77)
    x = rng.uniform(size=(d, N))
    y = np.sin(4 * x[0]) + 0.1 * rng.standard_normal(N)
    e = np.full(N, 0.1)
    s, ex = ref_cpu.sigma_grid()
    lo, hi = ref_cpu.search_bounds(x)
    ctx.set_data(x, y, e)
    ctx.set_grid(s, ex, lo, hi)
    P = rng.uniform(0.1, 0.5, size=(32, d))
    want = ctx.eval_batch(P)
    monkeypatch.setenv("GPF_WAIT_SPINS", "0")
    with pytest.raises(RuntimeError, match="timed out"):
        ctx.eval_batch(P)
    monkeypatch.delenv("GPF_WAIT_SPINS")
    np.testing.assert_array_equal(ctx.eval_batch(P), want)


@pytest.mark.gpu
def test_factor128(ctx):
    """The 128x128 diagonal-block factor (csrc/gpf_diag.hip factor128, 16-blocked) against LAPACK:
    L = cholesky(A), U = L^-1, z = U y, the column partials colsum(U o U) and U^T z; exact zeros
    above both diagonals; garbage above A's diagonal never read; a padded block (identity in its
    lower right) factors to the identity there; a pivot that is not > 0 flagged. Matrices: a
    well-conditioned SPD one and kernel-like ones (SE covariance of 128 points + noise, the diagonal
    blocks the factorisation meets; cond up to ~1e8)."""
    rng = np.random.default_rng(128)
    n = 128
    g = rng.standard_normal((n, n))
    a0 = g @ g.T / n + np.eye(n)
    t = np.sort(rng.uniform(size=n))
    a1 = np.exp(-0.5 * (t[:, None] - t[None, :]) ** 2 / 0.2 ** 2) + np.diag(rng.uniform(1e-4, 1e-3, n))
    xs = rng.uniform(size=(3, n))
    r2 = sum((xs[k][:, None] - xs[k][None, :]) ** 2 for k in range(3)) / 0.3 ** 2
    a2 = np.exp(-0.5 * r2) + 0.01 * np.eye(n)
    a3 = a2.copy()  # padded: rows / columns 100.. are the identity, as the K build pads
    a3[100:, :] = 0.0
    a3[:, 100:] = 0.0
    a3[100:, 100:] = np.eye(n - 100)
    mats = [a0, a1, a2, a3]
    up = np.triu(np.full((n, n), 7.0), 1)  # garbage above the diagonal must not be read
    A = np.stack([np.tril(a) + up for a in mats])
    Y = rng.standard_normal((len(mats), n))
    Y[3, 100:] = 0.0
    out = ctx.debug_factor128(A, Y)
    assert out["bad"].tolist() == [0, 0, 0, 0]
    for k, a in enumerate(mats):
        L, U, z = out["L"][k], out["U"][k], out["z"][k]
        Lr = np.linalg.cholesky(a)
        Ur = np.linalg.inv(Lr)
        assert np.all(np.triu(L, 1) == 0) and np.all(np.triu(U, 1) == 0)
        cond = np.linalg.cond(a)
        assert np.abs(L - Lr).max() <= 1e-13 * np.abs(Lr).max() * max(1.0, np.sqrt(cond))
        assert np.abs(L @ L.T - a).max() <= 1e-14 * n * np.abs(a).max()
        assert np.abs(U @ L - np.eye(n)).max() <= 1e-15 * n * cond
        assert np.abs(z - Ur @ Y[k]).max() <= 1e-15 * n * cond * max(1.0, np.abs(Y[k]).max())
        np.testing.assert_allclose(out["s2"][k], np.sum(U * U, axis=0), rtol=1e-15 * n * cond, atol=0)
        np.testing.assert_allclose(out["sz"][k], U.T @ z, rtol=1e-15 * n * cond,
                                   atol=1e-15 * n * cond * np.abs(U.T @ z).max())
    np.testing.assert_array_equal(out["L"][3][100:, 100:], np.eye(n - 100))
    np.testing.assert_array_equal(out["U"][3][100:, 100:], np.eye(n - 100))
    np.testing.assert_array_equal(out["z"][3][100:], 0.0)
    assert np.all(out["cycles"] > 0)
    # a pivot that is not > 0: flagged (numpy raises LinAlgError, GP_func.py:22); in every panel
    bads = []
    for piv in (5, 40, 77, 127):
        ab = a0.copy()
        ab[piv, piv] = -1.0
        bads.append(np.tril(ab))
    out = ctx.debug_factor128(np.stack([np.tril(a0)] + bads), np.zeros((5, n)))
    assert out["bad"].tolist() == [0, 1, 1, 1, 1]
