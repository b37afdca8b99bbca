"""The score stage (csrc/gpf_objective.hip: k_points, k_score) on grids other than the default.

The reference is the literal formula in float64 NumPy (oracle.ref_cpu.coverage_loss and
proximity_penalty, both pinned to the reference's fixtures), applied to the device's OWN mu, sd
from eval_batch(..., want_mu_sd=True). That isolates the stage: the CPU oracle's mu differs from
the device's in the last bits, which at a tie flips a comparison and moves the loss by width/N.

Every comparison against that reference is bitwise. k_points claims the same comparisons and the
same IEEE division as the reference (bisected instead of enumerated), k_score the same count/N and
NumPy's pairwise summation order (tests/test_oracle.py::test_pairwise_sum_order pins that order
to the installed NumPy), and the library is built with -ffp-contract=off: nothing here has a
measured tolerance. A case that is not bitwise is a finding about the kernel.

Each case prints N, K, the number of exact ties |pull| == 1 in the reference and the number of
grid columns whose count differs between `<=` and `<` (run with -s;
profiles/score_stage/pytest_gpu.log).
"""
import functools

import numpy as np
import pytest

from oracle import ref_cpu

pytestmark = pytest.mark.gpu

RTOL_LOSS = 1e-8  # the file-wide objective tolerance of tests/test_gpu.py (end-to-end comparisons only)
SIZES = [1, 2, 129, 300]  # one and several k_points workgroups, one / two / three factor tiles


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def recipe(N):
    """The data of tests/test_gpu.py::test_tile_boundaries_vs_oracle (shared, read-only)."""
    rng = np.random.default_rng(N)
    d = 2
    x = rng.uniform(size=(d, N))
    y = np.sin(3 * x[0]) + x[1] + 0.1 * rng.standard_normal(N)
    e = rng.uniform(0.05, 0.2, size=N)
    lo, hi = np.full(d, 1e-3), np.full(d, 2.0)
    P = rng.uniform(0.05, 0.8, size=(5, d))
    return _frozen(x, y, e, lo, hi, P)


@functools.lru_cache(maxsize=None)
def oracle_gp(N, k):
    """The CPU oracle's mu, sd of particle k of recipe(N) (computed once per session)."""
    x, y, e, _, _, P = recipe(N)
    return _frozen(*ref_cpu.GP(x, y, e, x, P[k], batch_size=N))


def pulls_of(mu, sd, y, s):
    """find_len_scales.py:161-162, the expression inside ref_cpu.coverage_loss."""
    return (mu[:, None] - y[:, None]) / np.maximum(sd[:, None] * s[None, :], 1e-12)


def score_ref(mu, sd, y, s, ex, ls, lo, hi):
    """The literal score of one particle from given mu, sd: loss = -(-W - 0.01 proximity)."""
    W = ref_cpu.coverage_loss(mu, sd, y, s, ex)
    return -(-W - 0.01 * ref_cpu.proximity_penalty(ls, lo, hi))


def score_ref_batch(mu, sd, y, s, ex, P, lo, hi):
    return np.array([score_ref(mu[k], sd[k], y, s, ex, P[k], lo, hi) for k in range(len(P))])


def tie_stats(mu, sd, y, s):
    """(exact ties |pull| == 1, grid columns whose count differs between <= and <) over a batch."""
    ties = cols = 0
    for m, g in zip(mu, sd):
        a = np.abs(pulls_of(m, g, y, s))
        ties += int(np.count_nonzero(a == 1.0))
        cols += int(np.count_nonzero((a <= 1).sum(axis=0) != (a < 1).sum(axis=0)))
    return ties, cols


def report(what, N, K, mu, sd, y, s):
    ties, cols = tie_stats(mu, sd, y, s)
    print(f"[score_stage] {what}: N={N} K={K} exact_ties={ties} columns_le_differs_from_lt={cols}")
    return ties, cols


def adversarial_grid(r, K, seed):
    """A sorted K-point grid through the residuals r_i = |mu_i - y_i| / sd_i of one particle: every
    r_i (|pull| lands on 1 there), its two float neighbours, 0.0 twice and 1e-300 (the denominator
    clip), 1e6, and the first min(N, 20) r_i again as duplicated knots (zero-width trapezoids; pairs,
    never triples, so a wrong count at a knot still meets a non-zero width). K entries are drawn
    without replacement, order kept; a short grid is padded with uniform(0, 4). expected is
    uniform(0, 1): no symmetry hides a shifted index. All values finite: with inf in the grid W
    itself is inf or NaN in the reference."""
    rng = np.random.default_rng(seed)
    g = np.concatenate([r, np.nextafter(r, np.inf), np.nextafter(r, 0.0), [0.0, 0.0, 1e-300, 1e6],
                        r[:min(len(r), 20)]])
    g = np.sort(g)
    if len(g) < K:
        g = np.sort(np.concatenate([g, rng.uniform(0.0, 4.0, K - len(g))]))
    elif len(g) > K:
        g = g[np.sort(rng.choice(len(g), K, replace=False))]
    ex = rng.uniform(0.0, 1.0, K)
    assert g.shape == (K,) and np.all(np.isfinite(g)) and np.all(np.diff(g) >= 0)
    return g, ex


def eval_both_paths(c, P):
    """eval_batch without mu / sd (at N <= 256 the replayed HIP graph) and with them (plain
    launches): the scores must agree bit for bit. Returns (loss, mu, sd)."""
    replay = c.eval_batch(P)
    loss, mu, sd = c.eval_batch(P, want_mu_sd=True)
    np.testing.assert_array_equal(replay, loss)
    return loss, mu, sd


def fresh_eval(x, y, e, s, ex, lo, hi, P):
    """The scores of a context that has seen nothing but this data and this grid."""
    import gpfit
    c = gpfit.Context(0)
    try:
        c.set_data(x, y, e)
        c.set_grid(s, ex, lo, hi)
        return c.eval_batch(P)
    finally:
        c.close()


@pytest.fixture(scope="module")
def ctx():
    import gpfit
    c = gpfit.Context(0)
    yield c
    c.close()


# ---------------------------------------------------------------------------------------------
# a. K sweep on regular grids. K - 1 trapezoid terms = 1; 7 / 8 / 9 (the leaf's unrolled-by-8
# boundary); 128 / 129 (one leaf against the first split); 136; 255 - 257 (scan entries per
# thread 1 -> 2); 999; 1024; 4094 / 4095 (16 per thread, the deepest tree, the full KGRID_MAX).
# ---------------------------------------------------------------------------------------------
K_SWEEP = [2, 3, 8, 9, 10, 129, 130, 137, 256, 257, 258, 1000, 1025, 4095, 4096]


@pytest.mark.parametrize("K", K_SWEEP)
@pytest.mark.parametrize("N", SIZES)
def test_k_sweep_regular_grid(ctx, N, K):
    x, y, e, lo, hi, P = recipe(N)
    P = P[:3]
    s = np.linspace(0.001, 3, K)
    ex = ref_cpu.sigma_to_percent(s)
    # A statement about the inputs, not about the code under test: the end-to-end comparison below
    # means something only where no oracle pull sits near 1 (the device's mu, sd differ from the
    # oracle's by about 1e-12; the smallest margin of these inputs is 7.3e-8 at N=300, K=4095).
    # If it fails after a change of inputs, change the inputs.
    margin = min(np.min(np.abs(np.abs(pulls_of(*oracle_gp(N, k), y, s)) - 1.0)) for k in range(3))
    assert margin > 1e-9, margin
    ctx.set_data(x, y, e)
    ctx.set_grid(s, ex, lo, hi)
    loss, mu, sd = eval_both_paths(ctx, P)
    report("k_sweep", N, K, mu, sd, y, s)
    np.testing.assert_array_equal(loss, score_ref_batch(mu, sd, y, s, ex, P, lo, hi))
    end_to_end = np.array([ref_cpu.evaluate_loss(P[k], x, y, e, s, ex, lo, hi) for k in range(3)])
    assert np.max(np.abs(loss - end_to_end) / np.abs(end_to_end)) < RTOL_LOSS, (loss, end_to_end)


# ---------------------------------------------------------------------------------------------
# b. Adversarial grids built from the device's own residuals: pulls exactly on 1, duplicated
# knots, the denominator clip, a non-symmetric expected.
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [3, 9, 129, 137, 257, 1000, 4096])
@pytest.mark.parametrize("N", SIZES)
def test_adversarial_grid_from_device_residuals(ctx, N, K):
    x, y, e, lo, hi, P = recipe(N)
    P = P[:3]
    ctx.set_data(x, y, e)
    ctx.set_grid(*ref_cpu.sigma_grid(), lo, hi)
    _, mu0, sd0 = ctx.eval_batch(P, want_mu_sd=True)
    # the third word of the seed is the first for which, with the CPU oracle's mu, sd standing in for the
    # device's, every (N, K) here keeps at least two exact ties (K = 3 draws three of up to 924 entries)
    s, ex = adversarial_grid(np.abs(mu0[0] - y) / sd0[0], K, seed=[N, K, 7])
    ctx.set_grid(s, ex, lo, hi)
    loss, mu, sd = eval_both_paths(ctx, P)
    np.testing.assert_array_equal(mu, mu0)  # the grid has no part in mu, sd
    np.testing.assert_array_equal(sd, sd0)
    ties, cols = report("adversarial", N, K, mu, sd, y, s)
    # not vacuous: the reference holds a pull exactly on 1, and `<` for `<=` would change a count
    assert ties >= 1 and cols >= 1, (ties, cols)
    np.testing.assert_array_equal(loss, score_ref_batch(mu, sd, y, s, ex, P, lo, hi))


# ---------------------------------------------------------------------------------------------
# c. Both clips act: var < 1e-12 -> sd == 1e-6 exactly, and sd * s < 1e-12 in the denominator.
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [129, 300])
def test_variance_and_denominator_clips(ctx, N):
    x, y, e, lo, hi, _ = recipe(N)
    e = e.copy()
    e[::7] = 1e-7  # var = e^2 - e^4 dinv <= 1e-14: below the 1e-12 clip (covariance still PD, cond 1e2 .. 3e5)
    P = np.array([[0.03, 0.03], [0.1, 0.1]])
    ctx.set_data(x, y, e)
    s, ex = ref_cpu.sigma_grid()
    ctx.set_grid(s, ex, lo, hi)
    loss, mu, sd = eval_both_paths(ctx, P)
    for k in range(len(P)):
        assert np.count_nonzero(sd[k] == 1e-6) == len(e[::7]), k
    report("clips_default_grid", N, len(s), mu, sd, y, s)
    np.testing.assert_array_equal(loss, score_ref_batch(mu, sd, y, s, ex, P, lo, hi))
    K = 1000  # more than the 3 N + 24 constructed entries: all are kept, 0.0 and 1e-300 among them
    s, ex = adversarial_grid(np.abs(mu[0] - y) / sd[0], K, seed=[N, K, 1])
    assert s[0] == 0.0 and s[1] == 0.0 and np.any(s == 1e-300)
    assert np.count_nonzero(sd[:, :, None] * s[None, None, :] < 1e-12) >= 3 * N  # the denominator clip acts
    ctx.set_grid(s, ex, lo, hi)
    loss2, mu2, sd2 = eval_both_paths(ctx, P)
    np.testing.assert_array_equal(mu2, mu)
    np.testing.assert_array_equal(sd2, sd)
    ties, cols = report("clips_adversarial_grid", N, K, mu, sd, y, s)
    assert ties >= 1 and cols >= 1
    np.testing.assert_array_equal(loss2, score_ref_batch(mu, sd, y, s, ex, P, lo, hi))


# ---------------------------------------------------------------------------------------------
# d. Proximity term: clip(1 - 2 min_k min(to_lo_k, to_hi_k), 0, 1) over a heterogeneous box.
# ---------------------------------------------------------------------------------------------
def _step(v, n):
    """v moved n floats up (n > 0) or down (n < 0)."""
    for _ in range(abs(n)):
        v = np.nextafter(v, np.inf if n > 0 else -np.inf)
    return v


def _midpoint(lo, hi):
    """Per dimension the double nearest (lo + hi) / 2 whose smaller distance to the box, in the
    reference's expression, is largest (0.5 where the rounding allows it)."""
    span = hi - lo
    out = np.empty(len(lo))
    for k in range(len(lo)):
        c = np.array([_step((lo[k] + hi[k]) / 2, n) for n in range(-4, 5)])
        out[k] = c[np.argmax(np.minimum((c - lo[k]) / span[k], (hi[k] - c) / span[k]))]
    return out


def _tied_pair(lo, hi, j0, j1, t=0.2):
    """Length scales in dimensions j0, j1 whose distances to lo (the reference's expression) are the
    same double: searched over a few floats around lo + t span."""
    span = hi - lo
    steps = np.arange(-40, 41)
    c0 = np.array([_step(lo[j0] + t * span[j0], int(n)) for n in steps])
    c1 = np.array([_step(lo[j1] + t * span[j1], int(n)) for n in steps])
    a0 = (c0 - lo[j0]) / span[j0]
    a1 = (c1 - lo[j1]) / span[j1]
    i0, i1 = np.nonzero(a0[:, None] == a1[None, :])
    assert len(i0) > 0, "no exactly tied pair near lo + t span: change t"
    return c0[i0[0]], c1[i1[0]]


@functools.lru_cache(maxsize=None)
def proximity_case(d):
    N = 129
    rng = np.random.default_rng(1000 + d)
    # at d = 32 (DMAX) a spread of 0.1 per dimension against length scales of order 1 keeps the
    # covariance well away from the identity, and positive definite through diag(e^2)
    x = (0.1 if d == 32 else 1.0) * rng.uniform(size=(d, N))
    y = np.sin(3 * x[0]) + x[-1] + 0.1 * rng.standard_normal(N)
    e = rng.uniform(0.05, 0.2, size=N)
    lo = 0.01 * (np.arange(d) + 1.0)
    hi = 1.0 + 0.5 * np.arange(d)
    inner = lambda: lo + (hi - lo) * rng.uniform(0.3, 0.7, size=d)  # noqa: E731
    rows, names = [], []
    rows.append(_midpoint(lo, hi)); names.append("midpoint")         # proximity 0
    p = inner(); p[d - 1] = _step(lo[d - 1], 3); rows.append(p); names.append("inside_lo")  # about 1
    p = inner(); p[0] = _step(hi[0], -3); rows.append(p); names.append("inside_hi")         # about 1
    if d >= 2:
        p = inner(); p[0], p[d - 1] = _tied_pair(lo, hi, 0, d - 1); rows.append(p); names.append("tied_minimum")
    rows.append(lo + (hi - lo) * rng.uniform(0.05, 0.95, size=d)); names.append("generic")
    return _frozen(x, y, e, lo, hi, np.array(rows)) + (names,)


@pytest.mark.parametrize("d", [1, 3, 32])
def test_proximity_term(ctx, d):
    x, y, e, lo, hi, P, names = proximity_case(d)
    N = x.shape[1]
    prox = np.array([ref_cpu.proximity_penalty(p, lo, hi) for p in P])
    # statements about the inputs: the cases are what their names say
    # (0 exactly at d = 1; elsewhere some dimension's midpoint is no double, which leaves one ulp of 1)
    assert prox[names.index("midpoint")] <= 2.0 ** -52 and (d > 1 or prox[names.index("midpoint")] == 0.0)
    assert prox[names.index("inside_lo")] > 1 - 1e-12 and prox[names.index("inside_hi")] > 1 - 1e-12
    if d >= 2:
        t = P[names.index("tied_minimum")]
        to_lo, to_hi = (t - lo) / (hi - lo), (hi - t) / (hi - lo)
        m = np.minimum(to_lo, to_hi)
        assert m[0] == m[d - 1] == m.min() and np.count_nonzero(m == m.min()) == 2
    assert 0.0 < prox[names.index("generic")] < 1.0
    s, ex = ref_cpu.sigma_grid()
    ctx.set_data(x, y, e)
    ctx.set_grid(s, ex, lo, hi)
    loss, mu, sd = eval_both_paths(ctx, P)
    print(f"[score_stage] proximity: N={N} K={len(s)} d={d} proximity={prox.tolist()}")
    report("proximity", N, len(s), mu, sd, y, s)
    np.testing.assert_array_equal(loss, score_ref_batch(mu, sd, y, s, ex, P, lo, hi))
    perm = np.roll(np.arange(len(P)), 1)  # a cyclic shift: no row keeps its place
    np.testing.assert_array_equal(eval_both_paths(ctx, P[perm])[0], loss[perm])


# ---------------------------------------------------------------------------------------------
# e. Grid changes on a live context; histogram rows reused chunk after chunk and after a failure.
# ---------------------------------------------------------------------------------------------
def _grid_sequence():
    """K: 1000 -> 3 -> 4096 -> 1000 (same K as the first, other values, other expected), then the
    bounds alone."""
    x, y, e, lo, hi, P = recipe(129)
    rng = np.random.default_rng(5)
    s0, ex0 = ref_cpu.sigma_grid()
    s1 = np.linspace(0.001, 3, 3)
    s2 = np.sort(rng.uniform(0.0, 4.0, 4096))
    s3 = np.sort(rng.uniform(0.0, 2.5, 1000))
    lo2, hi2 = np.array([0.01, 0.02]), np.array([1.5, 0.9])
    assert np.all(P > lo2) and np.all(P < hi2)
    ex3 = rng.uniform(0, 1, 1000)
    return [("K=1000 default", s0, ex0, lo, hi),
            ("K=3", s1, ref_cpu.sigma_to_percent(s1), lo, hi),
            ("K=4096", s2, rng.uniform(0, 1, 4096), lo, hi),
            ("K=1000 other values", s3, ex3, lo, hi),
            ("K=1000 other bounds", s3, ex3, lo2, hi2)]


def test_grid_changes_on_live_context():
    import gpfit
    x, y, e, _, _, P = recipe(129)
    P = P[:3]
    live = gpfit.Context(0)
    try:
        live.set_data(x, y, e)
        seen = []
        for what, s, ex, lo, hi in _grid_sequence():
            live.set_grid(s, ex, lo, hi)
            # without mu / sd: the graph captured for this K (free_work dropped the old K's graphs);
            # with them: plain launches
            loss, mu, sd = eval_both_paths(live, P)
            report(f"live_context {what}", 129, len(s), mu, sd, y, s)
            np.testing.assert_array_equal(loss, score_ref_batch(mu, sd, y, s, ex, P, lo, hi), err_msg=what)
            np.testing.assert_array_equal(loss, fresh_eval(x, y, e, s, ex, lo, hi, P), err_msg=what)
            seen.append(loss)
        for a, b in zip(seen, seen[1:]):
            assert np.all(a != b)  # every change of grid or bounds moved every score
    finally:
        live.close()


def test_chunked_batch_reuses_histogram_rows(ctx, monkeypatch):
    import gpfit
    x, y, e, lo, hi, P = recipe(129)  # all five particles
    ctx.set_data(x, y, e)
    ctx.set_grid(*ref_cpu.sigma_grid(), lo, hi)
    _, mu0, sd0 = ctx.eval_batch(P, want_mu_sd=True)
    s, ex = adversarial_grid(np.abs(mu0[0] - y) / sd0[0], 4096, seed=[129, 4096, 2])
    ctx.set_grid(s, ex, lo, hi)
    whole, mu, sd = eval_both_paths(ctx, P)
    report("chunked", 129, 4096, mu, sd, y, s)
    np.testing.assert_array_equal(whole, score_ref_batch(mu, sd, y, s, ex, P, lo, hi))
    monkeypatch.setenv("GPF_MAX_CHUNK", "2")  # chunks of 2, 2, 1 through the same two histogram rows
    c = gpfit.Context(0)
    try:
        c.set_data(x, y, e)
        c.set_grid(s, ex, lo, hi)
        np.testing.assert_array_equal(c.eval_batch(P), whole)
        loss, mu2, sd2 = c.eval_batch(P, want_mu_sd=True)
        np.testing.assert_array_equal(loss, whole)
        np.testing.assert_array_equal(mu2, mu)
        np.testing.assert_array_equal(sd2, sd)
    finally:
        c.close()


def _half_singular_case():
    """recipe(129) with points 0 and 1 at the same x0, half a unit apart in x1 and free of noise. A
    length scale of 1e12 in x1 makes their rows of the covariance the same doubles (the x1 term,
    2.5e-25, is lost against any other), so the second pivot is exactly 0: not positive definite,
    like tests/test_gpu.py::test_not_positive_definite_raises_like_numpy's duplicate point. With
    length scales of order 0.1 .. 1 in x1 the same data factorises."""
    x, y, e, lo, hi, P = recipe(129)
    x, e = x.copy(), e.copy()
    x[:, 0], x[:, 1] = (0.5, 0.25), (0.5, 0.75)
    e[:2] = 0.0
    hi = np.array([2.0, 1e13])
    bad = np.array([0.4, 1e12])
    return x, y, e, lo, hi, P[:3], bad


def test_histogram_clean_after_failed_particle():
    import gpfit
    x, y, e, lo, hi, P, bad = _half_singular_case()
    with pytest.raises(np.linalg.LinAlgError):
        ref_cpu.GP(x, y, e, x, bad, batch_size=129)
    s, ex = ref_cpu.sigma_grid()
    want = fresh_eval(x, y, e, s, ex, lo, hi, P)
    mixed = np.stack([P[0], bad, P[1]])
    c = gpfit.Context(0)
    try:
        c.set_data(x, y, e)
        c.set_grid(s, ex, lo, hi)
        for want_mu_sd in (False, True):  # the failing batch through the graph replay, then plain launches
            with pytest.raises(np.linalg.LinAlgError, match="not positive definite") as err:
                c.eval_batch(mixed, want_mu_sd=want_mu_sd)
            assert err.value.particle == 1
            # the failed particle's points were counted into the histogram row that the next batch reuses;
            # k_score must have left every bucket it reads (0 .. K-1) zeroed. Bucket K, where a point that
            # passes at no grid value goes, is written and zeroed but never read: nothing observable
            # depends on it.
            loss, mu, sd = eval_both_paths(c, P)
            np.testing.assert_array_equal(loss, want)
            np.testing.assert_array_equal(loss, score_ref_batch(mu, sd, y, s, ex, P, lo, hi))
        report("after_failed_particle", 129, len(s), mu, sd, y, s)
    finally:
        c.close()


# ---------------------------------------------------------------------------------------------
# f. Validation: the bisection needs a finite, non-decreasing grid (a deliberate deviation from
# the reference, which computes something for any order), and set_grid reads K resp. d doubles.
# ---------------------------------------------------------------------------------------------
def _bad_grids():
    s, ex = ref_cpu.sigma_grid()
    d = 2
    lo, hi = np.full(d, 1e-3), np.full(d, 2.0)
    swapped = s.copy()
    swapped[[500, 501]] = swapped[[501, 500]]
    with_nan, with_inf, ex_nan = s.copy(), s.copy(), ex.copy()
    with_nan[10] = np.nan
    with_inf[-1] = np.inf
    ex_nan[3] = np.nan
    s4097 = np.linspace(0.001, 3, 4097)
    return {
        "descending": (s[::-1], ex[::-1], lo, hi, r"sigma_vals\[1\]"),
        "swapped_pair": (swapped, ex, lo, hi, r"sigma_vals\[501\]"),
        "nan_in_grid": (with_nan, ex, lo, hi, r"sigma_vals\[10\]"),
        "inf_in_grid": (with_inf, ex, lo, hi, r"sigma_vals\[999\]"),
        "nan_in_expected": (s, ex_nan, lo, hi, r"expected\[3\]"),
        "expected_shorter": (s, ex[:-1], lo, hi, "expected"),
        "expected_longer": (s[:-1], ex, lo, hi, "expected"),
        "grid_two_dimensional": (s.reshape(2, 500), ex.reshape(2, 500), lo, hi, "one-dimensional"),
        "lo_shorter": (s, ex, lo[:1], hi, "lo"),
        "hi_longer": (s, ex, lo, np.full(d + 1, 2.0), "hi"),
        "K_1": (s[:1], ex[:1], lo, hi, "grid"),
        "K_4097": (s4097, ref_cpu.sigma_to_percent(s4097), lo, hi, "grid"),
    }


@pytest.mark.parametrize("case", list(_bad_grids()))
def test_set_grid_validation(ctx, case):
    x, y, e, lo, hi, P = recipe(129)
    P = P[:3]
    rng = np.random.default_rng(9)
    s = np.sort(rng.uniform(0.0, 4.0, 1000))  # K = 1000 like most of the rejected grids: their
    ex = rng.uniform(0.0, 1.0, 1000)          # values would fit the buffers of this one
    ctx.set_data(x, y, e)
    ctx.set_grid(s, ex, lo, hi)
    before, mu, sd = eval_both_paths(ctx, P)
    np.testing.assert_array_equal(before, score_ref_batch(mu, sd, y, s, ex, P, lo, hi))
    bs, bex, blo, bhi, msg = _bad_grids()[case]
    with pytest.raises(ValueError, match=msg):
        ctx.set_grid(bs, bex, blo, bhi)
    # the grid set before is still in force, not half overwritten
    np.testing.assert_array_equal(eval_both_paths(ctx, P)[0], before)


def test_dropin_evaluate_loss_rejects_descending_grid():
    import find_len_scales as fls
    x, y, e, lo, hi, P = recipe(129)
    s, ex = ref_cpu.sigma_grid()
    good = fls.evaluate_loss(P[0], x, y, e, s, ex, lo, hi)
    with pytest.raises(ValueError, match="non-decreasing"):
        fls.evaluate_loss(P[0], x, y, e, s[::-1], ex[::-1], lo, hi)
    with pytest.raises(ValueError, match="non-decreasing"):
        fls.wass_loss(P[0], x, y, e, s[::-1], ex[::-1], lo, hi)
    assert fls.evaluate_loss(P[0], x, y, e, s, ex, lo, hi) == good
