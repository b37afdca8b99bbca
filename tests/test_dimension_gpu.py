"""Every kernel path whose shape follows the input dimension, at d = 5 .. 32 (DMAX): the generic
cross-covariance builders k_cross_cov<0> / k_cross_cov_batch<0> (dynamic LDS (d + 1) 288 x 8 bytes: 64,512
at d = 27, 66,816 at d = 28, 76,032 at d = 32), the covariance tile seed cov_tile_acc of every
factorisation schedule (at d = 32 it stages 256 doubles more than the GEMM stages hold), k_lml_grad's
d-strided reductions, k_km_assign's run-time-d path, and the dimension contract of the API. Each result
against the closed forms the suite already has, imported from their modules.

Inputs (`recipe`): x ~ U(0,1)^d, y = sin(3 x_0) + x_{d-1} + 0.1 randn, e ~ U(0.05, 0.2); three
length-scale rows per case: generic sqrt(d) U(0.3, 1.2) per dimension, the same with l_{d-1} = 0.5
(last-dominant) and the same with l_0 = 0.5 (first-dominant); further rows, where a case takes more
than three particles, are generic. No dominant scale is shorter than 0.5: at 0.15 the float64 NumPy
kernel is already 4e-14 from long double (cancellation in |a|^2 + |b|^2 - 2 a.b).

Tolerances are those of each entry point's own module, unchanged. What the float64 references
themselves lose against the same formulas in np.longdouble was measured on the CPU for every (N, d, row)
used below; each tolerance stands because the reference's own error is at least 10x inside it:
  kernel    (rtol 1e-13, atol 1e-15) |ref_cpu.kernel_func - long double| <= 0.0095 (generic), 0.015
            (last-dominant), 0.052 (first-dominant) of atol + rtol |K|, i.e. within 5.2e-15 relative, over the ten
            dimensions and three shapes;
  factor    (1e-11 normwise) L 3.2e-14, U 3.8e-13, z 7.5e-13, alpha 9.98e-13; cond(K + diag e^2) <= 1.6e5 at
            N = 641 (<= 9.7e4 at 300). alpha is the factor's two solves, solve(L^T, solve(L, y)):
            np.linalg.solve(Kn, y) itself was 1.31e-12 at N = 641, d = 5, less than 10x inside, so that form
            is not used; no input was changed;
  eval      (RTOL_MU_SD = 1e-6) ref_cpu.GP at the training points, N = 641, d = 17 and 32, five rows: mu 8.0e-13,
            sd 1.3e-12;
  predict   (1e-6) mu 5.5e-11, sd 2.1e-12;
  the prediction family (1e-9) at N = 300, d = 5 and 32: predict_cov Sigma 6.0e-15, mu 1.3e-13; predict_linear
            cov / s 1.7e-15, prior / s 7.6e-16, mean 2.8e-13; predict_conditioned mean 1.3e-13, variance 9.2e-15,
            chi2 4.2e-13 (cond(H) <= 91, the smallest conditioned variance 2.4e-4: the 1e-12 clip never acts);
            predict_batch mu 1.3e-13, variance 9.9e-15;
  lml_batch (1e-9) value 3.6e-12, gradient 4.2e-13 of its largest component; the components span 3.6e-3 .. 3.6e2.

The measured GPU maxima are printed with a [dimension] prefix (run with -s); one MI355X's are in
profiles/dimension/pytest_gpu.log.
"""
import numpy as np
import pytest

import test_conditioned_gpu as t_con
import test_lml_grad_gpu as t_lml
import test_posterior_draws_gpu as t_draws
import test_predict_batch_gpu as t_batch
import test_predict_cov_gpu as t_cov
import test_predict_linear_gpu as t_lin
from oracle import ref_cpu
from test_gpu import RTOL_MU_SD, _rel, assert_loss_or_ties
from test_mle_host import lml_closed_form

pytestmark = pytest.mark.gpu

DIMS = (5, 6, 7, 8, 9, 16, 27, 28, 31, 32)   # 27 | 28: either side of 64 KiB of dynamic LDS; 7, 9: no templated kmeans
FACTOR_DIMS = (5, 17, 28, 32)
ROWS = ("generic", "last-dominant", "first-dominant")
TOL_FACTOR = 1e-11
TOL = 1e-9


@pytest.fixture(scope="module")
def ctx():
    import gpfit
    c = gpfit.Context(0)
    yield c
    c.close()


def length_rows(rng, d, P=3):
    """(P, d): the generic row, the same with l_{d-1} = 0.5, the same with l_0 = 0.5, then generic rows."""
    g = np.sqrt(d) * rng.uniform(0.3, 1.2, size=(max(P - 2, 1), d))
    ls = np.concatenate([g[:1], g[:1], g[:1], g[1:]])
    ls[1, d - 1] = 0.5
    ls[2, 0] = 0.5
    return np.ascontiguousarray(ls[:max(P, 3)])


def recipe(N, d, P=3):
    """(x (d, N), y, e, ls (max(P, 3), d)) of the module docstring from default_rng(100000 + 1000 d + N); the
    data and the first rows do not depend on P."""
    rng = np.random.default_rng(100000 + 1000 * d + N)
    x = rng.uniform(size=(d, N))
    y = np.sin(3 * x[0]) + x[d - 1] + 0.1 * rng.standard_normal(N)
    e = rng.uniform(0.05, 0.2, size=N)
    return x, y, e, length_rows(rng, d, P)


def case(N, d, M):
    """recipe(N, d) with M queries, in the form of test_predict_cov_gpu._case: U(-0.1, 1.1)^d from
    default_rng(1000 + M), the first min(N, M) // 4 on training points, the last two a duplicate pair."""
    x, y, e, ls = recipe(N, d)
    q = np.random.default_rng(1000 + M).uniform(-0.1, 1.1, (d, M))
    k = min(N, M) // 4
    q[:, :k] = x[:, :k]
    if M > 2:
        q[:, -1] = q[:, -2]
    return x, y, e, ls, q


def box(d):
    """A search box that holds every row of length_rows."""
    return np.full(d, 1e-3), np.full(d, 2.0 * np.sqrt(d))


def say(text):
    print(f"[dimension] {text}")


_REF = {}


def shared(key, make):
    """make() once per key; the arrays it returns are shared among the tests and read-only."""
    if key not in _REF:
        out = make()
        for a in out if isinstance(out, tuple) else (out,):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _REF[key] = out
    return _REF[key]


# ---------------------------------------------------------------------------------------------
# 1. Context.kernel: k_cross_cov<0> alone, across its 32-row and 256-column blocks.
# ---------------------------------------------------------------------------------------------
def kernel_case(d, n1, n2):
    rng = np.random.default_rng(300000 + 1000 * d + n1 + n2)
    return rng.uniform(size=(d, n1)), rng.uniform(size=(d, n2)), length_rows(rng, d)


@pytest.mark.parametrize("n1,n2", [(33, 257), (32, 256), (1, 300)])
@pytest.mark.parametrize("d", DIMS)
def test_kernel_vs_oracle(ctx, d, n1, n2):
    x1, x2, ls = kernel_case(d, n1, n2)
    for name, l in zip(ROWS, ls):
        want = ref_cpu.kernel_func(x1, x2, l)
        got = ctx.kernel(x1, x2, l)
        assert got.shape == (n1, n2)
        err = np.max(np.abs(got - want) / (1e-15 + 1e-13 * np.abs(want)))
        say(f"kernel d={d} ({n1}, {n2}) {name}: max |got - want| / (atol + rtol |want|) = {err:.3e}, "
            f"K in [{want.min():.3f}, {want.max():.3f}]")
        np.testing.assert_allclose(got, want, rtol=1e-13, atol=1e-15, err_msg=f"d={d} ({n1}, {n2}) {name}")


# ---------------------------------------------------------------------------------------------
# 2. The factor of one particle (the all-tile split with the flat finish): L, U, z, alpha.
# ---------------------------------------------------------------------------------------------
def factor_reference(N, d, row):
    def make():
        x, y, e, ls = recipe(N, d)
        Kn = ref_cpu.kernel_func(x, x, ls[row]) + np.diag(e ** 2)
        L = np.linalg.cholesky(Kn)
        z = np.linalg.solve(L, y)
        # (alpha by the factor's two solves: np.linalg.solve(Kn, y) itself is up to 1.3e-12 from long double
        # at N = 641, less than 10x inside the tolerance; this form is within 1.0e-12)
        return L, np.linalg.solve(L, np.eye(N)), z, np.linalg.solve(L.T, z)
    return shared(("factor", N, d, row), make)


@pytest.mark.parametrize("N", [300, 641])
@pytest.mark.parametrize("d", FACTOR_DIMS)
def test_factor_vs_lapack(ctx, monkeypatch, d, N):
    """3 and 6 block columns (15 off-diagonal seeds), the metric of test_single_particle_split_factor_tight:
    normwise, max |got - ref| / max |ref| < 1e-11."""
    import gpfit
    monkeypatch.delenv("GPF_SPLIT_K", raising=False)
    x, y, e, ls = recipe(N, d)
    ctx.set_data(x, y, e)
    for row, name in enumerate(ROWS):
        got = ctx.debug_factor(ls[row])
        for what, a, b in zip(("L", "U", "z", "alpha"), got, factor_reference(N, d, row)):
            a = np.tril(a)[:N, :N] if a.ndim == 2 else a[:N]
            err = np.max(np.abs(a - b)) / np.max(np.abs(b))
            say(f"factor N={N} d={d} {name} {what}: max |got - ref| / max |ref| = {err:.3e}")
            assert err < TOL_FACTOR, (N, d, name, what, err)
    if N == 641:
        assert gpfit.plan_check(1, 6)["split_tiles"] == 30   # the all-tile split ran: every tile in pieces


# ---------------------------------------------------------------------------------------------
# 3. eval_batch on every schedule that seeds tiles with cov_tile_acc.
# ---------------------------------------------------------------------------------------------
KNOBS = ("GPF_SPLIT_K", "GPF_LA_ALL", "GPF_LOOKAHEAD", "GPF_EARLY_DIAG", "GPF_PERSIST", "GPF_GROUPS", "GPF_DEFER_SYRK",
         "GPF_PAIR")
# name -> (environment, what the plan must show). At 5 particles and 6 block columns the default is the
# all-tile split (as for one particle); GPF_SPLIT_K=1 gives the unsplit early-diagonal launches, on which
# the look-ahead knobs act, and which the bitwise relations of the suite are about.
SCHEDULES = {
    "default": ({}, {"split_tiles": 150}),
    "la_all0": ({"GPF_LA_ALL": "0"}, {}),
    "lookahead0": ({"GPF_LOOKAHEAD": "0"}, {}),
    "early_diag0": ({"GPF_EARLY_DIAG": "0"}, {}),
    "persist1": ({"GPF_PERSIST": "1"}, {"persistent": 1}),
    "persist0_groups1": ({"GPF_PERSIST": "0", "GPF_GROUPS": "1"}, {"persistent": 0, "groups": 1}),
    "unsplit": ({"GPF_SPLIT_K": "1"}, {"S": 1, "split_tiles": 0, "diag_workgroups": 30}),
    "unsplit_la_all0": ({"GPF_SPLIT_K": "1", "GPF_LA_ALL": "0"}, {"S": 1, "split_tiles": 0, "diag_workgroups": 30}),
    "unsplit_lookahead0": ({"GPF_SPLIT_K": "1", "GPF_LOOKAHEAD": "0"}, {"S": 1, "diag_workgroups": 30}),
    "unsplit_la_all0_early_diag0": ({"GPF_SPLIT_K": "1", "GPF_LA_ALL": "0", "GPF_EARLY_DIAG": "0"},
                                    {"S": 1, "diag_workgroups": 0}),
    "unsplit_la_all0_groups1": ({"GPF_SPLIT_K": "1", "GPF_LA_ALL": "0", "GPF_PERSIST": "0", "GPF_GROUPS": "1"},
                                {"S": 1, "groups": 1}),
}


def oracle_at_training_points(N, d, P):
    def make():
        x, y, e, ls = recipe(N, d, P)
        s, ex = ref_cpu.sigma_grid()
        lo, hi = box(d)
        mu, sd = zip(*(ref_cpu.GP(x, y, e, x, l, batch_size=N) for l in ls))
        loss = [ref_cpu.coverage_loss(m, v, y, s, ex) + 0.01 * ref_cpu.proximity_penalty(l, lo, hi)
                for m, v, l in zip(mu, sd, ls)]
        return np.array(loss), np.array(mu), np.array(sd)
    return shared(("eval", N, d, P), make)


def check_against_oracle(tag, got, ref, y, s):
    loss, mu, sd = got
    em, es = _rel(mu, ref[1]), _rel(sd, ref[2])
    el = np.max(np.abs(loss - ref[0]) / np.abs(ref[0]))
    say(f"{tag}: mu err {em:.3e}, sd err {es:.3e}, loss err {el:.3e}")
    assert em < RTOL_MU_SD and es < RTOL_MU_SD, (tag, em, es)
    for k in range(len(loss)):
        assert_loss_or_ties(loss[k], ref[0][k], ref[1][k], ref[2][k], y, s, what=(tag, k))


def close_or_ties(tag, a, b, y, s):
    """mu and sd within 1e-10, the objective within 1e-10 or explained by threshold ties: what the suite
    allows between two correct runs whose sums round differently (_reference_share,
    test_all_tile_lookahead_pieces, test_all_tile_split_live_counts)."""
    em, es = _rel(a[1], b[1]), _rel(a[2], b[2])
    say(f"{tag}: mu {em:.3e}, sd {es:.3e}")
    assert em < 1e-10 and es < 1e-10, (tag, em, es)
    for k in range(len(a[0])):
        if abs(a[0][k] - b[0][k]) > 1e-10 * abs(b[0][k]):
            assert_loss_or_ties(a[0][k], b[0][k], b[1][k], b[2][k], y, s, what=(tag, k))


def bitwise(tag, a, b):
    for what, u, v in zip(("loss", "mu", "sd"), a, b):
        np.testing.assert_array_equal(u, v, err_msg=f"{tag}: {what}")


@pytest.mark.parametrize("d", [17, 32])
def test_eval_batch_schedules_vs_oracle(ctx, monkeypatch, d):
    """N = 641 (6 block columns), 5 particles. Every schedule against ref_cpu.GP at the training points and
    the oracle's scoring of those; among themselves only the relations the suite asserts at low d:
    the persistent factorisation, one particle group, the fused diagonal factor (without the look-ahead
    pieces) and the critical-tile look-ahead switched off are bitwise the unsplit launches they are
    compared with there (test_persistent_factor_bitwise, _reference_share,
    test_early_diagonal_factor_matches_fused, test_critical_tile_lookahead_bitwise); the look-ahead pieces
    and the split sum partials in another order and are within 1e-10 (close_or_ties). One particle is
    the split again (test_split_k_matches_unsplit_and_oracle's 1e-10 against the unsplit launches)."""
    import gpfit
    N, P = 641, 5
    x, y, e, ls = recipe(N, d, P)
    s, ex = ref_cpu.sigma_grid()
    lo, hi = box(d)
    ref = oracle_at_training_points(N, d, P)
    ctx.set_data(x, y, e)
    ctx.set_grid(s, ex, lo, hi)
    out = {}
    for name, (env, plan) in SCHEDULES.items():
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        st = gpfit.plan_check(P, 6)
        assert all(st[k] == v for k, v in plan.items()), (name, plan, st)
        out[name] = ctx.eval_batch(ls, want_mu_sd=True)
        check_against_oracle(f"eval_batch N={N} d={d} {name}", out[name], ref, y, s)
        if name in ("default", "unsplit"):
            bitwise(f"d={d} {name}: second run", ctx.eval_batch(ls, want_mu_sd=True), out[name])
    base = out["unsplit_la_all0"]
    bitwise(f"d={d}: GPF_PERSIST=1 vs the unsplit launches", out["persist1"], base)
    bitwise(f"d={d}: one group vs the unsplit launches", out["unsplit_la_all0_groups1"], base)
    bitwise(f"d={d}: fused vs early diagonal factor", out["unsplit_la_all0_early_diag0"], base)
    bitwise(f"d={d}: critical-tile look-ahead off vs on", out["unsplit_lookahead0"], out["unsplit"])
    close_or_ties(f"d={d}: look-ahead pieces vs none", out["unsplit"], base, y, s)
    for name in ("default", "la_all0", "lookahead0", "early_diag0", "persist0_groups1"):
        close_or_ties(f"d={d}: {name} vs the unsplit launches", out[name], base, y, s)
    # one particle: split-K by default
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    assert gpfit.plan_check(1, 6)["split_tiles"] == 30
    for row, name in enumerate(ROWS):
        one = ctx.eval_batch(ls[row:row + 1], want_mu_sd=True)
        ref1 = tuple(a[row:row + 1] for a in ref)
        check_against_oracle(f"eval_batch N={N} d={d} P=1 {name}", one, ref1, y, s)
        monkeypatch.setenv("GPF_SPLIT_K", "1")
        unsplit = ctx.eval_batch(ls[row:row + 1], want_mu_sd=True)
        monkeypatch.delenv("GPF_SPLIT_K")
        check_against_oracle(f"eval_batch N={N} d={d} P=1 {name} unsplit", unsplit, ref1, y, s)
        close_or_ties(f"d={d} P=1 {name}: split vs unsplit", one, unsplit, y, s)


# ---------------------------------------------------------------------------------------------
# 4. predict: k_cross_cov<0> with its padding contract behind the factor.
# ---------------------------------------------------------------------------------------------
def predict_reference(N, d, M, row):
    def make():
        x, y, e, ls, q = case(N, d, M)
        return ref_cpu.GP(x, y, e, q, ls[row], batch_size=10000)
    return shared(("predict", N, d, M, row), make)


@pytest.mark.parametrize("N,M", [(300, 700), (129, 257)])
@pytest.mark.parametrize("d", [5, 27, 28, 32])
def test_predict_vs_oracle(ctx, d, N, M):
    x, y, e, ls, q = case(N, d, M)
    ctx.set_data(x, y, e)
    for row, name in enumerate(ROWS):
        m0, s0 = predict_reference(N, d, M, row)
        mu, sd = ctx.predict(ls[row], q)
        em, es = _rel(mu, m0), _rel(sd, s0)
        say(f"predict N={N} M={M} d={d} {name}: mu err {em:.3e}, sd err {es:.3e}, sd in [{s0.min():.3e}, {s0.max():.3f}]")
        assert em < RTOL_MU_SD and es < RTOL_MU_SD, (N, M, d, name, em, es)
        mu7, sd7 = ctx.predict(ls[row], q, batch_size=7)
        np.testing.assert_array_equal(mu7, mu)
        np.testing.assert_array_equal(sd7, sd)


# ---------------------------------------------------------------------------------------------
# 5. The other prediction entry points, each through its own module's check on this recipe.
# ---------------------------------------------------------------------------------------------
@pytest.fixture
def prefixed(monkeypatch):
    """What the other modules' checks print carries this module's prefix in front of their own."""
    for mod in (t_cov, t_lin, t_con, t_batch, t_draws, t_lml):
        monkeypatch.setattr(mod, "print", say, raising=False)   # a module global shadows the builtin there


@pytest.fixture
def own_module_checks(monkeypatch, prefixed):
    """The modules of the other prediction entry points draw their inputs from test_predict_cov_gpu._case:
    with `case` in its place their own closed forms, metrics and tolerances run on this module's recipe
    (their reference caches are keyed by (N, d, M, ..): d = 5, 9 and 32 are not used there)."""
    for mod in (t_cov, t_lin, t_con, t_batch, t_draws):
        monkeypatch.setattr(mod, "_case", case)


@pytest.mark.parametrize("d", [5, 32])
def test_predict_cov_own_check(ctx, own_module_checks, d):
    t_cov._check_case(ctx, 300, d, 257)


@pytest.mark.parametrize("d", [5, 32])
def test_predict_linear_own_check(ctx, own_module_checks, d):
    t_lin._check_case(ctx, 300, d, 700, 6)


@pytest.mark.parametrize("d", [5, 32])
def test_predict_conditioned_own_check(ctx, own_module_checks, d):
    t_con._check_case(ctx, 300, d, 700, 6)


@pytest.mark.parametrize("d", [5, 32])
def test_predict_batch_own_check(ctx, own_module_checks, d):
    t_batch.test_tile_boundaries_vs_closed_form(ctx, 300, d, 700, 3)
    t_batch.test_one_particle_is_bitwise_predict(ctx, 300, d, 700)


@pytest.mark.parametrize("d", [5, 32])
def test_posterior_draws_own_check(ctx, own_module_checks, d):
    t_draws.test_parity_with_predict_cov(ctx, 300, d, 257, 5)


@pytest.mark.parametrize("d", [9, 32])
def test_cross_cov_batch_is_bitwise_cross_cov(ctx, monkeypatch, own_module_checks, d):
    """test_predict_batch_gpu's comparison of k_cross_cov_batch<0> with k_cross_cov<0> on this recipe, where
    K_s is of order 1 (on that module's own length scales it is below 1e-20 at these dimensions)."""
    t_batch.test_cross_cov_batch_is_bitwise_cross_cov(ctx, monkeypatch, d)
    x, y, e, ls, q = case(257, d, 300)
    ks = ref_cpu.kernel_func(x, q, ls[0])
    assert 0.3 < np.median(ks) < 1.0


# ---------------------------------------------------------------------------------------------
# 6. lml_batch: k_lml_grad's coordinates in the GEMM stages, red[wave * DMAX + k], the d-strided partials.
# ---------------------------------------------------------------------------------------------
def lml_reference(N, d, P):
    def make():
        x, y, e, ls = recipe(N, d, P)
        vals, grads = zip(*(lml_closed_form(x, y, e, l) for l in ls))
        return np.array(vals), np.array(grads)
    return shared(("lml", N, d, P), make)


def check_lml(tag, lml, grad, want, gwant):
    """Every gradient component on its own first, so that a single bad coordinate names itself, then
    test_lml_grad_gpu._check (the value, and the gradient per particle)."""
    scale = np.max(np.abs(gwant), axis=1)
    err = np.abs(grad - gwant) / scale[:, None]
    p, k = np.unravel_index(np.argmax(err), err.shape)
    say(f"{tag}: worst gradient component k={k} of particle {p}: {err[p, k]:.3e} of max_k |ref_k|; "
        f"|ref| in [{np.min(np.abs(gwant)):.3e}, {np.max(np.abs(gwant)):.3e}]")
    for p in range(err.shape[0]):
        for k in range(err.shape[1]):
            assert err[p, k] <= TOL, (f"{tag}: particle {p}, gradient component k={k}: got {grad[p, k]!r}, "
                                      f"reference {gwant[p, k]!r}, |difference| / max_k |ref_k| = {err[p, k]:.3e}")
    t_lml._check(tag, lml, grad, want, gwant)


@pytest.mark.parametrize("d", [5, 8, 17, 31, 32])
def test_lml_batch_vs_closed_form(ctx, prefixed, d):
    N, P = 300, 5
    x, y, e, ls = recipe(N, d, P)
    want, gwant = lml_reference(N, d, P)
    ctx.set_data(x, y, e)
    lml, grad = ctx.lml_batch(ls)
    assert grad.shape == (P, d)
    check_lml(f"lml_batch N={N} d={d} P={P}", lml, grad, want, gwant)


def test_lml_batch_chunked_is_bitwise(ctx, monkeypatch, prefixed):
    """5 particles at d = 32 through a workspace capped at 2 per chunk (a fresh context: the cap is read
    when the workspace is sized): chunks of 2, 2 and 1, every row bitwise the single-chunk run's."""
    import gpfit
    N, d, P = 300, 32, 5
    x, y, e, ls = recipe(N, d, P)
    want, gwant = lml_reference(N, d, P)
    ctx.set_data(x, y, e)
    lml, grad = ctx.lml_batch(ls)
    monkeypatch.setenv("GPF_MAX_CHUNK", "2")
    c = gpfit.Context(0)
    try:
        c.set_data(x, y, e)
        lml2, grad2 = c.lml_batch(ls)
    finally:
        c.close()
    check_lml(f"lml_batch N={N} d={d} P={P}, chunks of 2", lml2, grad2, want, gwant)
    np.testing.assert_array_equal(lml2, lml)
    np.testing.assert_array_equal(grad2, grad)


# ---------------------------------------------------------------------------------------------
# 8. The dimension changes on a live context.
# ---------------------------------------------------------------------------------------------
def _all_calls(c, d):
    N, M, P = 300, 257, 5
    x, y, e, ls, q = case(N, d, M)
    ls = recipe(N, d, P)[3]
    s, ex = ref_cpu.sigma_grid()
    c.set_data(x, y, e)
    c.set_grid(s, ex, *box(d))
    out = list(c.eval_batch(ls, want_mu_sd=True))
    out.append(c.eval_batch(ls))
    out += list(c.predict(ls[1], q))
    out += list(c.lml_batch(ls))
    out += list(c.predict_batch(ls[:3], q)[:2])
    rng = np.random.default_rng(d)
    X = rng.uniform(size=(400, d))
    c.kmeans_set(X)
    out += [a for a in c.kmeans_step(X[rng.choice(400, 40, replace=False)], update=True, want_dist=True)]
    assert all(np.all(np.isfinite(a)) for a in out)
    return out


def test_dimension_changes_on_a_live_context():
    """d = 2, then 32, then 2 again on one context (set_data, set_grid, eval_batch, predict, lml_batch,
    predict_batch, a kmeans step): every result bitwise that of a fresh context at that d — the staged
    length scales, the kept prediction sets, the gradient partials and the kmeans buffers follow d."""
    import gpfit
    fresh = {}
    for d in (2, 32):
        c = gpfit.Context(0)
        try:
            fresh[d] = _all_calls(c, d)
        finally:
            c.close()
    live = gpfit.Context(0)
    try:
        for step, d in enumerate((2, 32, 2)):
            got = _all_calls(live, d)
            assert len(got) == len(fresh[d])
            for i, (a, b) in enumerate(zip(got, fresh[d])):
                np.testing.assert_array_equal(a, b, err_msg=f"step {step} (d = {d}): output {i}")
    finally:
        live.close()


# ---------------------------------------------------------------------------------------------
# 9. The dimension contract at the API.
# ---------------------------------------------------------------------------------------------
def test_wrong_dimension_is_value_error_and_leaves_the_context_usable():
    """Every array whose dimension does not match the data's is refused with ValueError before the library
    reads it (the C side reads d doubles per row whatever the buffer holds), d = 33 is refused by the
    library, and gpf_eval_batch refuses to run on the box of another dimension. After each refusal the
    same good calls give the same bits as before."""
    import gpfit
    N, d, M = 129, 6, 130
    x, y, e, ls, q = case(N, d, M)
    s, ex = ref_cpu.sigma_grid()
    lo, hi = box(d)
    c = gpfit.Context(0)
    comm = gpfit.Comm(0, 1, transport="host")

    def good():
        out = list(c.eval_batch(ls, want_mu_sd=True)) + [c.eval_batch_sharded(comm, ls)]
        out += list(c.predict(ls[0], q)) + [c.kernel(x, q, ls[1]), c.log_marginal_likelihood(ls[2])]
        out += [np.tril(a) if a.ndim == 2 else a for a in c.debug_factor(ls[0])]
        return out

    def refused(what, call, match=None):
        with pytest.raises(ValueError, match=match):
            call()
        for i, (a, b) in enumerate(zip(good(), before)):
            np.testing.assert_array_equal(a, b, err_msg=f"after {what}: output {i}")

    wide, narrow = np.hstack([ls, ls[:, :1]]), ls[:, :-1]
    x33 = np.random.default_rng(33).uniform(size=(33, 40))
    try:
        c.set_data(x, y, e)
        c.set_grid(s, ex, lo, hi)
        before = good()
        np.testing.assert_array_equal(before[3], before[0])   # one rank: the sharded scores are eval_batch's
        refused("set_data d=33", lambda: c.set_data(x33, y[:40], e[:40]), "DMAX")
        assert (c.N, c.d) == (N, d)
        refused("kernel d=33", lambda: c.kernel(x33, x33, np.ones(33)))
        refused("kmeans_set d=33", lambda: c.kmeans_set(x33.T.copy()))
        for P in (wide, narrow):
            refused("eval_batch", lambda: c.eval_batch(P), "positions")
            refused("eval_batch_sharded", lambda: c.eval_batch_sharded(comm, P), "positions")
            refused("predict lengths", lambda: c.predict(P[0], q), "lengths")
            refused("kernel l", lambda: c.kernel(x, q, P[0]))
            refused("log_marginal_likelihood", lambda: c.log_marginal_likelihood(P[0]), "lengths")
            refused("debug_factor", lambda: c.debug_factor(P[0]), "lengths")
        refused("predict x_fit d+1", lambda: c.predict(ls[0], np.vstack([q, q[:1]])), "x_fit")
        refused("predict x_fit d-1", lambda: c.predict(ls[0], q[:-1]), "x_fit")
        refused("kernel x2 d-1", lambda: c.kernel(x, q[:-1], ls[0]))
        refused("kernel x2 d+1", lambda: c.kernel(x, np.vstack([q, q[:1]]), ls[0]))
        # kmeans_step reads k x d doubles with the d of kmeans_set
        Xk = np.ascontiguousarray(x.T)
        c.kmeans_set(Xk)
        km = c.kmeans_step(Xk[:10], update=True, want_dist=True)
        for C in (Xk[:10, :-1], np.hstack([Xk[:10], Xk[:10, :1]])):
            with pytest.raises(ValueError, match="centers"):
                c.kmeans_step(C)
            for a, b in zip(c.kmeans_step(Xk[:10], update=True, want_dist=True), km):
                np.testing.assert_array_equal(a, b)
        # a new d without a new grid: the box of the old d would be indexed past its end (larger d) or hold
        # the bounds of other dimensions
        for d2 in (d + 3, d - 2):
            x2, y2, e2, ls2 = recipe(N, d2)
            c.set_data(x2, y2, e2)
            with pytest.raises(ValueError, match="gpf_set_grid"):
                c.eval_batch(ls2)
            lml, _ = c.lml_batch(ls2)   # what needs no grid still runs
            assert np.all(np.isfinite(lml))
            with pytest.raises(ValueError, match="gpf_set_grid"):
                c.eval_batch(ls2)       # (lml_batch sized the workspace: still no grid)
            c.set_grid(s, ex, *box(d2))
            got = c.eval_batch(ls2)
            f = gpfit.Context(0)
            try:
                f.set_data(x2, y2, e2)
                f.set_grid(s, ex, *box(d2))
                np.testing.assert_array_equal(got, f.eval_batch(ls2), err_msg=f"d = {d2} after a new grid")
            finally:
                f.close()
        c.set_data(x, y, e)
        c.set_grid(s, ex, lo, hi)
        for i, (a, b) in enumerate(zip(good(), before)):
            np.testing.assert_array_equal(a, b, err_msg=f"back at d = {d}: output {i}")
    finally:
        comm.close()
        c.close()
    # a context that never had a grid: a call that needs none gives K a placeholder of 2, which must neither
    # let eval_batch through nor keep a 2-point grid set afterwards from being stored
    two = (s[[0, -1]], ex[[0, -1]], lo, hi)
    out = []
    for first in (True, False):
        f = gpfit.Context(0)
        try:
            f.set_data(x, y, e)
            if first:
                assert np.isfinite(f.log_marginal_likelihood(ls[0]))
                with pytest.raises(ValueError, match="gpf_set_grid"):
                    f.eval_batch(ls)
            f.set_grid(*two)
            out.append(f.eval_batch(ls))
        finally:
            f.close()
    assert np.all(np.isfinite(out[0])) and np.all(out[0] < 1e13)
    np.testing.assert_array_equal(out[0], out[1])
