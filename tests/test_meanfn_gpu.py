"""gpf_lml_mean_batch and gpf_predict_mean (the marginalised polynomial mean: the restricted likelihood and
its gradient in (l, a, s), beta, Q', and the prediction) against gpfit.meanfn's float64 NumPy closed
forms, which work straight from Kn by Rasmussen & Williams eq. 2.41-2.45 and form neither the
unit-amplitude matrix nor the orthonormalised basis nor the residual the device uses.

Recipe: conftest.synth_data(N, d, heteroscedastic, seed N) with a constant 5 added to y; five particles
from default_rng(N + 1): l ~ U(0.05, 0.8), a ~ U(0.5, 3), s = a U(0.7, 1.5). Rows of H beyond the named
polynomial basis are rng.standard_normal.

Tolerance: 1e-9 + 10 gap64 for the value, Q' (|got - want| / max(|want|, 1)), beta and the gradient (largest
component error over the largest reference component, all d + 2 components), gap64 being the float64
closed form's own distance from the same formulas in np.longdouble (tests/test_meanfn_host.py's
mean_longdouble) for that particle and quantity: tests/test_loo_gpu.py's rule. On every case below gap64
is under 1e-10 on the CPU (largest: 9.5e-12 value at N = 257, 2.8e-12 gradient, 1.4e-12 beta, 1.1e-12 Q'),
so the bound is 1e-9 to within 10%; `check` asserts that too. The measured maxima are printed (run with
-s). The shift-invariance test compares the device with itself: at an offset of 1000 the closed form
(which works from Kn^-1 y) is itself 5e-8 off, while in NumPy the residual form Q' = zr^T zr the device
uses moves by 5e-13 at N = 300 and y^T alt - c^T beta by 2e-11.

At N = 5 the six-row quadratic basis has more rows than the call allows (m < N): its first four are used.
"""
import numpy as np
import pytest

from conftest import synth_data
from test_meanfn_host import gaps, mean_longdouble

pytestmark = pytest.mark.gpu

TOL = 1e-9
OFFSET = 5.0


@pytest.fixture(scope="module")
def ctx():
    import gpfit
    c = gpfit.Context(0)
    yield c
    c.close()


def recipe(N, d, P=5):
    x, y, e = synth_data(N, d, True, N)
    rng = np.random.default_rng(N + 1)
    ls = rng.uniform(0.05, 0.8, size=(P, d))
    a = rng.uniform(0.5, 3.0, size=P)
    return x, y + OFFSET, e, np.column_stack([ls, a, a * rng.uniform(0.7, 1.5, size=P)])


def basis_m(x, m, kind="quadratic"):
    """The first m rows of the polynomial basis, or all of them and standard-normal rows up to m."""
    from gpfit.meanfn import basis
    H = basis(x, kind)[0]
    if m is None or m == H.shape[0]:
        return H
    if m < H.shape[0]:
        return H[:m]
    return np.vstack([H, np.random.default_rng(1000 + m).standard_normal((m - H.shape[0], x.shape[1]))])


_REF = {}


def reference(key, x, y, e, H, theta):
    """(value, grad, beta, Q', gap64 (P, 4)) of every particle from the float64 closed form, and its
    distance from the longdouble one; computed once per case, shared and read-only."""
    from gpfit.meanfn import mean_closed_form
    if key not in _REF:
        rows = [mean_closed_form(x, y, e, H, p) for p in theta]
        gap = np.array([gaps(r, mean_longdouble(x, y, e, H, p)) for r, p in zip(rows, theta)])
        out = tuple(np.array(v) for v in zip(*rows)) + (gap,)
        for a in out:
            a.setflags(write=False)
        _REF[key] = out
    return _REF[key]


def check(tag, got, ref, rows=None):
    """got = (lml, grad, beta, q) of the batch against the reference rows."""
    want, gwant, bwant, qwant, gap = ref
    rows = list(range(len(want)) if rows is None else rows)
    err = np.array([gaps((got[0][p], got[1][p], got[2][p], got[3][p]), (want[p], gwant[p], bwant[p], qwant[p]))
                    for p in rows])
    tol = TOL + 10.0 * gap[rows]
    names = ("value", "gradient", "beta", "Q'")
    print(f"[meanfn] {tag}: " + ", ".join(f"{n} {np.max(err[:, k]):.2e} (gap64 {np.max(gap[rows][:, k]):.1e})"
                                           for k, n in enumerate(names)))
    assert np.max(gap[rows]) < 1e-10, f"{tag}: the float64 closed form is {gap[rows]} from longdouble"
    for k, n in enumerate(names):
        assert np.all(err[:, k] < tol[:, k]), f"{tag}: {n} errors {err[:, k]} (tolerances {tol[:, k]})"


def run(c, x, y, e, H, th, **kw):
    c.set_data(x, y, e)
    c.set_basis(H)
    lml, g, q, beta = c.lml_mean_batch(th, want_q=True, want_beta=True, **kw)
    return lml, g, beta, q


@pytest.mark.parametrize("N", [5, 127, 128, 129, 257, 300])
def test_sizes_quadratic_basis(ctx, N):
    """d = 2, the quadratic basis (m = 6; at N = 5 its first 4 rows: m < N)."""
    x, y, e, th = recipe(N, 2)
    H = basis_m(x, 4 if N == 5 else None)
    assert H.shape[0] == (4 if N == 5 else 6)
    got = run(ctx, x, y, e, H, th)
    assert got[1].shape == (5, 4) and got[2].shape == (5, H.shape[0])
    check(f"N={N} d=2 m={H.shape[0]}", got, reference(("size", N), x, y, e, H, th))


@pytest.mark.parametrize("m", [1, 16, 17, 32])
def test_basis_rows_across_the_mpad_boundary(ctx, m):
    x, y, e, th = recipe(300, 2)
    H = basis_m(x, m)
    assert H.shape == (m, 300)
    check(f"N=300 d=2 m={m}", run(ctx, x, y, e, H, th), reference(("rows", m), x, y, e, H, th))


@pytest.mark.parametrize("d", [1, 3, 4])
def test_dimensions(ctx, d):
    x, y, e, th = recipe(200, d)
    H = basis_m(x, None)
    assert H.shape[0] == 1 + d + d * (d + 1) // 2
    check(f"N=200 d={d} m={H.shape[0]}", run(ctx, x, y, e, H, th), reference(("dim", d), x, y, e, H, th))


def test_repeat_call_and_value_only_give_the_same_bits(ctx):
    x, y, e, th = recipe(300, 2)
    H = basis_m(x, None)
    first = run(ctx, x, y, e, H, th)
    again = run(ctx, x, y, e, H, th)
    for a, b in zip(first, again):
        np.testing.assert_array_equal(a, b)
    lml, none, q, beta = ctx.lml_mean_batch(th, grad=False, want_q=True, want_beta=True)
    assert none is None
    np.testing.assert_array_equal(lml, first[0])
    np.testing.assert_array_equal(beta, first[2])
    np.testing.assert_array_equal(q, first[3])
    assert len(ctx.lml_mean_batch(th, grad=False)) == 2
    assert ctx.lml_mean_batch(np.empty((0, 4)))[0].shape == (0,)


def test_shift_invariance(ctx):
    """What the basis spans moves beta and nothing else, at an offset of 1000: the residual form.
    (In NumPy, Q' = zr^T zr at this N and offset is 1e-12 from its unshifted value; y^T alt - c^T beta
    is not.)"""
    from gpfit.meanfn import basis
    N = 300
    x, y, e, th = recipe(N, 2)
    ctx.set_data(x, y, e)
    ctx.set_basis(basis(x, "constant")[0])
    lml, g, q, beta = ctx.lml_mean_batch(th, want_q=True, want_beta=True)
    ctx.set_data(x, y + 1000.0, e)
    ctx.set_basis(basis(x, "constant")[0])
    lml2, g2, q2, beta2 = ctx.lml_mean_batch(th, want_q=True, want_beta=True)
    ev = np.max(np.abs(lml2 - lml) / np.abs(lml))
    eg = np.max(np.max(np.abs(g2 - g), axis=1) / np.max(np.abs(g), axis=1))
    eb = np.max(np.abs((beta2 - beta)[:, 0] - 1000.0))
    print(f"[meanfn] constant basis, y + 1000: lml moves {ev:.2e} relative, gradient {eg:.2e}, beta_0 - 1000: {eb:.2e}")
    assert ev < 1e-9, ev
    assert eb < 1e-9 * 1000.0, eb  # (the gradient's figure is printed: at = alt - Bt^T t carries the offset in alt)
    # the linear basis: an added linear trend moves only beta
    H, _ = basis(x, "linear")
    c = np.array([300.0, -50.0, 20.0])
    ctx.set_data(x, y, e)
    ctx.set_basis(H)
    lml, g, q, beta = ctx.lml_mean_batch(th, want_q=True, want_beta=True)
    ctx.set_data(x, y + H.T @ c, e)
    ctx.set_basis(H)
    lml2, g2, q2, beta2 = ctx.lml_mean_batch(th, want_q=True, want_beta=True)
    ev = np.max(np.abs(lml2 - lml) / np.abs(lml))
    eq = np.max(np.abs(q2 - q) / np.abs(q))
    eb = np.max(np.abs(beta2 - beta - c))
    print(f"[meanfn] linear basis, y + trend: lml moves {ev:.2e} relative, Q' {eq:.2e}, beta - c: {eb:.2e}")
    assert ev < 1e-9 and eq < 1e-9 and eb < 1e-9 * 300.0, (ev, eq, eb)


def _chunk_case():
    x, y, e, th = recipe(300, 2, P=10)
    H = basis_m(x, None)
    return x, y, e, H, th, reference(("chunk", 300), x, y, e, H, th)


def test_chunked_batch(monkeypatch):
    """10 particles through a workspace capped at 4 per chunk (a fresh context: the cap is read when
    the workspace is sized): every chunk's particles get their own amplitudes, noise factors and rows."""
    import gpfit
    x, y, e, H, th, ref = _chunk_case()
    monkeypatch.setenv("GPF_MAX_CHUNK", "4")
    c = gpfit.Context(0)
    try:
        check("N=300 d=2 P=10, chunks of 4", run(c, x, y, e, H, th), ref)
    finally:
        c.close()


def test_persistent_factorisation(ctx, monkeypatch):
    import gpfit
    x, y, e, th = recipe(300, 2)
    H = basis_m(x, None)
    monkeypatch.setenv("GPF_PERSIST", "1")
    assert gpfit.plan_check(5, 3)["persistent"] == 1
    check("N=300 d=2 GPF_PERSIST=1", run(ctx, x, y, e, H, th), reference(("size", 300), x, y, e, H, th))


@pytest.mark.parametrize("bad", [1, 5])
def test_non_pd_particle_in_the_first_and_in_a_later_chunk(monkeypatch, bad):
    """The clustered zero-noise points of tests/test_loo_gpu.py's non-PD tests (the cluster at the origin,
    where the kernel's rounding does not decide the comparison; l = 0.2 fails inside the cluster, l in
    [0.011, 0.016] is well conditioned) with a level of 5, six particles through chunks of 4: the failing
    row's status, -inf and NaN rows land at its index in the batch, the others are right."""
    import gpfit
    from gpfit.meanfn import basis
    from test_loo_gpu import _cluster_at_origin
    N, c0, P = 300, 144, 6
    x, y, e = _cluster_at_origin(N, c0)
    y = y + OFFSET
    H, _ = basis(x, "linear")
    rng = np.random.default_rng(P)
    a = rng.uniform(0.5, 3.0, size=P)
    good = np.column_stack([rng.uniform(0.011, 0.016, size=P), a, a * rng.uniform(0.7, 1.5, size=P)])
    ref = reference(("cluster", N), x, y, e, H, good)
    Q = good.copy()
    Q[bad, 0] = 0.2
    others = [p for p in range(P) if p != bad]
    monkeypatch.setenv("GPF_MAX_CHUNK", "4")
    c = gpfit.Context(0)
    try:
        c.set_data(x, y, e)
        c.set_basis(H)
        lml, g, q, beta = c.lml_mean_batch(Q, strict=False, want_q=True, want_beta=True)
        assert lml[bad] == -np.inf and np.all(np.isnan(g[bad])) and np.isnan(q[bad]) and np.all(np.isnan(beta[bad]))
        for v in (lml, g, q, beta):
            assert np.all(np.isfinite(v[others]))
        check(f"cluster N=300, non-PD row {bad}", (lml, g, beta, q), ref, rows=others)
        with pytest.raises(np.linalg.LinAlgError, match="Matrix is not positive definite") as ei:
            c.lml_mean_batch(Q)
        assert ei.value.particle == bad
        lml, g, q, beta = c.lml_mean_batch(good, want_q=True, want_beta=True)
        check("cluster N=300, clean batch after the failure", (lml, g, beta, q), ref)
    finally:
        c.close()


def test_rank_deficient_basis_is_not_pd_and_says_which(ctx):
    """A basis with a row of zeros gets past the C call's own checks (the binding's rank check is the
    guard) and fails in the factor of H Kt^-1 H^T with a pivot of exactly 0 for every particle:
    GPF_NOT_PD, and the message names that matrix, not Kt."""
    import ctypes
    x, y, e, th = recipe(129, 2)
    H = basis_m(x, 3)
    Hd = np.ascontiguousarray(np.vstack([H, np.zeros(129)]))
    ctx.set_data(x, y, e)
    with pytest.raises(ValueError, match="rank-deficient"):
        ctx.set_basis(Hd)
    dp = ctypes.POINTER(ctypes.c_double)
    assert ctx.lib.gpf_set_basis(ctx._h, Hd.ctypes.data_as(dp), 4) == 0
    ctx.m = 4
    try:
        lml, g, q, beta = ctx.lml_mean_batch(th, strict=False, want_q=True, want_beta=True)
        assert np.all(lml == -np.inf) and np.all(np.isnan(g)) and np.all(np.isnan(q)) and np.all(np.isnan(beta))
        assert "H Kt^-1 H^T" in ctx.lib.gpf_last_error(ctx._h).decode()
        with pytest.raises(np.linalg.LinAlgError) as ei:
            ctx.lml_mean_batch(th)
        assert ei.value.particle == 0
        hf = np.ones((4, 3))
        with pytest.raises(np.linalg.LinAlgError):
            ctx.predict_mean(th[0, :2], x[:, :3], hf)
        assert "H Kt^-1 H^T" in ctx.lib.gpf_last_error(ctx._h).decode()
    finally:
        ctx.set_basis(H)
    assert np.all(np.isfinite(ctx.lml_mean_batch(th)[0]))


@pytest.mark.parametrize("N", [200, 300])
def test_neighbours_untouched(N):
    """eval_batch, lml_batch, lml_hyper_batch and loo_batch give the same bits before and after mean
    calls on a larger batch (the workspace grows) and on the same one (N = 200: the replayed-graph path)."""
    import gpfit
    from oracle import ref_cpu
    x, y, e, th = recipe(N, 2, P=12)
    ls = np.ascontiguousarray(th[:, :2])
    H = basis_m(x, None)
    s, ex = ref_cpu.sigma_grid()
    c = gpfit.Context(0)
    try:
        c.set_data(x, y, e)
        c.set_grid(s, ex, np.full(2, 1e-3), np.full(2, 2.0))

        def neighbours():
            return (c.eval_batch(ls[:5]),) + c.lml_batch(ls[:5]) + c.lml_hyper_batch(th[:5], want_q=True) + \
                c.loo_batch(ls[:5])
        first = neighbours()
        assert all(np.all(np.isfinite(v)) for v in first)
        c.set_basis(H)
        lml, g = c.lml_mean_batch(th)
        assert np.all(np.isfinite(lml)) and np.all(np.isfinite(g))
        for a, b in zip(first, neighbours()):
            np.testing.assert_array_equal(a, b)
        c.lml_mean_batch(th[:5])
        c.predict_mean(ls[0], x[:, :40], H[:, :40])
        for a, b in zip(first, neighbours()):
            np.testing.assert_array_equal(a, b)
    finally:
        c.close()


def test_set_data_discards_the_basis():
    import ctypes
    import gpfit
    x, y, e, th = recipe(129, 2)
    H = basis_m(x, None)
    c = gpfit.Context(0)
    try:
        with pytest.raises(ValueError, match="set_data first"):
            c.set_basis(H)
        with pytest.raises(ValueError, match="gpf_set_data"):
            c.lml_mean_batch(th)
        c.set_data(x, y, e)
        with pytest.raises(ValueError, match="no basis"):
            c.lml_mean_batch(th)
        c.set_basis(H)
        lml, _ = c.lml_mean_batch(th, grad=False)
        c.set_data(x, y + 1.0, e)
        with pytest.raises(ValueError, match="no basis"):
            c.lml_mean_batch(th)
        with pytest.raises(ValueError, match="no basis"):
            c.predict_mean(th[0, :2], x[:, :3], H[:, :3])
        # the library's own rule, past the binding's bookkeeping
        out = np.zeros(5)
        dp = ctypes.POINTER(ctypes.c_double)
        rc = c.lib.gpf_lml_mean_batch(c._h, th.ctypes.data_as(dp), 5, out.ctypes.data_as(dp), None, None, None, None, None)
        assert rc == gpfit._lib.GPF_BAD_ARG and b"gpf_set_basis" in c.lib.gpf_last_error(c._h)
        # a rejected basis leaves the one in force
        c.set_basis(H)
        bad = np.ascontiguousarray(H.copy())
        bad[2, 7] = np.inf
        assert c.lib.gpf_set_basis(c._h, bad.ctypes.data_as(dp), 6) == gpfit._lib.GPF_BAD_ARG
        assert c.lib.gpf_set_basis(c._h, H.ctypes.data_as(dp), 33) == gpfit._lib.GPF_BAD_ARG
        c.set_data(x, y, e)
        c.set_basis(H)
        np.testing.assert_array_equal(c.lml_mean_batch(th, grad=False)[0], lml)
    finally:
        c.close()


_PRED = {}


def _predict_case(N):
    from gpfit.meanfn import basis, predict_mean_closed_form
    if N not in _PRED:
        x, y, e, th = recipe(N, 2)
        kind = "linear" if N == 5 else "quadratic"
        H, box = basis(x, kind)
        xf = np.random.default_rng(N + 2).uniform(-0.25, 1.25, size=(2, 1000))
        hf = basis(xf, kind, box)[0]
        l = th[0, :2]
        ref = predict_mean_closed_form(x, y, e, H, np.append(l, [1.0, 1.0]), xf, hf)
        for a in ref:
            a.setflags(write=False)
        _PRED[N] = (x, y, e, H, l, xf, hf, ref)
    return _PRED[N]


@pytest.mark.parametrize("N", [5, 129, 300])
@pytest.mark.parametrize("M", [1, 128, 129, 1000])
def test_predict_mean_against_the_closed_form(ctx, N, M):
    x, y, e, H, l, xf, hf, (rmu, rsd, rbeta, rcov) = _predict_case(N)
    ctx.set_data(x, y, e)
    ctx.set_basis(H)
    xq, hq = np.ascontiguousarray(xf[:, :M]), np.ascontiguousarray(hf[:, :M])
    mu, sd, beta, bcov = ctx.predict_mean(l, xq, hq, want_beta=True)
    em = np.max(np.abs(mu - rmu[:M]) / np.maximum(np.abs(rmu[:M]), 1.0))
    es = np.max(np.abs(sd - rsd[:M]) / rsd[:M])
    eb = np.max(np.abs(beta - rbeta)) / np.max(np.abs(rbeta))
    # cov(beta) against inv(H Kn^-1 H^T)
    ec = np.max(np.abs(bcov - rcov)) / np.max(np.abs(rcov))
    print(f"[meanfn] predict N={N} M={M}: mu {em:.2e}, sd {es:.2e}, beta {eb:.2e}, cov(beta) {ec:.2e}")
    assert max(em, es, eb, ec) < TOL, (em, es, eb, ec)
    np.testing.assert_array_equal(bcov, bcov.T)
    # the query chunking does not change the bits
    mu2, sd2 = ctx.predict_mean(l, xq, hq, batch_size=128)
    np.testing.assert_array_equal(mu2, mu)
    np.testing.assert_array_equal(sd2, sd)
    assert len(ctx.predict_mean(l, xq[:, :0], hq[:, :0])[0]) == 0


def test_predict_mean_two_chunks_and_far_from_the_data(ctx):
    """A query set past gpf_predict's chunk floor of 16384 points: batch 128 takes it in two chunks,
    batch 20000 in one, with the same bits. And far from the data the mean tends to h^T beta, not to 0,
    with the sd of not knowing beta on top of the prior's."""
    from gpfit.meanfn import basis
    x, y, e, H, l, xf, hf, (rmu, rsd, rbeta, rcov) = _predict_case(300)
    ctx.set_data(x, y, e)
    ctx.set_basis(H)
    _, box = basis(x, "quadratic")
    big = np.random.default_rng(9).uniform(-0.25, 1.25, size=(2, 20000))
    hbig = basis(big, "quadratic", box)[0]
    one = ctx.predict_mean(l, big, hbig, batch_size=20000)
    two = ctx.predict_mean(l, big, hbig, batch_size=128)
    np.testing.assert_array_equal(two[0], one[0])
    np.testing.assert_array_equal(two[1], one[1])
    mu, sd, beta, bcov = ctx.predict_mean(l, xf, hf, want_beta=True)
    np.testing.assert_array_equal(ctx.predict_mean(l, np.ascontiguousarray(big[:, :1000]),
                                                   np.ascontiguousarray(hbig[:, :1000]))[0], one[0][:1000])
    far = np.array([[40.0, -30.0], [25.0, 60.0]])
    hfar = basis(far, "quadratic", box)[0]
    mf, sf = ctx.predict_mean(l, far, hfar)
    want = hfar.T @ beta
    assert np.all(np.abs(want) > 1.0)
    np.testing.assert_allclose(mf, want, rtol=1e-9)
    np.testing.assert_allclose(sf ** 2, 1.0 + np.sum(hfar * (bcov @ hfar), axis=0), rtol=1e-9)
    # the zero-mean model returns to 0 there
    m0, s0 = ctx.predict(l, far)
    assert np.all(np.abs(m0) < 1e-6) and np.all(np.abs(s0 - 1.0) < 1e-9)


def test_not_pd_leaves_the_outputs_untouched(ctx):
    from gpfit.meanfn import basis
    from test_loo_gpu import _cluster_at_origin
    x, y, e = _cluster_at_origin(300, 144)
    H, box = basis(x, "linear")
    ctx.set_data(x, y + OFFSET, e)
    ctx.set_basis(H)
    xf = np.linspace(0.0, 10.0, 7)[None, :]
    with pytest.raises(np.linalg.LinAlgError, match="Matrix is not positive definite"):
        ctx.predict_mean(np.array([0.2]), xf, basis(xf, "linear", box)[0])
    mu, sd = ctx.predict_mean(np.array([0.015]), xf, basis(xf, "linear", box)[0])
    assert np.all(np.isfinite(mu)) and np.all(sd > 0)


def test_fit_mean_end_to_end(ctx):
    """fit_mean on the device: tests/test_mle_host.py's first recipe (seed 0, d = 2, N = 150) times 2.5
    plus 5. The device value at the result is the closed form's and no lower than at the generating theta;
    the zero-mean fit of the same data needs a larger amplitude; then predict_mean with the result."""
    from gpfit.amplitude import fit_hyper
    from gpfit.meanfn import basis, fit_mean, mean_closed_form, predict_mean, predict_mean_closed_form
    from test_mle_host import FIT_RECIPES, gp_sample
    seed, d, N, l_true = FIT_RECIPES[0]
    x, y, e = gp_sample(seed, d, N, l_true)
    y, e, gen = 2.5 * y + 5.0, 2.5 * e, np.array(list(l_true) + [2.5, 1.0])
    best, info = fit_mean(x, y, e, kind="constant", num_starts=16, num_polish=1, max_points=N, seed=0, ctx=ctx,
                          verbose=False)
    H, _ = basis(x, "constant")
    at_best, _, beta = ctx.lml_mean_batch(best[None, :], grad=False, want_beta=True)
    truth = ctx.lml_mean_batch(gen[None, :], grad=False)[0][0]
    ref = mean_closed_form(x, y, e, H, best)
    print(f"[meanfn] fit {info['lml']:.4f} at {best}, beta {info['beta']}, generating theta {truth:.4f}, "
          f"evals {info['evals']}, grad evals {info['grad_evals']}")
    assert abs(at_best[0] - ref[0]) < TOL * max(abs(ref[0]), 1.0)
    assert abs(info["lml"] - at_best[0]) < TOL * max(abs(at_best[0]), 1.0)
    assert info["lml"] >= truth
    np.testing.assert_array_equal(info["beta"], beta[0])
    np.testing.assert_allclose(info["beta"], ref[2], rtol=1e-8)
    lower, upper = info["box"]
    assert np.all(best >= lower) and np.all(best <= upper)
    assert info["grad_evals"] < info["evals"]  # the starts were scored without the gradient pass
    zero, _ = fit_hyper(x, y, e, num_starts=16, num_polish=1, max_points=N, seed=0, ctx=ctx, verbose=False)
    assert zero[d] > best[d], (zero, best)
    xf = np.random.default_rng(3).uniform(-0.2, 1.2, size=(d, 60))
    mu, sd, b, bc = predict_mean(x, y, e, xf, best, "constant", ctx=ctx, want_beta=True)
    rmu, rsd, rb, rc = predict_mean_closed_form(x, y, e, H, best, xf, np.ones((1, 60)))
    assert np.max(np.abs(mu - rmu) / np.maximum(np.abs(rmu), 1.0)) < TOL
    assert np.max(np.abs(sd - rsd) / rsd) < TOL
    assert abs(b[0] - rb[0]) < TOL * abs(rb[0]) and abs(bc[0, 0] - rc[0, 0]) < TOL * rc[0, 0]
