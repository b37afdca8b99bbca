"""The covariance kernel family without a GPU: gpfit.kernels' closed forms (the yardstick of
tests/test_kernel_family_gpu.py, which imports the model closed forms below from here), the name checks of
Context.set_kernel and of every kernel= keyword, and options.yaml's `kernel` key.

The model closed forms (`parts`, `lml_form`, `loo_form`, `hyper_form`, `mean_form`) are the suite's existing
ones (test_mle_host.lml_closed_form, test_loo_host._loo_from, test_amplitude_host._hyper_from,
gpfit.meanfn.reml_from) with the kernel's value phi where K stands for the covariance and its derivative
weight psi where K stands for dK/dl; for "se" phi = psi and they are those forms. With dtype=np.longdouble
they run in long double throughout (a hand-written Cholesky factor and forward substitution: LAPACK has no
long double), which is how the float64 forms' own error is measured.
"""
import numpy as np
import pytest

from oracle import ref_cpu

MATERN = ("matern32", "matern52")
ALL = ("se",) + MATERN
LOG_2PI = 1.8378770664093453


# ---------------------------------------------------------------------------------------------
# closed forms of the models, kernel by name, float64 (LAPACK) or long double (hand-written factor)
# ---------------------------------------------------------------------------------------------
def phi_psi(r2, kind):
    """(phi, psi) of r2 in r2's dtype: gpfit.kernels' formulas, written again so that they also run in
    np.longdouble."""
    t = r2.dtype.type
    if kind == "se":
        k = np.exp(-r2 / 2)
        return k, k
    if kind == "matern32":
        s = np.sqrt(3 * r2)
        return (1 + s) * np.exp(-s), 3 * np.exp(-s)
    assert kind == "matern52", kind
    s = np.sqrt(5 * r2)
    return (1 + s + s * s / 3) * np.exp(-s), t(5) / 3 * (1 + s) * np.exp(-s)


def sqdist(xa, xb, l):
    a, b = xa / l[:, None], xb / l[:, None]
    r2 = np.sum(a ** 2, axis=0)[:, None] + np.sum(b ** 2, axis=0)[None, :] - 2 * (a.T @ b)
    return np.maximum(r2, r2.dtype.type(0))


def chol_any(A):
    """Lower Cholesky factor in A's dtype; LinAlgError when a pivot is not > 0."""
    if A.dtype == np.float64:
        return np.linalg.cholesky(A)
    N = A.shape[0]
    L = np.zeros_like(A)
    for j in range(N):
        piv = A[j, j] - L[j, :j] @ L[j, :j]
        if not piv > 0:
            raise np.linalg.LinAlgError("Matrix is not positive definite")
        L[j, j] = np.sqrt(piv)
        L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def tri_inv(L):
    """L^-1 of a lower-triangular L in its dtype (float64: a LAPACK solve)."""
    if L.dtype == np.float64:
        return np.linalg.solve(L, np.eye(L.shape[0]))
    U = np.zeros_like(L)
    for i in range(L.shape[0]):
        row = -(L[i, :i] @ U[:i, :])
        row[i] += 1
        U[i] = row / L[i, i]
    return U


def parts(x, y, e, l, kind, a=1.0, s=1.0, dtype=np.float64):
    """dict of x, y, e, l, K = phi, psi, L = chol(Kn), W = Kn^-1 (float64: np.linalg.inv, as the suite's
    closed forms; long double: U^T U), Kn = a^2 K + s^2 diag(e^2), all in ``dtype``."""
    x, y, e = (np.asarray(v, dtype=dtype) for v in (x, y, e))
    l = np.asarray(l, dtype=dtype).reshape(-1)
    a, s = dtype(a), dtype(s)
    K, psi = phi_psi(sqdist(x, x, l), kind)
    Kn = a * a * K + s * s * np.diag(e ** 2)
    L = chol_any(Kn)
    if dtype == np.float64:
        W = np.linalg.inv(Kn)
    else:
        U = tri_inv(L)
        W = U.T @ U
    return dict(x=x, y=y, e=e, l=l, a=a, s=s, K=K, psi=psi, Kn=Kn, L=L, W=W)


def dl_sums(M, p):
    """g_k = 1/2 sum_ij M_ij psi_ij (x_ik - x_jk)^2 / l_k^3 = sum_{i>j} .. for a symmetric M."""
    x, l = p["x"], p["l"]
    Mp = M * p["psi"]
    return np.array([np.sum(Mp * (x[k][:, None] - x[k][None, :]) ** 2) / 2 / l[k] ** 3 for k in range(len(l))])


def lml_form(p):
    """(LML, dLML/dl (d,)) of parts p at a = s = 1."""
    y, W = p["y"], p["W"]
    t = W.dtype.type
    al = W @ y
    lml = -(y @ al) / 2 - np.sum(np.log(np.diag(p["L"]))) - len(y) * t(LOG_2PI) / 2
    return lml, dl_sums(np.outer(al, al) - W, p)


def loo_form(p):
    """(mu (N,), sd (N,), lpd, dlpd/dl (d,)) of parts p at a = s = 1 (test_loo_host._loo_from)."""
    y, W = p["y"], p["W"]
    t = W.dtype.type
    al = W @ y
    w = np.diag(W).copy()
    q = al * al / w
    lpd = np.sum(np.log(w) / 2 - q / 2) - len(y) * t(LOG_2PI) / 2
    u = W @ (al / w)
    G = (W * ((1 + q) / w / 2)[None, :]) @ W
    return y - al / w, np.sqrt(1 / w), lpd, dl_sums(np.outer(u, al) + np.outer(al, u) - 2 * G, p)


def hyper_form(p):
    """(LML, dLML/d(l, a, s) (d + 2,)) of parts p (test_amplitude_host._hyper_from)."""
    y, e, W, a, s = p["y"], p["e"], p["W"], p["a"], p["s"]
    t = W.dtype.type
    al = W @ y
    lml = -(y @ al) / 2 - np.sum(np.log(np.diag(p["L"]))) - len(y) * t(LOG_2PI) / 2
    M = np.outer(al, al) - W
    return lml, np.concatenate([a * a * dl_sums(M, p), [a * np.sum(M * p["K"]), s * np.sum(np.diag(M) * e ** 2)]])


def mean_form(p, H):
    """(restricted LML, its gradient (d + 2,), beta (m,)) of parts p under the basis H (m, N)
    (gpfit.meanfn.reml_from)."""
    from gpfit.meanfn import chol_small, tri_inverse
    y, e, W, a, s = p["y"], p["e"], p["W"], p["a"], p["s"]
    t = W.dtype.type
    H = np.asarray(H, dtype=W.dtype)
    N, m = len(y), H.shape[0]
    WH = W @ H.T
    La = chol_small(H @ WH)
    Ai = tri_inverse(La)
    Ainv = Ai.T @ Ai
    beta = Ainv @ (WH.T @ y)
    P = W - WH @ Ainv @ WH.T
    ap = P @ y
    lml = -(y @ ap) / 2 - np.sum(np.log(np.diag(p["L"]))) - np.sum(np.log(np.diag(La))) - (N - m) * t(LOG_2PI) / 2
    M = np.outer(ap, ap) - P
    g = np.concatenate([a * a * dl_sums(M, p), [a * np.sum(M * p["K"]), s * np.sum(np.diag(M) * e ** 2)]])
    return lml, g, beta


def gap(g, ref):
    """max |g - ref| / max |ref|: the suite's normwise error measure."""
    ref = np.asarray(ref, dtype=np.longdouble)
    return float(np.max(np.abs(np.asarray(g, dtype=np.longdouble) - ref)) / np.max(np.abs(ref)))


# ---------------------------------------------------------------------------------------------
# gpfit.kernels
# ---------------------------------------------------------------------------------------------
def _points(d, n, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(size=(d, n)), np.sqrt(d) * rng.uniform(0.3, 1.2, size=d)


@pytest.mark.parametrize("kind", MATERN)
def test_unit_diagonal_symmetry_and_positive_semidefiniteness(kind):
    from gpfit.kernels import kernel_dweight, kernel_matrix, kernel_value
    assert kernel_value(0.0, kind) == 1.0
    assert np.isfinite(kernel_dweight(0.0, kind)) and kernel_dweight(0.0, kind) > 0
    for d in (1, 3):
        x, l = _points(d, 60, 7 + d)
        K = kernel_matrix(x, x, l, kind)
        assert K.shape == (60, 60)
        np.testing.assert_array_equal(K, K.T)
        # (kernel_func's r2 of a point with itself can round a few ulp above 0: 1 - phi <= psi(0) r2 / 2)
        assert np.max(np.abs(np.diag(K) - 1.0)) < 1e-14
        assert np.all(K > 0) and np.all(K <= 1.0)
        lam = np.linalg.eigvalsh(K)
        assert lam[0] > -1e-12 * lam[-1], (kind, d, lam[0])
    # coincident points: phi = 1 and a finite weight, no special case
    x = np.array([[0.25, 0.25, 0.75]])
    K = kernel_matrix(x, x, np.array([0.5]), kind)
    assert K[0, 1] == 1.0 and K[0, 0] == 1.0 and 0 < K[0, 2] < 1


@pytest.mark.parametrize("d", [1, 3])
@pytest.mark.parametrize("kind", ALL)
def test_dweight_is_the_derivative_of_the_matrix(kind, d):
    """kernel_dweight against central differences of kernel_matrix in every l_k: step h = 1e-5 l_k, whose
    truncation error is of order h^2 and whose rounding error eps / h ~ 2e-11 of K <= 1."""
    from gpfit.kernels import kernel_dweight, kernel_matrix, scaled_sqdist
    x, l = _points(d, 40, 11 + d)
    psi = kernel_dweight(scaled_sqdist(x, x, l), kind)
    for k in range(d):
        h = 1e-5 * l[k]
        lp, lm = l.copy(), l.copy()
        lp[k] += h
        lm[k] -= h
        fd = (kernel_matrix(x, x, lp, kind) - kernel_matrix(x, x, lm, kind)) / (lp[k] - lm[k])
        want = psi * (x[k][:, None] - x[k][None, :]) ** 2 / l[k] ** 3
        assert np.max(np.abs(fd - want)) < 1e-8 * max(np.max(np.abs(want)), 1.0), (kind, d, k)
    # ... and of this module's long-double forms, which the GPU tests' distances are measured with
    r2 = scaled_sqdist(x, x, l)
    phi, psi2 = phi_psi(r2, kind)
    np.testing.assert_allclose(psi2, psi, rtol=1e-14)
    np.testing.assert_allclose(phi, kernel_matrix(x, x, l, kind), rtol=1e-14)


def test_se_matrix_is_bitwise_the_oracle_kernel():
    from gpfit.kernels import kernel_dweight, kernel_matrix, scaled_sqdist
    for d, n1, n2 in ((1, 40, 33), (3, 60, 60), (5, 33, 257)):
        rng = np.random.default_rng(d)
        xa, xb, l = rng.uniform(size=(d, n1)), rng.uniform(size=(d, n2)), rng.uniform(0.2, 1.5, size=d)
        np.testing.assert_array_equal(kernel_matrix(xa, xb, l, "se"), ref_cpu.kernel_func(xa, xb, l))
        np.testing.assert_array_equal(kernel_matrix(xa, xb, l), ref_cpu.kernel_func(xa, xb, l))
        r2 = scaled_sqdist(xa, xb, l)
        np.testing.assert_array_equal(kernel_dweight(r2, "se"), ref_cpu.kernel_func(xa, xb, l))


def test_se_forms_are_the_suites_closed_forms():
    """With "se" the forms above are the existing modules': the new tests' yardstick is theirs."""
    from test_amplitude_host import hyper_closed_form
    from test_loo_host import loo_closed_form
    from test_mle_host import lml_closed_form
    rng = np.random.default_rng(3)
    x, y, e = rng.uniform(size=(2, 50)), rng.standard_normal(50), rng.uniform(0.05, 0.2, size=50)
    l = np.array([0.4, 0.7])
    v, g = lml_form(parts(x, y, e, l, "se"))
    v0, g0 = lml_closed_form(x, y, e, l)
    assert abs(v - v0) < 1e-12 * abs(v0) and gap(g, g0) < 1e-12
    for got, want in zip(loo_form(parts(x, y, e, l, "se")), loo_closed_form(x, y, e, l)):
        assert gap(np.atleast_1d(got), np.atleast_1d(want)) < 1e-12
    v, g = hyper_form(parts(x, y, e, l, "se", a=1.3, s=0.8))
    v0, g0 = hyper_closed_form(x, y, e, np.array([0.4, 0.7, 1.3, 0.8]))
    assert abs(v - v0) < 1e-12 * abs(v0) and gap(g, g0) < 1e-12


@pytest.mark.parametrize("kind", MATERN)
def test_closed_form_gradients_are_the_derivatives(kind):
    """The four model gradients against central differences of their own values (h = 1e-5 relative)."""
    from gpfit.meanfn import basis
    rng = np.random.default_rng(5)
    d, N = 2, 40
    x, y, e = rng.uniform(size=(d, N)), rng.standard_normal(N), rng.uniform(0.05, 0.2, size=N)
    H, _ = basis(x, "linear")
    th = np.array([0.6, 0.9, 1.3, 0.8])
    forms = {
        "lml": (lambda t: lml_form(parts(x, y, e, t[:d], kind))[:2], d),
        "loo": (lambda t: loo_form(parts(x, y, e, t[:d], kind))[2:], d),
        "hyper": (lambda t: hyper_form(parts(x, y, e, t[:d], kind, t[d], t[d + 1])), d + 2),
        "mean": (lambda t: mean_form(parts(x, y, e, t[:d], kind, t[d], t[d + 1]), H)[:2], d + 2),
    }
    for name, (f, n) in forms.items():
        _, g = f(th)
        fd = np.empty(n)
        for k in range(n):
            tp, tm = th.copy(), th.copy()
            tp[k] *= 1 + 1e-5
            tm[k] *= 1 - 1e-5
            fd[k] = (f(tp)[0] - f(tm)[0]) / (tp[k] - tm[k])
        assert gap(g[:n], fd) < 1e-6, (kind, name, g, fd)


# ---------------------------------------------------------------------------------------------
# names: Context.set_kernel and the kernel= keywords, without a library
# ---------------------------------------------------------------------------------------------
class _NoLibrary:
    """Stands where a context or its library would be: any use is a failure."""

    def __getattr__(self, name):
        raise AssertionError(f"the library was touched ({name})")


def test_kernel_names():
    from gpfit.kernels import KINDS, kernel_kind
    assert KINDS == ("se", "matern32", "matern52")
    assert [kernel_kind(k) for k in KINDS] == [0, 1, 2]
    for bad in ("matern12", "SE", "", None, 1, b"se"):
        with pytest.raises(ValueError, match="matern32"):
            kernel_kind(bad)


def test_set_kernel_rejects_an_unknown_name_before_the_library(monkeypatch):
    import gpfit._lib as L
    monkeypatch.setattr(L, "load_library", lambda: pytest.fail("load_library ran"))
    c = object.__new__(L.Context)   # no gpf_open: the name is checked first
    c.lib, c._h = _NoLibrary(), None
    for bad in ("matern12", "rbf", None, 2):
        with pytest.raises(ValueError, match="'se', 'matern32', 'matern52'"):
            c.set_kernel(bad)
    c._h = None


def test_kernel_keywords_reject_an_unknown_name_before_any_context(monkeypatch):
    import find_len_scales
    import GP_func
    import gpfit._lib as L
    from gpfit import amplitude, conditioned, hyper, linear, loo, meanfn, mle, posterior, swarm
    for mod in (L, GP_func, find_len_scales, amplitude, conditioned, hyper, linear, loo, meanfn, mle, posterior, swarm):
        monkeypatch.setattr(mod, "default_context", lambda: pytest.fail("default_context ran"), raising=False)
    monkeypatch.setattr(L, "load_library", lambda: pytest.fail("load_library ran"))
    rng = np.random.default_rng(0)
    d, n, m = 2, 12, 5
    x, y, e = rng.uniform(size=(d, n)), rng.standard_normal(n), np.full(n, 0.1)
    q, l, th = rng.uniform(size=(d, m)), np.full(d, 0.5), np.array([0.5, 0.5, 1.0, 1.0])
    w = np.ones((1, m))
    bad = dict(kernel="matern12")
    calls = [
        lambda: GP_func.GP_kernel(x, y, e, q, l, "matern12"),
        lambda: GP_func.GP_cov(x, y, e, q, l, **bad),
        lambda: GP_func.GP_draws(x, y, e, q, l, 2, **bad),
        lambda: GP_func.GP_linear(x, y, e, q, l, w, **bad),
        lambda: GP_func.GP_conditioned(x, y, e, q, l, w, [0.0], [0.1], **bad),
        lambda: GP_func.GP_marginal(x, y, e, q, l[None, :], **bad),
        lambda: GP_func.GP_loo(x, y, e, l, **bad),
        lambda: GP_func.GP_hyper(x, y, e, q, th, **bad),
        lambda: GP_func.GP_mean(x, y, e, q, th, **bad),
        lambda: mle.fit_lml(x, y, e, verbose=False, **bad),
        lambda: loo.fit_loo(x, y, e, verbose=False, **bad),
        lambda: amplitude.fit_hyper(x, y, e, verbose=False, **bad),
        lambda: meanfn.fit_mean(x, y, e, verbose=False, **bad),
        lambda: loo.loo_predict(x, y, e, l, **bad),
        lambda: amplitude.predict_hyper(x, y, e, q, th, **bad),
        lambda: meanfn.predict_mean(x, y, e, q, th, **bad),
        lambda: linear.predict_linear(x, y, e, q, l, w, **bad),
        lambda: conditioned.predict_conditioned(x, y, e, q, l, w, [0.0], [0.1], **bad),
        lambda: posterior.sample_posterior(x, y, e, q, l, 2, **bad),
        lambda: posterior.sample_posterior(x, y, e, q, l, 2, method="device", **bad),
        lambda: hyper.sample_hyper(x, y, e, **bad),
        lambda: hyper.predict_marginal(x, y, e, q, ls=l[None, :], **bad),
        lambda: find_len_scales.len_scale_opt(x, y, e, False, **bad),
        lambda: find_len_scales.len_scale_opt(x, y, e, False, objective="marginal_likelihood", **bad),
        lambda: find_len_scales.len_scale_opt(x, y, e, False, objective="loo", **bad),
        lambda: swarm.particle_swarm(x, y, e, False, verbose=False, **bad),
    ]
    for i, call in enumerate(calls):
        with pytest.raises(ValueError, match="'se', 'matern32', 'matern52'"):
            call()
            pytest.fail(f"call {i} accepted kernel='matern12'")


def test_stand_in_context_is_squared_exponential_only():
    """A context without set_kernel (the host tests' stand-ins) serves "se" untouched and refuses the rest."""
    from gpfit._lib import use_kernel

    class Plain:
        pass

    class Recording:
        def __init__(self):
            self.seen = []

        def set_kernel(self, k):
            self.seen.append(k)

    use_kernel(Plain(), "se")
    with pytest.raises(ValueError, match="set_kernel"):
        use_kernel(Plain(), "matern52")
    r = Recording()
    for k in ALL:
        use_kernel(r, k)
    assert r.seen == list(ALL)   # "se" is set too: a shared context may hold another kernel
    with pytest.raises(ValueError, match="matern32"):
        use_kernel(r, "matern")
    assert r.seen == list(ALL)


def test_injected_evaluators_take_the_keyword():
    """fit_lml with a NumPy Matern evaluator: the keyword is accepted and no context is made."""
    from gpfit.mle import fit_lml
    rng = np.random.default_rng(1)
    x, e = rng.uniform(size=(1, 30)), np.full(30, 0.1)
    y = np.sin(6 * x[0]) + 0.1 * rng.standard_normal(30)

    def value_and_grad(positions):
        out = [lml_form(parts(x, y, e, p, "matern52")) for p in np.atleast_2d(positions)]
        return np.array([v for v, _ in out]), np.array([g for _, g in out])

    best, info = fit_lml(x, y, e, num_starts=6, num_polish=2, seed=0, value_and_grad=value_and_grad, verbose=False,
                         kernel="matern52")
    assert best.shape == (1,) and np.isfinite(info["lml"])
    assert info["lml"] >= max(info["starts"][1]) - 1e-9


def test_len_scale_opt_hands_the_kernel_on(monkeypatch):
    """Every objective receives kernel=, and a call without it makes exactly the calls made before."""
    import find_len_scales as fls
    import gpfit.loo
    import gpfit.mle
    seen = []

    def fake(name):
        def f(x, y, e, *a, **kw):
            seen.append((name, kw.get("kernel", "absent")))
            return np.ones(x.shape[0]), {}
        return f

    monkeypatch.setattr(gpfit.mle, "fit_lml", fake("lml"))
    monkeypatch.setattr(gpfit.loo, "fit_loo", fake("loo"))
    monkeypatch.setattr(fls, "particle_swarm", fake("swarm"))
    x, y, e = np.zeros((2, 4)), np.zeros(4), np.ones(4)
    for obj, name in (("calibration", "swarm"), ("marginal_likelihood", "lml"), ("loo", "loo")):
        for kernel, want in ((None, "absent"), ("se", "absent"), ("matern32", "matern32"), ("matern52", "matern52")):
            kw = {} if kernel is None else {"kernel": kernel}
            fls.len_scale_opt(x, y, e, False, objective=obj, **kw)
            assert seen[-1] == (name, want)


# ---------------------------------------------------------------------------------------------
# options.yaml
# ---------------------------------------------------------------------------------------------
def _options(tmp_path, text):
    p = tmp_path / "options.yaml"
    p.write_text(text)
    return str(p)


def test_options_yaml_kernel_key(tmp_path):
    import GP_fit
    assert GP_fit._kernel(_options(tmp_path, "resolution: [0.1]\n")) is None
    assert GP_fit._kernel(str(tmp_path / "missing.yaml")) is None
    for k in ALL:
        assert GP_fit._kernel(_options(tmp_path, f"kernel: {k}\n")) == k
    for bad in ("matern12", "rbf", "3", "[se]", "SE"):
        with pytest.raises(ValueError, match="se, matern32 or matern52"):
            GP_fit._kernel(_options(tmp_path, f"kernel: {bad}\n"))


@pytest.mark.parametrize("extra,fit,predict", [
    ("", "opt", "GP"),
    ("kernel: se\n", "opt", "GP_kernel"),
    ("kernel: matern52\n", "opt", "GP_kernel"),
    ("kernel: matern32\nlen_scale_objective: loo\n", "opt", "GP_kernel"),
    ("kernel: matern52\nhyper_samples: 4\nlen_scale_objective: marginal_likelihood\n", "opt", "marginal"),
    ("kernel: matern32\nlen_scale_objective: marginal_likelihood_full\n", "fit_hyper", "GP_hyper"),
    ("kernel: matern52\nlen_scale_objective: marginal_likelihood_full\nmean_function: linear\n", "fit_mean", "GP_mean"),
])
def test_options_yaml_kernel_reaches_fit_and_prediction(tmp_path, monkeypatch, extra, fit, predict):
    """The key combines with every objective, with hyper_samples and with mean_function: the fit and the
    prediction both receive it. Absent: the calls carry no kernel at all (the outputs of before)."""
    import GP_fit
    import gpfit.amplitude
    import gpfit.hyper
    import gpfit.meanfn
    import yaml
    want = (yaml.safe_load(extra) or {}).get("kernel", "absent")
    seen = {}

    def fitter(name, n_extra):
        def f(x, y, e, *a, **kw):
            seen["fit"] = (name, kw.get("kernel", "absent"))
            return np.ones(np.asarray(x).shape[0] + n_extra), {}
        return f

    def predictor(name, kernel_at=None):
        def f(xk, yk, ek, grid, ls, *a, **kw):
            k = a[kernel_at] if kernel_at is not None else kw.get("kernel", "absent")
            seen["predict"] = (name, k)
            return np.zeros(grid.shape[1]), np.ones(grid.shape[1])
        return f

    def marginal(x, y, e, x_fit, **kw):
        seen["predict"] = ("marginal", kw.get("kernel", "absent"))
        return np.zeros(x_fit.shape[1]), np.ones(x_fit.shape[1]), {}

    monkeypatch.setattr(GP_fit, "len_scale_opt", lambda x, y, e, progress, **kw: fitter("opt", 0)(x, y, e, **kw)[0])
    monkeypatch.setattr(gpfit.amplitude, "fit_hyper", fitter("fit_hyper", 2))
    monkeypatch.setattr(gpfit.meanfn, "fit_mean", fitter("fit_mean", 2))
    monkeypatch.setattr(GP_fit, "GP", predictor("GP"))
    monkeypatch.setattr(GP_fit, "GP_kernel", predictor("GP_kernel", kernel_at=0))
    monkeypatch.setattr(GP_fit, "GP_hyper", predictor("GP_hyper"))
    monkeypatch.setattr(GP_fit, "GP_mean", predictor("GP_mean"))
    monkeypatch.setattr(gpfit.hyper, "predict_marginal", marginal)
    monkeypatch.setattr(GP_fit, "read_yaml", lambda: ([0.1], False, str(tmp_path / "out.txt"), ["x", "q", "err"],
                                                      [("f.txt", [np.linspace(0, 1, 5)[None, :]],
                                                        [(np.zeros(5), np.ones(5))], ["x", "q", "err"])], False, False))
    monkeypatch.setattr(GP_fit, "fill_convex_hull", lambda pts, res: pts)
    monkeypatch.chdir(tmp_path)
    (tmp_path / "options.yaml").write_text("resolution: [0.1]\n" + extra)
    GP_fit.create_GP()
    assert seen["fit"] == (fit, want), seen
    assert seen["predict"] == (predict, want), seen
    # a bad value stops the run before anything is fitted
    seen.clear()
    (tmp_path / "options.yaml").write_text("resolution: [0.1]\nkernel: matern12\n")
    with pytest.raises(ValueError, match="se, matern32 or matern52"):
        GP_fit.create_GP()
    assert not seen


def test_c_entry_points_without_a_device():
    """gpf_set_kernel / gpf_get_kernel refuse a null context before anything else."""
    import ctypes
    import gpfit._lib as L
    lib = L.load_library()
    assert lib.gpf_set_kernel(None, 0) == L.GPF_BAD_ARG
    assert lib.gpf_set_kernel(None, 7) == L.GPF_BAD_ARG
    k = ctypes.c_int(5)
    assert lib.gpf_get_kernel(None, ctypes.byref(k)) == L.GPF_BAD_ARG and k.value == 5
