"""gpfit.conditioned's host half (no GPU): conditioned_from against the closed form written out
independently (solve-based, no Cholesky factor), the augmentation identity (conditioning on one point
functional equals adding a training point), R = 0, the argument errors, a singular H, and
predict_conditioned's routes with a stand-in context object."""
import numpy as np
import pytest


def _posterior(m, seed=3):
    rng = np.random.default_rng(seed)
    g = rng.standard_normal((m, m))
    return rng.standard_normal(m), g @ g.T / m


def _kernel(a, b, l):
    """kernel_func (GP_func.py:49-65) in float64 NumPy."""
    a, b = a / l[:, None], b / l[:, None]
    r2 = (np.sum(a * a, axis=0)[:, None] + np.sum(b * b, axis=0)[None, :]) - 2.0 * (a.T @ b)
    return np.exp(-0.5 * np.maximum(r2, 0.0))


def _gp(x, y, e, q, l):
    """Latent joint posterior (mu, Sigma) at q of the GP with training data (x, y, e)."""
    kn = _kernel(x, x, l) + np.diag(e ** 2)
    ks = _kernel(x, q, l)
    kss = _kernel(q, q, l)
    np.fill_diagonal(kss, 1.0)
    return ks.T @ np.linalg.solve(kn, y), kss - ks.T @ np.linalg.solve(kn, ks)


def test_conditioned_from_against_solve_based_closed_form():
    from gpfit.conditioned import conditioned_from
    m, r = 11, 4
    mu, cov = _posterior(m)
    rng = np.random.default_rng(5)
    a = rng.uniform(-1.0, 1.0, (r, m))
    b, s = rng.standard_normal(r), np.array([0.1, 0.0, 0.3, 0.05])
    mu2, cov2, info = conditioned_from(mu, cov, a, b, s)
    h = a @ cov @ a.T + np.diag(s ** 2)
    c = cov @ a.T
    res = b - a @ mu
    want_mu = mu + c @ np.linalg.solve(h, res)
    want_cov = cov - c @ np.linalg.solve(h, c.T)
    want_chi2 = res @ np.linalg.solve(h, res)
    assert mu2.shape == (m,) and cov2.shape == (m, m)
    assert np.max(np.abs(mu2 - want_mu)) < 1e-12 * max(1.0, np.max(np.abs(want_mu)))
    assert np.max(np.abs(cov2 - want_cov)) < 1e-12 * np.max(np.abs(cov))
    assert abs(info["chi2"] - want_chi2) < 1e-12 * max(1.0, want_chi2)
    np.testing.assert_array_equal(info["fmean"], a @ mu)
    np.testing.assert_allclose(info["fcov"], a @ cov @ a.T, rtol=0, atol=1e-14)
    # the functional measured exactly (s = 0) is reproduced exactly, with no variance left
    assert abs(a[1] @ mu2 - b[1]) < 1e-12
    assert abs(a[1] @ cov2 @ a[1]) < 1e-12


def test_augmentation_identity():
    """A posterior on N = 40 points conditioned on the point functional (q_j, b, s) is the posterior on
    the N + 1 points: mean and full covariance at every query, to 1e-10."""
    from gpfit.conditioned import conditioned_from
    rng = np.random.default_rng(21)
    n, d, m, j = 40, 2, 25, 7
    x = rng.uniform(0.0, 1.0, (d, n))
    y = np.sin(3.0 * x[0]) + x[1] + 0.05 * rng.standard_normal(n)
    e = rng.uniform(0.03, 0.08, n)
    q = rng.uniform(-0.1, 1.1, (d, m))
    l = np.array([0.3, 0.45])
    bj, sj = 0.7, 0.1
    mu, cov = _gp(x, y, e, q, l)
    a = np.zeros((1, m))
    a[0, j] = 1.0
    mu2, cov2, _ = conditioned_from(mu, cov, a, [bj], [sj])
    mu_aug, cov_aug = _gp(np.hstack([x, q[:, j:j + 1]]), np.append(y, bj), np.append(e, sj), q, l)
    em, ec = np.max(np.abs(mu2 - mu_aug)), np.max(np.abs(cov2 - cov_aug))
    assert em < 1e-10, f"mean differs by {em:.3e}"
    assert ec < 1e-10, f"covariance differs by {ec:.3e}"
    assert np.max(np.abs(mu2 - mu)) > 1e-3  # the conditioning moved something


def test_no_functionals_returns_the_inputs():
    from gpfit.conditioned import conditioned_from
    mu, cov = _posterior(6)
    mu2, cov2, info = conditioned_from(mu, cov, np.empty((0, 6)), [], [])
    np.testing.assert_array_equal(mu2, mu)
    np.testing.assert_array_equal(cov2, cov)
    assert info["chi2"] == 0.0 and info["fmean"].shape == (0,) and info["fcov"].shape == (0, 0)


def test_argument_errors_and_singular_h():
    from gpfit.conditioned import conditioned_from
    m = 6
    mu, cov = _posterior(m)
    a = np.random.default_rng(6).uniform(-1.0, 1.0, (2, m))
    for args in ((a[:, :-1], [0.0, 1.0], [0.1, 0.1]),           # weights' shape
                 (a, [0.0, 1.0, 2.0], [0.1, 0.1]),              # values' shape
                 (a, [0.0, 1.0], [0.1]),                        # noise's shape
                 (a, [0.0, np.nan], [0.1, 0.1]),                # NaN value
                 (a, [0.0, 1.0], [0.1, np.inf]),                # non-finite noise
                 (a, [0.0, 1.0], [0.1, -0.1])):                 # negative noise
        with pytest.raises(ValueError):
            conditioned_from(mu, cov, *args)
    with pytest.raises(ValueError):
        conditioned_from(mu, cov[:, :-1], a, [0.0, 1.0], [0.1, 0.1])
    # two identical functionals measured exactly: H is singular, no jitter is added
    one = np.zeros((2, m))
    one[:, 2] = 1.0
    with pytest.raises(np.linalg.LinAlgError):
        conditioned_from(mu, cov, one, [0.3, 0.3], [0.0, 0.0])
    # with an error on one of them H is regular
    conditioned_from(mu, cov, one, [0.3, 0.3], [0.0, 0.1])


class _StandIn:
    """A context that records its calls and serves a fixed joint posterior."""

    def __init__(self, mu, cov):
        self.mu, self.cov, self.calls = mu, cov, []

    def set_data(self, x, y, e):
        self.calls.append("set_data")

    def predict_cov(self, lengths, x_fit):
        self.calls.append("predict_cov")
        return self.mu, self.cov

    def predict_conditioned(self, lengths, x_fit, weights, values, noise, chunk=0, want_functionals=False):
        self.calls.append(("predict_conditioned", chunk, want_functionals))
        return self.mu + 1.0, np.full(self.mu.shape, 0.5), {"chi2": 2.0, "fmean": None, "fcov": None}


def test_predict_conditioned_routes_and_argument_checks():
    from gpfit.conditioned import conditioned_from, predict_conditioned
    m, r, n, d = 9, 3, 5, 2
    mu, cov = _posterior(m, seed=8)
    rng = np.random.default_rng(9)
    a = rng.uniform(-1.0, 1.0, (r, m))
    b, s = rng.standard_normal(r), np.full(r, 0.2)
    x, y, e = rng.uniform(size=(d, n)), rng.standard_normal(n), np.full(n, 0.1)
    q, ls = rng.uniform(size=(d, m)), np.full(d, 0.3)
    c = _StandIn(mu, cov)
    mu2, sd2, info = predict_conditioned(x, y, e, q, ls, a, b, s, method="dense", ctx=c)
    want_mu, want_cov, want = conditioned_from(mu, cov, a, b, s)
    np.testing.assert_array_equal(mu2, want_mu)
    np.testing.assert_array_equal(sd2, np.sqrt(np.maximum(np.diag(want_cov), 1e-12)))
    assert info["method"] == "dense" and info["chi2"] == want["chi2"] and c.calls == ["set_data", "predict_cov"]
    # R = 0 on the dense route: the plain prediction
    mu0, sd0, info0 = predict_conditioned(x, y, e, q, ls, np.empty((0, m)), [], [], method="dense", ctx=_StandIn(mu, cov))
    np.testing.assert_array_equal(mu0, mu)
    np.testing.assert_array_equal(sd0, np.sqrt(np.maximum(np.diag(cov), 1e-12)))
    # the stream route hands everything to the context's entry point
    c = _StandIn(mu, cov)
    mu2, sd2, info = predict_conditioned(x, y, e, q, ls, a, b, s, method="stream", chunk=256, ctx=c)
    assert info["method"] == "stream" and info["chi2"] == 2.0
    assert c.calls == ["set_data", ("predict_conditioned", 256, True)]
    np.testing.assert_array_equal(mu2, mu + 1.0)
    # bad arguments raise before the context is touched
    c = _StandIn(mu, cov)
    bad = a.copy()
    bad[1, 2] = np.nan
    nanb = b.copy()
    nanb[0] = np.nan
    for kw in (dict(weights=a[:, :-1]), dict(weights=a[0]), dict(weights=bad), dict(method="sparse"), dict(chunk=-1),
               dict(x_fit=q[:1]), dict(values=b[:-1]), dict(values=nanb), dict(noise=-s), dict(noise=s[:-1]),
               dict(noise=np.full(r, np.inf))):
        args = dict(x_fit=q, weights=a, values=b, noise=s, method="dense")
        args.update(kw)
        with pytest.raises(ValueError):
            predict_conditioned(x, y, e, args.pop("x_fit"), ls, args.pop("weights"), args.pop("values"), args.pop("noise"),
                                ctx=c, **args)
    assert c.calls == []


def test_gp_func_exposes_gp_conditioned():
    import GP_func
    assert callable(GP_func.GP_conditioned)
