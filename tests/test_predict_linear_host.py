"""gpfit.linear's host half (no GPU): functionals_from against explicit loops, region_weights, and
predict_linear(method="dense") with a stand-in context object."""
import numpy as np
import pytest


def _posterior(m, seed=3):
    rng = np.random.default_rng(seed)
    g = rng.standard_normal((m, m))
    return rng.standard_normal(m), g @ g.T / m


def test_functionals_from_against_loops():
    from gpfit.linear import functionals_from
    m, r = 7, 3
    mu, cov = _posterior(m)
    a = np.random.default_rng(4).uniform(-1.0, 1.0, (r, m))
    mean, c = functionals_from(mu, cov, a)
    assert mean.shape == (r,) and c.shape == (r, r)
    for i in range(r):
        want = sum(a[i, q] * mu[q] for q in range(m))
        assert abs(mean[i] - want) < 1e-14 * max(1.0, abs(want))
        for j in range(r):
            want = sum(a[i, p] * cov[p, q] * a[j, q] for p in range(m) for q in range(m))
            assert abs(c[i, j] - want) < 1e-13 * max(1.0, abs(want))
    # identity weights give the posterior back
    mean, c = functionals_from(mu, cov, np.eye(m))
    np.testing.assert_array_equal(mean, mu)
    np.testing.assert_allclose(c, cov, rtol=0, atol=1e-15)
    with pytest.raises(ValueError):
        functionals_from(mu, cov, np.ones((2, m + 1)))
    with pytest.raises(ValueError):
        functionals_from(mu, cov[:, :-1], np.ones((2, m)))


def test_region_weights():
    from gpfit.linear import region_weights
    # a 4 x 3 grid on [0, 3] x [0, 2]
    gx, gy = np.meshgrid(np.arange(4.0), np.arange(3.0), indexing="ij")
    x = np.stack([gx.ravel(), gy.ravel()])
    boxes = [[(0.0, 3.0), (0.0, 2.0)],      # everything
             [(0.5, 2.5), (-1.0, 0.5)],     # x in {1, 2}, y = 0
             [(1.0, 1.0), (0.0, 2.0)]]      # a degenerate box: the points on its edge belong to it
    w = region_weights(x, boxes)
    assert w.shape == (3, 12)
    np.testing.assert_allclose(w.sum(axis=1), 1.0, rtol=0, atol=1e-15)
    np.testing.assert_array_equal(w[0], np.full(12, 1.0 / 12))
    np.testing.assert_array_equal(np.flatnonzero(w[1]), [3, 6])
    np.testing.assert_array_equal(np.flatnonzero(w[2]), [3, 4, 5])
    s = region_weights(x, boxes, kind="sum")
    np.testing.assert_array_equal(s.sum(axis=1), [12.0, 2.0, 3.0])
    np.testing.assert_array_equal(s != 0, w != 0)
    # a point exactly on a box edge is inside; just outside it is not
    assert region_weights(x, [[(2.0, 3.0), (2.0, 2.0)]], kind="sum").sum() == 2.0
    assert region_weights(x, [[(np.nextafter(2.0, 3.0), 3.0), (2.0, 2.0)]], kind="sum").sum() == 1.0
    with pytest.raises(ValueError, match="region 1"):
        region_weights(x, [boxes[0], [(0.2, 0.8), (0.2, 0.8)]])
    with pytest.raises(ValueError, match="kind"):
        region_weights(x, boxes, kind="median")
    with pytest.raises(ValueError, match="region 0"):
        region_weights(x, [[(0.0, 1.0)]])


class _StandIn:
    """A context that records its calls and serves a fixed joint posterior."""

    def __init__(self, mu, cov):
        self.mu, self.cov, self.calls = mu, cov, []

    def set_data(self, x, y, e):
        self.calls.append("set_data")

    def predict_cov(self, lengths, x_fit):
        self.calls.append("predict_cov")
        return self.mu, self.cov

    def predict_linear(self, lengths, x_fit, weights, chunk=0, want_prior=False):
        self.calls.append(("predict_linear", chunk, want_prior))
        a = np.asarray(weights)
        return a @ self.mu, a @ self.cov @ a.T, a @ a.T


def test_predict_linear_dense_route_and_argument_checks():
    from gpfit.linear import predict_linear
    m, r, n, d = 9, 4, 5, 2
    mu, cov = _posterior(m, seed=8)
    rng = np.random.default_rng(9)
    a = rng.uniform(-1.0, 1.0, (r, m))
    x, y, e = rng.uniform(size=(d, n)), rng.standard_normal(n), np.full(n, 0.1)
    q, ls = rng.uniform(size=(d, m)), np.full(d, 0.3)
    c = _StandIn(mu, cov)
    mean, cv, info = predict_linear(x, y, e, q, ls, a, method="dense", ctx=c)
    np.testing.assert_array_equal(mean, a @ mu)
    np.testing.assert_array_equal(cv, a @ cov @ a.T)
    assert info["method"] == "dense" and c.calls == ["set_data", "predict_cov"]
    # the stream route hands the weights and the chunk to the context's entry point
    c = _StandIn(mu, cov)
    mean, cv, info = predict_linear(x, y, e, q, ls, a, method="stream", chunk=256, ctx=c)
    assert info["method"] == "stream" and c.calls == ["set_data", ("predict_linear", 256, True)]
    np.testing.assert_array_equal(mean, a @ mu)
    np.testing.assert_array_equal(info["prior"], a @ a.T)
    # bad arguments raise before the context is touched
    c = _StandIn(mu, cov)
    bad = a.copy()
    bad[1, 2] = np.nan
    for kw in (dict(weights=a[:, :-1]), dict(weights=a[0]), dict(weights=bad), dict(weights=a, method="sparse"),
               dict(weights=a, chunk=-1), dict(weights=a, x_fit=q[:1])):
        args = dict(x_fit=q, method="dense")
        args.update(kw)
        with pytest.raises(ValueError):
            predict_linear(x, y, e, args.pop("x_fit"), ls, args.pop("weights"), ctx=c, **args)
    assert c.calls == []


def test_gp_func_exposes_gp_linear():
    import GP_func
    assert callable(GP_func.GP_linear)
