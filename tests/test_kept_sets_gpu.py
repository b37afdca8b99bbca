"""The kept buffer sets of the posterior entry points are independent of each other:
every entry point on one context, interleaved at two widths and across a regrow of the factorisation
workspace, returns the same bits for the same call."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, D, R, S, P = 200, 2, 3, 5, 3  # two row tiles, the last one ragged


def _basis(x):
    """The constant + linear basis at the points x (d, m): the rows 1, x_1 .. x_d."""
    return np.vstack([np.ones(x.shape[1]), x])


def _inputs(rng, m):
    """One call's arguments for each of the nine entry points at width m (query points, rows of the
    probability surface and the dense matrix's order alike)."""
    b = rng.standard_normal((m, m))
    tails = np.empty((m, 4 if m < 200 else 8))
    tails[:, 0::2] = rng.normal(size=(m, tails.shape[1] // 2))
    tails[:, 1::2] = rng.uniform(0.05, 0.5, size=(m, tails.shape[1] // 2))
    return {
        "xf": rng.uniform(size=(D, m)),
        "w": rng.standard_normal((R, m)) / m,
        "b": rng.standard_normal(R),
        "s": rng.uniform(0.05, 0.2, size=R),
        "z": rng.standard_normal((S, m)),
        "a": b @ b.T / m + np.eye(m),
        "tails": tails,
    }


def _calls(ctx, ls, lsP, a):
    """name -> () -> tuple of the call's output arrays (the wrappers raise unless the call returns GPF_OK)."""
    def draws():
        mu, dr, info = ctx.posterior_draws(ls, a["xf"], a["z"], want_chol=True)
        return mu, dr, info["chol"], np.array([info["jitter"], info["tries"]])

    def conditioned():
        mu, sd, info = ctx.predict_conditioned(ls, a["xf"], a["w"], a["b"], a["s"], want_functionals=True)
        return mu, sd, info["fmean"], info["fcov"], np.array(info["chi2"])

    def batch():
        mu, sd, info = ctx.predict_batch(lsP, a["xf"], want_each=True)
        return mu, sd, info["mu"], info["sd"]

    def dense():
        L, info = ctx.chol_dense(a["a"])
        return L, np.array([info["jitter"], info["tries"]])

    def psurf():
        y, p, ok = ctx.prob_surface(a["tails"])
        return ok, y[ok], p[ok]  # (skipped rows' y and p are not written)

    return {
        "predict": lambda: ctx.predict(ls, a["xf"]),
        "predict_cov": lambda: ctx.predict_cov(ls, a["xf"]),
        "posterior_draws": draws,
        "predict_linear": lambda: ctx.predict_linear(ls, a["xf"], a["w"], want_prior=True),
        "predict_conditioned": conditioned,
        "predict_batch": batch,
        "predict_mean": lambda: ctx.predict_mean(ls, a["xf"], _basis(a["xf"]), want_beta=True),
        "chol_dense": dense,
        "prob_surface": psurf,
    }


@pytest.mark.parametrize("keep_mb", [None, "0"])
def test_kept_sets_are_independent(monkeypatch, keep_mb):
    """All nine entry points at M = 130 (the first values), at M = 300 in another order, at M = 130
    again, after set_data with N = 300 (the workspace regrows and releases every set) and back on the
    first data at M = 130 once more: every M = 130 output is bitwise its first value, with the sets kept
    (GPF_PREDICT_KEEP_MB unset) and given back after every call (= 0)."""
    import gpfit
    if keep_mb is None:
        monkeypatch.delenv("GPF_PREDICT_KEEP_MB", raising=False)
    else:
        monkeypatch.setenv("GPF_PREDICT_KEEP_MB", keep_mb)
    rng = np.random.default_rng(23)

    def data(n):
        x = rng.uniform(size=(D, n))
        return x, np.sin(4 * x[0]) + np.cos(3 * x[1]) + 0.1 * rng.standard_normal(n), rng.uniform(0.05, 0.2, size=n)

    first, other = data(N), data(300)
    ls, lsP = rng.uniform(0.2, 0.5, size=D), rng.uniform(0.2, 0.5, size=(P, D))
    ctx = gpfit.Context(0)
    try:
        ctx.set_data(*first)
        ctx.set_basis(_basis(first[0]))
        small, wide = _calls(ctx, ls, lsP, _inputs(rng, 130)), _calls(ctx, ls, lsP, _inputs(rng, 300))
        names = list(small)
        want = {k: small[k]() for k in names}

        def check(order, when):
            for k in order:
                for i, (got, ref) in enumerate(zip(small[k](), want[k])):
                    np.testing.assert_array_equal(got, ref, err_msg=f"{k} output {i} {when}")

        for k in names[::-1]:
            wide[k]()
        check(names[3:] + names[:3], "after the wider calls")
        ctx.set_data(*other)
        ctx.predict(ls, other[0][:, :130])  # ensure_work regrows the workspace for the new N
        ctx.set_data(*first)
        ctx.set_basis(_basis(first[0]))  # (set_data with other data discarded it)
        check(names[::2] + names[1::2], "after other training data")
    finally:
        ctx.close()
