"""gpfit.posterior (draws from the joint posterior, host side) and gpf_predict_cov's argument check:
no GPU. The covariances come from the float64 NumPy closed form of Sigma = K_ss - K_s^T Kn^-1 K_s."""
import numpy as np
import pytest


def _kernel(a, b, l):
    a, b = a / l[:, None], b / l[:, None]
    r2 = (np.sum(a * a, axis=0)[:, None] + np.sum(b * b, axis=0)[None, :]) - 2.0 * (a.T @ b)
    return np.exp(-0.5 * np.maximum(r2, 0.0))


def _closed_form(N, d, M, seed=0, dup=False, scale=0.3):
    """(mu, Sigma, (x, y, e, q, l)) of a GP on N points at M queries in the unit cube, l = scale in
    every coordinate; dup: the last query repeats the one before it."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(size=(d, N))
    y = np.sin(3 * x[0]) + 0.1 * rng.standard_normal(N)
    e = rng.uniform(0.05, 0.2, size=N)
    l = np.full(d, scale)
    q = rng.uniform(size=(d, M))
    if dup:
        q[:, -1] = q[:, -2]
    Kn = _kernel(x, x, l) + np.diag(e ** 2)
    Ks = _kernel(x, q, l)
    v = np.linalg.solve(np.linalg.cholesky(Kn), Ks)
    Kss = _kernel(q, q, l)
    np.fill_diagonal(Kss, 1.0)
    cov = Kss - v.T @ v
    cov = np.tril(cov) + np.tril(cov, -1).T  # exactly symmetric, as gpf_predict_cov returns it
    return Ks.T @ np.linalg.solve(Kn, y), cov, (x, y, e, q, l)


def test_null_context_is_bad_arg_without_a_device():
    import gpfit._lib as L
    lib = L.load_library()
    assert lib.gpf_predict_cov(None, None, None, 0, None, None) == L.GPF_BAD_ARG
    assert lib.gpf_predict_cov(None, None, None, 5, None, None) == L.GPF_BAD_ARG


def test_draws_from_well_conditioned():
    from gpfit.posterior import draws_from
    mu, cov, _ = _closed_form(40, 2, 50, scale=0.08)
    assert np.linalg.eigvalsh(cov)[0] > 1e-6
    draws, info = draws_from(mu, cov, z=np.eye(50))
    assert info["jitter"] == 1e-12 and draws.shape == (50, 50)
    Lc = np.linalg.cholesky(cov + 1e-12 * np.eye(50))
    np.testing.assert_allclose(draws - mu, Lc.T, rtol=0, atol=1e-15)
    a, ia = draws_from(mu, cov, n_draws=4, seed=3)
    b, _ = draws_from(mu, cov, n_draws=4, seed=3)
    assert a.shape == (4, 50) and ia["jitter"] == 1e-12
    np.testing.assert_array_equal(a, b)
    assert not np.array_equal(a, draws_from(mu, cov, n_draws=4, seed=4)[0])
    np.testing.assert_array_equal(a, draws_from(mu, cov, z=np.random.default_rng(3).standard_normal((4, 50)))[0])
    with pytest.raises(ValueError):
        draws_from(mu, cov[:, :-1])
    with pytest.raises(ValueError):
        draws_from(mu, cov, z=np.zeros((2, 49)))


def test_draws_from_singular_needs_a_larger_jitter():
    """A duplicated query column makes Sigma exactly singular (two identical rows); minus 1e-11 I it
    cannot factorise at the first jitter of 1e-12."""
    from gpfit.posterior import draws_from
    mu, cov, _ = _closed_form(40, 2, 30, seed=1, dup=True)
    np.testing.assert_array_equal(cov[-1, :-2], cov[-2, :-2])
    cov[-1, -1] = cov[-2, -2]
    cov[-1, -2] = cov[-2, -1] = cov[-2, -2]  # rows -1 and -2 identical: exactly singular
    np.testing.assert_array_equal(cov[-1], cov[-2])
    cov = cov - 1e-11 * np.eye(30)
    with pytest.raises(np.linalg.LinAlgError):
        np.linalg.cholesky(cov + 1e-12 * np.eye(30))
    z = np.random.default_rng(2).standard_normal((5, 30))
    draws, info = draws_from(mu, cov, z=z)
    assert 1e-12 < info["jitter"] <= 1e-8 and info["tries"] >= 2
    gap = np.max(np.abs(draws[:, -1] - draws[:, -2]))
    bound = 10 * np.sqrt(info["jitter"]) * np.max(np.abs(z))
    print(f"[posterior] singular Sigma: jitter {info['jitter']:.0e}, duplicate coordinates differ by {gap:.3e} (bound {bound:.3e})")
    assert gap < bound


def test_draws_from_rejects_an_indefinite_matrix():
    from gpfit.posterior import draws_from
    _, cov, _ = _closed_form(40, 2, 12, seed=2)
    w, Q = np.linalg.eigh(cov)
    w[0] = -1e-3
    bad = (Q * w) @ Q.T
    bad = 0.5 * (bad + bad.T)
    assert np.linalg.eigvalsh(bad)[0] < -0.9e-3
    with pytest.raises(np.linalg.LinAlgError):
        draws_from(np.zeros(12), bad, n_draws=2, seed=0)


def test_sample_covariance_of_draws():
    """20,000 seeded draws at M = 8: every entry of the sample covariance within 5 sqrt(2 / n) of
    Sigma. For Gaussian draws var(S_ij) = (Sigma_ii Sigma_jj + Sigma_ij^2) / (n - 1) <= 2 / (n - 1)
    with Sigma's entries at most 1, so the bound is five standard deviations; deterministic under
    the seed."""
    from gpfit.posterior import draws_from
    n = 20000
    mu, cov, _ = _closed_form(30, 2, 8, seed=5)
    draws, info = draws_from(mu, cov, n_draws=n, seed=123)
    assert draws.shape == (n, 8) and info["jitter"] == 1e-12
    err = np.max(np.abs(np.cov(draws, rowvar=False) - cov))
    em = np.max(np.abs(draws.mean(axis=0) - mu))
    print(f"[posterior] sample covariance error {err:.3e} (bound {5 * np.sqrt(2 / n):.3e}), mean error {em:.3e}")
    assert err < 5 * np.sqrt(2 / n)
    assert em < 5 * np.sqrt(1 / n)


def test_sample_posterior_with_injected_evaluator_opens_no_context(monkeypatch):
    import gpfit.posterior as P
    mu, cov, (x, y, e, q, l) = _closed_form(30, 2, 10, seed=6)
    calls = []

    def boom(*a, **k):
        raise AssertionError("sample_posterior opened a device context")

    def mean_and_cov(x_fit, lengths):
        calls.append((x_fit.shape, tuple(lengths)))
        return mu, cov

    monkeypatch.setattr(P, "default_context", boom)
    draws, info = P.sample_posterior(x, y, e, q, l, 6, seed=9, mean_and_cov=mean_and_cov)
    assert calls == [((2, 10), (0.3, 0.3))]
    assert draws.shape == (6, 10) and info["jitter"] == 1e-12
    np.testing.assert_array_equal(draws, P.draws_from(mu, cov, n_draws=6, seed=9)[0])
    assert info["mu"] is mu and info["cov"] is cov
