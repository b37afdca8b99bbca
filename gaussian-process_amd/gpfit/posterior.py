"""Joint posterior of a set of query points and draws from it.

``gpf_predict`` gives the marginal standard deviation of every query point; neighbouring points
of a dense grid are almost perfectly correlated, so anything that combines several of them (a sum
over a region, a later fit) needs the joint covariance
Sigma = K_ss - K_s^T Kn^-1 K_s (``Context.predict_cov``, gpf_predict_cov), or draws from
N(mu, Sigma):

  ``draws_from(mu, cov, ...)``        draws = mu + z L^T, L = cholesky(cov + jitter I) on the host;
  ``sample_posterior(x, y, e, ...)``  method="host": the device's (mu, cov) of the query points, then
                                      draws_from; method="device": Sigma, its factor and the product
                                      stay on the device (``Context.posterior_draws``).

Sigma is latent (noise-free) and its diagonal is not clipped: where query points coincide with
each other or with a noise-free training point it is singular up to rounding. The jitter starts
at 1e-12, the reference's own variance floor (GP_func.py:39), and is multiplied by 100 after every
failed factorisation up to 1e-6; a matrix that still fails is not a covariance and the
LinAlgError is raised. With method="host" the Cholesky factor of Sigma is taken by NumPy, which
costs a copy of the whole M x M matrix and an O(M^3) host factorisation; method="device" runs the
same ladder with the dense blocked factorisation of gpf_densechol.hip (gpf_posterior_draws) and
copies only the mean and the draws back. Both paths draw the same normals from a seed.

Model: fixed amplitude 1, fixed noise e^2, ARD squared-exponential, as GP_func.py.
"""
from __future__ import annotations

import numpy as np

from ._lib import JITTERS, check_jitters, default_context, use_kernel   # JITTERS: from GP_func.py:39's variance floor, x 100 per failure
from .kernels import kernel_kind

METHODS = ("host", "device")


def draws_from(mu, cov, n_draws=1, seed=None, z=None):
    """Draws from N(mu, cov): (draws (n_draws, M), info).

    draws = mu + z L^T with L = cholesky(cov + jitter I); ``z`` (n_draws, M) standard normals can be
    injected for reproducibility, otherwise they come from default_rng(seed). info: "jitter" (the
    value that factorised: 1e-12, 1e-10, 1e-8 or 1e-6) and "tries". LinAlgError if cov + 1e-6 I is
    still not positive definite.
    """
    mu = np.asarray(mu, dtype=np.float64).reshape(-1)
    cov = np.asarray(cov, dtype=np.float64)
    m = mu.shape[0]
    if cov.shape != (m, m):
        raise ValueError(f"cov must be ({m}, {m})")
    if z is None:
        z = np.random.default_rng(seed).standard_normal((int(n_draws), m))
    else:
        z = np.asarray(z, dtype=np.float64)
        if z.ndim != 2 or z.shape[1] != m:
            raise ValueError(f"z must be (n_draws, {m})")
    for tries, jitter in enumerate(JITTERS, 1):
        try:
            L = np.linalg.cholesky(cov + jitter * np.eye(m))
            break
        except np.linalg.LinAlgError:
            if jitter == JITTERS[-1]:
                raise
    return mu + z @ L.T, {"jitter": jitter, "tries": tries}


def sample_posterior(x_known, y_known, e_known, x_fit, lengths, n_draws, seed=None, ctx=None, mean_and_cov=None,
                     method="host", jitters=JITTERS, kernel="se"):
    """n_draws joint draws of the latent GP at x_fit (d, M): (draws (n_draws, M), info).

    method="host" (the default): ``mean_and_cov(x_fit, lengths) -> (mu (M,), cov (M, M))`` injects
    an evaluator (the CPU tests); the default is gpf_predict_cov on this process's GPU after
    set_data(x_known, y_known, e_known). info: draws_from's, plus "mu" and "cov".

    method="device": gpf_posterior_draws on this process's GPU; Sigma never reaches the host. The
    normals are default_rng(seed).standard_normal((n_draws, M)), exactly draws_from's, so a seed
    means the same normals on both paths. ``jitters`` is the ladder (ascending, >= 0). info: "mu",
    "jitter", "tries"; no "cov".

    ``kernel``: the covariance kernel, "se" (default), "matern32" or "matern52" (gpfit.kernels), set on the context on every call. An injected
    ``mean_and_cov`` brings its own.
    """
    kernel_kind(kernel)
    if method not in METHODS:
        raise ValueError(f"method must be one of {METHODS}, not {method!r}")
    x_fit = np.asarray(x_fit, dtype=np.float64)
    lengths = np.asarray(lengths, dtype=np.float64).reshape(-1)
    if method == "device":
        if mean_and_cov is not None:
            raise ValueError('mean_and_cov injects a host evaluator: use method="host"')
        jitters = check_jitters(jitters)
        x_known = np.asarray(x_known, dtype=np.float64)
        if x_fit.ndim != 2 or x_known.ndim != 2 or x_fit.shape[0] != x_known.shape[0]:
            raise ValueError("x_fit must be (d, M) with the same d as x_known")
        z = np.random.default_rng(seed).standard_normal((int(n_draws), x_fit.shape[1]))
        if ctx is None:
            ctx = default_context()
        ctx.set_data(x_known, y_known, e_known)
        use_kernel(ctx, kernel)
        mu, draws, info = ctx.posterior_draws(lengths, x_fit, z, jitters=jitters)
        info["mu"] = mu
        return draws, info
    if mean_and_cov is None:
        x_known = np.asarray(x_known, dtype=np.float64)
        if x_fit.ndim != 2 or x_fit.shape[0] != x_known.shape[0]:
            raise ValueError("x_fit must be (d, M) with the same d as x_known")
        if ctx is None:
            ctx = default_context()
        ctx.set_data(x_known, y_known, e_known)
        use_kernel(ctx, kernel)
        mu, cov = ctx.predict_cov(lengths, x_fit)
    else:
        mu, cov = mean_and_cov(x_fit, lengths)
    draws, info = draws_from(mu, cov, n_draws=n_draws, seed=seed)
    info["mu"], info["cov"] = mu, cov
    return draws, info
