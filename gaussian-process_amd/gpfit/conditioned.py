"""The GP posterior conditioned on measured linear functionals of the latent function: an integrated
value, averages in another experiment's bins, any fixed weights A (R, M) over the M query points, each
measured as values[r] = sum_q A[r, q] f(x_q) + N(0, noise[r]^2) with independent errors.

  ``conditioned_from(mu, cov, weights, values, noise)``  pure NumPy: the conditioned joint posterior
                                          (mu', cov', info) from a joint posterior; the host half of
                                          the dense route and the yardstick of the other
  ``predict_conditioned(x, y, e, ...)``   method="stream": gpf_predict_conditioned, streamed over the
                                          query axis on the device, no M x M matrix anywhere;
                                          method="dense": gpf_predict_cov's (mu, cov), then
                                          conditioned_from (M is capped by the dense covariance)

With H = A cov A^T + diag(noise^2) and C = cov A^T:
    mu' = mu + C H^-1 (b - A mu),   cov' = cov - C H^-1 C^T,   chi2 = (b - A mu)^T H^-1 (b - A mu).
chi2 measures the agreement of the measurements with the fit before conditioning (about R is
expected). Conditioning on one point functional (x_q, b, s) equals adding the training point
(x_q, b, s). ``gpfit.linear.region_weights`` builds the weights of bins.
"""
from __future__ import annotations

import numpy as np

from ._lib import default_context, use_kernel
from .kernels import kernel_kind
from .linear import check_weights

METHODS = ("stream", "dense")


def check_measurements(values, noise, r):
    """(values, noise) as float64 (r,) arrays; ValueError for another shape, a non-finite value or a
    noise that is negative or not finite (checked before the library is touched)."""
    b = np.ascontiguousarray(values, dtype=np.float64).reshape(-1)
    s = np.ascontiguousarray(noise, dtype=np.float64).reshape(-1)
    if b.shape != (r,) or s.shape != (r,):
        raise ValueError(f"values and noise must be ({r},), not {b.shape} and {s.shape}")
    if not np.all(np.isfinite(b)):
        raise ValueError("values must be finite")
    if not np.all(np.isfinite(s)) or np.any(s < 0.0):
        raise ValueError("noise must be finite and >= 0")
    return b, s


def conditioned_from(mu, cov, weights, values, noise):
    """(mu' (M,), cov' (M, M), info) for the joint posterior (mu (M,), cov (M, M)) conditioned on
    values = A f + N(0, diag(noise^2)), A = weights (R, M). info: "chi2", "fmean" = A mu and "fcov" =
    A cov A^T (before conditioning). H = fcov + diag(noise^2) is factorised without jitter: a singular
    H (redundant functionals with zero noise) raises LinAlgError. R = 0 returns the inputs."""
    mu, cov = np.asarray(mu, dtype=np.float64), np.asarray(cov, dtype=np.float64)
    if mu.ndim != 1 or cov.shape != (mu.shape[0], mu.shape[0]):
        raise ValueError("mu must be (M,) and cov (M, M)")
    a = check_weights(weights, mu.shape[0])
    b, s = check_measurements(values, noise, a.shape[0])
    fmean, c = a @ mu, cov @ a.T
    fcov = a @ c
    if a.shape[0] == 0:
        return mu, cov, {"chi2": 0.0, "fmean": fmean, "fcov": fcov}
    lh = np.linalg.cholesky(fcov + np.diag(s * s))
    e = np.linalg.solve(lh, c.T).T      # C Lh^-T
    g = np.linalg.solve(lh, b - fmean)
    return mu + e @ g, cov - e @ e.T, {"chi2": float(g @ g), "fmean": fmean, "fcov": fcov}


def predict_conditioned(x_known, y_known, e_known, x_fit, lengths, weights, values, noise, method="stream", chunk=0,
                        ctx=None, kernel="se"):
    """The latent GP at x_fit (d, M) conditioned on the training data and on the measured functionals:
    (mu' (M,), sd' (M,), info), sd' = sqrt(clip(var', 1e-12)) as GP()'s. info: "chi2", "fmean", "fcov"
    (the functionals before conditioning) and "method".

    method="stream" (the default): gpf_predict_conditioned on this process's GPU, ``chunk`` query
    points per pass (0: the library's default). method="dense": predict_cov's (mu, Sigma) copied back,
    then conditioned_from. With R = 0 the plain prediction. ``ctx``: the context to use (default: this
    process's). ``kernel``: the covariance kernel, "se" (default), "matern32" or "matern52" (gpfit.kernels), set on the context on every call."""
    kernel_kind(kernel)
    if method not in METHODS:
        raise ValueError(f"method must be one of {METHODS}, not {method!r}")
    x_known = np.asarray(x_known, dtype=np.float64)
    x_fit = np.asarray(x_fit, dtype=np.float64)
    lengths = np.asarray(lengths, dtype=np.float64).reshape(-1)
    if x_fit.ndim != 2 or x_known.ndim != 2 or x_fit.shape[0] != x_known.shape[0]:
        raise ValueError("x_fit must be (d, M) with the same d as x_known")
    w = check_weights(weights, x_fit.shape[1])
    b, s = check_measurements(values, noise, w.shape[0])
    if int(chunk) < 0:
        raise ValueError("chunk must be >= 0")
    if ctx is None:
        ctx = default_context()
    ctx.set_data(x_known, y_known, e_known)
    use_kernel(ctx, kernel)
    if method == "dense":
        mu, cov, info = conditioned_from(*ctx.predict_cov(lengths, x_fit), w, b, s)
        return mu, np.sqrt(np.maximum(np.diag(cov), 1e-12)), dict(info, method=method)
    mu, sd, info = ctx.predict_conditioned(lengths, x_fit, w, b, s, chunk=int(chunk), want_functionals=True)
    return mu, sd, dict(info, method=method)
