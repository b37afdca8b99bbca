"""Linear functionals of the GP posterior at a set of query points: sums and averages over regions,
differences, any fixed weights A (R, M) over the M points.

  ``functionals_from(mu, cov, weights)``  pure NumPy: (A mu, A cov A^T) from a joint posterior; the
                                          host half of the dense route and the yardstick of the other
  ``region_weights(x_fit, regions)``      one row of weights per axis-aligned box over the query points
  ``predict_linear(x, y, e, ...)``        method="stream": gpf_predict_linear, the query axis folded away
                                          on the device chunk by chunk, no M x M matrix anywhere;
                                          method="dense": gpf_predict_cov's (mu, cov), then
                                          functionals_from (M is capped by the dense covariance)

Neighbouring query points are almost perfectly correlated, so the error of a sum over a region is not
the root sum of squares of the marginal errors: it needs the joint covariance, which the functionals
carry as their own R x R covariance.
"""
from __future__ import annotations

import numpy as np

from ._lib import default_context, use_kernel
from .kernels import kernel_kind

METHODS = ("stream", "dense")
KINDS = ("mean", "sum")


def check_weights(weights, m):
    """The weights as a C-contiguous float64 (R, m) array; ValueError for another shape or a
    non-finite entry (checked before the library is touched)."""
    w = np.ascontiguousarray(weights, dtype=np.float64)
    if w.ndim != 2 or w.shape[1] != m:
        raise ValueError(f"weights must be (R, {m}), not {w.shape}")
    if not np.all(np.isfinite(w)):
        raise ValueError("weights must be finite")
    return w


def functionals_from(mu, cov, weights):
    """(A mu (R,), A cov A^T (R, R)) for the joint posterior (mu (M,), cov (M, M)) and A = weights (R, M)."""
    mu, cov = np.asarray(mu, dtype=np.float64), np.asarray(cov, dtype=np.float64)
    if mu.ndim != 1 or cov.shape != (mu.shape[0], mu.shape[0]):
        raise ValueError("mu must be (M,) and cov (M, M)")
    a = check_weights(weights, mu.shape[0])
    return a @ mu, a @ cov @ a.T


def region_weights(x_fit, regions, kind="mean"):
    """Weights (len(regions), M) of axis-aligned boxes over the query points x_fit (d, M): regions is a
    sequence of boxes, a box a sequence of d pairs (lo, hi), and a point belongs to a box when
    lo <= x <= hi on every axis (the edges included). kind="mean": every member weighs 1 / count, so a
    row sums to 1 (the average over the region); kind="sum": every member weighs 1. A box without
    points is a ValueError that names its index."""
    if kind not in KINDS:
        raise ValueError(f"kind must be one of {KINDS}, not {kind!r}")
    x = np.asarray(x_fit, dtype=np.float64)
    if x.ndim != 2:
        raise ValueError("x_fit must be (d, M)")
    d, m = x.shape
    w = np.zeros((len(regions), m))
    for i, box in enumerate(regions):
        b = np.asarray(box, dtype=np.float64)
        if b.shape != (d, 2):
            raise ValueError(f"region {i} must be {d} pairs (lo, hi)")
        inside = np.all((x >= b[:, :1]) & (x <= b[:, 1:]), axis=0)
        n = int(np.count_nonzero(inside))
        if n == 0:
            raise ValueError(f"region {i} contains no query point")
        w[i, inside] = 1.0 / n if kind == "mean" else 1.0
    return w


def predict_linear(x_known, y_known, e_known, x_fit, lengths, weights, method="stream", chunk=0, ctx=None, kernel="se"):
    """The functionals A f of the latent GP f at x_fit (d, M), A = weights (R, M):
    (mean (R,), cov (R, R), info) with mean = A mu and cov = A Sigma A^T.

    method="stream" (the default): gpf_predict_linear on this process's GPU, ``chunk`` query points per
    pass (0: the library's default); info also carries "prior" = A K_ss A^T, the functionals' prior
    covariance. method="dense": predict_cov's (mu, Sigma) copied back, then functionals_from.
    info["method"] reports the method. ``ctx``: the context to use (default: this process's).
    ``kernel``: the covariance kernel, "se" (default), "matern32" or "matern52" (gpfit.kernels), set on the context on every call."""
    kernel_kind(kernel)
    if method not in METHODS:
        raise ValueError(f"method must be one of {METHODS}, not {method!r}")
    x_known = np.asarray(x_known, dtype=np.float64)
    x_fit = np.asarray(x_fit, dtype=np.float64)
    lengths = np.asarray(lengths, dtype=np.float64).reshape(-1)
    if x_fit.ndim != 2 or x_known.ndim != 2 or x_fit.shape[0] != x_known.shape[0]:
        raise ValueError("x_fit must be (d, M) with the same d as x_known")
    w = check_weights(weights, x_fit.shape[1])
    if int(chunk) < 0:
        raise ValueError("chunk must be >= 0")
    if ctx is None:
        ctx = default_context()
    ctx.set_data(x_known, y_known, e_known)
    use_kernel(ctx, kernel)
    if method == "dense":
        mean, cov = functionals_from(*ctx.predict_cov(lengths, x_fit), w)
        return mean, cov, {"method": method}
    mean, cov, prior = ctx.predict_linear(lengths, x_fit, w, chunk=int(chunk), want_prior=True)
    return mean, cov, {"method": method, "prior": prior}
