"""Prediction with the length scales marginalised instead of fixed at the fit's optimum.

Every fit here ends with one length-scale vector, although the marginal likelihood in l is broad at
the reference's 100 fit points; the sd of a prediction at that one vector is therefore too small.
The standard remedy predicts at K samples of the length scales and combines the K predictions as a
mixture (law of total variance):

    mix_mu = sum_k w_k mu_k,   mix_sd^2 = sum_k w_k (sd_k^2 + (mu_k - mix_mu)^2).

  ``mixture_from(mu, sd, weights)``  pure NumPy, two-pass: the yardstick of the device mixture
  ``sample_hyper(x, y, e, ...)``     K length-scale samples and their importance weights from a
                                     Laplace proposal around the maximum-marginal-likelihood fit
  ``predict_marginal(x, y, e, ...)`` method="batch": gpf_predict_batch (one batched factorisation, the
                                     mixture reduced on the device); method="loop": K predict() calls
                                     and mixture_from — the yardstick route

Prior: flat in t = log l on the fit's search box (``gpfit.mle``: the reference's box with the lower
bound raised to 1e-3 of the upper), so the posterior of t on the box is proportional to exp(LML(t)).
Model: fixed amplitude 1, fixed noise e^2, ARD squared-exponential, as GP_func.py; only the length
scales are marginalised.
"""
from __future__ import annotations

import numpy as np

from ._lib import default_comm, default_context, use_kernel
from .kernels import kernel_kind
from .mle import LOWER_FRACTION, _call, _device_evaluator, fit_lml
from .swarm import MAX_POINTS, prepare, share_seed

METHODS = ("batch", "loop")
HESSIAN_STEP = 1e-4     # central-difference step in t = log l
MAX_REDRAWS = 1000      # rounds of redrawing the proposals that fell outside the box


def check_mixture_weights(weights, p):
    """The weights as a float64 (p,) array normalised to sum 1 (None: equal); ValueError for another
    shape, a weight that is negative or not finite, or a zero sum."""
    if weights is None:
        if p == 0:
            raise ValueError("a mixture needs at least one component")
        return np.full(p, 1.0 / p)
    w = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
    if w.shape != (p,):
        raise ValueError(f"weights must be ({p},), not {w.shape}")
    if not np.all(np.isfinite(w)) or np.any(w < 0.0):
        raise ValueError("weights must be finite and >= 0")
    s = float(np.sum(w))
    if not s > 0.0:
        raise ValueError("the weights must not sum to 0")
    return w / s


def mixture_from(mu_PM, sd_PM, weights=None):
    """(mix_mu (M,), mix_sd (M,)) of the mixture of P Gaussians N(mu_PM[p], sd_PM[p]^2) per column with
    the weights (P,) (None: equal; normalised to sum 1), in two passes: the mean first, then the
    variance about it."""
    mu = np.asarray(mu_PM, dtype=np.float64)
    sd = np.asarray(sd_PM, dtype=np.float64)
    if mu.ndim != 2 or sd.shape != mu.shape:
        raise ValueError("mu_PM and sd_PM must both be (P, M)")
    w = check_mixture_weights(weights, mu.shape[0])[:, None]
    mix_mu = np.sum(w * mu, axis=0)
    var = np.sum(w * (sd * sd + (mu - mix_mu[None, :]) ** 2), axis=0)
    return mix_mu, np.sqrt(var)


def sample_hyper(x, y, e, best_l=None, n_samples=32, inflate=1.5, seed=None, max_points=MAX_POINTS,
                 value_and_grad=None, ctx=None, verbose=False, kernel="se"):
    """K = n_samples length-scale samples and their weights: (ls (K, d), weights (K,), info).

    The data preparation and the box are fit_lml's; best_l=None runs fit_lml first. In t = log l the
    Hessian of -LML at t* = log best_l is taken by central differences (step 1e-4) of the gradient, the
    2d points in ONE batched call, and symmetrised. Its eigenvalues are floored at
    (inflate / the box's smallest width in t)^2, so that no proposal standard deviation exceeds the box
    width (a flat or indefinite direction gets the box-wide proposal). K proposals are drawn from
    N(t*, inflate^2 H^-1) with default_rng(seed), truncated to the box by redrawing, and scored in ONE
    batched value call. The weights are self-normalised importance weights
    w_k proportional to exp(LML_k - max LML) / q(t_k) (prior: flat in log l on the box; the truncation
    rescales q by a constant, which cancels); a sample whose covariance is not positive definite
    gets weight 0.

    ``value_and_grad(positions (P, d)) -> (lml (P,), grad (P, d))``, the gradient in l, injects an
    evaluator exactly as in fit_lml; the default is gpf_lml_batch on this process's GPU.
    info: "ess" (= 1 / sum w^2), "hessian", "cov" (the proposal's), "lml" (K,), "best_l", "evals"
    (value evaluations, fit_lml's included) and "box". ``kernel`` as fit_lml's."""
    kernel_kind(kernel)
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    e = np.asarray(e, dtype=np.float64)
    K = int(n_samples)
    if K < 1:
        raise ValueError("n_samples must be >= 1")
    if not (np.isfinite(inflate) and inflate > 0.0):
        raise ValueError("inflate must be finite and > 0")
    injected = value_and_grad is not None
    if not injected and ctx is None:
        ctx = default_context()
    evals = 0
    if best_l is None:
        best_l, fit = fit_lml(x, y, e, max_points=max_points, seed=seed, value_and_grad=value_and_grad, ctx=ctx,
                              verbose=verbose, kernel=kernel)
        evals += fit["evals"]
    xs, ys, es, lower, upper, _, _ = prepare(x, y, e, max_points=max_points, verbose=verbose,
                                             ctx=None if injected else ctx)
    lower = np.maximum(lower, LOWER_FRACTION * upper)
    if not np.all(upper > lower):
        raise ValueError("sample_hyper: the search box is empty (a coordinate has no spread)")
    d = xs.shape[0]
    best_l = np.asarray(best_l, dtype=np.float64).reshape(-1)
    if best_l.shape != (d,) or not np.all(np.isfinite(best_l)) or np.any(best_l <= 0.0):
        raise ValueError(f"best_l must be ({d},), finite and > 0")
    if injected:
        comm = default_comm()
    else:
        ctx.set_data(xs, ys, es)
        use_kernel(ctx, kernel)
        value_and_grad = _device_evaluator(ctx)
        comm = default_comm(ctx)
    seed = share_seed(seed, comm)
    tlo, thi = np.log(lower), np.log(upper)
    ts = np.clip(np.log(best_l), tlo, thi)

    # Hessian of -LML in t: central differences of dLML/dt_k = l_k dLML/dl_k, 2d particles in one call
    h = HESSIAN_STEP
    pts = np.concatenate([ts[None, :] + h * np.eye(d), ts[None, :] - h * np.eye(d)])
    ls_h = np.exp(pts)
    _, g = _call(value_and_grad, ls_h, True)
    evals += 2 * d
    gt = g * ls_h
    hess = -(gt[:d] - gt[d:]).T / (2.0 * h)     # column k: d(-grad)/dt_k
    hess = 0.5 * (hess + hess.T)
    floor = (float(inflate) / float(np.min(thi - tlo))) ** 2
    if np.all(np.isfinite(hess)):
        lam, vec = np.linalg.eigh(hess)
    else:   # a difference point that did not factorise: the box-wide proposal
        lam, vec = np.full(d, floor), np.eye(d)
    lam = np.maximum(lam, floor)
    scale = vec * (float(inflate) / np.sqrt(lam))[None, :]   # t = t* + scale z, z ~ N(0, I)
    cov = scale @ scale.T
    prec = (vec * (lam / float(inflate) ** 2)[None, :]) @ vec.T

    rng = np.random.default_rng(seed)
    t = ts[None, :] + rng.standard_normal((K, d)) @ scale.T
    for _ in range(MAX_REDRAWS):
        out = np.any((t < tlo) | (t > thi), axis=1)
        n_out = int(np.count_nonzero(out))
        if n_out == 0:
            break
        t[out] = ts[None, :] + rng.standard_normal((n_out, d)) @ scale.T
    t = np.clip(t, tlo, thi)    # (only reached after MAX_REDRAWS rounds)
    ls = np.exp(t)

    lml, _ = _call(value_and_grad, ls, False)
    evals += K
    ok = np.isfinite(lml)
    if not np.any(ok):
        raise np.linalg.LinAlgError("sample_hyper: no sample's covariance is positive definite")
    dt = t - ts[None, :]
    logq = -0.5 * np.einsum("ki,ij,kj->k", dt, prec, dt)
    logw = np.where(ok, lml, -np.inf) - logq
    w = np.where(ok, np.exp(logw - np.max(logw[ok])), 0.0)
    w = w / np.sum(w)
    info = {"ess": float(1.0 / np.sum(w * w)), "hessian": hess, "cov": cov, "lml": np.where(ok, lml, -np.inf),
            "best_l": best_l.copy(), "evals": int(evals), "box": (lower, upper)}
    return ls, w, info


def predict_marginal(x, y, e, x_fit, ls=None, weights=None, method="batch", chunk=0, ctx=None, kernel="se",
                     **sample_kwargs):
    """The prediction at x_fit (d, M) marginalised over the length scales: (mix_mu (M,), mix_sd (M,),
    info). ``ls`` (K, d) with ``weights`` (K,) (None: equal) are the samples; ls=None draws them with
    sample_hyper(x, y, e, **sample_kwargs). The prediction itself uses all of (x, y, e), as GP() does.

    method="batch": one gpf_predict_batch call on this process's GPU, ``chunk`` query points per pass
    (0: the library's default). method="loop": K predict() calls and mixture_from, the yardstick.
    info: "ls", "weights" (normalised), "method", "ess" and, when the samples were drawn here,
    sample_hyper's info under "sample". ``kernel``: the covariance kernel of the sampling and of the
    prediction ("se", "matern32" or "matern52"; gpfit.kernels), set on the context on every call."""
    kernel_kind(kernel)
    if method not in METHODS:
        raise ValueError(f"method must be one of {METHODS}, not {method!r}")
    x = np.asarray(x, dtype=np.float64)
    x_fit = np.asarray(x_fit, dtype=np.float64)
    if x.ndim != 2 or x_fit.ndim != 2 or x_fit.shape[0] != x.shape[0]:
        raise ValueError("x_fit must be (d, M) with the same d as x")
    if int(chunk) < 0:
        raise ValueError("chunk must be >= 0")
    info = {"method": method}
    if ls is None:
        if weights is not None:
            raise ValueError("weights need their ls")
        if ctx is None and sample_kwargs.get("value_and_grad") is None:
            ctx = default_context()
        ls, weights, sample = sample_hyper(x, y, e, ctx=ctx, kernel=kernel, **sample_kwargs)
        info["sample"] = sample
    elif sample_kwargs:
        raise ValueError(f"with ls given, sample_hyper's arguments {sorted(sample_kwargs)} are not used")
    ls = np.ascontiguousarray(ls, dtype=np.float64)
    if ls.ndim == 1:
        ls = ls.reshape(1, -1)
    if ls.ndim != 2 or ls.shape[1] != x.shape[0] or ls.shape[0] < 1:
        raise ValueError(f"ls must be (K, {x.shape[0]}) with K >= 1")
    if not np.all(np.isfinite(ls)) or np.any(ls <= 0.0):
        raise ValueError("ls must be finite and > 0")
    w = check_mixture_weights(weights, ls.shape[0])
    info.update(ls=ls, weights=w, ess=float(1.0 / np.sum(w * w)))
    if ctx is None:
        ctx = default_context()
    ctx.set_data(x, y, e)
    use_kernel(ctx, kernel)
    if method == "batch":
        mix_mu, mix_sd, _ = ctx.predict_batch(ls, x_fit, weights=w, chunk=int(chunk))
        return mix_mu, mix_sd, info
    each = [ctx.predict(l, x_fit) for l in ls]
    mix_mu, mix_sd = mixture_from(np.stack([m for m, _ in each]), np.stack([s for _, s in each]), w)
    return mix_mu, mix_sd, info
