"""Maximum-marginal-likelihood fit of the length scales.

The reference's only fit is a 500-iteration particle swarm over a calibration loss
(find_len_scales.py:22-150). With the gradient of the log marginal likelihood
(``gpf_lml_batch``) a fit takes tens of evaluations instead of 20,000:

  stage 1  ``num_starts`` centred-Latin-hypercube starts in the search box, scored in one
           batched value call;
  stage 2  the ``num_polish`` best starts polished by scipy's L-BFGS-B in log l inside the box,
           dLML/dlog l_k = l_k dLML/dl_k.

The data preparation is the swarm's (``gpfit.swarm.prepare``: the KMeans subsample above
``max_points`` and the reference's search box). The reference's lower bound (the smallest
positive gap between coordinates) can be 0, where log l is not defined, so the box used here
starts at max(lower, 1e-3 * upper).

Model: fixed amplitude 1, fixed noise e^2, ARD squared-exponential, as GP_func.py (gpfit.amplitude
fits an amplitude and a noise scale as well, with this module's stage 2).
"""
from __future__ import annotations

import inspect

import numpy as np

from ._lib import default_comm, default_context, use_kernel
from .kernels import kernel_kind
from .swarm import MAX_POINTS, centred_lhs, prepare, share_seed

NUM_STARTS = 40
NUM_POLISH = 4
LOWER_FRACTION = 1e-3   # box lower bound: max(reference lower, LOWER_FRACTION * upper)
BAD_VALUE = 1e300       # -LML of a non-positive-definite point: a losing, finite value for the line search


def _device_evaluator(ctx):
    def value_and_grad(positions, grad=True):
        return ctx.lml_batch(positions, grad=grad, strict=False)
    return value_and_grad


def _takes_grad(value_and_grad):
    try:
        return "grad" in inspect.signature(value_and_grad).parameters
    except (TypeError, ValueError):
        return False


def _call(value_and_grad, positions, grad):
    """value_and_grad(positions) -> (lml, grad); an evaluator with a grad= parameter (the device's)
    is spared the gradient pass on value-only calls."""
    if _takes_grad(value_and_grad):
        lml, g = value_and_grad(positions, grad=grad)
    else:
        lml, g = value_and_grad(positions)
    lml = np.asarray(lml, dtype=np.float64).reshape(-1)
    if grad:
        g = np.asarray(g, dtype=np.float64).reshape(positions.shape)
    return lml, (g if grad else None)


def polish_log(value_and_grad, starts, start_val, order, lower, upper, key, counts):
    """Stage 2 of the fits: the starts ``order`` polished by L-BFGS-B on minus the evaluator's value in
    t = log(position) inside the box, d/dlog p_k = p_k d/dp_k. One dict per polished start (start, x,
    key, start_<key>, nfev, nit, message); counts["evals"] and ["grad_evals"] are advanced."""
    from scipy.optimize import minimize

    d = starts.shape[1]
    tlo, thi = np.log(lower), np.log(upper)

    def neg(t):
        ls = np.exp(t).reshape(1, d)
        lml, g = _call(value_and_grad, ls, True)
        counts["evals"] += 1
        counts["grad_evals"] += 1
        if not np.isfinite(lml[0]) or not np.all(np.isfinite(g[0])):
            return BAD_VALUE, np.zeros(d)
        return -lml[0], -(g[0] * ls[0])

    polished = []
    for s in order:
        t0 = np.clip(np.log(starts[s]), tlo, thi)
        res = minimize(neg, t0, jac=True, method="L-BFGS-B", bounds=list(zip(tlo, thi)))
        ls = np.clip(np.exp(res.x), lower, upper)
        val = -float(res.fun) if res.fun < BAD_VALUE else -np.inf
        if not val >= start_val[s]:  # (a line search that only met losing points: keep the start)
            ls, val = starts[s].copy(), float(start_val[s])
        polished.append({"start": starts[s].copy(), "x": ls, key: val, "start_" + key: float(start_val[s]),
                         "nfev": int(res.nfev), "nit": int(res.nit), "message": str(res.message)})
    return polished


def fit_gradient(x, y, e, *, who, key, done_msg, value_label, device_evaluator, num_starts, num_polish, max_points,
                 seed, value_and_grad, ctx, verbose, kernel="se"):
    """The two-stage driver behind fit_lml and gpfit.loo.fit_loo: maximises the value an evaluator
    returns with its gradient in the length scales. ``who`` names the caller in messages, ``key`` the
    value in info ("lml", "lpd"), ``device_evaluator(ctx)`` builds the default evaluator."""
    kernel_kind(kernel)
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    e = np.asarray(e, dtype=np.float64)
    injected = value_and_grad is not None
    if not injected and ctx is None:
        ctx = default_context()
    x, y, e, lower, upper, _, _ = prepare(x, y, e, max_points=max_points, verbose=verbose,
                                          ctx=None if injected else ctx)
    lower = np.maximum(lower, LOWER_FRACTION * upper)
    if not np.all(upper > lower):
        raise ValueError(f"{who}: the search box is empty (a coordinate has no spread)")
    if injected:
        comm = default_comm()
    else:
        ctx.set_data(x, y, e)
        use_kernel(ctx, kernel)
        value_and_grad = device_evaluator(ctx)
        comm = default_comm(ctx)
    seed = share_seed(seed, comm)
    counts = {"evals": 0, "grad_evals": 0}

    # stage 1: every start in one batched value call
    starts = centred_lhs(lower, upper, int(num_starts), seed)
    start_lml, _ = _call(value_and_grad, starts, False)
    counts["evals"] += starts.shape[0]
    start_lml = np.where(np.isfinite(start_lml), start_lml, -np.inf)
    order = np.argsort(-start_lml, kind="stable")[:max(1, int(num_polish))]

    # stage 2: L-BFGS-B on -LML in t = log l
    polished = polish_log(value_and_grad, starts, start_lml, order, lower, upper, key, counts)
    best = max(polished, key=lambda r: r[key])
    if verbose:
        print(done_msg)
        print("Optimal length scale found:")
        print(best["x"])
        print(value_label)
        print(best[key])
    info = {key: best[key], "evals": counts["evals"], "grad_evals": counts["grad_evals"],
            "box": (lower, upper), "starts": (starts, start_lml), "polished": polished}
    return best["x"].copy(), info


def fit_lml(x, y, e, *, num_starts=NUM_STARTS, num_polish=NUM_POLISH, max_points=MAX_POINTS, seed=None,
            value_and_grad=None, ctx=None, verbose=True, kernel="se"):
    """Length scales that maximise the log marginal likelihood: (best_l (d,), info).

    ``value_and_grad(positions (P, d)) -> (lml (P,), grad (P, d))`` injects an evaluator (the CPU
    tests); the default is gpf_lml_batch on this process's GPU. A point whose covariance is not
    positive definite (lml = -inf or NaN) is a losing point, never an error. Under WORLD_SIZE > 1
    every rank runs the same seeded fit redundantly. info: "lml" (at best_l), "evals" (value
    evaluations), "grad_evals", "box" (lower, upper), "starts" (positions, lml) and "polished" (one
    dict per polished start: start, x, lml, start_lml, nfev, nit, message).
    ``kernel``: the covariance kernel, "se" (default), "matern32" or "matern52" (gpfit.kernels), set on the context on every call. An injected
    evaluator brings its own.
    """
    return fit_gradient(x, y, e, who="fit_lml", key="lml", done_msg="Marginal-likelihood fit completed.",
                        value_label="Log marginal likelihood:", device_evaluator=_device_evaluator,
                        num_starts=num_starts, num_polish=num_polish, max_points=max_points, seed=seed,
                        value_and_grad=value_and_grad, ctx=ctx, verbose=verbose, kernel=kernel)
