"""Prior amplitude and noise scale: the marginal-likelihood fit of (l, a, s) and prediction with them.

Every other module assumes Kn = K(l) + diag(e^2): prior variance exactly 1, the quoted errors taken
at face value. Here

  Kn = a^2 K(l) + s^2 diag(e^2) = a^2 Kt,   Kt = K(l) + (s/a)^2 diag(e^2),

a > 0 the prior sd of f, s > 0 a factor on the quoted errors; theta = (l_1 .. l_d, a, s).
``gpf_lml_hyper_batch`` returns the log marginal likelihood and its gradient in all d + 2, and
Q = y^T Kt^-1 y: for fixed l and s/a the likelihood is maximal at a^2 = Q / N, where it is

  LML(a) = LML(1) + Q/2 - Q / (2 a^2) - N log a.

``fit_hyper`` is gpfit.mle's two-stage fit with that: Latin-hypercube starts in (log l, log s/a)
scored in one batched value call at a = 1 and given their best amplitude in closed form, then
L-BFGS-B in (log l, log a, log s).

Nothing downstream needs a kernel of its own: the model with (a, s) on (x, y, e) is the unit model on
(x, y / a, e s / a) with mu a, sd a and cov a^2 (``scaled_data``, ``predict_hyper``).

Not built: per-particle (a, s) in gpf_predict_batch and gpfit.hyper.sample_hyper, leave-one-out with
(a, s). (A mean function: gpfit.meanfn, which shares this module's two-stage driver.)
"""
from __future__ import annotations

import inspect

import numpy as np

from ._lib import default_comm, default_context, use_kernel
from .kernels import kernel_kind
from .mle import LOWER_FRACTION, NUM_POLISH, NUM_STARTS, _call, polish_log
from .swarm import MAX_POINTS, centred_lhs, prepare, share_seed

RATIO_BOX = (0.1, 10.0)       # stage 1: s / a
A_BOX = (1e-3, 1e3)           # stage 2: a, in units of std(y)
S_BOX = (1e-2, 1e2)           # stage 2: s


def scaled_data(y, e, a, s):
    """(y / a, e s / a): the data on which the unit-amplitude, face-value-noise model is the model
    with amplitude a and noise scale s."""
    y = np.asarray(y, dtype=np.float64)
    e = np.asarray(e, dtype=np.float64)
    a, s = float(a), float(s)
    if not (np.isfinite(a) and a > 0 and np.isfinite(s) and s > 0):
        raise ValueError("scaled_data: a and s must be finite and > 0")
    return y / a, e * (s / a)


def predict_hyper(x, y, e, x_fit, theta, ctx=None, kernel="se"):
    """GP mean and sd at x_fit (d, M) under theta = (l_1 .. l_d, a, s): (mu (M,), sd (M,)), a times
    the unit model's prediction on ``scaled_data`` (sd: of the latent f, clipped as GP's).
    ``kernel``: the covariance kernel, "se" (default), "matern32" or "matern52" (gpfit.kernels), set on the context on every call."""
    kernel_kind(kernel)
    x = np.asarray(x, dtype=np.float64)
    theta = np.asarray(theta, dtype=np.float64).reshape(-1)
    if theta.shape[0] != x.shape[0] + 2:
        raise ValueError(f"theta must be ({x.shape[0] + 2},): the length scales, then a and s")
    a, s = theta[-2], theta[-1]
    ys, es = scaled_data(y, e, a, s)
    if ctx is None:
        ctx = default_context()
    ctx.set_data(x, ys, es)
    use_kernel(ctx, kernel)
    mu, sd = ctx.predict(theta[:-2], np.asarray(x_fit, dtype=np.float64))
    return mu * a, sd * a


def _device_evaluator(ctx):
    def value_and_grad(theta, grad=True, want_q=False):
        return ctx.lml_hyper_batch(theta, grad=grad, strict=False, want_q=want_q)
    return value_and_grad


def _value_and_q(value_and_grad, theta, n, counts):
    """(lml, Q) of every row of theta. An evaluator with a want_q= parameter (the device's) returns Q
    from a value-only call; from any other, Q = a^2 (N + a dLML/da + s dLML/ds)."""
    counts["evals"] += theta.shape[0]
    try:
        takes_q = "want_q" in inspect.signature(value_and_grad).parameters
    except (TypeError, ValueError):
        takes_q = False
    if takes_q:
        lml, _, q = value_and_grad(theta, grad=False, want_q=True)
        return np.asarray(lml, dtype=np.float64).reshape(-1), np.asarray(q, dtype=np.float64).reshape(-1)
    lml, g = _call(value_and_grad, theta, True)
    counts["grad_evals"] += theta.shape[0]
    a, s = theta[:, -2], theta[:, -1]
    return lml, a * a * (n + a * g[:, -2] + s * g[:, -1])


def _fit_theta(x, y, e, *, who, lost, pin, setup, done_msg, num_starts, num_polish, max_points, seed, value_and_grad,
               ctx, verbose, kernel="se"):
    """The two-stage driver behind fit_hyper and gpfit.meanfn.fit_mean. ``lost``: the degrees of freedom
    a marginalised mean takes (m; 0 for fit_hyper), so the best amplitude of a start is
    sqrt(Q / (N - lost)). ``setup(ctx or None, x, y, e)`` (optional) is called with the prepared points
    once the data are on the device and returns the evaluator (fit_mean sets its basis there); without
    it the evaluator is the injected one or gpf_lml_hyper_batch. ``pin``: a = s = 1, only the length
    scales are fitted (the starts in the length-scale box, stage 2 in log l)."""
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
    scale = float(np.std(y))
    if not (np.isfinite(scale) and scale > 0):
        raise ValueError(f"{who}: y has no spread")
    if injected:
        comm = default_comm()
        if setup is not None:
            value_and_grad = setup(None, x, y, e)
    else:
        ctx.set_data(x, y, e)
        use_kernel(ctx, kernel)
        value_and_grad = setup(ctx, x, y, e) if setup is not None else _device_evaluator(ctx)
        comm = default_comm(ctx)
    seed = share_seed(seed, comm)
    d, n = x.shape[0], y.reshape(-1).shape[0] - int(lost)
    if n < 1:
        raise ValueError(f"{who}: the mean function needs fewer coefficients than there are points")
    counts = {"evals": 0, "grad_evals": 0}
    if pin:
        lower = np.concatenate([lower, [1.0, 1.0]])
        upper = np.concatenate([upper, [1.0, 1.0]])
        ls = centred_lhs(lower[:d], upper[:d], int(num_starts), seed)
        starts = np.column_stack([ls, np.ones(len(ls)), np.ones(len(ls))])
        start_lml, _ = _call(value_and_grad, starts, False)
        counts["evals"] += starts.shape[0]
        start_lml = np.where(np.isfinite(start_lml), start_lml, -np.inf)
        order = np.argsort(-start_lml, kind="stable")[:max(1, int(num_polish))]

        def lengths_only(pos, grad=True):
            th = np.column_stack([pos, np.ones(len(pos)), np.ones(len(pos))])
            lml, g = _call(value_and_grad, th, grad)
            return lml, (g[:, :d] if grad else None)
        polished = polish_log(lengths_only, starts[:, :d], start_lml, order, lower[:d], upper[:d], "lml", counts)
        for r in polished:
            r["start"], r["x"] = np.append(r["start"], [1.0, 1.0]), np.append(r["x"], [1.0, 1.0])
        return _fit_result(polished, counts, lower, upper, starts, start_lml, d, done_msg, verbose)
    lower = np.concatenate([lower, [A_BOX[0] * scale, S_BOX[0]]])
    upper = np.concatenate([upper, [A_BOX[1] * scale, S_BOX[1]]])
    # stage 1: (l, s/a) starts in one batched call at a = 1, then the best amplitude of each
    u = np.exp(centred_lhs(np.log(np.append(lower[:d], RATIO_BOX[0])), np.log(np.append(upper[:d], RATIO_BOX[1])),
                           int(num_starts), seed))
    ratio = u[:, d]
    unit, q = _value_and_q(value_and_grad, np.column_stack([u[:, :d], np.ones(len(u)), ratio]), n, counts)
    ok = np.isfinite(unit) & np.isfinite(q) & (q > 0)
    # a = sqrt(Q / N) inside the a box and where s = ratio a is inside the s box (s/a is kept: the value
    # below is exact there); a start with no such a is a losing one
    alo = np.maximum(lower[d], lower[d + 1] / ratio)
    ahi = np.minimum(upper[d], upper[d + 1] / ratio)
    ok &= ahi >= alo
    a = np.clip(np.sqrt(np.where(ok, q, n) / n), alo, np.maximum(ahi, alo))
    starts = np.column_stack([u[:, :d], a, np.clip(ratio * a, lower[d + 1], upper[d + 1])])
    with np.errstate(invalid="ignore"):
        start_lml = np.where(ok, unit + 0.5 * q - 0.5 * q / (a * a) - n * np.log(a), -np.inf)
    order = np.argsort(-start_lml, kind="stable")[:max(1, int(num_polish))]

    # stage 2: L-BFGS-B on -LML in t = log theta
    polished = polish_log(value_and_grad, starts, start_lml, order, lower, upper, "lml", counts)
    return _fit_result(polished, counts, lower, upper, starts, start_lml, d, done_msg, verbose)


def _fit_result(polished, counts, lower, upper, starts, start_lml, d, done_msg, verbose):
    best = max(polished, key=lambda r: r["lml"])
    if verbose:
        print(done_msg)
        print("Optimal length scale found:")
        print(best["x"][:d])
        print("Amplitude and noise scale:")
        print(best["x"][d:])
        print("Log marginal likelihood:")
        print(best["lml"])
    info = {"lml": best["lml"], "evals": counts["evals"], "grad_evals": counts["grad_evals"],
            "box": (lower, upper), "starts": (starts, start_lml), "polished": polished}
    return best["x"].copy(), info


def fit_hyper(x, y, e, *, num_starts=NUM_STARTS, num_polish=NUM_POLISH, max_points=MAX_POINTS, seed=None,
              value_and_grad=None, ctx=None, verbose=True, kernel="se"):
    """theta = (l_1 .. l_d, a, s) that maximises the log marginal likelihood: (theta (d + 2,), info).

    fit_lml's signature and semantics. ``value_and_grad(theta (P, d + 2)) -> (lml (P,), grad (P, d + 2))``
    injects an evaluator (the CPU tests); the default is gpf_lml_hyper_batch on this process's GPU. A
    point whose covariance is not positive definite is a losing point, never an error.

      stage 1  ``num_starts`` centred-Latin-hypercube starts in (log l in fit_lml's box, log(s/a) in
               [log 0.1, log 10]), scored in one batched value call at a = 1; each gets its best
               amplitude a = sqrt(Q / N) (kept inside stage 2's box) and the value there, in closed form;
      stage 2  the ``num_polish`` best polished by L-BFGS-B in (log l, log a, log s); a in
               [1e-3, 1e3] std(y), s in [1e-2, 1e2].

    info: "lml" (at theta), "evals", "grad_evals", "box" (lower, upper: d + 2 each), "starts"
    (theta (num_starts, d + 2), lml) and "polished" (one dict per polished start: start, x, lml,
    start_lml, nfev, nit, message). ``kernel`` as fit_lml's.
    """
    return _fit_theta(x, y, e, who="fit_hyper", lost=0, pin=False, setup=None,
                      done_msg="Marginal-likelihood fit of length scales, amplitude and noise scale completed.",
                      num_starts=num_starts, num_polish=num_polish, max_points=max_points, seed=seed,
                      value_and_grad=value_and_grad, ctx=ctx, verbose=verbose, kernel=kernel)
