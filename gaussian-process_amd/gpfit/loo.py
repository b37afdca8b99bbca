"""Leave-one-out (LOO) cross-validation of the GP and a LOO fit of the length scales.

The calibration loss and the log marginal likelihood both score a length-scale vector on data the
model has seen. The LOO check predicts every training point from the other N - 1 (Rasmussen &
Williams, section 5.4.2), in closed form from one factorisation: with W = Kn^-1, alpha = W y and
w_i = W_ii,

  mu_i = y_i - alpha_i / w_i,  sd_i = sqrt(1 / w_i)   (the sd of the measured value, e_i^2 included),
  pull_i = (y_i - mu_i) / sd_i = alpha_i / sqrt(w_i)  ~ N(0, 1) under the model,
  lpd = sum_i [1/2 log w_i - 1/2 alpha_i^2 / w_i] - N/2 log(2 pi).

``loo_predict`` is the validation report; ``fit_loo`` maximises lpd with its gradient
(``gpf_loo_batch``) by gpfit.mle's two-stage driver: Latin-hypercube starts in one batched value
call, then L-BFGS-B in log l.

Model: fixed amplitude 1, fixed noise e^2, ARD squared-exponential, as GP_func.py.
"""
from __future__ import annotations

import numpy as np

from ._lib import default_context, use_kernel
from .kernels import kernel_kind
from .mle import NUM_POLISH, NUM_STARTS, fit_gradient
from .swarm import MAX_POINTS


def loo_predict(x, y, e, lengths, ctx=None, kernel="se"):
    """Every training point predicted from the others at the length scales ``lengths`` (d,):
    (mu (N,), sd (N,), info). info: "lpd" (the LOO log predictive density), "pulls"
    ((y - mu) / sd) and "coverage" (the fractions of |pull| <= 1 and <= 2: 0.683 and 0.954 for
    honest error bars). LinAlgError if the covariance is not positive definite.
    ``kernel``: the covariance kernel, "se" (default), "matern32" or "matern52" (gpfit.kernels), set on the context on every call."""
    kernel_kind(kernel)
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    e = np.asarray(e, dtype=np.float64)
    if ctx is None:
        ctx = default_context()
    ctx.set_data(x, y, e)
    use_kernel(ctx, kernel)
    lpd, _, mu, sd = ctx.loo_batch(np.asarray(lengths, dtype=np.float64).reshape(1, -1), grad=False, points=True)
    mu, sd = mu[0], sd[0]
    pulls = (y.reshape(-1) - mu) / sd
    info = {"lpd": float(lpd[0]), "pulls": pulls,
            "coverage": (float(np.mean(np.abs(pulls) <= 1.0)), float(np.mean(np.abs(pulls) <= 2.0)))}
    return mu, sd, info


def _device_evaluator(ctx):
    def value_and_grad(positions, grad=True):
        return ctx.loo_batch(positions, grad=grad, strict=False)
    return value_and_grad


def fit_loo(x, y, e, *, num_starts=NUM_STARTS, num_polish=NUM_POLISH, max_points=MAX_POINTS, seed=None,
            value_and_grad=None, ctx=None, verbose=True, kernel="se"):
    """Length scales that maximise the LOO log predictive density: (best_l (d,), info).

    fit_lml's signature and semantics with lpd in place of the log marginal likelihood:
    ``value_and_grad(positions (P, d)) -> (lpd (P,), grad (P, d))`` injects an evaluator (the CPU
    tests); the default is gpf_loo_batch on this process's GPU. A point whose covariance is not
    positive definite is a losing point, never an error. info: "lpd" (at best_l), "evals",
    "grad_evals", "box", "starts" (positions, lpd) and "polished" (one dict per polished start:
    start, x, lpd, start_lpd, nfev, nit, message). ``kernel`` as fit_lml's.
    """
    return fit_gradient(x, y, e, who="fit_loo", key="lpd", done_msg="Leave-one-out fit completed.",
                        value_label="LOO log predictive density:", device_evaluator=_device_evaluator,
                        num_starts=num_starts, num_polish=num_polish, max_points=max_points, seed=seed,
                        value_and_grad=value_and_grad, ctx=ctx, verbose=verbose, kernel=kernel)
