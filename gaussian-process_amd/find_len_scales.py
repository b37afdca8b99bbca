"""Drop-in for the reference's find_len_scales.py, computed on the MI355X.

Public surface of find_len_scales.py (rferguson22/Gaussian-Process):
    len_scale_opt(x_known, y_known, e_known, PSO_progress)        :22-150
    wass_loss(ls, x, y, e, sigma_vals, expected, lower, upper)     :154-177
    evaluate_loss(lengths, ...)                                    :181-182
    evaluate_loss_helper(args)                                     :186-188
    sigma_to_percent(x)                                            :192-201

Every objective evaluation runs in libgpfit (gpf_eval_batch): the reference's
fork pool over particles becomes one batched call per PSO iteration.
len_scale_opt keeps the reference defaults (40 particles, 500 iterations,
KMeans subsample above 100 points) and adds keyword-only overrides used by the
benchmarks and the tests: num_particles, max_iter, max_points,
init_positions, seed.

objective="marginal_likelihood" replaces the swarm by a maximum-marginal-likelihood
fit (gpfit.mle.fit_lml: batched starts, then L-BFGS-B with the gradient from
gpf_lml_batch); objective="loo" maximises the leave-one-out log predictive density
instead (gpfit.loo.fit_loo, gradient from gpf_loo_batch). Both take num_starts,
max_points and seed. The default, objective="calibration", is the reference's search.

kernel="se" | "matern32" | "matern52" (gpfit.kernels) chooses the covariance kernel of any of the
three objectives, on every rank of a sharded swarm; wass_loss and evaluate_loss keep the reference's
signatures and are always squared-exponential.
"""
import numpy as np

from gpfit._lib import default_context
from gpfit.kernels import kernel_kind
from gpfit.swarm import particle_swarm
from gpfit.swarm import sigma_to_percent as _sigma_to_percent

__all__ = ["len_scale_opt", "wass_loss", "evaluate_loss", "evaluate_loss_helper", "sigma_to_percent"]


def len_scale_opt(x_known, y_known, e_known, PSO_progress, *, num_particles=40, max_iter=500,
                  max_points=100, init_positions=None, seed=None, objective="calibration", num_starts=40, kernel="se"):
    """PSO search for the per-dimension length scales (find_len_scales.py:22-150), or with
    objective="marginal_likelihood" the maximum-marginal-likelihood fit (gpfit.mle.fit_lml), with
    objective="loo" the leave-one-out fit (gpfit.loo.fit_loo). ``kernel``: the covariance kernel of the
    objective ("se", the reference's; "matern32"; "matern52"); an unknown name is a ValueError."""
    # (the default is not handed on: a call without the keyword makes exactly the calls it made before)
    kw = {} if kernel_kind(kernel) == 0 else {"kernel": kernel}
    if objective == "marginal_likelihood":
        from gpfit.mle import fit_lml
        best, _ = fit_lml(np.asarray(x_known, dtype=np.float64), np.asarray(y_known, dtype=np.float64),
                          np.asarray(e_known, dtype=np.float64), num_starts=num_starts, max_points=max_points,
                          seed=seed, verbose=bool(PSO_progress), **kw)
        return best
    if objective == "loo":
        from gpfit.loo import fit_loo
        best, _ = fit_loo(np.asarray(x_known, dtype=np.float64), np.asarray(y_known, dtype=np.float64),
                          np.asarray(e_known, dtype=np.float64), num_starts=num_starts, max_points=max_points,
                          seed=seed, verbose=bool(PSO_progress), **kw)
        return best
    if objective != "calibration":
        raise ValueError(f"len_scale_opt: unknown objective {objective!r} (calibration, marginal_likelihood or loo)")
    best, _ = particle_swarm(np.asarray(x_known, dtype=np.float64), np.asarray(y_known, dtype=np.float64),
                             np.asarray(e_known, dtype=np.float64), PSO_progress,
                             num_particles=num_particles, max_iter=max_iter, max_points=max_points,
                             init_positions=init_positions, seed=seed, **kw)
    return best


def wass_loss(ls, x_known, y_known, e_known, sigma_vals, expected_percents, lower_bounds, upper_bounds):
    """Negated calibration loss of one particle (find_len_scales.py:154-177)."""
    return -evaluate_loss(ls, x_known, y_known, e_known, sigma_vals, expected_percents,
                          lower_bounds, upper_bounds)


def evaluate_loss(lengths, x_known, y_known, e_known, sigma_vals, expected_percents, lower_bounds, upper_bounds):
    """find_len_scales.py:181-182: W + 0.01 * proximity, or 1e13 outside the box."""
    ctx = default_context()
    ctx.set_data(x_known, y_known, e_known)
    ctx.set_kernel("se")
    ctx.set_grid(sigma_vals, expected_percents, lower_bounds, upper_bounds)
    return float(ctx.eval_batch(np.asarray(lengths, dtype=np.float64).reshape(1, -1))[0])


def evaluate_loss_helper(args):
    """find_len_scales.py:186-188 (tuple-unpacking task body)."""
    return evaluate_loss(*args)


def sigma_to_percent(x):
    """Phi(x) - Phi(-x) (find_len_scales.py:192-201)."""
    return _sigma_to_percent(x)
