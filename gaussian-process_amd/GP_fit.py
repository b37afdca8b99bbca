"""Drop-in for the reference's GP_fit.py: per-experiment fit + prediction + CSV writers.

Orchestration stays on the host; the two calls that matter
run on the MI355X: len_scale_opt (batched PSO objective, gpf_eval_batch) and GP on
the hull grid (gpf_predict). Column naming, file naming, merge semantics and
messages follow GP_fit.py:20-164.

Optional options.yaml keys (absent = reference behaviour): pso_num_particles (40),
pso_max_iter (500), pso_max_points (100), pso_seed (none: unseeded global RNG);
len_scale_objective ("calibration": the reference's swarm; "marginal_likelihood": the
maximum-marginal-likelihood fit; "loo": the leave-one-out fit; both reuse pso_max_points and pso_seed;
"marginal_likelihood_full": the marginal-likelihood fit of the length scales, a prior amplitude and a
factor on the quoted errors, gpfit.amplitude.fit_hyper, and the prediction with them, GP_hyper; it
reuses pso_max_points, pso_seed and mle_num_starts and does not combine with hyper_samples),
mle_num_starts (40) and hyper_samples (K >= 1: the written mean and sd are marginalised over K
length-scale samples, gpfit.hyper.predict_marginal, instead of taken at the one fitted vector; it
reuses pso_max_points and pso_seed) and mean_function ("constant", "linear" or "quadratic": a polynomial
mean with its coefficients integrated out, gpfit.meanfn.fit_mean and GP_mean; valid only with
len_scale_objective: marginal_likelihood_full) and kernel ("se", "matern32" or "matern52": the covariance
kernel of the fit and of the prediction, gpfit.kernels; it combines with every len_scale_objective, with
hyper_samples and with mean_function).
"""
from functools import reduce
from pathlib import Path

import pandas as pd
import yaml

from convex_hull import fill_convex_hull
from find_len_scales import len_scale_opt
from GP_func import GP, GP_hyper, GP_kernel, GP_mean
from read_in import read_yaml

__all__ = ["process_experiment", "write_individual_file", "write_grouped_file", "write_combined_file",
           "create_GP"]

_PSO_KEYS = {"pso_num_particles": "num_particles", "pso_max_iter": "max_iter", "pso_max_points": "max_points",
             "pso_seed": "seed", "len_scale_objective": "objective", "mle_num_starts": "num_starts"}


def _pso_overrides(options_path="options.yaml"):
    try:
        with open(options_path, "r") as f:
            opts = yaml.safe_load(f) or {}
    except OSError:
        return {}
    return {kw: opts[key] for key, kw in _PSO_KEYS.items() if opts.get(key) is not None}


def _hyper_samples(options_path="options.yaml"):
    """options.yaml's hyper_samples as an int K >= 1, or None (absent: the reference's prediction at the
    fitted length scales, byte-identical outputs)."""
    try:
        with open(options_path, "r") as f:
            opts = yaml.safe_load(f) or {}
    except OSError:
        return None
    k = opts.get("hyper_samples")
    if k is None:
        return None
    if isinstance(k, bool) or not isinstance(k, int) or k < 1:
        raise ValueError(f"options.yaml: hyper_samples must be an integer >= 1, not {k!r}")
    return k


def _mean_function(options_path="options.yaml"):
    """options.yaml's mean_function ("constant", "linear" or "quadratic"), or None (absent: the zero-mean
    model, byte-identical outputs)."""
    try:
        with open(options_path, "r") as f:
            opts = yaml.safe_load(f) or {}
    except OSError:
        return None
    kind = opts.get("mean_function")
    if kind is None:
        return None
    if kind not in ("constant", "linear", "quadratic"):
        raise ValueError(f"options.yaml: mean_function must be constant, linear or quadratic, not {kind!r}")
    if opts.get("len_scale_objective") != "marginal_likelihood_full":
        raise ValueError("options.yaml: mean_function is valid only with len_scale_objective: "
                         "marginal_likelihood_full (the fit of length scales, amplitude and noise scale), not with "
                         f"{opts.get('len_scale_objective', 'calibration')!r}")
    return kind


def _kernel(options_path="options.yaml"):
    """options.yaml's kernel ("se", "matern32" or "matern52"), or None (absent: the squared-exponential
    model through exactly the calls made without the key, byte-identical outputs)."""
    try:
        with open(options_path, "r") as f:
            opts = yaml.safe_load(f) or {}
    except OSError:
        return None
    kernel = opts.get("kernel")
    if kernel is None:
        return None
    if not isinstance(kernel, str) or kernel not in ("se", "matern32", "matern52"):
        raise ValueError(f"options.yaml: kernel must be se, matern32 or matern52, not {kernel!r}")
    return kernel


def _marginal(x_known, y_known, e_known, x_fit, ls, k, pso):
    """predict_marginal's mean and sd at K samples around the marginal likelihood's optimum: the fitted
    vector when the fit maximised it, else gpfit.mle.fit_lml's (the swarm's optimum of the calibration
    loss is not the centre of the likelihood)."""
    from gpfit.hyper import predict_marginal
    kw = {key: pso[key] for key in ("max_points", "seed", "kernel") if key in pso}
    best = ls if pso.get("objective") == "marginal_likelihood" else None
    mu, sd, _ = predict_marginal(x_known, y_known, e_known, x_fit, best_l=best, n_samples=k, **kw)
    return mu, sd


def _fit_full(x_known, y_known, e_known, progress, pso, mean_function=None):
    """theta = (l.., a, s) of len_scale_objective: marginal_likelihood_full (gpfit.amplitude.fit_hyper;
    with a mean function gpfit.meanfn.fit_mean)."""
    import numpy as np
    kw = {key: pso[key] for key in ("num_starts", "max_points", "seed", "kernel") if key in pso}
    data = (np.asarray(x_known, dtype=np.float64), np.asarray(y_known, dtype=np.float64),
            np.asarray(e_known, dtype=np.float64))
    if mean_function is not None:
        from gpfit.meanfn import fit_mean
        return fit_mean(*data, kind=mean_function, verbose=bool(progress), **kw)[0]
    from gpfit.amplitude import fit_hyper
    theta, _ = fit_hyper(*data, verbose=bool(progress), **kw)
    return theta


def _merge(frames, on):
    return reduce(lambda a, b: pd.merge(a, b, on=on, how="outer"), frames).fillna(float("inf"))


def process_experiment(x_known, y_known, e_known, resolution, dim_labels, filename, exp_idx, total_exps,
                       PSO_progress, hyper_samples=None, mean_function=None, **pso):
    """Length scales by PSO, hull grid, GP prediction -> DataFrame (GP_fit.py:20-46). hyper_samples=K
    writes the prediction marginalised over K length-scale samples instead of GP's. A ``kernel`` in pso
    (options.yaml's, absent for the default) is the covariance kernel of the fit and of the prediction."""
    if x_known.shape[1] == 0:
        print("  Skipping experiment: no valid data points")
        return None
    full = pso.get("objective") == "marginal_likelihood_full"
    if mean_function is not None and not full:
        raise ValueError("mean_function is valid only with len_scale_objective: marginal_likelihood_full")
    if full:
        if hyper_samples is not None:
            raise ValueError("options.yaml: hyper_samples does not combine with len_scale_objective: "
                             "marginal_likelihood_full")
        ls = _fit_full(x_known, y_known, e_known, PSO_progress, pso, mean_function)
    else:
        ls = len_scale_opt(x_known, y_known, e_known, PSO_progress, **pso)
    grid = fill_convex_hull(x_known.T, resolution)
    kkw = {"kernel": pso["kernel"]} if "kernel" in pso else {}
    if full and mean_function is not None:
        mu, sd = GP_mean(x_known, y_known, e_known, grid.T, ls, mean_function, **kkw)
    elif full:
        mu, sd = GP_hyper(x_known, y_known, e_known, grid.T, ls, **kkw)
    elif hyper_samples is None and kkw:
        mu, sd = GP_kernel(x_known, y_known, e_known, grid.T, ls, pso["kernel"])
    elif hyper_samples is None:
        mu, sd = GP(x_known, y_known, e_known, grid.T, ls)
    else:
        mu, sd = _marginal(x_known, y_known, e_known, grid.T, ls, hyper_samples, pso)
    frame = pd.DataFrame(grid, columns=dim_labels)
    if total_exps == 1:
        qcol, ecol = f"{filename}", f"{filename}_unc"
    else:
        qcol, ecol = f"{filename}_exp{exp_idx}", f"{filename}_unc{exp_idx}"
    frame[qcol] = mu.flatten()
    frame[ecol] = sd.flatten()
    return frame


def write_individual_file(df, filename, out_path, total_exps, exp_idx):
    """One experiment per file (GP_fit.py:50-66)."""
    folder = out_path if out_path.is_dir() else out_path.parent
    folder.mkdir(parents=True, exist_ok=True)
    name = f"{filename}_GP_results.txt" if total_exps == 1 else f"{filename}_exp{exp_idx}_GP_results.txt"
    target = folder / name
    df.to_csv(target, index=False)
    print(f"Written individual output file: {target}")


def write_grouped_file(file_dfs, filename, out_path, dim_labels):
    """All experiments of one input file merged on the grid (GP_fit.py:70-85)."""
    folder = out_path if out_path.is_dir() else out_path.parent
    folder.mkdir(parents=True, exist_ok=True)
    target = folder / f"{filename}_GP_results.txt"
    _merge(file_dfs, dim_labels).to_csv(target, index=False)
    print(f"Written grouped output file: {target}")


def write_combined_file(experiment_dfs, out_path, dim_labels):
    """Every experiment merged into one file (GP_fit.py:89-108)."""
    if str(out_path).endswith("/"):
        out_path.mkdir(parents=True, exist_ok=True)
        target = out_path / "GP_results.txt"
    else:
        target = out_path
        target.parent.mkdir(parents=True, exist_ok=True)
    merged = _merge(experiment_dfs, dim_labels)
    merged.to_csv(target, index=False)
    print(f"Combined results written to {target}")
    return merged


def create_GP():
    """Fit every experiment of every configured file and write the outputs (GP_fit.py:112-164).

    Returns (merged DataFrame, number of kinematic dimensions).
    """
    resolution, progress, out_name, labels, data_list, write_ind, group_exps = read_yaml()
    pso = _pso_overrides()
    hyper = _hyper_samples()
    if hyper is not None:
        pso = dict(pso, hyper_samples=hyper)
    mean_function = _mean_function()
    if mean_function is not None:
        pso = dict(pso, mean_function=mean_function)
    kernel = _kernel()
    if kernel is not None:
        pso = dict(pso, kernel=kernel)
    nd = len(resolution)
    dim_labels = labels[:nd]
    out_path = Path(out_name) if out_name else Path("GP_results.txt")

    if write_ind:
        print("Writing individual output files")
        print("Writing experiments from the same file together" if group_exps
              else "Writing experiments from the same file separately")
    else:
        print("Writing combined output file")

    all_dfs = []
    for file_idx, (file_path, xs, pairs, _labels) in enumerate(data_list, start=1):
        stem = Path(file_path).stem
        n_exp = len(xs)
        file_dfs = []
        for idx, (x, (y, e)) in enumerate(zip(xs, pairs), start=1):
            print(f"Processing experiment {idx}/{n_exp} from file {file_idx}/{len(data_list)}: {stem}")
            df = process_experiment(x, y, e, resolution, dim_labels, stem, idx, n_exp, progress, **pso)
            if df is None:
                continue
            all_dfs.append(df)
            file_dfs.append(df)
            if write_ind and not group_exps:
                write_individual_file(df, stem, out_path, n_exp, idx)
        if write_ind and group_exps and file_dfs:
            write_grouped_file(file_dfs, stem, out_path, dim_labels)

    if not write_ind and all_dfs:
        return write_combined_file(all_dfs, out_path, dim_labels), nd
    if all_dfs:
        return _merge(all_dfs, dim_labels), nd
    print("No experiment data to return")
    return pd.DataFrame(), nd
