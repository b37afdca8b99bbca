"""Time the calls that evaluate the covariance under each kernel of the family (gpf_set_kernel), the kinds
alternating in one run: eval_batch, lml_batch value only and value + gradient, and predict at M query points.

Data and particles as bench.py's headline (synthetic(N, d, seed); interior particles l ~ U[0.05, 0.6]^d from
default_rng(seed + 1000), a fresh batch per step, the same batch for the three kinds); the queries are
U(0, 1)^d. Every step times the legs of se, matern32 and matern52 one after the other, so clock drift falls
on all three alike. Prints one JSON line (and writes it to --out): per kind and leg the median, min and max
ms per call, the ratios of the medians to se's, and the library's build hash.

--trace-only runs each leg `--steps` times per kind without timing, for a kernel-trace run of its own
(rocprofv3 --kernel-trace --stats -- python scripts/kernel_family_bench.py --trace-only --steps 3): the
instantiations of k_cross_cov, k_lml_grad, k_step and k_build_cov carry the kind in their template arguments.
Usage: python scripts/kernel_family_bench.py [--n 4096] [--d 3] [--particles 64] [--m 10000] [--steps 10]
       [--warmup 2] [--seed 1] [--out FILE] [--trace-only]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gaussian-process_amd"))

import numpy as np  # noqa: E402

KINDS = ("se", "matern32", "matern52")
LEGS = ("eval_batch", "lml_value", "lml_value_grad", "predict")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--d", type=int, default=3)
    ap.add_argument("--particles", type=int, default=64)
    ap.add_argument("--m", type=int, default=10000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-only", action="store_true")
    args = ap.parse_args()
    import gpfit
    from gpfit.swarm import search_bounds, sigma_grid

    N, d, P, M = args.n, args.d, args.particles, args.m
    rng = np.random.default_rng(args.seed)  # bench.synthetic
    x = rng.uniform(0.0, 1.0, size=(d, N))
    y = np.sum(np.sin(2 * np.pi * x), axis=0) + 0.1 * rng.standard_normal(N)
    e = np.full(N, 0.1)
    q = rng.uniform(0.0, 1.0, size=(d, M))
    ctx = gpfit.Context(int(os.environ.get("GPFIT_DEVICE", "0")))
    ctx.set_data(x, y, e)
    lo, hi = search_bounds(x)
    ctx.set_grid(*sigma_grid(), lo, hi)
    prng = np.random.default_rng(args.seed + 1000)
    legs = {"eval_batch": lambda ls: ctx.eval_batch(ls),
            "lml_value": lambda ls: ctx.lml_batch(ls, grad=False, strict=False),
            "lml_value_grad": lambda ls: ctx.lml_batch(ls, grad=True, strict=False),
            "predict": lambda ls: ctx.predict(ls[0], q)}
    ms = {k: {leg: [] for leg in LEGS} for k in KINDS}
    warmup = 0 if args.trace_only else args.warmup
    for step in range(warmup + args.steps):
        ls = prng.uniform(0.05, 0.6, size=(P, d))
        for leg in LEGS:
            for kind in KINDS:
                ctx.set_kernel(kind)
                ctx.synchronize()
                t0 = time.perf_counter()
                legs[leg](ls)
                ctx.synchronize()
                if step >= warmup:
                    ms[kind][leg].append((time.perf_counter() - t0) * 1e3)
    ctx.set_kernel("se")
    stat = {k: {leg: {"median_ms": round(float(np.median(v)), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}
                for leg, v in legs_.items()} for k, legs_ in ms.items()}
    ratio = {k: {leg: round(stat[k][leg]["median_ms"] / stat["se"][leg]["median_ms"], 4) for leg in LEGS}
             for k in KINDS[1:]}
    out = {"bench": "kernel_family", "N": N, "d": d, "particles": P, "M": M, "steps": args.steps, "seed": args.seed,
           "trace_only": bool(args.trace_only), **stat, "ratio_to_se": ratio, "build": gpfit.build_info()}
    ctx.close()
    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
