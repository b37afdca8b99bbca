"""Time gpf_lml_hyper_batch against gpf_lml_batch at one configuration, the calls alternating in the
same run: value only and value + gradient of both.

Data and particles as bench.py's headline (synthetic(N, d, seed); interior particles
l ~ U[0.05, 0.6]^d from default_rng(seed + 1000)); the hyper call gets the same length scales with
a ~ U[0.5, 3], s = a U[0.7, 1.5]. Every round times the four legs one after the other on a fresh batch,
so clock drift falls on all four alike. Prints one JSON line: per leg the median, min and max ms per
call over the rounds, the medians' differences (what a, s and Q cost) beside lml_batch's own min-max
range, and the library's build hash.
Usage: python scripts/hyper_lml_bench.py [--n 4096] [--d 3] [--particles 64] [--steps 20] [--warmup 3] [--seed 1]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gaussian-process_amd"))

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--d", type=int, default=3)
    ap.add_argument("--particles", type=int, default=64)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    import gpfit

    N, d, P = args.n, args.d, args.particles
    rng = np.random.default_rng(args.seed)  # bench.synthetic
    x = rng.uniform(0.0, 1.0, size=(d, N))
    y = np.sum(np.sin(2 * np.pi * x), axis=0) + 0.1 * rng.standard_normal(N)
    e = np.full(N, 0.1)
    ctx = gpfit.Context(int(os.environ.get("GPFIT_DEVICE", "0")))
    ctx.set_data(x, y, e)
    prng = np.random.default_rng(args.seed + 1000)
    legs = {"lml_value": lambda ls, th: ctx.lml_batch(ls, grad=False),
            "hyper_value": lambda ls, th: ctx.lml_hyper_batch(th, grad=False, want_q=True),
            "lml_value_grad": lambda ls, th: ctx.lml_batch(ls, grad=True),
            "hyper_value_grad": lambda ls, th: ctx.lml_hyper_batch(th, grad=True, want_q=True)}
    ms = {k: [] for k in legs}
    for step in range(args.warmup + args.steps):
        ls = prng.uniform(0.05, 0.6, size=(P, d))
        a = prng.uniform(0.5, 3.0, size=P)
        th = np.column_stack([ls, a, a * prng.uniform(0.7, 1.5, size=P)])
        for name, call in legs.items():
            ctx.synchronize()
            t0 = time.perf_counter()
            call(ls, th)
            ctx.synchronize()
            if step >= args.warmup:
                ms[name].append((time.perf_counter() - t0) * 1e3)
    stat = {k: {"median_ms": round(float(np.median(v)), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}
            for k, v in ms.items()}
    out = {"bench": "lml_hyper_batch", "N": N, "d": d, "particles": P, "steps": args.steps, "seed": args.seed, **stat,
           "value_extra_ms": round(stat["hyper_value"]["median_ms"] - stat["lml_value"]["median_ms"], 3),
           "lml_value_range_ms": round(stat["lml_value"]["max_ms"] - stat["lml_value"]["min_ms"], 3),
           "value_grad_extra_ms": round(stat["hyper_value_grad"]["median_ms"] - stat["lml_value_grad"]["median_ms"], 3),
           "lml_value_grad_range_ms": round(stat["lml_value_grad"]["max_ms"] - stat["lml_value_grad"]["min_ms"], 3),
           "build": gpfit.build_info()}
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
