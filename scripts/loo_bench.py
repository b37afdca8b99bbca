"""Time gpf_loo_batch against gpf_lml_batch at one configuration, in one run, alternating the calls:
lml_batch value only and value + gradient (the yardstick), loo_batch value only and value + gradient.

Data and particles as bench.py's headline (synthetic(N, d, seed); interior particles
l ~ U[0.05, 0.6]^d from default_rng(seed + 1000), a fresh batch per round, the same batch for the
four calls of a round). Prints one JSON line and, with --out, writes it: the median and the range
(min, max) of the per-call milliseconds over the rounds (a host clock around calls that end in a
device synchronise), the gradient passes' share (the difference of the medians) and the library's
build hash. The kernels' own times (k_loo_w, k_loo_grad next to k_lml_grad) come from a kernel trace
of a short run of this script, taken in a run of its own: --trace-csv reads the trace's
kernel-stats CSV and adds the per-kernel mean times and rates (k_lml_grad and k_loo_w: P N^3 / 3
flop as the library counts them, sum over the lower tiles of 2 T^3 (nt - I); k_loo_grad:
P ntile 2 T^3 nt).
Usage: python scripts/loo_bench.py [--n 4096] [--d 3] [--particles 64] [--rounds 8] [--warmup 2] [--seed 1]
                                   [--out profiles/loo/bench.json] [--trace-csv kernel_stats.csv]
"""
import argparse
import csv
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gaussian-process_amd"))

import numpy as np  # noqa: E402

T = 128


def kernel_flops(N, P):
    nt = (N + T - 1) // T
    ntile = nt * (nt + 1) // 2
    tri = sum(2.0 * T ** 3 * (nt - i) * (i + 1) for i in range(nt))
    return {"k_lml_grad": tri * P, "k_loo_w": tri * P, "k_loo_grad": 2.0 * T ** 3 * nt * ntile * P}


def read_trace(path, N, P):
    """Per-kernel calls, mean ms and TF/s from a kernel-stats CSV (columns Name, Calls, AverageNs)."""
    fl = kernel_flops(N, P)
    out = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Name", "")
            for k in fl:
                if re.search(r"(?:^|::|\s)" + k + r"(?:\(|\.kd|<|$)", name):
                    ms = float(row["AverageNs"]) * 1e-6
                    out[k] = {"calls": int(row["Calls"]), "mean_ms": round(ms, 3),
                              "tflops": round(fl[k] / (ms * 1e-3) / 1e12, 2)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--d", type=int, default=3)
    ap.add_argument("--particles", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-csv", default=None)
    args = ap.parse_args()
    import gpfit

    N, d, P = args.n, args.d, args.particles
    rng = np.random.default_rng(args.seed)  # bench.synthetic
    x = rng.uniform(0.0, 1.0, size=(d, N))
    y = np.sum(np.sin(2 * np.pi * x), axis=0) + 0.1 * rng.standard_normal(N)
    e = np.full(N, 0.1)
    ctx = gpfit.Context(int(os.environ.get("GPFIT_DEVICE", "0")))
    ctx.set_data(x, y, e)
    legs = {"lml_value": lambda ls: ctx.lml_batch(ls, grad=False),
            "lml_value_grad": lambda ls: ctx.lml_batch(ls, grad=True),
            "loo_value": lambda ls: ctx.loo_batch(ls, grad=False),
            "loo_value_grad": lambda ls: ctx.loo_batch(ls, grad=True)}
    times = {k: [] for k in legs}
    prng = np.random.default_rng(args.seed + 1000)
    for r in range(args.warmup + args.rounds):
        ls = prng.uniform(0.05, 0.6, size=(P, d))
        for name, call in legs.items():
            ctx.synchronize()
            t0 = time.perf_counter()
            call(ls)
            ctx.synchronize()
            if r >= args.warmup:
                times[name].append((time.perf_counter() - t0) * 1e3)
    out = {"bench": "loo_batch", "N": N, "d": d, "particles": P, "rounds": args.rounds, "seed": args.seed}
    for name, t in times.items():
        out[name + "_ms"] = {"median": round(float(np.median(t)), 3), "min": round(min(t), 3), "max": round(max(t), 3)}
    med = {k: out[k + "_ms"]["median"] for k in legs}
    out["lml_grad_pass_ms"] = round(med["lml_value_grad"] - med["lml_value"], 3)
    out["loo_grad_pass_ms"] = round(med["loo_value_grad"] - med["loo_value"], 3)
    out["loo_value_over_lml_value"] = round(med["loo_value"] / med["lml_value"], 4)
    out["loo_value_grad_over_lml_value_grad"] = round(med["loo_value_grad"] / med["lml_value_grad"], 3)
    if args.trace_csv:
        out["kernels"] = read_trace(args.trace_csv, N, P)
        k = out["kernels"]
        if all(n in k for n in ("k_lml_grad", "k_loo_w", "k_loo_grad")):
            out["k_loo_w_rate_over_k_lml_grad"] = round(k["k_loo_w"]["tflops"] / k["k_lml_grad"]["tflops"], 3)
            out["k_loo_grad_rate_over_k_lml_grad"] = round(k["k_loo_grad"]["tflops"] / k["k_lml_grad"]["tflops"], 3)
    out["build"] = gpfit.build_info()
    ctx.close()
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
