"""Time gpf_lml_mean_batch against gpf_lml_hyper_batch, and gpf_predict_mean against gpf_predict, at one
configuration, the calls alternating in the same run.

Data and particles as scripts/hyper_lml_bench.py (bench.py's synthetic(N, d, seed) with a level of 5
added; interior particles l ~ U[0.05, 0.6]^d, a ~ U[0.5, 3], s = a U[0.7, 1.5]); the quadratic basis
(m = 10 at d = 3). Every round times the four batched legs one after the other on a fresh batch, so
clock drift falls on all four alike; then the two prediction legs at M query points, alternating. Prints
one JSON line: per leg the median, min and max ms per call over the rounds, the medians' differences
(what the mean function costs) beside the hyper call's own min-max range, the bytes the two skinny
passes move, and the library's build hash. With --trace-only the timed loop is short and unreported: the
run is for rocprofv3 --kernel-trace --stats.
Usage: python scripts/meanfn_bench.py [--n 4096] [--d 3] [--particles 64] [--steps 20] [--warmup 3] [--m-query 10000]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gaussian-process_amd"))

import numpy as np  # noqa: E402


def stats(v):
    return {"median_ms": round(float(np.median(v)), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--d", type=int, default=3)
    ap.add_argument("--particles", type=int, default=64)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--m-query", type=int, default=10000)
    ap.add_argument("--kind", default="quadratic")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--trace-only", action="store_true")
    args = ap.parse_args()
    import gpfit
    from gpfit.meanfn import basis

    N, d, P, M = args.n, args.d, args.particles, args.m_query
    rng = np.random.default_rng(args.seed)  # bench.synthetic
    x = rng.uniform(0.0, 1.0, size=(d, N))
    y = np.sum(np.sin(2 * np.pi * x), axis=0) + 0.1 * rng.standard_normal(N) + 5.0
    e = np.full(N, 0.1)
    H, box = basis(x, args.kind)
    m = H.shape[0]
    xf = rng.uniform(0.0, 1.0, size=(d, M))
    hf = basis(xf, args.kind, box)[0]
    ctx = gpfit.Context(int(os.environ.get("GPFIT_DEVICE", "0")))
    ctx.set_data(x, y, e)
    ctx.set_basis(H)
    prng = np.random.default_rng(args.seed + 1000)
    legs = {"hyper_value": lambda th: ctx.lml_hyper_batch(th, grad=False, want_q=True),
            "mean_value": lambda th: ctx.lml_mean_batch(th, grad=False, want_q=True, want_beta=True),
            "hyper_value_grad": lambda th: ctx.lml_hyper_batch(th, grad=True, want_q=True),
            "mean_value_grad": lambda th: ctx.lml_mean_batch(th, grad=True, want_q=True, want_beta=True)}
    ms = {k: [] for k in legs}
    warm, steps = (1, 2) if args.trace_only else (args.warmup, args.steps)
    for step in range(warm + steps):
        ls = prng.uniform(0.05, 0.6, size=(P, d))
        a = prng.uniform(0.5, 3.0, size=P)
        th = np.column_stack([ls, a, a * prng.uniform(0.7, 1.5, size=P)])
        for name, call in legs.items():
            ctx.synchronize()
            t0 = time.perf_counter()
            call(th)
            ctx.synchronize()
            if step >= warm:
                ms[name].append((time.perf_counter() - t0) * 1e3)
    plegs = {"predict": lambda l: ctx.predict(l, xf), "predict_mean": lambda l: ctx.predict_mean(l, xf, hf)}
    pms = {k: [] for k in plegs}
    for step in range(warm + steps):
        l = prng.uniform(0.05, 0.6, size=d)
        for name, call in plegs.items():
            ctx.synchronize()
            t0 = time.perf_counter()
            call(l)
            ctx.synchronize()
            if step >= warm:
                pms[name].append((time.perf_counter() - t0) * 1e3)
    stat = {k: stats(v) for k, v in {**ms, **pms}.items()}
    npad = (N + 127) // 128 * 128
    nt = npad // 128
    out = {"bench": "lml_mean_batch", "N": N, "d": d, "particles": P, "kind": args.kind, "m": m, "m_query": M,
           "steps": steps, "seed": args.seed, **stat,
           "value_extra_ms": round(stat["mean_value"]["median_ms"] - stat["hyper_value"]["median_ms"], 3),
           "hyper_value_range_ms": round(stat["hyper_value"]["max_ms"] - stat["hyper_value"]["min_ms"], 3),
           "value_grad_extra_ms": round(stat["mean_value_grad"]["median_ms"] - stat["hyper_value_grad"]["median_ms"], 3),
           "hyper_value_grad_range_ms": round(stat["hyper_value_grad"]["max_ms"] - stat["hyper_value_grad"]["min_ms"], 3),
           "predict_extra_ms": round(stat["predict_mean"]["median_ms"] - stat["predict"]["median_ms"], 3),
           "predict_range_ms": round(stat["predict"]["max_ms"] - stat["predict"]["min_ms"], 3),
           # the lower tiles of U, once per pass: P nt (nt + 1) / 2 tiles of 128 x 128 doubles
           "skinny_pass_bytes": P * (nt * (nt + 1) // 2) * 128 * 128 * 8,
           "build": gpfit.build_info()}
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
