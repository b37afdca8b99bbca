"""Time gpf_predict_linear (R linear functionals of the posterior over M query points, the query axis
folded away on the device) at the fixed shape N=4096, d=3, R=128:

  M = --m (4096), where both routes exist: method "stream" (Context.predict_linear) against method
      "dense" (Context.predict_cov, then gpfit.linear.functionals_from on the host) in the same run on
      the same box; the dense route runs only code the parent commit has, so it is the yardstick;
  M = --big-m (200000), which the dense route cannot do: the time per call for each --chunks value,
      the library's own profile classes, and per kernel (a child run of this script under
      `rocprofv3 --kernel-trace --stats`) the time per call of the cross-covariance builds, the two
      skinny products with their reduction and the reused kernels, with the TF/s of the products on
      their algorithmic flop: k_lin_nn 2 Npad Mpad Rpad + 2 Mpad^2 Rpad, k_lin_tn (Mpad + Npad) Rpad^2
      per lower tile pair.

Data as bench.py's headline (synthetic(N, d, seed)); queries U[0, 1]^d from default_rng(seed + 2000),
l = 0.3; weights: every row U(0.5, 1.5) on a random 30% of the points (default_rng(seed + 3000)),
normalised to sum 1. Every call is timed on its own (wall clock around the call, which returns after
its own copy back, the upload of the weights included): median, minimum and maximum over the steps.

Usage: python scripts/predict_linear_bench.py [--n 4096] [--d 3] [--r 128] [--m 4096] [--big-m 200000]
       [--chunks 0,4096] [--steps 10] [--big-steps 3] [--warmup 2] [--seed 1] [--no-kernels]
       [--out profiles/predict_linear/bench.json]
"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402

T = 128
KERNELS = ("k_lin_nn", "k_lin_tn", "k_lin_reduce", "k_lin_wt", "k_lin_unit_diag", "k_cross_cov", "k_predict_v",
           "k_predict_out", "k_mirror_lower")


def stats(ms):
    ms = np.asarray(ms)
    return {"median": round(float(np.median(ms)), 3), "min": round(float(ms.min()), 3), "max": round(float(ms.max()), 3)}


def problem(args, m):
    rng = np.random.default_rng(args.seed)  # bench.synthetic
    x = rng.uniform(0.0, 1.0, size=(args.d, args.n))
    y = np.sum(np.sin(2 * np.pi * x), axis=0) + 0.1 * rng.standard_normal(args.n)
    e = np.full(args.n, 0.1)
    q = np.random.default_rng(args.seed + 2000).uniform(0.0, 1.0, size=(args.d, m))
    wr = np.random.default_rng(args.seed + 3000)
    w = wr.uniform(0.5, 1.5, size=(args.r, m)) * (wr.random((args.r, m)) < 0.3)
    w[:, 0] += 1.0  # no empty row
    w /= w.sum(axis=1, keepdims=True)
    return x, y, e, q, np.full(args.d, 0.3), np.ascontiguousarray(w)


def timed(fn, steps, warmup, ctx):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(steps):
        ctx.synchronize()
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def kernel_stats(args, chunk, calls):
    """Per call of gpf_predict_linear at M = --big-m: launches and ms of every kernel, from a rocprofv3
    kernel trace of a child run that makes `calls` calls."""
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(exe):
        return None, "rocprofv3 not found"
    with tempfile.TemporaryDirectory() as td:
        cmd = [exe, "--kernel-trace", "--stats", "-d", td, "-o", "kt", "--output-format", "csv", "--", sys.executable,
               os.path.abspath(__file__), "--child", "--n", str(args.n), "--d", str(args.d), "--r", str(args.r),
               "--big-m", str(args.big_m), "--chunks", str(chunk), "--big-steps", str(calls), "--seed", str(args.seed)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        except subprocess.TimeoutExpired:
            return None, "the traced child run timed out"
        files = glob.glob(os.path.join(td, "**", "*kernel_stats.csv"), recursive=True)
        if r.returncode or not files:
            return None, f"rocprofv3 failed (exit {r.returncode}): {r.stderr[-300:]}"
        out = {}
        with open(files[0], newline="") as f:
            for row in csv.DictReader(f):
                for k in KERNELS:
                    if f"gpf::{k}(" in row["Name"] or f"gpf::{k}<" in row["Name"]:
                        o = out.setdefault(k, {"launches": 0, "total_ns": 0.0})
                        o["launches"] += int(row["Calls"])
                        o["total_ns"] += float(row["TotalDurationNs"])
    return {k: {"launches_per_call": v["launches"] / calls, "ms_per_call": round(v["total_ns"] / calls * 1e-6, 3)}
            for k, v in out.items()}, None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--d", type=int, default=3)
    ap.add_argument("--r", type=int, default=128)
    ap.add_argument("--m", type=int, default=4096)
    ap.add_argument("--big-m", type=int, default=200000)
    ap.add_argument("--chunks", default="0,4096", help="chunk values timed at --big-m; the first one is traced")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--big-steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    chunks = [int(v) for v in args.chunks.split(",")]

    # the traced child first: this process has not opened the device yet
    kern, why = (None, "not requested") if (args.child or args.no_kernels or args.big_m <= 0) else \
        kernel_stats(args, chunks[0], args.big_steps)

    sys.path.insert(0, os.path.join(ROOT, "gaussian-process_amd"))
    import gpfit
    from gpfit.linear import functionals_from

    ctx = gpfit.Context(int(os.environ.get("GPFIT_DEVICE", "0")))
    if args.child:
        x, y, e, q, ls, w = problem(args, args.big_m)
        ctx.set_data(x, y, e)
        for _ in range(args.big_steps):
            ctx.predict_linear(ls, q, w, chunk=chunks[0])
        ctx.close()
        return

    N, d, R = args.n, args.d, args.r
    Np, Rp = -(-N // T) * T, -(-R // T) * T
    out = {"bench": "predict_linear", "N": N, "d": d, "R": R, "steps": args.steps, "warmup": args.warmup, "seed": args.seed,
           "build": gpfit.build_info()}

    # both routes at M = --m, alternating twice
    x, y, e, q, ls, w = problem(args, args.m)
    ctx.set_data(x, y, e)
    both = {"M": args.m}
    for rnd in (1, 2):
        both[f"stream_ms_{rnd}"] = stats(timed(lambda: ctx.predict_linear(ls, q, w), args.steps, args.warmup, ctx))
        both[f"dense_ms_{rnd}"] = stats(timed(lambda: functionals_from(*ctx.predict_cov(ls, q), w), args.steps, args.warmup, ctx))
    ms, cs = ctx.predict_linear(ls, q, w)
    md, cd = functionals_from(*ctx.predict_cov(ls, q), w)
    both["max_abs_diff_stream_vs_dense"] = {"mean": float(np.max(np.abs(ms - md))), "cov": float(np.max(np.abs(cs - cd)))}
    out["both_routes"] = both

    if args.big_m > 0:
        M = args.big_m
        Mp = -(-M // T) * T
        x, y, e, q, ls, w = problem(args, M)
        ctx.set_data(x, y, e)
        big = {"M": M, "steps": args.big_steps, "weights_MB": round(w.nbytes / 1e6, 1)}
        nn_flops = 2.0 * Np * Mp * Rp + 2.0 * float(Mp) * Mp * Rp
        ntri = (Rp // T) * (Rp // T + 1) // 2
        tn_flops = 2.0 * T * T * (Mp + Np) * ntri
        for ch in chunks:
            leg = {"wall_ms": stats(timed(lambda: ctx.predict_linear(ls, q, w, chunk=ch), args.big_steps, 1, ctx))}
            ctx.set_profiling(True)
            ctx.reset_profile()
            ctx.predict_linear(ls, q, w, chunk=ch)
            prof = ctx.profile()
            ctx.set_profiling(False)
            leg["profile_products_plus_v_ms"] = round(prof["predict_ms"], 3)
            leg["profile_products_flops"] = prof["predict_flops"]
            leg["profile_cross_cov_ms"] = round(prof["predict_cov_ms"], 3)
            leg["profile_cross_cov_bytes"] = prof["predict_cov_bytes"]
            leg["profile_cross_cov_TBps"] = round(prof["predict_cov_bytes"] / (prof["predict_cov_ms"] * 1e-3) / 1e12, 2)
            big[f"chunk_{ch}"] = leg
        big["flops"] = {"k_lin_nn": nn_flops, "k_lin_tn": tn_flops}
        big["kernels_chunk"] = chunks[0]
        big["kernels"] = kern
        if kern is None:
            big["kernels_note"] = why
        else:
            for k, fl in (("k_lin_nn", nn_flops), ("k_lin_tn", tn_flops)):
                if k in kern:
                    kern[k]["tflops"] = round(fl / (kern[k]["ms_per_call"] * 1e-3) / 1e12, 2)
        big["yardstick_tflops"] = {"k_post_cov": [47.7, 57.5]}
        out["big"] = big
    ctx.close()
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
