"""Time gpf_predict_cov (joint posterior covariance of M query points) at one configuration, with
gpf_predict at the same M before and after it in the same run.

Data as bench.py's headline (synthetic(N, d, seed)); queries U[0, 1]^d from default_rng(seed + 2000),
l = 0.3. Every call is timed on its own (wall clock around the call, which returns after its own
copy back): the JSON line carries the median, the minimum and the maximum over the steps, so the
run-to-run spread sits beside every figure. Per-kernel times come from a child run of this script
under `rocprofv3 --kernel-trace --stats` (the library's own profile keeps k_predict_v and k_post_cov
in one class; its sum is reported next to them as a cross-check). Flops: k_predict_v as gpf_predict
counts V = U K_s; k_post_cov Npad Mpad^2 for the lower half plus Npad Mpad 128 for the diagonal tiles.

--predict-only times gpf_predict alone; with --pkg DIR (a directory holding another build's gpfit
package and libgpfit.so) it does so on that build: the A/B of gpf_predict against the parent commit.
Usage: python scripts/predict_cov_bench.py [--n 4096] [--d 3] [--m 4096] [--steps 20] [--warmup 3]
       [--seed 1] [--no-kernels] [--predict-only] [--pkg DIR] [--out profiles/predict_cov/bench.json]
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
KERNELS = ("k_predict_v", "k_post_cov", "k_mirror_lower", "k_predict_vsq", "k_cross_cov")


def stats(ms):
    ms = np.asarray(ms)
    return {"median": round(float(np.median(ms)), 3), "min": round(float(ms.min()), 3), "max": round(float(ms.max()), 3)}


def problem(args):
    rng = np.random.default_rng(args.seed)  # bench.synthetic
    x = rng.uniform(0.0, 1.0, size=(args.d, args.n))
    y = np.sum(np.sin(2 * np.pi * x), axis=0) + 0.1 * rng.standard_normal(args.n)
    e = np.full(args.n, 0.1)
    q = np.random.default_rng(args.seed + 2000).uniform(0.0, 1.0, size=(args.d, args.m))
    return x, y, e, q, np.full(args.d, 0.3)


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


def kernel_stats(args):
    """Average ns per launch of the prediction kernels from a rocprofv3 kernel trace of a child run."""
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(exe):
        return None, "rocprofv3 not found"
    with tempfile.TemporaryDirectory() as td:
        cmd = [exe, "--kernel-trace", "--stats", "-d", td, "-o", "kt", "--output-format", "csv", "--", sys.executable,
               os.path.abspath(__file__), "--child", "--n", str(args.n), "--d", str(args.d), "--m", str(args.m),
               "--steps", str(min(args.steps, 5)), "--warmup", "1", "--seed", str(args.seed), "--pkg", args.pkg]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
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
                        o = out.setdefault(k, {"calls": 0, "total_ns": 0.0})
                        o["calls"] += int(row["Calls"])
                        o["total_ns"] += float(row["TotalDurationNs"])
    return {k: {"calls": v["calls"], "avg_ms": round(v["total_ns"] / v["calls"] * 1e-6, 4)} for k, v in out.items()}, None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--d", type=int, default=3)
    ap.add_argument("--m", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--pkg", default=os.path.join(ROOT, "gaussian-process_amd"))
    ap.add_argument("--predict-only", action="store_true")
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    args.pkg = os.path.abspath(args.pkg)  # (gpfit loads the libgpfit.so that sits beside the package)

    # the traced child first: this process has not opened the device yet
    kern, why = (None, "not requested") if (args.child or args.predict_only or args.no_kernels) else kernel_stats(args)

    sys.path.insert(0, args.pkg)
    import gpfit

    x, y, e, q, ls = problem(args)
    ctx = gpfit.Context(int(os.environ.get("GPFIT_DEVICE", "0")))
    ctx.set_data(x, y, e)
    if args.child:
        timed(lambda: ctx.predict_cov(ls, q), args.steps, args.warmup, ctx)
        timed(lambda: ctx.predict(ls, q), args.steps, args.warmup, ctx)
        ctx.close()
        return

    N, d, M = args.n, args.d, args.m
    Np, Mp = -(-N // T) * T, -(-M // T) * T
    nt = Np // T
    out = {"bench": "predict_only" if args.predict_only else "predict_cov", "N": N, "d": d, "M": M, "steps": args.steps,
           "warmup": args.warmup, "seed": args.seed, "build": gpfit.build_info()}
    before = timed(lambda: ctx.predict(ls, q), args.steps, args.warmup, ctx)
    out["predict_ms_before"] = stats(before)
    if not args.predict_only:
        out["predict_cov_wall_ms"] = stats(timed(lambda: ctx.predict_cov(ls, q), args.steps, args.warmup, ctx))
        out["predict_ms_after"] = stats(timed(lambda: ctx.predict(ls, q), args.steps, args.warmup, ctx))
        v_flops = 2.0 * T * T * Mp * (nt * (nt + 1) / 2) - float(T) * T * Mp * nt
        c_flops = float(Np) * Mp * (Mp + T)
        # the library's own profile: both GEMM kernels in one class
        ctx.set_profiling(True)
        ctx.reset_profile()
        for _ in range(args.steps):
            ctx.predict_cov(ls, q)
        prof = ctx.profile()
        ctx.set_profiling(False)
        out["profile_v_plus_cov_ms_per_call"] = round(prof["predict_ms"] / args.steps, 4)
        out["profile_cross_cov_plus_mirror_ms_per_call"] = round(prof["predict_cov_ms"] / args.steps, 4)
        out["flops"] = {"k_predict_v": v_flops, "k_post_cov": c_flops}
        out["kernels"] = kern
        if kern is None:
            out["kernels_note"] = why
        else:
            for k, fl in (("k_predict_v", v_flops), ("k_post_cov", c_flops)):
                if k in kern:
                    kern[k]["tflops"] = round(fl / (kern[k]["avg_ms"] * 1e-3) / 1e12, 2)
        out["yardsticks_tflops"] = {"k_post_cov": 62.0, "k_predict_v": 66.5}
    ctx.close()
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
