"""Time joint posterior draws on the device (sample_posterior(method="device"): gpf_posterior_draws)
against the host path (method="host": gpf_predict_cov, the copy of Sigma, numpy.linalg.cholesky) on
the same box in the same run.

Data as bench.py's headline (synthetic(N, d, seed)); queries U[0, 1]^d from default_rng(seed + 2000),
l = 0.3, the default jitter ladder. Both methods are timed through gpfit.posterior.sample_posterior
with one seed, so each call draws its S x M normals on the host and returns after its own copy back;
the context-level calls with the normals made beforehand are timed beside them. Every call is timed
on its own: the JSON line carries the median, the minimum and the maximum over the steps.

Per-kernel times come from a child run of this script under `rocprofv3 --kernel-trace --stats`: the
average per launch of every kernel of the call, and per call the span of the dense factorisation's
chain (k_dc_init's start to the last k_dc_* kernel's end, launch gaps included) with its
TF/s on M^3 / 3 flop. The library's own profile (the prediction classes) is reported as a cross-check.

Usage: python scripts/posterior_draws_bench.py [--n 4096] [--d 3] [--m 4096] [--s 100] [--steps 10]
       [--host-steps 5] [--warmup 2] [--seed 1] [--no-kernels] [--out profiles/posterior_draws/bench.json]
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
CHAIN = ("k_dc_init", "k_dc_diag", "k_dc_finish", "k_dc_trail")
KERNELS = CHAIN + ("k_draws", "k_predict_v", "k_post_cov", "k_mirror_lower", "k_cross_cov")


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


def _which(name):
    for k in KERNELS:
        if f"gpf::{k}(" in name or f"gpf::{k}<" in name:
            return k
    return None


def kernel_stats(args):
    """Per-kernel averages and the factorisation chain's span per call, from a rocprofv3 kernel trace of
    a child run that makes only posterior_draws calls."""
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(exe):
        return None, "rocprofv3 not found"
    with tempfile.TemporaryDirectory() as td:
        cmd = [exe, "--kernel-trace", "--stats", "-d", td, "-o", "kt", "--output-format", "csv", "--", sys.executable,
               os.path.abspath(__file__), "--child", "--n", str(args.n), "--d", str(args.d), "--m", str(args.m),
               "--s", str(args.s), "--steps", str(min(args.steps, 4)), "--warmup", "1", "--seed", str(args.seed)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        except subprocess.TimeoutExpired:
            return None, "the traced child run timed out"
        files = glob.glob(os.path.join(td, "**", "*kernel_stats.csv"), recursive=True)
        if r.returncode or not files:
            return None, f"rocprofv3 failed (exit {r.returncode}): {r.stderr[-300:]}"
        per = {}
        with open(files[0], newline="") as f:
            for row in csv.DictReader(f):
                k = _which(row["Name"])
                if k:
                    o = per.setdefault(k, {"calls": 0, "total_ns": 0.0})
                    o["calls"] += int(row["Calls"])
                    o["total_ns"] += float(row["TotalDurationNs"])
        out = {"kernels": {k: {"launches": v["calls"], "avg_ms": round(v["total_ns"] / v["calls"] * 1e-6, 4),
                               "total_ms": round(v["total_ns"] * 1e-6, 3)} for k, v in per.items()}}
        # the chain's span per call from the trace itself: every call ends with its k_draws launch
        traces = glob.glob(os.path.join(td, "**", "*kernel_trace.csv"), recursive=True)
        spans, busy, launches = [], [], []
        if traces:
            rows = []
            with open(traces[0], newline="") as f:
                for row in csv.DictReader(f):
                    k = _which(row.get("Kernel_Name", ""))
                    if k in CHAIN or k == "k_draws":
                        rows.append((int(row["Start_Timestamp"]), int(row["End_Timestamp"]), k))
            rows.sort()
            cur = []
            for s, e, k in rows:
                if k == "k_draws":
                    if cur:
                        spans.append((max(c[1] for c in cur) - cur[0][0]) * 1e-6)
                        busy.append(sum(c[1] - c[0] for c in cur) * 1e-6)
                        launches.append(len(cur))
                    cur = []
                else:
                    cur.append((s, e))
        if spans:
            out["chain"] = {"calls": len(spans), "launches_per_call": int(np.median(launches)),
                            "span_ms": stats(spans), "kernel_sum_ms": stats(busy)}
    return out, None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--d", type=int, default=3)
    ap.add_argument("--m", type=int, default=4096)
    ap.add_argument("--s", type=int, default=100)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--host-steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    # the traced child first: this process has not opened the device yet
    kern, why = (None, "not requested") if (args.child or args.no_kernels) else kernel_stats(args)

    sys.path.insert(0, os.path.join(ROOT, "gaussian-process_amd"))
    import gpfit
    from gpfit.posterior import draws_from, sample_posterior

    x, y, e, q, ls = problem(args)
    z = np.random.default_rng(args.seed).standard_normal((args.s, args.m))
    ctx = gpfit.Context(int(os.environ.get("GPFIT_DEVICE", "0")))
    ctx.set_data(x, y, e)
    if args.child:
        timed(lambda: ctx.posterior_draws(ls, q, z), args.steps, args.warmup, ctx)
        ctx.close()
        return

    N, d, M, S = args.n, args.d, args.m, args.s
    Mp = -(-M // T) * T
    out = {"bench": "posterior_draws", "N": N, "d": d, "M": M, "S": S, "steps": args.steps, "host_steps": args.host_steps,
           "warmup": args.warmup, "seed": args.seed, "build": gpfit.build_info(), "cpus": len(os.sched_getaffinity(0))}
    dev = lambda: sample_posterior(x, y, e, q, ls, S, seed=args.seed, ctx=ctx, method="device")
    host = lambda: sample_posterior(x, y, e, q, ls, S, seed=args.seed, ctx=ctx, method="host")
    dd, di = dev()
    dh, hi = host()
    out["jitter"] = {"device": di["jitter"], "host": hi["jitter"]}
    out["max_abs_device_minus_host"] = float(np.max(np.abs(dd - dh)))
    out["device_wall_ms"] = stats(timed(dev, args.steps, args.warmup, ctx))
    out["host_wall_ms"] = stats(timed(host, args.host_steps, 1, ctx))
    out["host_over_device"] = round(out["host_wall_ms"]["median"] / out["device_wall_ms"]["median"], 2)
    # the same without the normals' generation: the context-level calls, and the host path's legs
    out["device_call_ms"] = stats(timed(lambda: ctx.posterior_draws(ls, q, z), args.steps, args.warmup, ctx))
    out["predict_cov_ms"] = stats(timed(lambda: ctx.predict_cov(ls, q), args.steps, args.warmup, ctx))
    mu, cov = ctx.predict_cov(ls, q)
    out["host_factor_and_product_ms"] = stats(timed(lambda: draws_from(mu, cov, z=z), args.host_steps, 1, ctx))
    out["normals_ms"] = stats(timed(lambda: np.random.default_rng(args.seed).standard_normal((S, M)), args.steps, 1, ctx))
    # the library's own profile of the device call: the prediction classes
    ctx.set_profiling(True)
    ctx.reset_profile()
    for _ in range(args.steps):
        ctx.posterior_draws(ls, q, z)
    prof = ctx.profile()
    ctx.set_profiling(False)
    out["profile_per_call"] = {"predict_ms": round(prof["predict_ms"] / args.steps, 4),
                               "predict_launches": round(prof["predict_launches"] / args.steps, 1),
                               "predict_cov_ms": round(prof["predict_cov_ms"] / args.steps, 4),
                               "predict_cov_launches": round(prof["predict_cov_launches"] / args.steps, 1)}
    out["factor_flops_M3_over_3"] = float(M) ** 3 / 3.0
    out["kernel_trace"] = kern
    if kern is None:
        out["kernel_trace_note"] = why
    elif "chain" in kern:
        ch = kern["chain"]
        ch["tflops_on_M3_over_3"] = round(out["factor_flops_M3_over_3"] / (ch["span_ms"]["median"] * 1e-3) / 1e12, 2)
        if "k_draws" in kern["kernels"]:
            kd = kern["kernels"]["k_draws"]
            kd["tflops"] = round(2.0 * T * T * T * (-(-S // T)) * (Mp // T) * (Mp // T + 1) / 2 / (kd["avg_ms"] * 1e-3) / 1e12, 2)
    ctx.close()
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
