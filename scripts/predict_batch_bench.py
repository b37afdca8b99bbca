"""Time gpf_predict_batch (prediction at P length-scale samples in one batched call, the mixture
reduced on the device) against the route it replaces, a loop of P Context.predict calls plus
gpfit.hyper.mixture_from, in the same run on the same box, at the shapes

  (N=4096, d=3, P=64, M=10000), (N=4096, d=3, P=64, M=1024), (N=100, d=3, P=64, M=10000).

Per shape, in two alternating rounds: the batched call under both dispatch orders of
k_predict_vsq_batch (GPF_PREDBATCH_ORDER=0: one particle after the other; 1: the deepest row tiles of
all particles first; where M > 2048 also with one pass over all query points, chunk=16384 with the
buffers kept) and both builders of the K_s blocks (GPF_PREDBATCH_KS=0: k_cross_cov once per
particle; 1: k_cross_cov_batch once per pass), the loop, and for information the batched call with its buffers kept between
calls whatever their size (GPF_PREDICT_KEEP_MB=65536), at chunk=16384 (one pass where M allows; above the
default limit the buffers are then freed after every call) and at chunk=1024. Every call is timed on its own (wall clock around
the call, which returns after its own copy back): median, minimum and maximum over the steps. The bar:
the batched call's median must not exceed the loop's median by more than the loop's own range
(max - min over its steps).

Kernel rate (a child run of this script under `rocprofv3 --kernel-trace`): TF/s of every k_predict_vsq
launch of the loop and of every k_predict_vsq_batch launch under either order, algorithmic flops as the
library's profile counts them (2 T^2 Cm nt (nt + 1) / 2 - T^2 Cm nt per particle).

Data as bench.py's headline (synthetic(N, d, seed)); queries U[0, 1]^d from default_rng(seed + 2000);
length scales U[0.2, 0.5]^d from default_rng(seed + 5000), equal weights.

Usage: python scripts/predict_batch_bench.py [--steps 5] [--warmup 1] [--seed 1] [--no-kernels]
       [--shapes 4096,3,64,10000 4096,3,64,1024 100,3,64,10000] [--out profiles/predict_batch/bench.json]
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
SHAPES = ("4096,3,64,10000", "4096,3,64,1024", "100,3,64,10000")


def stats(v):
    v = np.asarray(v)
    return {"median": round(float(np.median(v)), 3), "min": round(float(v.min()), 3), "max": round(float(v.max()), 3)}


def problem(n, d, p, m, seed):
    rng = np.random.default_rng(seed)  # bench.synthetic
    x = rng.uniform(0.0, 1.0, size=(d, n))
    y = np.sum(np.sin(2 * np.pi * x), axis=0) + 0.1 * rng.standard_normal(n)
    e = np.full(n, 0.1)
    q = np.random.default_rng(seed + 2000).uniform(0.0, 1.0, size=(d, m))
    ls = np.random.default_rng(seed + 5000).uniform(0.2, 0.5, size=(p, d))
    return x, y, e, q, ls


def vsq_flops(n, m):
    nt, cm = -(-n // T), -(-m // T) * T
    return 2.0 * T * T * cm * (nt * (nt + 1) / 2) - float(T) * T * cm * nt


def timed(fn, steps, warmup, ctx, env=None):
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})  # the library reads its knobs per call
    try:
        for _ in range(warmup):
            fn()
        out = []
        for _ in range(steps):
            ctx.synchronize()
            t0 = time.perf_counter()
            fn()
            out.append((time.perf_counter() - t0) * 1e3)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return out


def loop_route(ctx, ls, q):
    from gpfit.hyper import mixture_from
    each = [ctx.predict(l, q) for l in ls]
    return mixture_from(np.stack([m for m, _ in each]), np.stack([s for _, s in each]))


def child(args, shape):
    """The traced run: `steps` loops, then `steps` batched calls under order 0, then under order 1."""
    import gpfit
    n, d, p, m = shape
    x, y, e, q, ls = problem(n, d, p, m, args.seed)
    ctx = gpfit.Context(int(os.environ.get("GPFIT_DEVICE", "0")))
    ctx.set_data(x, y, e)
    for _ in range(args.steps):
        for l in ls:
            ctx.predict(l, q)
    if args.wide:  # one pass over all query points, its buffers kept between the calls
        os.environ["GPF_PREDICT_KEEP_MB"] = "65536"
    for order in ("0", "1"):
        os.environ["GPF_PREDBATCH_ORDER"] = order
        for _ in range(args.steps):
            ctx.predict_batch(ls, q, chunk=16384 if args.wide else 0)
    ctx.close()


def kernel_rates(args, shape, wide=False):
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(exe):
        return {"note": "rocprofv3 not found"}
    n, d, p, m = shape
    with tempfile.TemporaryDirectory() as td:
        cmd = [exe, "--kernel-trace", "-d", td, "-o", "kt", "--output-format", "csv", "--", sys.executable,
               os.path.abspath(__file__), "--child", "--shapes", ",".join(map(str, shape)), "--steps", str(args.steps),
               "--seed", str(args.seed)] + (["--wide"] if wide else [])
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        except subprocess.TimeoutExpired:
            return {"note": "the traced child run timed out"}
        files = glob.glob(os.path.join(td, "**", "*kernel_trace.csv"), recursive=True)
        if r.returncode or not files:
            return {"note": f"rocprofv3 failed (exit {r.returncode}): {r.stderr[-300:]}"}
        single, batch = [], []
        with open(files[0], newline="") as f:
            for row in csv.DictReader(f):
                name = row["Kernel_Name"]
                ns = float(row["End_Timestamp"]) - float(row["Start_Timestamp"])
                if "k_predict_vsq_batch" in name:
                    batch.append((float(row["Start_Timestamp"]), ns))
                elif "k_predict_vsq" in name:
                    single.append(ns)
    fl = vsq_flops(n, m)
    out = {"flops_per_particle": fl, "k_predict_vsq": {"launches": len(single)}}
    if single:
        out["k_predict_vsq"].update(tflops=stats([fl / ns * 1e-3 for ns in single]), ms=stats([ns * 1e-6 for ns in single]))
    batch.sort()
    npass, rest = divmod(len(batch), 2 * args.steps)
    if rest or not npass:
        out["k_predict_vsq_batch"] = {"launches": len(batch), "note": "not a whole number of launches per call"}
        return out
    # a call's launches (one per pass over the query chunks) together: their column counts add up to Mpad
    for i, key in enumerate(("k_predict_vsq_batch_order0", "k_predict_vsq_batch_order1")):
        part = [ns for _, ns in batch[i * args.steps * npass:(i + 1) * args.steps * npass]]
        calls = [sum(part[j * npass:(j + 1) * npass]) for j in range(args.steps)]
        out[key] = {"launches_per_call": npass, "tflops": stats([fl * p / ns * 1e-3 for ns in calls]),
                    "ms_per_call": stats([ns * 1e-6 for ns in calls])}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES), help="N,d,P,M")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--wide", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    shapes = [tuple(int(v) for v in s.split(",")) for s in args.shapes]
    sys.path.insert(0, os.path.join(ROOT, "gaussian-process_amd"))
    if args.child:
        child(args, shapes[0])
        return

    # the traced children first: this process has not opened the device yet
    kern = {}
    if not args.no_kernels:
        for shape in shapes:
            kern[shape] = kernel_rates(args, shape)
            if shape[3] > 2048:  # the same with one pass over all query points (chunk=16384, buffers kept)
                kern[shape]["one_pass"] = kernel_rates(args, shape, wide=True)

    import gpfit
    ctx = gpfit.Context(int(os.environ.get("GPFIT_DEVICE", "0")))
    out = {"bench": "predict_batch", "steps": args.steps, "warmup": args.warmup, "seed": args.seed,
           "build": gpfit.build_info(), "shapes": []}
    for shape in shapes:
        n, d, p, m = shape
        x, y, e, q, ls = problem(n, d, p, m, args.seed)
        ctx.set_data(x, y, e)
        leg = {"N": n, "d": d, "P": p, "M": m}
        batch = lambda **kw: ctx.predict_batch(ls, q, **kw)  # noqa: E731
        for rnd in (1, 2):
            for order in ("0", "1"):
                leg[f"batch_order{order}_ms_{rnd}"] = stats(timed(batch, args.steps, args.warmup, ctx, {"GPF_PREDBATCH_ORDER": order}))
            if m > 2048:  # the orders again with one pass over all query points (chunk=16384), the buffers kept
                for order in ("0", "1"):
                    leg[f"batch_one_pass_order{order}_ms_{rnd}"] = stats(timed(
                        lambda: batch(chunk=16384), args.steps, args.warmup, ctx,
                        {"GPF_PREDBATCH_ORDER": order, "GPF_PREDICT_KEEP_MB": "65536"}))
            for ks in ("0", "1"):  # the K_s blocks: k_cross_cov once per particle / k_cross_cov_batch once per pass
                leg[f"batch_ks{ks}_ms_{rnd}"] = stats(timed(batch, args.steps, args.warmup, ctx, {"GPF_PREDBATCH_KS": ks}))
            leg[f"loop_ms_{rnd}"] = stats(timed(lambda: loop_route(ctx, ls, q), args.steps, args.warmup, ctx))
            leg[f"batch_default_ms_{rnd}"] = stats(timed(batch, args.steps, args.warmup, ctx))
            lo = leg[f"loop_ms_{rnd}"]
            leg[f"ratio_loop_over_batch_{rnd}"] = round(lo["median"] / leg[f"batch_default_ms_{rnd}"]["median"], 3)
            leg[f"within_bar_{rnd}"] = bool(leg[f"batch_default_ms_{rnd}"]["median"] <= lo["median"] + (lo["max"] - lo["min"]))
        leg["batch_kept_buffers_ms"] = stats(timed(batch, args.steps, args.warmup, ctx, {"GPF_PREDICT_KEEP_MB": "65536"}))
        leg["batch_chunk16384_ms"] = stats(timed(lambda: batch(chunk=16384), args.steps, args.warmup, ctx))
        leg["batch_chunk1024_ms"] = stats(timed(lambda: batch(chunk=1024), args.steps, args.warmup, ctx))
        for ks in ("0", "1"):  # the library's own event timing of one call (the K_s entry spans all its launches)
            os.environ["GPF_PREDBATCH_KS"] = ks
            ctx.set_profiling(True)
            ctx.reset_profile()
            batch()
            prof = ctx.profile()
            ctx.set_profiling(False)
            os.environ.pop("GPF_PREDBATCH_KS")
            leg[f"profile_ks{ks}"] = {k: round(prof[k], 4) for k in ("factor_wall_ms", "predict_ms", "predict_launches", "predict_cov_ms",
                                                                     "predict_cov_launches", "loss_ms")}
        mu_b, sd_b, _ = batch()
        mu_l, sd_l = loop_route(ctx, ls, q)
        leg["max_abs_diff_batch_vs_loop"] = {"mix_mu": float(np.max(np.abs(mu_b - mu_l))), "mix_sd": float(np.max(np.abs(sd_b - sd_l)))}
        leg["kernels"] = kern.get(shape)
        out["shapes"].append(leg)
    ctx.close()
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
