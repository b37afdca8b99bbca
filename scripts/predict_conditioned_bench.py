"""Time gpf_predict_conditioned (the posterior at M query points conditioned on R measured linear
functionals, streamed over the query axis) at the fixed shape N=4096, d=3, R=128:

  M = --m (4096), where both routes exist: method "stream" (Context.predict_conditioned) against method
      "dense" (Context.predict_cov, then gpfit.conditioned.conditioned_from on the host);
  M = --big-m (200000), which the dense route cannot do: stream only.

The yardstick at either M is gpf_predict_linear plus gpf_predict at the same shapes in the same run on
the same box (the new call contains both: the first's whole pipeline, the second's K_s block and
V = U K_s reduction per chunk): the ratio of the conditioned call to that sum is recorded. Per kernel (a
child run of this script under `rocprofv3 --kernel-trace --stats`) the time per call and the share of
the call's kernel time of what is new: k_con_tn, the inverse (k_dc_inv_diag / _sum / _fin), k_con_out,
k_con_h and k_con_g. Their flop count is 2 Npad M Rpad + 2 M Rpad^2 against Npad^2 M for k_predict_vsq.

Data as bench.py's headline (synthetic(N, d, seed)); queries U[0, 1]^d from default_rng(seed + 2000),
l = 0.3; weights as predict_linear_bench.py's; s_r = 0.05, b = A sum sin(2 pi q) + s randn
(default_rng(seed + 4000)). Every call is timed on its own (wall clock around the call, which returns
after its own copy back, the uploads included): median, minimum and maximum over the steps.

Usage: python scripts/predict_conditioned_bench.py [--n 4096] [--d 3] [--r 128] [--m 4096] [--big-m 200000]
       [--steps 10] [--big-steps 3] [--warmup 2] [--seed 1] [--no-kernels]
       [--out profiles/predict_conditioned/bench.json]
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
NEW = ("k_con_tn", "k_dc_inv_diag", "k_dc_inv_sum", "k_dc_inv_fin", "k_con_out", "k_con_h", "k_con_g")
KERNELS = NEW + ("k_predict_vsq", "k_lin_nn", "k_lin_tn", "k_lin_reduce", "k_lin_wt", "k_lin_unit_diag", "k_cross_cov",
                 "k_predict_v", "k_predict_out", "k_mirror_lower", "k_dc_init", "k_dc_diag", "k_dc_finish", "k_dc_trail")


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
    s = np.full(args.r, 0.05)
    b = w @ np.sum(np.sin(2 * np.pi * q), axis=0) + s * np.random.default_rng(args.seed + 4000).standard_normal(args.r)
    return x, y, e, q, np.full(args.d, 0.3), np.ascontiguousarray(w), b, s


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


def kernel_stats(args, m, calls):
    """Per call of gpf_predict_conditioned at M = m: launches and ms of every kernel, from a rocprofv3
    kernel trace of a child run that makes `calls` calls (and nothing else on the device)."""
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(exe):
        return None, "rocprofv3 not found"
    with tempfile.TemporaryDirectory() as td:
        cmd = [exe, "--kernel-trace", "--stats", "-d", td, "-o", "kt", "--output-format", "csv", "--", sys.executable,
               os.path.abspath(__file__), "--child", "--n", str(args.n), "--d", str(args.d), "--r", str(args.r),
               "--big-m", str(m), "--big-steps", str(calls), "--seed", str(args.seed)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        except subprocess.TimeoutExpired:
            return None, "the traced child run timed out"
        files = glob.glob(os.path.join(td, "**", "*kernel_stats.csv"), recursive=True)
        if r.returncode or not files:
            return None, f"rocprofv3 failed (exit {r.returncode}): {r.stderr[-300:]}"
        out, total = {}, 0.0
        with open(files[0], newline="") as f:
            for row in csv.DictReader(f):
                total += float(row["TotalDurationNs"])
                for k in KERNELS:
                    if f"gpf::{k}(" in row["Name"] or f"gpf::{k}<" in row["Name"]:
                        o = out.setdefault(k, {"launches": 0, "total_ns": 0.0})
                        o["launches"] += int(row["Calls"])
                        o["total_ns"] += float(row["TotalDurationNs"])
    res = {k: {"launches_per_call": v["launches"] / calls, "ms_per_call": round(v["total_ns"] / calls * 1e-6, 3),
               "share_of_kernel_time": round(v["total_ns"] / total, 4)} for k, v in out.items()}
    res["all_kernels_ms_per_call"] = round(total / calls * 1e-6, 3)
    share = lambda ks: round(sum(out[k]["total_ns"] for k in ks if k in out) / total, 4)  # noqa: E731
    res["share"] = {"k_con_tn": share(("k_con_tn",)), "inverse": share(("k_dc_inv_diag", "k_dc_inv_sum", "k_dc_inv_fin")),
                    "k_con_out": share(("k_con_out",)), "all_new": share(NEW)}
    return res, None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--d", type=int, default=3)
    ap.add_argument("--r", type=int, default=128)
    ap.add_argument("--m", type=int, default=4096)
    ap.add_argument("--big-m", type=int, default=200000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--big-steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    # the traced children first: this process has not opened the device yet
    kern = {}
    if not (args.child or args.no_kernels):
        for m in (args.m, args.big_m):
            if m > 0:
                k, why = kernel_stats(args, m, args.big_steps)
                kern[m] = k if k is not None else {"note": why}

    sys.path.insert(0, os.path.join(ROOT, "gaussian-process_amd"))
    import gpfit
    from gpfit.conditioned import conditioned_from

    ctx = gpfit.Context(int(os.environ.get("GPFIT_DEVICE", "0")))
    if args.child:
        x, y, e, q, ls, w, b, s = problem(args, args.big_m)
        ctx.set_data(x, y, e)
        for _ in range(args.big_steps):
            ctx.predict_conditioned(ls, q, w, b, s)
        ctx.close()
        return

    N, d, R = args.n, args.d, args.r
    Np, Rp = -(-N // T) * T, -(-R // T) * T
    out = {"bench": "predict_conditioned", "N": N, "d": d, "R": R, "steps": args.steps, "warmup": args.warmup,
           "seed": args.seed, "build": gpfit.build_info()}

    def dense(ls, q, w, b, s):
        mu, cov, info = conditioned_from(*ctx.predict_cov(ls, q), w, b, s)
        return mu, np.sqrt(np.maximum(np.diag(cov), 1e-12)), info

    for name, m, steps, with_dense in (("both_routes", args.m, args.steps, True), ("big", args.big_m, args.big_steps, False)):
        if m <= 0:
            continue
        x, y, e, q, ls, w, b, s = problem(args, m)
        ctx.set_data(x, y, e)
        leg = {"M": m, "steps": steps}
        for rnd in (1, 2):  # alternating twice
            leg[f"conditioned_ms_{rnd}"] = stats(timed(lambda: ctx.predict_conditioned(ls, q, w, b, s), steps, args.warmup, ctx))
            leg[f"predict_linear_ms_{rnd}"] = stats(timed(lambda: ctx.predict_linear(ls, q, w), steps, args.warmup, ctx))
            leg[f"predict_ms_{rnd}"] = stats(timed(lambda: ctx.predict(ls, q), steps, args.warmup, ctx))
            if with_dense:
                leg[f"dense_ms_{rnd}"] = stats(timed(lambda: dense(ls, q, w, b, s), steps, args.warmup, ctx))
            leg[f"ratio_to_linear_plus_predict_{rnd}"] = round(
                leg[f"conditioned_ms_{rnd}"]["median"] / (leg[f"predict_linear_ms_{rnd}"]["median"] + leg[f"predict_ms_{rnd}"]["median"]), 3)
        mu, sd, info = ctx.predict_conditioned(ls, q, w, b, s)
        leg["chi2"] = info["chi2"]
        if with_dense:
            md, sdd, info_d = dense(ls, q, w, b, s)
            leg["max_abs_diff_stream_vs_dense"] = {"mean": float(np.max(np.abs(mu - md))), "var": float(np.max(np.abs(sd * sd - sdd * sdd))),
                                                   "chi2": abs(info["chi2"] - info_d["chi2"])}
        Mp = -(-m // T) * T
        leg["flops"] = {"new_products": 2.0 * Np * Mp * Rp + 2.0 * Mp * Rp * Rp, "k_predict_vsq": float(Np) * Np * Mp}
        leg["kernels"] = kern.get(m)
        out[name] = leg
    ctx.close()
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
