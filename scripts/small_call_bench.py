"""Host-path timing of the entry points that keep a buffer set: the wall time of one
repeated small call per entry point at N=100, d=3, M=128 (R=3 functionals, S=5 draws, P=3 particles,
a dense matrix of n=128, 128 probability-surface rows), where the kept set is hit and the host path
dominates ("kept"), and the same with GPF_PREDICT_KEEP_MB=0, where every call gives its set back and the
next one allocates it again ("regrow": the first call's path). Median, minimum and maximum over the
steps, microseconds. The library is the one GPFIT_LIB names (default: the tree's).

Usage: python scripts/small_call_bench.py [--steps 300] [--warmup 30] [--out FILE.json]
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
    ap.add_argument("--n", type=int, default=100)
    ap.add_argument("--m", type=int, default=128)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import gpfit
    rng = np.random.default_rng(1)
    n, m, d, r, s, p = args.n, args.m, 3, 3, 5, 3
    x = rng.uniform(size=(d, n))
    y = np.sum(np.sin(2 * np.pi * x), axis=0) + 0.1 * rng.standard_normal(n)
    q, ls, lsp = rng.uniform(size=(d, m)), rng.uniform(0.2, 0.5, size=d), rng.uniform(0.2, 0.5, size=(p, d))
    w, b, sv, z = rng.standard_normal((r, m)) / m, rng.standard_normal(r), np.full(r, 0.1), rng.standard_normal((s, m))
    a = rng.standard_normal((m, m))
    a = a @ a.T / m + np.eye(m)
    tails = np.empty((m, 4))
    tails[:, 0::2], tails[:, 1::2] = rng.normal(size=(m, 2)), rng.uniform(0.05, 0.5, size=(m, 2))
    ctx = gpfit.Context(int(os.environ.get("GPFIT_DEVICE", "0")))
    ctx.set_data(x, y, np.full(n, 0.1))
    calls = {
        "predict": lambda: ctx.predict(ls, q),
        "predict_cov": lambda: ctx.predict_cov(ls, q),
        "posterior_draws": lambda: ctx.posterior_draws(ls, q, z),
        "predict_linear": lambda: ctx.predict_linear(ls, q, w),
        "predict_conditioned": lambda: ctx.predict_conditioned(ls, q, w, b, sv),
        "predict_batch": lambda: ctx.predict_batch(lsp, q),
        "chol_dense": lambda: ctx.chol_dense(a),
        "prob_surface": lambda: ctx.prob_surface(tails),
    }
    out = {"bench": "small_call", "N": n, "M": m, "steps": args.steps, "warmup": args.warmup, "build": gpfit.build_info(),
           "unit": "us", "kept": {}, "regrow": {}}
    for leg, keep in (("kept", None), ("regrow", "0")):
        if keep is None:
            os.environ.pop("GPF_PREDICT_KEEP_MB", None)
        else:
            os.environ["GPF_PREDICT_KEEP_MB"] = keep
        for name, f in calls.items():
            for _ in range(args.warmup):
                f()
            t = np.empty(args.steps)
            for i in range(args.steps):
                t0 = time.perf_counter()
                f()
                t[i] = (time.perf_counter() - t0) * 1e6
            out[leg][name] = {"median": round(float(np.median(t)), 1), "min": round(float(t.min()), 1),
                              "max": round(float(t.max()), 1)}
    os.environ.pop("GPF_PREDICT_KEEP_MB", None)
    ctx.close()
    line = json.dumps(out)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
