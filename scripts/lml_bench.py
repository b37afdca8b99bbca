"""Time gpf_lml_batch at one configuration: value only (the factorisation and the small value
kernels) against value + gradient (the same plus k_lml_grad), in the same run.

Data and particles as bench.py's headline (synthetic(N, d, seed); interior particles
l ~ U[0.05, 0.6]^d from default_rng(seed + 1000), a fresh batch per step). Prints one JSON line:
ms per step of both, the gradient pass's ms (the difference) and its TF/s (P N^3 / 3 flop), the
ratio, and the library's build hash.
Usage: python scripts/lml_bench.py [--n 4096] [--d 3] [--particles 64] [--steps 20] [--warmup 3] [--seed 1]
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

    def timed(grad):
        prng = np.random.default_rng(args.seed + 1000)
        for _ in range(args.warmup):
            ctx.lml_batch(prng.uniform(0.05, 0.6, size=(P, d)), grad=grad)
        ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            ctx.lml_batch(prng.uniform(0.05, 0.6, size=(P, d)), grad=grad)
        ctx.synchronize()
        return (time.perf_counter() - t0) * 1e3 / args.steps

    value_ms = timed(False)
    both_ms = timed(True)
    value_ms2 = timed(False)  # again after the gradient leg (reported only: it brackets clock drift)
    grad_ms = both_ms - value_ms
    out = {"bench": "lml_batch", "N": N, "d": d, "particles": P, "steps": args.steps, "seed": args.seed,
           "value_ms_per_step": round(value_ms, 3), "value_ms_per_step_after": round(value_ms2, 3),
           "value_grad_ms_per_step": round(both_ms, 3), "grad_pass_ms": round(grad_ms, 3),
           "grad_pass_tflops": round(P * float(N) ** 3 / 3.0 / (grad_ms * 1e-3) / 1e12, 2) if grad_ms > 0 else None,
           "ratio_value_grad_over_value": round(both_ms / value_ms, 3),
           "target_ratio": 2.1, "build": gpfit.build_info()}
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
