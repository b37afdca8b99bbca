"""The np.longdouble leave-one-out reference of the GPU tests' large case (tests/test_loo_gpu.py:
N = 1100, d = 3, 6 particles on tests/test_lml_grad_gpu.py's recipe), which takes too long to compute
inside a test (about 15 s per particle on one core):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_loo_golden.py

writes tests/golden/loo_longdouble.npz: arrays only. mu, sd (P, N), lpd (P,) and grad (P, d) are
tests/test_loo_host.py's loo_longdouble rounded to float64; ls (P, d) are the particles and sha256 the
hash of the inputs the test regenerates; gap64 (P,) is the float64 closed form's gradient error
against the longdouble one, max_k |g64 - g| / max_k |g| per particle, which sets the GPU test's
gradient tolerance, and gap64_points (3,) the largest float64 errors of mu, sd and lpd (for the record).
Pure NumPy: nothing but this repository's tests is read.
"""
import sys
import time
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))

import conftest  # noqa: E402,F401  (the BLAS thread pins and the import paths of the tests)
import numpy as np  # noqa: E402

from test_lml_grad_gpu import _recipe  # noqa: E402
from test_loo_host import gradient_gap, loo_closed_form, loo_longdouble  # noqa: E402

N, D, P = 1100, 3, 6


def main():
    x, y, e, ls = _recipe(N, D, P=P)
    mu, sd, lpd, grad, gap = [], [], [], [], []
    pts = np.zeros(3)
    for p, l in enumerate(ls):
        t0 = time.time()
        m, s, v, g = loo_longdouble(x, y, e, l)
        m64, s64, v64, g64 = loo_closed_form(x, y, e, l)
        gap.append(gradient_gap(g64, g))
        pts = np.maximum(pts, [float(np.max(np.abs(m64 - m)) / np.max(np.abs(m))), float(np.max(np.abs(s64 - s) / s)),
                               float(abs(v64 - v) / abs(v))])
        mu.append(m.astype(np.float64))
        sd.append(s.astype(np.float64))
        lpd.append(np.float64(v))
        grad.append(g.astype(np.float64))
        print(f"particle {p}: lpd {float(v):.6f}, float64 gradient gap {gap[-1]:.3e}, {time.time() - t0:.1f} s", flush=True)
    np.savez(HERE / "loo_longdouble.npz", ls=ls, mu=np.array(mu), sd=np.array(sd), lpd=np.array(lpd), grad=np.array(grad),
             gap64=np.array(gap), gap64_points=pts, sha256=np.array(conftest.data_sha256(x, y, e, ls)))
    print(f"float64 vs longdouble: mu {pts[0]:.3e}, sd {pts[1]:.3e}, lpd {pts[2]:.3e}, gradient {max(gap):.3e}")


if __name__ == "__main__":
    main()
