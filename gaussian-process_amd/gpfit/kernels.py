"""The covariance kernel family of a context (gpf_set_kernel), in float64 NumPy: the closed forms the
tests compare the device against, and the place the formulas are written down.

With a_k = x_k / l_k and r2 = sum_k (a_ik - a_jk)^2, formed as kernel_func forms it (GP_func.py:56-63:
squared norms, one GEMM, clamp at 0),

    K_ij       = phi(r2)
    dK_ij/dl_k = psi(r2) (x_ik - x_jk)^2 / l_k^3,     psi = -2 phi'(r2)

    kind        s            phi                          psi
    se          -            exp(-r2 / 2)                 phi
    matern32    sqrt(3 r2)   (1 + s) exp(-s)              3 exp(-s)
    matern52    sqrt(5 r2)   (1 + s + s^2 / 3) exp(-s)    (5/3) (1 + s) exp(-s)

phi(0) = 1 for all three and psi is finite at 0. nu = 1/2 is left out: its psi is singular at 0.
Nothing here touches the device or loads the library.
"""
from __future__ import annotations

import numpy as np

KINDS = ("se", "matern32", "matern52")  # the index is the C-ABI's kind (GPF_KERNEL_*)


def kernel_kind(kernel):
    """The C-ABI kind (0, 1, 2) of a kernel name; ValueError naming the three for anything else."""
    if isinstance(kernel, str) and kernel in KINDS:
        return KINDS.index(kernel)
    raise ValueError(f"kernel must be one of 'se', 'matern32', 'matern52', got {kernel!r}")


def scaled_sqdist(xa, xb, l):
    """r2 (Na, Nb) of xa (d, Na) and xb (d, Nb) under the length scales l (d,), with kernel_func's
    operation order up to the clamp."""
    l = np.asarray(l, dtype=np.float64).reshape(-1)
    inv = l[:, None]
    a = np.asarray(xa, dtype=np.float64) / inv
    b = np.asarray(xb, dtype=np.float64) / inv
    na = np.sum(a ** 2, axis=0).reshape(-1, 1)
    nb = np.sum(b ** 2, axis=0).reshape(1, -1)
    r2 = na + nb - 2 * np.dot(a.T, b)
    return np.maximum(r2, 0)


def kernel_value(r2, kind="se"):
    """phi(r2), elementwise, r2 >= 0."""
    k = kernel_kind(kind)
    r2 = np.asarray(r2, dtype=np.float64)
    if k == 0:
        return np.exp(-0.5 * r2)
    if k == 1:
        s = np.sqrt(3.0 * r2)
        return (1.0 + s) * np.exp(-s)
    s = np.sqrt(5.0 * r2)
    return ((1.0 + s) + (s * s) / 3.0) * np.exp(-s)


def kernel_dweight(r2, kind="se"):
    """psi(r2) = -2 phi'(r2), elementwise, r2 >= 0: dK_ij/dl_k = psi(r2_ij) (x_ik - x_jk)^2 / l_k^3."""
    k = kernel_kind(kind)
    r2 = np.asarray(r2, dtype=np.float64)
    if k == 0:
        return np.exp(-0.5 * r2)
    if k == 1:
        return 3.0 * np.exp(-np.sqrt(3.0 * r2))
    s = np.sqrt(5.0 * r2)
    return ((5.0 / 3.0) * (1.0 + s)) * np.exp(-s)


def kernel_matrix(xa, xb, l, kind="se"):
    """K (Na, Nb) = phi(r2) of xa (d, Na) and xb (d, Nb); for "se" bitwise the reference's kernel_func."""
    return kernel_value(scaled_sqdist(xa, xb, l), kind)
