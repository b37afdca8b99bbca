"""A polynomial mean function with its coefficients integrated out (Rasmussen & Williams 2.7).

Every other module has prior mean zero: away from the data the fit returns to 0, and a zero-mean fit
of data with a level or a trend explains them with correlation (length scales too long, the amplitude
too large). Here

  f(x) = h(x)^T beta + g(x),   g ~ GP(0, a^2 K(l)),   y = f + noise,  noise_i ~ N(0, s^2 e_i^2),

h(x) a few fixed basis functions (``basis``: constant, linear or quadratic in coordinates mapped to
[-1, 1] by the training box; or any H (m, N) of the caller's, m <= 32) and beta integrated out under a
flat prior. theta = (l_1 .. l_d, a, s) as in gpfit.amplitude. With Kn = a^2 K + s^2 diag(e^2),
A = H Kn^-1 H^T and P = Kn^-1 - Kn^-1 H^T A^-1 H Kn^-1 the marginal likelihood is the restricted
likelihood (REML, R&W eq. 2.45)

  LML = -1/2 y^T P y - 1/2 log|Kn| - 1/2 log|A| - (N - m)/2 log(2 pi),
  dLML/dtheta = 1/2 ap^T (dKn/dtheta) ap - 1/2 tr(P dKn/dtheta),   ap = P y,

beta = A^-1 H Kn^-1 y with cov(beta) = A^-1, and at a query point with k the cross-covariance, h its
basis and R = h - H Kn^-1 k (R&W eq. 2.41-2.42)

  mu = k^T ap + h^T beta,   var = (a^2 - k^T Kn^-1 k) + R^T A^-1 R.

``Context.lml_mean_batch`` / ``Context.predict_mean`` (gpf_lml_mean_batch, gpf_predict_mean) compute
these on the device from the factorisation of the unit-amplitude Kt = Kn / a^2; ``mean_closed_form``
and ``predict_mean_closed_form`` are the float64 NumPy yardstick, straight from Kn. For fixed l and
s / a the likelihood is maximal at a^2 = Q' / (N - m), Q' = a^2 y^T P y: ``fit_mean`` is
gpfit.amplitude.fit_hyper with that.

Not built: the mean function in predict_cov, the posterior draws, predict_linear, predict_conditioned,
predict_batch, gpfit.hyper.sample_hyper and leave-one-out; the m dot products Z^T V folded into the
variance kernel's register reduction (it would save the prediction's K_s^T Bt^T pass); bases other
than the polynomial ones beyond an H of the caller's own.
"""
from __future__ import annotations

import numpy as np

from ._lib import MEAN_MAX, default_context, use_kernel
from .amplitude import _fit_theta, scaled_data
from .kernels import kernel_kind
from .mle import NUM_POLISH, NUM_STARTS
from .swarm import MAX_POINTS

KINDS = ("constant", "linear", "quadratic")
LOG_2PI = 1.8378770664093453


def basis_rows(kind, d):
    """Rows of the polynomial basis ``kind`` in d coordinates: 1, 1 + d, 1 + d + d (d + 1) / 2."""
    if kind not in KINDS:
        raise ValueError(f"mean function kind must be one of {', '.join(KINDS)}, got {kind!r}")
    return {"constant": 1, "linear": 1 + d, "quadratic": 1 + d + d * (d + 1) // 2}[kind]


def basis(x, kind, box=None):
    """(H (m, M), box): the polynomial basis ``kind`` at the points x (d, M) in the coordinates
    u = 2 (x - lo) / (hi - lo) - 1 of ``box`` = (lo (d,), hi (d,)) (None: the box of x itself, the
    training points; pass the returned box for the query points so that they use the same map; a
    coordinate without spread maps to 0). Rows: 1; then u_1 .. u_d; then u_i u_j for i <= j. ValueError
    when the basis has more than 32 rows."""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim != 2:
        raise ValueError("x must be (d, M)")
    d = x.shape[0]
    m = basis_rows(kind, d)
    if m > MEAN_MAX:
        raise ValueError(f"the {kind} basis in d = {d} has {m} rows, more than {MEAN_MAX}")
    if box is None:
        box = (np.min(x, axis=1), np.max(x, axis=1))
    lo, hi = (np.asarray(b, dtype=np.float64).reshape(-1) for b in box)
    if lo.shape != (d,) or hi.shape != (d,):
        raise ValueError(f"box must be (lo ({d},), hi ({d},))")
    span = hi - lo
    u = np.where(span[:, None] > 0, 2.0 * (x - lo[:, None]) / np.where(span > 0, span, 1.0)[:, None] - 1.0, 0.0)
    rows = [np.ones(x.shape[1])]
    if kind != "constant":
        rows += list(u)
    if kind == "quadratic":
        rows += [u[i] * u[j] for i in range(d) for j in range(i, d)]
    return np.array(rows), (lo, hi)


def _se_kernel(xa, xb, l):
    """GP_func.kernel_func: the ARD squared-exponential between the columns of xa (d, Na) and xb (d, Nb)."""
    a, b = xa / l[:, None], xb / l[:, None]
    sq = np.sum(a ** 2, axis=0)[:, None] + np.sum(b ** 2, axis=0)[None, :] - 2.0 * (a.T @ b)
    return np.exp(-0.5 * np.maximum(sq, 0.0))


def chol_small(A):
    """Lower Cholesky factor of a small symmetric matrix in the dtype of A (LAPACK has no long double);
    LinAlgError when a pivot is not > 0."""
    m = A.shape[0]
    L = np.zeros_like(A)
    for j in range(m):
        piv = A[j, j] - L[j, :j] @ L[j, :j]
        if not piv > 0:
            raise np.linalg.LinAlgError("H Kn^-1 H^T is not positive definite")
        L[j, j] = np.sqrt(piv)
        L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def tri_inverse(L):
    """L^-1 of a small lower-triangular L, row by row, in the dtype of L."""
    m = L.shape[0]
    X = np.zeros_like(L)
    for i in range(m):
        row = -(L[i, :i] @ X[:i, :])
        row[i] += 1
        X[i] = row / L[i, i]
    return X


def reml_from(W, logdet_half, K, x, y, e, H, theta):
    """(lml, grad (d + 2,), beta (m,), Q') from W = Kn^-1, sum log L_ii of Kn's factor and the noise-free
    K, in the dtype of W (the tests run it in np.longdouble too): the module docstring's formulas,
    dKn/dl_k = a^2 K o D_k / l_k^3 (D_k the squared coordinate differences), dKn/da = 2 a K,
    dKn/ds = 2 s diag(e^2)."""
    d = len(theta) - 2
    l, a, s = theta[:d], theta[d], theta[d + 1]
    N, m = len(y), H.shape[0]
    half = W.dtype.type(0.5)
    WH = W @ H.T
    La = chol_small(H @ WH)
    Ai = tri_inverse(La)
    Ainv = Ai.T @ Ai
    beta = Ainv @ (WH.T @ y)
    P = W - WH @ Ainv @ WH.T
    ap = P @ y
    ypy = y @ ap
    lml = -half * ypy - logdet_half - np.sum(np.log(np.diag(La))) - half * (N - m) * W.dtype.type(LOG_2PI)
    M = np.outer(ap, ap) - P
    MK = M * K
    g_l = [half * a * a * np.sum(MK * (x[k][:, None] - x[k][None, :]) ** 2) / l[k] ** 3 for k in range(d)]
    g_a = a * np.sum(MK)
    g_s = s * np.sum(np.diag(M) * e ** 2)
    return lml, np.array(g_l + [g_a, g_s]), beta, a * a * ypy


def _checked(x, y, e, H, theta):
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    e = np.asarray(e, dtype=np.float64).reshape(-1)
    H = np.atleast_2d(np.asarray(H, dtype=np.float64))
    theta = np.asarray(theta, dtype=np.float64).reshape(-1)
    if x.ndim != 2 or theta.shape[0] != x.shape[0] + 2:
        raise ValueError("theta must be (d + 2,): the length scales, then a and s")
    if H.shape[1] != y.shape[0] or not 1 <= H.shape[0] < y.shape[0]:
        raise ValueError("H must be (m, N) with 1 <= m < N")
    return x, y, e, H, theta


def mean_closed_form(x, y, e, H, theta):
    """(LML, dLML/dtheta (d + 2,), beta (m,), Q') in float64 NumPy, straight from
    Kn = a^2 K(l) + s^2 diag(e^2) by R&W eq. 2.45 (``reml_from``): the yardstick of gpf_lml_mean_batch.
    It never forms the unit-amplitude matrix, the orthonormalised Zo or the residual the device uses.
    LinAlgError when Kn or H Kn^-1 H^T is not positive definite."""
    x, y, e, H, theta = _checked(x, y, e, H, theta)
    d = x.shape[0]
    K = _se_kernel(x, x, theta[:d])
    Kn = theta[d] ** 2 * K + theta[d + 1] ** 2 * np.diag(e ** 2)
    L = np.linalg.cholesky(Kn)
    return reml_from(np.linalg.inv(Kn), np.sum(np.log(np.diag(L))), K, x, y, e, H, theta)


def predict_mean_closed_form(x, y, e, H, theta, x_fit, h_fit):
    """(mu (M,), sd (M,), beta (m,), cov(beta) (m, m)) at x_fit (d, M) with the basis h_fit (m, M) there,
    in float64 NumPy from Kn by R&W eq. 2.41-2.42 (sd: of the latent f; the GP part of the variance
    clipped at 1e-12 a^2 as GP's is)."""
    x, y, e, H, theta = _checked(x, y, e, H, theta)
    d = x.shape[0]
    a, s = theta[d], theta[d + 1]
    x_fit = np.asarray(x_fit, dtype=np.float64)
    h_fit = np.atleast_2d(np.asarray(h_fit, dtype=np.float64))
    Kn = a ** 2 * _se_kernel(x, x, theta[:d]) + s ** 2 * np.diag(e ** 2)
    ks = a ** 2 * _se_kernel(x, x_fit, theta[:d])
    L = np.linalg.cholesky(Kn)
    W = np.linalg.inv(Kn)
    WH = W @ H.T
    Ainv = np.linalg.inv(H @ WH)
    Ainv = 0.5 * (Ainv + Ainv.T)
    beta = Ainv @ (WH.T @ y)
    mu = ks.T @ (W @ (y - H.T @ beta)) + h_fit.T @ beta
    R = h_fit - WH.T @ ks
    v = np.linalg.solve(L, ks)  # GP_func.GP's variance: a^2 - sum v^2, v = L^-1 k
    var = np.maximum(a ** 2 - np.sum(v ** 2, axis=0), 1e-12 * a ** 2) + np.sum(R * (Ainv @ R), axis=0)
    return mu, np.sqrt(var), beta, Ainv


def predict_mean(x, y, e, x_fit, theta, kind="constant", ctx=None, want_beta=False, kernel="se"):
    """GP mean and sd at x_fit (d, M) under theta = (l_1 .. l_d, a, s) with the marginalised polynomial
    mean ``kind``: (mu (M,), sd (M,)), a times the unit model's gpf_predict_mean on ``scaled_data``; with
    want_beta also (beta (m,), cov(beta) (m, m)) in the data's units.
    ``kernel``: the covariance kernel, "se" (default), "matern32" or "matern52" (gpfit.kernels), set on the context on every call."""
    kernel_kind(kernel)
    x = np.asarray(x, dtype=np.float64)
    theta = np.asarray(theta, dtype=np.float64).reshape(-1)
    if x.ndim != 2 or theta.shape[0] != x.shape[0] + 2:
        raise ValueError(f"theta must be ({x.shape[0] + 2},): the length scales, then a and s")
    x_fit = np.asarray(x_fit, dtype=np.float64)
    if x_fit.ndim != 2 or x_fit.shape[0] != x.shape[0]:
        raise ValueError(f"x_fit must be ({x.shape[0]}, M)")
    a, s = theta[-2], theta[-1]
    ys, es = scaled_data(y, e, a, s)
    H, box = basis(x, kind)
    h_fit, _ = basis(x_fit, kind, box)
    if ctx is None:
        ctx = default_context()
    ctx.set_data(x, ys, es)
    use_kernel(ctx, kernel)
    ctx.set_basis(H)
    out = ctx.predict_mean(theta[:-2], x_fit, h_fit, want_beta=want_beta)
    if want_beta:
        return out[0] * a, out[1] * a, out[2] * a, out[3] * (a * a)
    return out[0] * a, out[1] * a


def fit_mean(x, y, e, *, kind="constant", full=True, num_starts=NUM_STARTS, num_polish=NUM_POLISH,
             max_points=MAX_POINTS, seed=None, value_and_grad=None, ctx=None, verbose=True, kernel="se"):
    """theta = (l_1 .. l_d, a, s) that maximises the restricted log marginal likelihood under the
    marginalised polynomial mean ``kind``: (theta (d + 2,), info). gpfit.amplitude.fit_hyper's
    signature, stages and info (the same driver), with the best amplitude of a start a = sqrt(Q' / (N - m)),
    and info["beta"] (m,): the coefficients at theta, in the basis of ``basis(x, kind)`` on the
    (subsampled) points the fit ran on. ``full=False`` pins a = s = 1 and fits the length scales only.
    ``value_and_grad(theta (P, d + 2)) -> (lml (P,), grad (P, d + 2))`` injects an evaluator (the CPU
    tests; it is handed the prepared points as ``value_and_grad.bind(x, y, e, H)`` if it has that
    attribute); the default is gpf_lml_mean_batch on this process's GPU. ``kernel`` as fit_lml's."""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim != 2:
        raise ValueError("x must be (d, N)")
    m = basis_rows(kind, x.shape[0])
    if m > MEAN_MAX:
        raise ValueError(f"the {kind} basis in d = {x.shape[0]} has {m} rows, more than {MEAN_MAX}")
    state = {}

    def setup(ctx_, xp, yp, ep):
        """Called with the prepared points: sets the basis (device) and returns the evaluator."""
        H, _ = basis(xp, kind)
        state.update(x=xp, y=yp, e=ep, H=H)
        if ctx_ is None:  # injected
            if hasattr(value_and_grad, "bind"):
                value_and_grad.bind(xp, yp, ep, H)
            return value_and_grad
        ctx_.set_basis(H)

        def device(theta, grad=True, want_q=False):
            return ctx_.lml_mean_batch(theta, grad=grad, strict=False, want_q=want_q)
        return device

    best, info = _fit_theta(x, y, e, who="fit_mean", lost=m, pin=not full, setup=setup,
                            done_msg="Restricted-likelihood fit of length scales, amplitude and noise scale completed.",
                            num_starts=num_starts, num_polish=num_polish, max_points=max_points, seed=seed,
                            value_and_grad=value_and_grad, ctx=ctx, verbose=verbose, kernel=kernel)
    if value_and_grad is None:  # (the fit left its data and basis on the context)
        info["beta"] = (ctx or default_context()).lml_mean_batch(best[None, :], grad=False, strict=False,
                                                                 want_beta=True)[2][0]
    else:
        try:
            info["beta"] = mean_closed_form(state["x"], state["y"], state["e"], state["H"], best)[2]
        except np.linalg.LinAlgError:
            info["beta"] = np.full(m, np.nan)
    return best, info
