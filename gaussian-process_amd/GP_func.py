"""Drop-in for the reference's GP_func.py, computed on the MI355X.

Same public surface as /GP_func.py of rferguson22/Gaussian-Process:
    GP(x_known, y_known, e_known, x_fit, lengths, batch_size=10000) -> (mu, sigma)
        (GP_func.py:12-45)
    kernel_func(x1, x2, l) -> (N1, N2) array                       (GP_func.py:49-65)

Both run through libgpfit (include/gpfit.h: gpf_predict, gpf_kernel); a
non-positive-definite covariance raises numpy.linalg.LinAlgError like
numpy.linalg.cholesky does at GP_func.py:22. There is no CPU fallback.

The reference's two functions keep their signatures and are always squared-exponential. The
extensions (GP_cov .. GP_mean) take kernel="se" | "matern32" | "matern52" (gpfit.kernels), and
GP_kernel is GP() with that argument. Every call sets its kernel on the shared context, so a call
without the keyword is "se" whatever ran before.
"""
import numpy as np

from gpfit._lib import default_context
from gpfit.kernels import kernel_kind

__all__ = ["GP", "GP_cov", "GP_draws", "GP_hyper", "GP_kernel", "GP_loo", "GP_mean", "kernel_func"]


def GP(x_known, y_known, e_known, x_fit, lengths, batch_size=10000):
    """GP regression mean / sd at x_fit (GP_func.py:12-45).

    K = k(x,x) + diag(e^2) is factorised once on the device (L and L^-1);
    every query column gets mu = K_s^T alpha and
    sd = sqrt(clip(1 - ||L^-1 K_s||^2, 1e-12)) without materialising
    L^-1 K_s. ``batch_size`` is accepted for signature parity; on the device
    the query set is chunked by available memory and the chunking does not
    change the result (as in the reference).
    """
    x_known = np.asarray(x_known, dtype=np.float64)
    x_fit = np.asarray(x_fit, dtype=np.float64)
    if x_fit.ndim != 2 or x_fit.shape[0] != x_known.shape[0]:
        raise ValueError("x_fit must be (d, M) with the same d as x_known")
    ctx = default_context()
    ctx.set_data(x_known, y_known, e_known)
    ctx.set_kernel("se")
    return ctx.predict(lengths, x_fit, batch_size)


def GP_kernel(x_known, y_known, e_known, x_fit, lengths, kernel, batch_size=10000):
    """GP() under the covariance kernel ``kernel``: "se" (GP() itself, bit for bit), "matern32" or
    "matern52" (gpfit.kernels has the formulas)."""
    kernel_kind(kernel)
    x_known = np.asarray(x_known, dtype=np.float64)
    x_fit = np.asarray(x_fit, dtype=np.float64)
    if x_fit.ndim != 2 or x_fit.shape[0] != x_known.shape[0]:
        raise ValueError("x_fit must be (d, M) with the same d as x_known")
    ctx = default_context()
    ctx.set_data(x_known, y_known, e_known)
    ctx.set_kernel(kernel)
    return ctx.predict(lengths, x_fit, batch_size)


def GP_cov(x_known, y_known, e_known, x_fit, lengths, kernel="se"):
    """Joint latent posterior at x_fit (d, M): (mu (M,), cov (M, M)).

    mu is GP()'s mean bit for bit; cov = K_ss - K_s^T Kn^-1 K_s is dense, exactly symmetric and
    not clipped on its diagonal (GP()'s sigma is sqrt(clip(diag(cov), 1e-12))). The reference has
    no counterpart: GP_func.py:39 keeps the diagonal only. All M points go in one call: cov and
    the two N x M matrices behind it must fit the device (ValueError names the largest M).
    """
    x_known = np.asarray(x_known, dtype=np.float64)
    x_fit = np.asarray(x_fit, dtype=np.float64)
    if x_fit.ndim != 2 or x_fit.shape[0] != x_known.shape[0]:
        raise ValueError("x_fit must be (d, M) with the same d as x_known")
    kernel_kind(kernel)
    ctx = default_context()
    ctx.set_data(x_known, y_known, e_known)
    ctx.set_kernel(kernel)
    return ctx.predict_cov(lengths, x_fit)


def GP_linear(x_known, y_known, e_known, x_fit, lengths, weights, kernel="se"):
    """Linear functionals of the latent GP at x_fit (d, M) with the weights (R, M): (mean (R,),
    cov (R, R)) = (A mu, A cov A^T) of GP_cov's posterior — region sums and averages
    (gpfit.linear.region_weights), differences — without the M x M covariance: the query axis is
    folded away on the device chunk by chunk (gpf_predict_linear), so M is not capped by it."""
    from gpfit.linear import predict_linear
    return predict_linear(x_known, y_known, e_known, x_fit, lengths, weights, method="stream", kernel=kernel)[:2]


def GP_conditioned(x_known, y_known, e_known, x_fit, lengths, weights, values, noise, kernel="se"):
    """GP()'s (mu, sigma) at x_fit (d, M) after conditioning the latent GP on R measured linear
    functionals as well: values[r] = sum_q weights[r, q] f(x_fit[:, q]) + N(0, noise[r]^2) — an
    integrated value or bin averages of another experiment (gpfit.linear.region_weights builds the
    weights of bins). Exact, streamed over the query axis (gpf_predict_conditioned): no M x M matrix."""
    from gpfit.conditioned import predict_conditioned
    return predict_conditioned(x_known, y_known, e_known, x_fit, lengths, weights, values, noise, method="stream",
                               kernel=kernel)[:2]


def GP_marginal(x_known, y_known, e_known, x_fit, lengths_Pd, weights=None, kernel="se"):
    """GP()'s (mu, sigma) at x_fit (d, M) with the length scales marginalised over the samples
    lengths_Pd (P, d) with the weights (P,) (None: equal) instead of fixed: the mixture of the P
    predictions by the law of total variance, mix_mu = sum_p w_p mu_p and
    mix_sigma^2 = sum_p w_p (sigma_p^2 + (mu_p - mix_mu)^2), from one batched factorisation on the
    device (gpf_predict_batch). gpfit.hyper.sample_hyper draws samples and weights from the marginal
    likelihood."""
    from gpfit.hyper import predict_marginal
    return predict_marginal(x_known, y_known, e_known, x_fit, ls=lengths_Pd, weights=weights, method="batch",
                            kernel=kernel)[:2]


def GP_draws(x_known, y_known, e_known, x_fit, lengths, n_draws, seed=None, method="host", kernel="se"):
    """n_draws joint draws of the latent GP at x_fit: (n_draws, M), from N(GP_cov's mu, cov) by a
    Cholesky factor of cov + jitter I: method="host" takes it with NumPy from the copied-back cov
    (gpfit.posterior.draws_from), method="device" on the GPU without cov leaving it
    (gpf_posterior_draws). The normals are default_rng(seed)'s on both paths."""
    from gpfit.posterior import sample_posterior
    return sample_posterior(x_known, y_known, e_known, x_fit, lengths, n_draws, seed=seed, method=method,
                            kernel=kernel)[0]


def GP_loo(x_known, y_known, e_known, lengths, kernel="se"):
    """Leave-one-out check of the fit: (mu (N,), sd (N,)), every measured y_i predicted from the other
    N - 1 points, sd the predictive sd of the measurement (e_i^2 included), so (y - mu) / sd is N(0, 1)
    if the error bars are honest (gpf_loo_batch; gpfit.loo.loo_predict also returns the pulls, their
    coverage and the LOO log predictive density)."""
    from gpfit.loo import loo_predict
    return loo_predict(x_known, y_known, e_known, lengths, kernel=kernel)[:2]


def GP_hyper(x_known, y_known, e_known, x_fit, theta, kernel="se"):
    """GP() under a prior amplitude and a noise scale: theta = (l_1 .. l_d, a, s),
    Kn = a^2 K(l) + s^2 diag(e^2); (mu, sigma) at x_fit (d, M). It is a times GP() on (y / a, e s / a)
    (gpfit.amplitude.predict_hyper; theta from gpfit.amplitude.fit_hyper)."""
    from gpfit.amplitude import predict_hyper
    x_known = np.asarray(x_known, dtype=np.float64)
    x_fit = np.asarray(x_fit, dtype=np.float64)
    if x_fit.ndim != 2 or x_fit.shape[0] != x_known.shape[0]:
        raise ValueError("x_fit must be (d, M) with the same d as x_known")
    return predict_hyper(x_known, y_known, e_known, x_fit, theta, kernel=kernel)


def GP_mean(x_known, y_known, e_known, x_fit, theta, kind="constant", kernel="se"):
    """GP_hyper() with a polynomial mean function (kind: "constant", "linear" or "quadratic") whose
    coefficients are integrated out under a flat prior: away from the data the mean tends to the fitted
    polynomial, not to 0, and sigma includes the share of not knowing the coefficients
    (gpfit.meanfn.predict_mean, gpf_predict_mean; theta from gpfit.meanfn.fit_mean)."""
    from gpfit.meanfn import predict_mean
    x_known = np.asarray(x_known, dtype=np.float64)
    x_fit = np.asarray(x_fit, dtype=np.float64)
    if x_fit.ndim != 2 or x_fit.shape[0] != x_known.shape[0]:
        raise ValueError("x_fit must be (d, M) with the same d as x_known")
    return predict_mean(x_known, y_known, e_known, x_fit, theta, kind, kernel=kernel)


def kernel_func(x1, x2, l):
    """Unit-amplitude squared-exponential kernel between column sets (GP_func.py:49-65)."""
    x1 = np.asarray(x1, dtype=np.float64)
    x2 = np.asarray(x2, dtype=np.float64)
    ctx = default_context()
    ctx.set_kernel("se")
    return ctx.kernel(x1, x2, np.asarray(l, dtype=np.float64))
