/*
 * gpfit.h — C-ABI of the MI355X GP-fit hot path (libgpfit.so).
 *
 * The reference (rferguson22/Gaussian-Process) is pure Python: its "plugin
 * surface" for this path is a set of Python functions, not an FFI. Each entry
 * point below replaces one of those seams; the Python drop-in modules in
 * gaussian-process_amd/ bind them through ctypes.
 *
 *   gpf_eval_batch  replaces the particle fan-out
 *                     list(executor.map(evaluate_loss_helper, args))
 *                   at find_len_scales.py:77, :103, :134 — i.e. P calls of
 *                   evaluate_loss (:181) -> wass_loss (:154-177) -> GP(x,y,e,x,l,
 *                   batch_size=N) (GP_func.py:12-45, called at :159).
 *   gpf_predict     replaces GP(x_known,y_known,e_known,x_fit,lengths,batch_size)
 *                   (GP_func.py:12-45) for arbitrary query points (GP_fit.py:32).
 *   gpf_kernel      replaces kernel_func(x1,x2,l) (GP_func.py:49-65) under the
 *                   default kernel, se.
 *
 * Conventions (mirroring the reference):
 *   - all floating point is IEEE fp64;
 *   - x arrays are dims-major (d, N), C-contiguous (the Python side calls
 *     np.ascontiguousarray on the reference's F-order view, read_in.py:229);
 *   - host buffers are caller-owned; data set by gpf_set_data stays resident
 *     on the device until the next gpf_set_data / gpf_close;
 *   - a context drives ONE device and is not thread-safe (one host thread per
 *     context); one process per GPU, the swarm exchange between them is in this
 *     library (gpf_comm_*: RCCL over xGMI, or a host transport).
 *
 * Return codes: GPF_OK, GPF_NOT_PD (Cholesky pivot <= 0 or NaN: the Python side
 * raises numpy.linalg.LinAlgError("Matrix is not positive definite") exactly
 * like numpy.linalg.cholesky at GP_func.py:22), GPF_HIP_ERROR, GPF_BAD_ARG.
 */
#ifndef GPFIT_H
#define GPFIT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GPF_OK 0
#define GPF_NOT_PD 1
#define GPF_HIP_ERROR 2
#define GPF_BAD_ARG 3

#define GPF_ABI_VERSION 2  /* 2 (r6): gpf_plan_check's stats carry 11 entries */

typedef struct gpf_ctx gpf_ctx;

/* ABI version of the loaded library (== GPF_ABI_VERSION). */
int gpf_version(void);

/* Open a context on HIP device `device` (after HIP_VISIBLE_DEVICES). */
int gpf_open(int device, gpf_ctx** out);
void gpf_close(gpf_ctx* ctx);

/* Message for the last non-OK return on this context ("" if none). */
const char* gpf_last_error(gpf_ctx* ctx);

/* Training data: x_dN is (d, N) dims-major; y, e are (N,).
 * Reference: the (x_known, y_known, e_known) tuple members pickled per task at
 * find_len_scales.py:76,102,133; here uploaded once per len_scale_opt call.
 * 1 <= d <= 32 and 1 <= N <= 2^20, else GPF_BAD_ARG and the data set before stays.
 * Every later call reads d doubles per length-scale row and d rows of query
 * coordinates: the caller's buffers must have this d (the library cannot see
 * their size; the Python binding checks the shapes). A call that changes d
 * discards the search box of gpf_set_grid, which is per dimension: gpf_eval_batch
 * then returns GPF_BAD_ARG until gpf_set_grid has been called again. */
int gpf_set_data(gpf_ctx* ctx, const double* x_dN, const double* y,
                 const double* e, int64_t N, int d);

/* The covariance function of every call on this context (the context's kernel). With
 * a_k = x_k / l_k and r2 = sum_k (a_ik - a_jk)^2, formed and clamped at 0 as kernel_func does
 * (GP_func.py:56-63), K_ij = phi(r2):
 *   GPF_KERNEL_SE       (default)  exp(-r2 / 2)                       the reference's kernel_func
 *   GPF_KERNEL_MATERN32            (1 + s) exp(-s),            s = sqrt(3 r2)
 *   GPF_KERNEL_MATERN52            (1 + s + s^2 / 3) exp(-s),  s = sqrt(5 r2)
 * phi(0) = 1 for all three: the prior variance of every model below stays 1. The length-scale
 * gradients use dK_ij/dl_k = psi(r2) (x_ik - x_jk)^2 / l_k^3 with psi = -2 phi'(r2): phi, 3 exp(-s)
 * and (5/3) (1 + s) exp(-s)
 * (psi_ij in the gradient formulas below; K_ij itself under se).
 * Needs no data. The kind is a model choice, not a property of the points: it persists across
 * gpf_set_data. GPF_BAD_ARG for a null context, a null kind pointer or an unknown kind; the kind set
 * before stays. */
#define GPF_KERNEL_SE 0
#define GPF_KERNEL_MATERN32 1
#define GPF_KERNEL_MATERN52 2
int gpf_set_kernel(gpf_ctx* ctx, int kind);
int gpf_get_kernel(gpf_ctx* ctx, int* kind);

/* Objective grid and search box: sigma_vals/expected are the K-point grid of
 * find_len_scales.py:66-67 (K = 1000 in the reference), lo/hi the (d,) bounds of
 * :56-61. 2 <= K <= 4096; sigma_vals and expected hold K doubles, lo and hi d.
 * sigma_vals must be finite and non-decreasing (equal neighbours are allowed)
 * and expected finite: otherwise GPF_BAD_ARG, gpf_last_error names the first
 * offending index, and the grid set before stays in force untouched. This is a
 * deliberate deviation from the reference, which computes a score for any
 * order: the device finds each point's first covered multiple by bisection,
 * which equals the reference's K comparisons only on a sorted grid. Sort the
 * grid (and expected with it) before the call. */
int gpf_set_grid(gpf_ctx* ctx, const double* sigma_vals, const double* expected,
                 int K, const double* lo, const double* hi);

/* Batched objective. ls_Pd is (P, d) row-major particle positions. Writes
 * loss_P[p] = evaluate_loss(ls[p], ...) (find_len_scales.py:181); sentinel
 * particles (any ls <= lo or ls >= hi, :156-157) get 1e13 without touching the
 * GPU. mu_PN / sd_PN (nullable, (P, N) row-major) receive the GP mean / sd at
 * the training points (GP_func.py:36-40 with x_fit = x_known); rows of
 * sentinel particles are filled with NaN. On GPF_NOT_PD *bad_idx is the first
 * particle whose covariance is not positive definite. GPF_BAD_ARG, before
 * anything is read or written: no data, no grid, or no gpf_set_grid since the
 * gpf_set_data that gave the data its present d (the box would be indexed past
 * its end, or hold the bounds of other dimensions). */
int gpf_eval_batch(gpf_ctx* ctx, const double* ls_Pd, int P, double* loss_P,
                   double* mu_PN, double* sd_PN, int* bad_idx);

/* GP prediction at M query points xfit_dM (d, M), chunked by `batch` like
 * GP_func.py:28-30 (the chunking does not change the result here). */
int gpf_predict(gpf_ctx* ctx, const double* ls, const double* xfit_dM,
                int64_t M, int64_t batch, double* mu_M, double* sd_M);

/* Joint (latent, noise-free) posterior of the M query points xfit_dM (d, M):
 *   mu_M[q] = K_s[:, q]^T alpha — bitwise gpf_predict's mean for the same inputs;
 *   cov_MM  = K_ss - V^T V, V = L^-1 K_s: the full M x M row-major matrix, both triangles
 *             written, exactly symmetric (the upper triangle is a copy of the lower).
 * K_ss is the context's kernel (gpf_set_kernel; kernel_func under se) at (xfit, xfit, l) with the diagonal exactly 1.0 (the prior variance,
 * GP_func.py:34). The diagonal of cov_MM is NOT clipped at 1e-12 as gpf_predict's variance is
 * (GP_func.py:39): where a query point coincides with another one or with a noise-free training
 * point it can come out a few 1e-14 below zero; a caller that factorises cov_MM adds a jitter
 * (gpfit.posterior.draws_from). No chunking over M: K_s and V (Npad x Mpad each) and Sigma
 * (Mpad x Mpad) live on the device for the call; if they do not fit half of the free device
 * memory the call returns GPF_BAD_ARG and gpf_last_error names the largest M that fits. The
 * buffers are kept for the next call under GPF_PREDICT_KEEP_MB like gpf_predict's, and are
 * apart from them: interleaved gpf_predict calls are not disturbed.
 * GPF_NOT_PD as gpf_predict: mu_M and cov_MM are then untouched. GPF_BAD_ARG, before any
 * device work: null ctx, no data set, M < 0, null ls, a null buffer with M > 0, a length scale
 * that is not finite and > 0. M == 0 returns GPF_OK and writes nothing. Repeating a call on
 * the same context and data gives the same bits (fixed-order sums, no floating-point atomics). */
int gpf_predict_cov(gpf_ctx* ctx, const double* ls, const double* xfit_dM, int64_t M,
                    double* mu_M, double* cov_MM);

/* R linear functionals of the latent posterior at the M query points xfit_dM (d, M), without the
 * M x M covariance: with the weights w_RM (R, M) row-major, row r the weights of functional r,
 *   mean_R[r] = sum_q w[r,q] mu_q                               (A mu)
 *   cov_RR    = A K_ss A^T - V_A^T V_A, V_A = L^-1 (K_s A^T)    (A Sigma A^T, Sigma as gpf_predict_cov's)
 *   prior_RR  = A K_ss A^T (nullable): the prior covariance of the functionals.
 * The model is gpf_predict_cov's: K_ss = the context's kernel at (xfit, xfit, l) with the diagonal exactly 1.0, and
 * cov_RR is not clipped. cov_RR and prior_RR are full R x R row-major matrices, both triangles
 * written, exactly symmetric (the upper triangle is a copy of the lower).
 * The query axis is chunked: `chunk` query points per pass, rounded up to 128 and capped at 65536;
 * 0 means gpf_predict's default of 16384. Nothing of size M x M or Npad x M is allocated: K_s A^T
 * (Npad x Rpad) is accumulated over the chunks and K_ss A^T (Mpad x Rpad) over pairs of chunks, one
 * kernel block (max(Npad, chunk) x chunk) at a time. On the device for the call: the weights as given
 * and transposed (R x M, Mpad x Rpad), K_ss A^T (Mpad x Rpad), the coordinates (d x Mpad), one kernel
 * block, the Npad x Rpad and Rpad x Rpad operands and up to about 1024 + the output's tiles partial
 * 128 x 128 tiles. If that exceeds half of the free device memory, chunk is halved until it fits; if
 * it does not fit at chunk = 128 the call returns GPF_BAD_ARG and gpf_last_error names the largest M
 * that fits at this R. The buffers are kept under GPF_PREDICT_KEEP_MB, apart from those of gpf_predict,
 * gpf_predict_cov and gpf_posterior_draws: interleaved calls of those keep their bits.
 * Repeating a call with the same chunk gives the same bits (every sum runs in a fixed order that the
 * shapes alone decide; no floating-point atomics). Different chunk values change the order of the
 * sums over the query axis and may differ in the last bits.
 * GPF_NOT_PD as gpf_predict_cov: the outputs are then untouched. GPF_BAD_ARG, before any device
 * work: null ctx, no data set, M < 0, R < 0 or chunk < 0, null ls, a null buffer with M > 0 and R > 0
 * (prior_RR may be null), a length scale that is not finite and > 0, a non-finite weight, M > 2^30 or
 * R > 16384. M == 0 or R == 0 returns GPF_OK and writes nothing.
 * Measured on one MI355X at N=4096, d=3, R=128 (profiles/predict_linear/bench.json): M=4096 about
 * 3 ms per call against about 29 ms for gpf_predict_cov followed by A Sigma A^T on the host;
 * M=200000, which gpf_predict_cov cannot hold, about 250 ms per call at the default chunk and 1.1,
 * 1.8 and 2.8 times that at chunk 8192, 4096 and 2048 (smaller chunks give the products shorter
 * depth pieces and more launches). */
int gpf_predict_linear(gpf_ctx* ctx, const double* ls, const double* xfit_dM, int64_t M,
                       const double* w_RM, int R, int64_t chunk,
                       double* mean_R, double* cov_RR, double* prior_RR);

/* The latent posterior at the M query points xfit_dM (d, M) conditioned on R measured linear
 * functionals of it: b_R[r] = sum_q w[r,q] f(x_q) + noise_r, noise_r ~ N(0, s_R[r]^2) independent
 * (an integrated value, averages in another experiment's bins; s_r = 0 is an exact constraint). With
 * mu, Sigma the posterior of gpf_predict_cov and A = w_RM,
 *   H = A Sigma A^T + diag(s^2) = Lh Lh^T,  C = Sigma A^T,  E = C Lh^-T,  g = Lh^-1 (b - A mu)
 *   mu_M[q] = mu_q + E[q,:] . g
 *   sd_M[q] = sqrt(max((1 - sum v^2) - sum_r E[q,r]^2, 1e-12))      (gpf_predict's variance and clip)
 *   *chi2   = g . g = (b - A mu)^T H^-1 (b - A mu) (nullable): how well the measurements agree with the
 *             fit before conditioning; about R is expected.
 * fmean_R, fcov_RR (nullable): A mu and A Sigma A^T BEFORE conditioning, bitwise gpf_predict_linear's
 * mean_R and cov_RR for the same inputs and chunk (the same launches in the same order).
 * Conditioning on one point functional (x_q, b, s) equals adding the training point (x_q, b, s).
 * chunk as gpf_predict_linear: query points per pass, rounded up to 128, 0 means 16384, capped at
 * 65536. Nothing of size M x M or Npad x M is allocated: behind gpf_predict_linear's pipeline,
 * W2 = L^-T V_A (Npad x Rpad) once, H's factor and its inverse (Rpad x Rpad; gpf_chol_dense's kernels,
 * no jitter, and a blocked forward substitution), then per chunk the K_s block again, gpf_predict's
 * V = U K_s reduction, C = K_ss A^T - K_s^T W2 and E (chunk x Rpad each). On the device for the call:
 * what gpf_predict_linear holds, the Npad x Rpad, Rpad x Rpad and chunk x Rpad operands above, the
 * partials of V (2 nt x chunk) and mu', sd' (2 Mpad). The call has its own buffers, kept under
 * GPF_PREDICT_KEEP_MB apart from those of the other prediction calls: interleaved calls of those keep
 * their bits. If the buffers exceed half of the free device memory, chunk is halved until they fit; if
 * they do not fit at chunk = 128 the call returns GPF_BAD_ARG and gpf_last_error names the largest M
 * that fits at this R. Repeating a call with the same chunk gives the same bits (every sum runs in a
 * fixed order that the shapes alone decide; no floating-point atomics).
 * GPF_NOT_PD: the covariance of the training points fails as in gpf_predict, or H has a pivot <= 0
 * (redundant functionals with zero error; no jitter is added); gpf_last_error says which. Every
 * output is then untouched (both factorisations finish before anything is copied back).
 * GPF_BAD_ARG, before any device work: everything gpf_predict_linear rejects, a null b_R, s_R, mu_M or
 * sd_M with M > 0 and R > 0, a non-finite b, an s_r that is negative or not finite, R > 1024 (larger R
 * is not built yet: the inverse of H's factor is formed densely). M == 0 or R == 0 returns GPF_OK and
 * writes nothing. */
int gpf_predict_conditioned(gpf_ctx* ctx, const double* ls, const double* xfit_dM, int64_t M,
                            const double* w_RM, int R, const double* b_R, const double* s_R, int64_t chunk,
                            double* mu_M, double* sd_M, double* fmean_R, double* fcov_RR, double* chi2);

/* Cholesky factor of a dense symmetric host matrix on the device: tries A + jitters[t] I for
 * t = 0, 1, .. until one factorises. L_nn: n x n row-major, zeros above the diagonal.
 * Only A's lower triangle is read. A blocked left-looking factorisation on 128-tiles with FP64
 * MFMA (gpf_densechol.hip), three launches per block column, A kept intact on the device between
 * the attempts. *jitter_used is the value that factorised, *tries the number of attempts.
 * GPF_NOT_PD if every jitter failed: L_nn and *jitter_used are untouched and *tries = nj.
 * GPF_BAD_ARG, before any device work: null ctx or buffer, n < 0, nj < 1, a non-finite jitter, or
 * a matrix that does not fit half of the free device memory with its factor. n == 0 returns GPF_OK.
 * Needs no gpf_set_data. The same bits on every call (fixed-order sums, no floating-point atomics). */
int gpf_chol_dense(gpf_ctx* ctx, const double* A_nn, int64_t n, const double* jitters, int nj,
                   double* L_nn, double* jitter_used, int* tries);

/* S joint draws of the latent posterior at M query points without Sigma leaving the device:
 * gpf_predict_cov's pipeline up to k_post_cov, the dense factorisation above with the same
 * jitter ladder, draws = mu + z L^T. z_SM: (S, M) standard normals from the caller.
 * chol_MM nullable: the factor that was used (M x M row-major), for callers and tests.
 * mu_M is bitwise gpf_predict_cov's (the same kernels in the same order). Nothing of size M x M is
 * copied to the host unless chol_MM is given. No chunking over M: gpf_predict_cov's buffers, the
 * factor (Mpad x Mpad), the normals and the draws (Spad x Mpad each) and a 128 x Mpad scratch must
 * fit half of the free device memory, else GPF_BAD_ARG and gpf_last_error names the largest M
 * that fits. The buffers are kept under GPF_PREDICT_KEEP_MB, apart from gpf_predict's and
 * gpf_predict_cov's. GPF_NOT_PD if the training covariance is not positive definite (as
 * gpf_predict_cov) or every jitter failed (*tries = nj): the outputs are then untouched.
 * GPF_BAD_ARG, before any device work: null ctx, no data set, M < 0 or S < 0, null ls, a null
 * buffer, nj < 1, a non-finite jitter, a length scale that is not finite and > 0. M == 0 or
 * S == 0 returns GPF_OK and writes nothing. */
int gpf_posterior_draws(gpf_ctx* ctx, const double* ls, const double* xfit_dM, int64_t M,
                        const double* z_SM, int64_t S, const double* jitters, int nj,
                        double* mu_M, double* draws_SM, double* chol_MM,
                        double* jitter_used, int* tries);

/* The context's kernel (gpf_set_kernel) at (x1, x2, l): out is (N1, N2) row-major. It is
 * kernel_func(x1, x2, l) (GP_func.py:49-65) only for se, the default. */
int gpf_kernel(gpf_ctx* ctx, const double* x1_dN1, int64_t N1,
               const double* x2_dN2, int64_t N2, int d, const double* l,
               double* out);

/* Diagnostic log marginal likelihood from the same factor (the reference has
 * none): -1/2 y^T alpha - sum log L_ii - N/2 log(2 pi). */
int gpf_log_marginal_likelihood(gpf_ctx* ctx, const double* ls, double* out);

/* Batched log marginal likelihood and its gradient in the length scales (fixed amplitude 1,
 * fixed noise e^2, the context's ARD kernel), the objective of a maximum-marginal-likelihood fit
 * (gpfit.mle.fit_lml). ls_Pd is (P, d) row-major. Needs gpf_set_data only (no grid, no box).
 *   lml_P[p]     = -1/2 y^T alpha - sum log L_ii - N/2 log(2 pi)
 *   grad_Pd[p,k] = dLML/dl_k = sum_{i>j} (alpha_i alpha_j - W_ij) psi_ij (x_ik - x_jk)^2 / l_k^3,
 *                  W = Kn^-1, psi the kernel's derivative weight (gpf_set_kernel; K_ij, the
 *                  noise-free kernel, under se) (nullable: without it the gradient pass
 *                  is not run)
 *   status_P[p]  = GPF_OK or GPF_NOT_PD (nullable)
 * Everything is computed on the device from the factorisation's L, U = L^-1 and alpha; the
 * particles are chunked as in gpf_eval_batch. A particle whose covariance is not positive
 * definite gets lml = -inf and a NaN gradient row and does not spoil the others: every other
 * output is written, then the call returns GPF_NOT_PD with *bad_idx the first such particle.
 * GPF_BAD_ARG, before any device work, if P < 0 or any length scale is not finite and > 0.
 * Repeating a call on the same context and data gives the same bits (fixed-order sums, no
 * floating-point atomics); results may differ in the last bits between batch sizes, as the
 * factorisation's schedule depends on the batch. */
int gpf_lml_batch(gpf_ctx* ctx, const double* ls_Pd, int P, double* lml_P, double* grad_Pd,
                  int* status_P, int* bad_idx);

/* Batched leave-one-out (LOO) cross-validation and the gradient of its log predictive density in the
 * length scales (same model as gpf_lml_batch; Rasmussen & Williams 5.4.2), the validation report and
 * the objective of gpfit.loo.fit_loo. ls_Pd is (P, d) row-major. Needs gpf_set_data only.
 * With W = Kn^-1, alpha = W y, w_i = W_ii:
 *   mu_PN[p,i]   = y_i - alpha_i / w_i: the prediction of the measured y_i from the other N - 1 points
 *                  (nullable)
 *   sd_PN[p,i]   = sqrt(1 / w_i): its predictive sd, e_i^2 included, not clipped (nullable)
 *   lpd_P[p]     = sum_i [1/2 log w_i - 1/2 alpha_i^2 / w_i] - N/2 log(2 pi)
 *   grad_Pd[p,k] = dlpd/dl_k = sum_{i>j} (u_i alpha_j + u_j alpha_i - 2 G_ij) psi_ij (x_ik - x_jk)^2 / l_k^3,
 *                  c_i = alpha_i / w_i, g_i = 1/2 (1 + alpha_i^2 / w_i) / w_i, u = W c, G = W diag(g) W,
 *                  psi the kernel's derivative weight (gpf_set_kernel; K_ij, the noise-free kernel,
 *                  under se) (nullable: without it neither O(N^3) pass is run)
 *   status_P[p]  = GPF_OK or GPF_NOT_PD (nullable)
 * The pull (y_i - mu_i) / sd_i = alpha_i / sqrt(w_i) is N(0, 1) under the model.
 * Everything is computed on the device from the factorisation's U = L^-1 and its partial sums of
 * diag(W) and alpha; the particles are chunked as in gpf_eval_batch, and with the gradient the chunk
 * is lowered to what a buffer of Npad^2 doubles per particle (B = diag(sqrt g) W) fits beside the
 * workspace. A particle whose covariance is not positive definite gets lpd = -inf and NaN gradient,
 * mu and sd rows and does not spoil the others: every other output is written, then the call
 * returns GPF_NOT_PD with *bad_idx the first such particle.
 * GPF_BAD_ARG, before any device work, for a null ctx, no data set, P < 0, a null ls_Pd or lpd_P with
 * P > 0, or any length scale that is not finite and > 0. P == 0 returns GPF_OK.
 * Repeating a call on the same context and data gives the same bits (fixed-order sums, no
 * floating-point atomics), and lpd, mu and sd do not depend on whether the gradient is asked for;
 * results may differ in the last bits between batch sizes, as the factorisation's schedule depends
 * on the batch. The call keeps its own buffers: it changes no bit of any other call. */
int gpf_loo_batch(gpf_ctx* ctx, const double* ls_Pd, int P, double* lpd_P, double* grad_Pd,
                  double* mu_PN, double* sd_PN, int* status_P, int* bad_idx);

/* Batched log marginal likelihood with a prior amplitude and a noise scale, and its gradient in all
 * of them: the objective of gpfit.amplitude.fit_hyper. th_Pd2 is (P, d + 2) row-major, each row
 * (l_1 .. l_d, a, s): a > 0 the prior sd of f, s > 0 a factor on the quoted errors,
 *   Kn = a^2 K(l) + s^2 diag(e^2) = a^2 Kt,  Kt = K(l) + r diag(e^2),  r = (s / a)^2.
 * Needs gpf_set_data only. The unit-amplitude Kt is factored by the kernels of every other call (the
 * K build adds e_i^2 r on the diagonal); with Lt = chol(Kt), Wt = Kt^-1, alt = Wt y, wt_i = Wt_ii,
 * Q = y^T alt and S = sum_i e_i^2 (alt_i^2 / a^2 - wt_i):
 *   lml_P[p]         = -Q / (2 a^2) - sum_i log Lt_ii - N log a - N/2 log(2 pi)
 *   grad_Pd2[p,k<d]  = sum_{i>j} (alt_i alt_j / a^2 - Wt_ij) psi_ij (x_ik - x_jk)^2 / l_k^3
 *   grad_Pd2[p,d]    = dLML/da = (Q / a^2 - N) / a - (s^2 / a^3) S
 *   grad_Pd2[p,d+1]  = dLML/ds = (s / a^2) S                        (grad_Pd2 nullable: no O(N^3) pass)
 *   q_P[p]           = Q: for fixed (l, r) the best amplitude is a^2 = Q / N (nullable)
 *   status_P[p]      = GPF_OK or GPF_NOT_PD (nullable)
 * At a = s = 1 lml_P and the first d gradient columns are gpf_lml_batch's for the same batch, bit for
 * bit. The model with (a, s) on (x, y, e) is the unit model on (x, y / a, e s / a) with mu a, sd a and
 * cov a^2: every other call serves it through that scaling (gpfit.amplitude).
 * A particle whose Kt is not positive definite gets lml = -inf and NaN in its gradient row and q and
 * does not spoil the others: every other output is written, then the call returns GPF_NOT_PD with
 * *bad_idx the first such particle.
 * GPF_BAD_ARG, before any device work, for a null ctx, no data set, P < 0, a null th_Pd2 or lml_P with
 * P > 0, any l, a or s that is not finite and > 0, or an (s / a)^2 that is not finite and > 0.
 * P == 0 returns GPF_OK. Repeating a call gives the same bits (fixed-order sums, no floating-point
 * atomics), and lml and q do not depend on whether the gradient is asked for. The call keeps its own
 * buffers: it changes no bit of any other call.
 * Not built: per-particle (a, s) in gpf_predict_batch and in the length-scale sampler, leave-one-out
 * with (a, s). */
int gpf_lml_hyper_batch(gpf_ctx* ctx, const double* th_Pd2, int P, double* lml_P, double* grad_Pd2,
                        double* q_P, int* status_P, int* bad_idx);

/* A marginalised polynomial mean function (Rasmussen & Williams 2.7): f(x) = h(x)^T beta + g(x) with g
 * the GP of every other call, h(x) the m basis functions the caller evaluates, and beta integrated
 * out under a flat prior.
 *
 * gpf_set_basis: H_mN is (m, N) row-major, the basis at the training points, kept on the device like
 * the data. GPF_BAD_ARG for a null ctx or H_mN, no data set, m < 1, m > 32, m >= N or an entry that
 * is not finite; the basis set before then stays in force. Every gpf_set_data discards the basis (it
 * belongs to the points it was evaluated at): gpf_lml_mean_batch and gpf_predict_mean then return
 * GPF_BAD_ARG until it is set again. H must have full row rank (the Python binding checks it; here a
 * rank-deficient H shows as GPF_NOT_PD in the calls below). */
int gpf_set_basis(gpf_ctx* ctx, const double* H_mN, int m);

/* The restricted log marginal likelihood (REML: beta integrated out) and its gradient in (l, a, s), for
 * a batch of particles. th_Pd2 as gpf_lml_hyper_batch. With Lt = chol(Kt), U = Lt^-1, z = U y,
 * Z = U H^T, At = Z^T Z = H Kt^-1 H^T = La La^T, Zo = Z La^-T, t = Zo^T z, zr = z - Zo t, Q' = zr^T zr,
 * Bt = Zo^T U, Pt = U^T U - Bt^T Bt, at = Pt y, pt_i = Pt_ii and S' = sum_i e_i^2 (at_i^2 / a^2 - pt_i):
 *   lml_P[p]         = -Q' / (2 a^2) - sum log Lt_ii - sum log La_rr - (N - m) log a - (N - m)/2 log(2 pi)
 *   grad_Pd2[p,k<d]  = sum_{i>j} (at_i at_j / a^2 - Pt_ij) psi_ij (x_ik - x_jk)^2 / l_k^3
 *   grad_Pd2[p,d]    = dLML/da = (Q' / a^2 - (N - m)) / a - (s^2 / a^3) S'
 *   grad_Pd2[p,d+1]  = dLML/ds = (s / a^2) S'                       (grad_Pd2 nullable: no O(N^3) pass)
 *   beta_Pm[p]       = La^-T t, the generalised-least-squares coefficients; they do not depend on a (nullable)
 *   q_P[p]           = Q': for fixed (l, r) the best amplitude is a^2 = Q' / (N - m) (nullable)
 *   status_P[p]      = GPF_OK or GPF_NOT_PD (nullable)
 * Q' is formed as the residual's sum of squares, so a large offset in y costs no digits of it.
 * A particle whose Kt, or whose At, has a pivot <= 0 is GPF_NOT_PD as in gpf_lml_hyper_batch (-inf,
 * NaN rows; the others are computed; *bad_idx the first); gpf_last_error says which of the two failed.
 * Argument checks, P == 0 and the same bits on a repeated call are gpf_lml_hyper_batch's, and
 * GPF_BAD_ARG also when no basis is set. lml, q and beta do not depend on whether the gradient is
 * asked for. The call keeps its own buffers: it changes no bit of any other call. */
int gpf_lml_mean_batch(gpf_ctx* ctx, const double* th_Pd2, int P, double* lml_P, double* grad_Pd2,
                       double* beta_Pm, double* q_P, int* status_P, int* bad_idx);

/* gpf_predict with the mean function, for the unit model a = s = 1 ((a, s) go through the data as in
 * gpfit.amplitude.scaled_data; beta scales by a). hfit_mM is (m, M) row-major, the basis at the query
 * points. With k_q = K_s[:, q], h_q the basis at query point q and R_q = h_q - H Kt^-1 k_q:
 *   mu_M[q] = k_q^T at + h_q^T beta
 *   sd_M[q] = sqrt(max(1 - sum v^2, 1e-12) + |La^-1 R_q|^2)
 * the first term gpf_predict's variance and clip, the second the share of not knowing beta.
 * beta_m (nullable): beta; bcov_mm (nullable, (m, m) row-major): cov(beta) = At^-1.
 * The query axis is chunked as gpf_predict's (batch), and the chunking does not change the bits.
 * M == 0 returns GPF_OK and writes nothing; on GPF_NOT_PD (Kt or At) no output is touched. The buffers
 * are a kept set of the call's own under GPF_PREDICT_KEEP_MB.
 * Not built: the mean function in gpf_predict_cov, the draws, gpf_predict_linear,
 * gpf_predict_conditioned, gpf_predict_batch, the length-scale sampler and leave-one-out; the m dot
 * products Z^T V folded into k_predict_vsq's register reduction (it would save the K_s^T Bt^T pass;
 * that kernel sits at 124 of 128 VGPRs); bases other than what the caller puts into H. */
int gpf_predict_mean(gpf_ctx* ctx, const double* ls_d, const double* xfit_dM, const double* hfit_mM, int64_t M,
                     int64_t batch, double* mu_M, double* sd_M, double* beta_m, double* bcov_mm);

/* gpf_predict for P length-scale samples at once, and their mixture: the length scales are not known
 * exactly (the fit ends with many nearly-as-good candidates), so the prediction is taken at P samples
 * ls_Pd (P, d) row-major with the weights w_P (nullable: equal; else >= 0, normalised to sum 1 here)
 * and combined by the law of total variance. Particle p gives mu_p, sd_p exactly as gpf_predict defines
 * them (latent, amplitude 1, variance clipped at 1e-12), and
 *   mix_mu_M[q] = sum_p w_p mu_p[q]
 *   mix_sd_M[q] = sqrt(sum_p w_p (sd_p[q]^2 + (mu_p[q] - mix_mu[q])^2))
 * mu_PM / sd_PM (nullable, (P, M) row-major) receive every particle's own mu_p / sd_p.
 * The particles are factorised in chunks by the batched factorisation (as gpf_lml_batch), which leaves
 * U = L^-1 and z = U y of the whole chunk on the device; per particle chunk and per chunk of query
 * points the call builds the particles' K_s blocks, reduces V = U K_s of all of them in one launch
 * (k_predict_vsq_batch: gpf_predict's tile with the particle on a grid axis) and folds the particles'
 * (mu_p, sd_p) into a per-column mixture state on the device (West's weighted update, the particles in
 * input order; a particle with weight 0 is predicted but not folded in). The query coordinates are
 * uploaded once. `chunk`: query points per pass, rounded up to 128; 0 means 16384, lowered to what keeps
 * the call's buffers within GPF_PREDICT_KEEP_MB (so that the next call finds them) while that leaves at
 * least 512 columns per pass; capped at 65536. The
 * particle-chunk capacity and the query chunk are planned together: the factorisation workspace of the
 * chunk's particles first (GPF_MAX_CHUNK caps it; a larger workspace the context already holds is kept if
 * the buffers fit beside it, else given back and regrown to the chunk), then the call's own buffers — per pass
 * pc (Npad + 2 nt + 3) chunk doubles, per call (d + 6) Mpad + P — must fit half of the remaining free
 * device memory; the query chunk is halved down to 128, then the particle chunk shrinks. If one particle
 * at chunk 128 does not fit the call returns GPF_BAD_ARG and gpf_last_error names the largest M (or N)
 * that fits. The call has buffers of its own, kept under GPF_PREDICT_KEEP_MB apart from those of every
 * other prediction call: interleaved calls of those keep their bits.
 * Repeating a call on the same context and data gives the same bits (fixed-order sums, no
 * floating-point atomics). Different chunk values give the same bits: every query column's sums are
 * independent of the other columns. Different particle-chunk capacities (GPF_MAX_CHUNK, free memory)
 * agree to rounding only, as the factorisation's schedule depends on the batch (gpf_lml_batch).
 * With P = 1, mu_PM, sd_PM, mix_mu_M and mix_sd_M are bitwise gpf_predict's mu and sd: the same
 * factorisation plan and every sum in the same order.
 * GPF_NOT_PD if any particle's covariance fails: *bad_idx is the first such particle in input order,
 * mix_mu_M and mix_sd_M are untouched and the rows of mu_PM / sd_PM are unspecified (some may have been
 * written). GPF_BAD_ARG, before any device work: null ctx, no data set, P < 0, M < 0 or chunk < 0,
 * a null ls_Pd, xfit_dM, mix_mu_M or mix_sd_M with P > 0 and M > 0, a length scale that is not finite and
 * > 0, a weight that is negative or not finite, weights that sum to 0, M > 2^30. P == 0 or M == 0
 * returns GPF_OK and writes nothing. */
int gpf_predict_batch(gpf_ctx* ctx, const double* ls_Pd, int P, const double* w_P,
                      const double* xfit_dM, int64_t M, int64_t chunk,
                      double* mix_mu_M, double* mix_sd_M,
                      double* mu_PM, double* sd_PM, int* bad_idx);

/* Host-only: the memory plan gpf_predict_batch makes (needs no device and no context; the same function,
 * not a second derivation), for given byte counts: free_b free device bytes, held_b the call's own kept
 * buffers, cap_slots particle slots of per_particle_b bytes the context's workspace holds, per_col_b bytes
 * per particle and padded query column of a pass, fixed_b bytes per call, Mpad the padded M, chunk as the
 * call's, keep_b the GPF_PREDICT_KEEP_MB limit in bytes, mem_fraction GPF_MEM_FRACTION. Writes the
 * particle-chunk capacity *pc, the query chunk *cq and *regrow = 1 where a workspace of at least *pc slots
 * is held but has to be given back and regrown to *pc slots for the call's buffers to fit half of what is
 * left. GPF_BAD_ARG if one particle at chunk 128 does not fit either way, or for a bad argument. */
int gpf_predict_batch_plan(double free_b, double held_b, int cap_slots, double per_particle_b,
                           double per_col_b, double fixed_b, int P, int64_t Mpad, int64_t chunk,
                           double keep_b, double mem_fraction, int* pc, int64_t* cq, int* regrow);

/* Probability surface of merged GP results (replaces calc_prob_surf.py:15-30,67-81; SURVEY.md
 * §8f row 4). tails: M rows x E entries (row-major) = each merged-frame row after its kinematic
 * columns, non-finite = missing. Per row: y[100] (the numpy.linspace grid), p[100] (bin
 * probabilities of the equal-weight Gaussian mixture), ok = 0 if the row is skipped (fewer than
 * 2 or an odd number of finite entries, calc_prob_surf.py:71-73), else 1. E <= 1024. */
int gpf_prob_surface(gpf_ctx* ctx, const double* tails, int64_t M, int E, double* y, double* p, int* ok);

/* Convex-hull grid fill (replaces the fill passes of convex_hull.py:122-155,203-224; SURVEY.md
 * §8f row 3). shell: n x d rows (row-major) = the rasterised hull facets (the reference's
 * concatenated facet surfaces, convex_hull.py:215-217); res: the d resolutions; decimals: the
 * digits after the point of str(res[j]) (numpy.around in round_to_res, convex_hull.py:13-24).
 * Runs the d sort + scan-fill passes and keeps the grid; *m = its row count. gpf_hull_fetch
 * copies it (m x d, rows sorted lexicographically, as fill_convex_hull returns them). */
int gpf_hull_fill(gpf_ctx* ctx, const double* shell, int64_t n, int d, const double* res, const int* decimals,
                  int64_t* m);
int gpf_hull_fetch(gpf_ctx* ctx, double* out);

/* KMeans subsample (the Lloyd iterations of find_len_scales.py:27-31, sklearn KMeans(n_clusters,
 * n_init='auto', random_state=0)). gpf_kmeans_set keeps n points x d
 * (row-major, already centred by their mean as sklearn's fit does) on the device. One
 * gpf_kmeans_step = the E-step (and with update != 0 the M-step sums) of sklearn's
 * lloyd_iter_chunked_dense with unit weights against k centres (k x d, row-major; k*(d+1) <= 8192,
 * else GPF_BAD_ARG and gpfit.kmeans keeps sklearn's host fit):
 * labels[i] = the first j minimising ||c_j||^2 - 2 x_i.c_j; sums (k x d) and counts (k) of each
 * cluster's members; dist[i] = ||x_i - c_labels[i]||^2 (optional, may be NULL). The host runs
 * sklearn's loop around it (gaussian-process_amd/gpfit/kmeans.py). */
int gpf_kmeans_set(gpf_ctx* ctx, const double* X, int64_t n, int d);
int gpf_kmeans_step(gpf_ctx* ctx, const double* centers, int k, int update, int* labels, double* sums, double* counts,
                    double* dist);

/* ---- swarm exchange across ranks (one process per GPU) ----
 *
 * Replaces the cross-process half of the particle fan-out: the reference's single process
 * scatters the swarm over a fork pool and gathers the scores (find_len_scales.py:73-77,
 * 102-104,133-135); here every rank scores its contiguous rows [rP/G, (r+1)P/G) and one
 * all-reduce (sum) of a zero-initialised [P + G] float64 vector hands every rank the full
 * score vector (exact: one non-zero contributor per entry), so all ranks take the same
 * first-index argmin (:81,110). The G trailing entries carry each rank's status, so a non-PD
 * particle or a device error on one rank is reported on every rank (same bad_idx, same code)
 * instead of leaving the others blocked in the collective.
 *
 * Transports: GPF_COMM_RCCL = ncclAllReduce on the context's device (RCCL over xGMI; rank 0
 * hands out the ncclUniqueId over TCP); GPF_COMM_HOST = the same exchange over the TCP
 * rendezvous sockets (rank 0 combines in rank order; needs no device). Rendezvous: rank 0
 * listens on host:port, the others connect (retrying until GPF_COMM_TIMEOUT_S, default 600 s).
 * A communicator is not thread-safe. */
#define GPF_COMM_RCCL 1
#define GPF_COMM_HOST 2
#define GPF_OP_SUM 0
#define GPF_OP_MAX 1

typedef struct gpf_comm gpf_comm;

/* Join rank `rank` of `nranks`. ctx: the rank's context (required for GPF_COMM_RCCL: the
 * communicator lives on its device; may be NULL for GPF_COMM_HOST). */
int gpf_comm_open(gpf_ctx* ctx, int rank, int nranks, const char* host, int port, int transport, gpf_comm** out);
void gpf_comm_close(gpf_comm* comm);
int gpf_comm_rank(const gpf_comm* comm);
int gpf_comm_size(const gpf_comm* comm);
const char* gpf_comm_last_error(const gpf_comm* comm);
/* Cumulative wall time spent inside gpf_comm_exchange_scores on this rank (the all-reduce,
 * including the wait for the slowest rank) and the number of exchanges. */
int gpf_comm_stats(const gpf_comm* comm, double* exchange_ms, long long* exchanges);

/* In-place all-reduce of n host doubles (GPF_OP_SUM or GPF_OP_MAX) across the ranks: the
 * seed broadcast of the PSO driver, the bench's barrier and max-over-ranks timing. */
int gpf_comm_allreduce(gpf_comm* comm, double* buf, int64_t n, int op);

/* The exchange step alone, given this rank's results for its rows [rP/G, (r+1)P/G):
 * local (hi - lo scores; ignored unless local_rc == GPF_OK), local_rc (GPF_OK / GPF_NOT_PD /
 * other), local_bad (the row, relative to lo, of the first non-PD particle). Fills loss_P on
 * every rank, or returns on every rank GPF_NOT_PD with *bad_idx = the smallest failing row of
 * the whole swarm (the particle the reference's in-order map would raise on first), or the
 * error code of the first failed rank. */
int gpf_comm_exchange_scores(gpf_comm* comm, int P, const double* local, int local_rc, int local_bad,
                             double* loss_P, int* bad_idx);

/* Sharded gpf_eval_batch: this rank scores its rows of ls_Pd (P, d) on its context, then
 * gpf_comm_exchange_scores. Every rank passes the same ls_Pd and receives the same loss_P. */
int gpf_eval_batch_sharded(gpf_ctx* ctx, gpf_comm* comm, const double* ls_Pd, int P, double* loss_P,
                           int* bad_idx);

/* Wait until all work queued by this library on the context's device has finished
 * (hipDeviceSynchronize on that device): the bench's timing fence. */
int gpf_sync(gpf_ctx* ctx);

/* ---- measurement hooks (bench.py) ---- */

/* Enable per-kernel-class HIP event timing on the context's stream. */
int gpf_set_profiling(gpf_ctx* ctx, int on);

/* Fill out[0..n) with accumulated counters since the last reset:
 *  [0] panel kernel ms   [1] panel launches  [2] panel algorithmic flops
 *  [3] diag kernel ms    [4] diag launches   [5] diag algorithmic flops
 *  [6] K-build ms        [7] K-build launches[8] K-build algorithmic bytes
 *  [9] loss kernel ms    [10] loss launches  [11] evals (non-sentinel)
 *       (gpf_lml_batch: its value kernels, one entry, and k_lml_grad with k_lml_grad_sum, one entry;
 *       gpf_loo_batch: k_loo_points; k_loo_w (flops ~ P N^3 / 3); k_loo_scale_mirror with k_loo_u;
 *       k_loo_grad (flops P ntile 2 T^3 nt) with k_lml_grad_sum — one entry each;
 *       gpf_lml_hyper_batch: as gpf_lml_batch, k_hyper_value among the value kernels and
 *       k_hyper_scale in the gradient entry)
 *  [12] factorisation wall ms (K build + diag + steps of all particle groups, which run
 *       on concurrent streams, so [0]/[3]/[6] may overlap)  [13] calls  [14] its flops
 *  [15] prediction V = U K_s kernel ms  [16] launches  [17] algorithmic flops
 *       (gpf_predict_cov: its V = U K_s and Sigma = K_ss - V^T V kernels, one launch each;
 *       gpf_chol_dense / gpf_posterior_draws: also the dense factorisation's launches and k_draws;
 *       gpf_predict_linear: its skinny products — a k_lin_nn or k_lin_tn launch with the product's
 *       flops 2 rows depth Rpad, and the k_lin_reduce launch behind it with none — and k_predict_v;
 *       gpf_predict_conditioned: gpf_predict_linear's, its k_con_tn / k_lin_nn products counted the
 *       same way, the dense factorisation of H, k_dc_inv_sum / k_dc_inv_fin and gpf_predict's
 *       k_predict_vsq per chunk;
 *       gpf_predict_batch: one k_predict_vsq_batch launch per particle chunk and query chunk, with the
 *       flops of all its particles)
 *  [18] prediction cross-covariance ms  [19] launches  [20] algorithmic bytes
 *       (gpf_predict_cov: K_s and K_ss in one entry, and the mirror copy of Sigma's lower triangle;
 *       gpf_chol_dense: the padding and mirror copy of the uploaded matrix;
 *       gpf_predict_linear: one entry per kernel block built, 8 bytes per element, the transposed
 *       copy of the weights and the two mirror copies;
 *       gpf_predict_conditioned: gpf_predict_linear's, the K_s block of every chunk once more, k_con_h
 *       and k_dc_inv_diag;
 *       gpf_predict_batch: one entry per particle chunk and query chunk, the K_s blocks of all its
 *       particles)
 *  [21] probability-surface kernel ms  [22] launches  [23] algorithmic bytes
 *  [24] shader clock (MHz) the factor kernels held while they ran (every workgroup's span in
 *       s_memtime clocks over its span in the 100 MHz s_memrealtime clock; profiled batches only)
 *  [25] compute units  [26] FP64 matrix ceiling at that clock, TFLOP/s (128 flop / CU / clock)
 * Returns the number of values written. */
int gpf_get_profile(gpf_ctx* ctx, double* out, int n);
int gpf_reset_profile(gpf_ctx* ctx);

/* Tile edge used by the factorisation (padding granule). */
int gpf_tile(void);

/* Build provenance baked in at compile time by __graft_entry__.build(): "src=<sha256 of the
 * csrc .hip and include .h sources> hipcc=<compiler version line>" ("unknown" if compiled by
 * hand). Tests compare it with the hash of the sources in the tree. */
const char* gpf_build_info(void);

/* Host-only structural check of the k_step dispatch plan (needs no device and no context):
 * for a chunk of pc particles with nt block columns, under the current GPF_* tuning environment
 * (read once per call), builds the plan run_factor walks (plan_factor, csrc/gpf_plan.hip: the same
 * object, not a second derivation) and decodes every workgroup of every launch with the kernel's
 * own decoder (gpf::step_decode). Checks that every (block column, particle, tile) is computed
 * exactly once (one whole-tile workgroup, or all S depth pieces exactly once, whose S arrivals
 * on a zeroed counter elect exactly one finisher), that pieces stay inside the split-K buffers,
 * and that concurrent particle groups never share partial slots or counters.
 * With the early diagonal factor it also checks that every launch starts with exactly one
 * diagonal workgroup per particle, ahead of all tiles; with the deferred diagonal update
 * (GPF_DEFER_SYRK, default on) that launches 1 .. nt-2 without the all-tile split carry exactly
 * one SYRK workgroup per particle right behind the diagonal workgroups, and no other launch any.
 * Under the persistent factorisation (GPF_PERSIST; default for chunks with more tiles per block
 * column than 512 workgroup slots) it instead decodes every ticket of every work queue with the
 * kernel's own decoder (gpf::p_decode): every (block column, particle, tile) exactly once, one
 * SYRK item per particle and block column 1 .. nt-2, and every item's inputs produced by items
 * earlier in its queue (what makes the persistent launch deadlock-free).
 * Paired block columns (GPF_PAIR; gpf::pair_decode): a lead launch J carries, per particle, every
 * tile of column J once, its SYRK workgroup, one look-ahead partial per tile of column J+1 that
 * exists (the tile's 8 or 16 ids behind, on the same XCD), and the partial SYRK of block J+2; it is
 * followed on its stream by the follow launch J+1, whose tiles read those partials (slots inside
 * the group's buffer).
 * Look-ahead pieces (GPF_LA_ALL; gpf::lall_decode): every piece of a producing launch once, inside
 * the piece buffer, consumed by the next launch of its group, under a tag that carries the group's
 * particle count whole (groups of more than 4095 particles plan without the pieces).
 * stats (nullable, 11 entries): launches, workgroups (persistent: items), whole tiles, split
 * tiles, S (all-tile split factor), largest split factor, particle groups, diagonal
 * workgroups, SYRK workgroups (items), persistent (0/1), lead launches of paired block columns. Returns GPF_OK, or
 * GPF_BAD_ARG with a description of the first violation in msg. */
int gpf_plan_check(int pc, int nt, long long* stats, char* msg, int msg_len);

/* Self-test of the f64 MFMA fragment layout: C = A(16x4) B(4x16) on device,
 * compared on the host by the caller. a: 16x4 row-major, b: 4x16 row-major,
 * c: 16x16 row-major. */
int gpf_selftest_mfma(gpf_ctx* ctx, const double* a, const double* b, double* c);

/* Diagnostic: factorise one particle and copy back its Npad x Npad L and
 * U = L^-1 (row-major; the strict upper triangles hold scratch), the
 * forward-substituted RHS z (Npad) and alpha (N). Npad = ceil(N/128)*128. */
int gpf_debug_factor(gpf_ctx* ctx, const double* ls, double* L, double* U, double* z, double* alpha);

/* Diagnostic / measurement: the 128x128 diagonal-block factor of the factorisation (factor128 in
 * csrc/gpf_diag.hip) on n blocks, one workgroup each. A: n x 128 x 128 row-major (lower triangles
 * read), y: n x 128. Out: L (zeros above the diagonal), U = L^-1 (likewise), z = U y, s2 / sz =
 * the column partials colsum(U o U) and U^T z, bad[b] = 1 where a pivot was not > 0, cycles
 * (nullable): each workgroup's shader cycles. */
int gpf_debug_factor128(gpf_ctx* ctx, const double* A, const double* y, int n, double* L, double* U, double* z,
                        double* s2, double* sz, int* bad, double* cycles);

/* Diagnostic: measured FP64 MFMA throughput (TFLOP/s) of a register-only
 * v_mfma_f64_16x16x4_f64 loop over `blocks` workgroups of 4 waves. */
int gpf_mfma_peak(gpf_ctx* ctx, int blocks, int iters, double* tflops);

/* The shader clock (MHz) the timed launches of the last gpf_mfma_peak or gpf_gemm_bench call
 * held (every workgroup's span in s_memtime clocks over its span in the 100 MHz s_memrealtime
 * clock; 0 before any such call). */
int gpf_bench_clock(gpf_ctx* ctx, double* mhz);

/* Measurement hook: TF/s of the block-column GEMM core alone (no factorisation):
 * P particles' Npad x Npad matrices, `tiles` workgroups per particle, depth D, `iters`
 * timed launches; mode 0 = per-particle operands, mode 1 = one shared (L2-resident) pair; mode
 * bit 2 (4): U-tile-shaped operands; bit 3 (8): zero operands instead of hashed values in [-1, 1);
 * bit 4 (16) / bit 5 (32): the 3- / 4-stage LDS pipeline (one workgroup per CU). */
int gpf_gemm_bench(gpf_ctx* ctx, int mode, int Npad, int P, int tiles, int D, int iters, double* tflops);

#ifdef __cplusplus
}
#endif

#endif /* GPFIT_H */
