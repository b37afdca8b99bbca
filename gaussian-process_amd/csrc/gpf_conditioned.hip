// gpf_conditioned.hip — the posterior at M query points conditioned on R measured linear
// functionals b = A f + noise, noise_r ~ N(0, s_r^2) independent (gpf_predict_conditioned):
//   H = A Sigma A^T + diag(s^2) = Lh Lh^T,   C = Sigma A^T = K_ss A^T - K_s^T W2,   W2 = U^T V_A,
//   E = C Lh^-T,   g = Lh^-1 (b - A mu),   mu' = mu + E g,   var' = (1 - sum v^2) - sum_r E[., r]^2.
// gpf_predict_linear's pipeline (gpf_linear.hip) leaves V_A, G = K_ss A^T, A Sigma A^T and A mu on the
// device; what is new here is the way back to the query points, a chunk of them per pass:
//   k_con_tn   the rectangular TN skinny product X^T Y with a leading dimension per operand, every
//              output tile (W2 once per call; K_s,chunk^T W2 once per chunk), depth pieces and
//              k_lin_reduce as the products of gpf_linear.hip
//   k_con_h    H and d = b - A mu, identity / zero padding
//   k_con_g    g = Lh^-1 d from the transposed inverse the dense Cholesky's k_dc_inv_* kernels build
//   k_con_out  mu', sd' per query point and chi2 = g . g
// Every sum runs in a fixed order that the shapes and the chunk alone decide; no atomics.
#pragma once
#include "gpf_common.hip"
#include "gpf_linear.hip"
#include "gpf_predict.hip"

namespace gpf {

// Partial tile (piece p, row tile rt, column tile ct) of X^T Y: X a [k][i] row-major panel with the
// leading dimension ldx, Y a [k][r] panel with ldy (the TN flavour of the streaming core, as k_lin_tn;
// that kernel takes one leading dimension and the lower tiles only). Piece p covers the depth tiles
// [p per, min((p + 1) per, dt)). skip: X is lower triangular by tiles (U: X[k][i] = 0 for k < i), the
// depth tiles k < rt hold exact zeros and are left out; a piece that ends up empty stores zeros.
// part: [piece][rt * nct + ct][128 x 128]
// grid: (nrt * nct, pieces)
__global__ __launch_bounds__(Geo<T>::NTH, 4) void k_con_tn(int nct, int dt, int per, int skip, const double* __restrict__ X,
                                                           int ldx, const double* __restrict__ Y, int ldy,
                                                           double* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) double smem[DL_STAGE];
  const int tile = blockIdx.x, p = blockIdx.y;
  const int rt = tile / nct, ct = tile - rt * nct;
  const int k1 = min(p * per + per, dt), k0 = min(max(p * per, skip ? rt : 0), k1);
  const Quad<T> qd;
  Acc<T> acc;
  acc.zero();
  gemm_stream_dl<true, false, TRI_NONE, 2, false, true>(acc, X + (size_t)k0 * T * ldx + (size_t)rt * T, ldx,
                                                        Y + (size_t)k0 * T * ldy + (size_t)ct * T, ldy, (k1 - k0) * T, smem, qd);
  acc.store(qd, part + ((size_t)p * gridDim.x + tile) * LIN_TT, (size_t)T);
}

// H = S + diag(s^2) (Rp x Rp, leading dimension Rp; S = A Sigma A^T with zero padding) with the
// padding's diagonal 1 (the identity block the dense Cholesky expects), and d = b - A mu with zero
// padding. One row per workgroup. grid: (Rp)
__global__ __launch_bounds__(NTHR) void k_con_h(int R, int Rp, const double* __restrict__ S, const double* __restrict__ b,
                                                const double* __restrict__ s, const double* __restrict__ amu,
                                                double* __restrict__ H, double* __restrict__ dv) {
  const int i = blockIdx.x;
  for (int j = threadIdx.x; j < Rp; j += NTHR) {
    double v = S[(size_t)i * Rp + j];
    if (i == j) v = i < R ? v + s[i] * s[i] : 1.0;
    H[(size_t)i * Rp + j] = v;
  }
  if (threadIdx.x == 0) dv[i] = i < R ? b[i] - amu[i] : 0.0;
}

// g = Lh^-1 d from Xt = Lh^-T (upper triangular, leading dimension Rp): g_r = sum_{k <= r} Xt[k][r] d_k,
// k ascending. grid: (Rp / 256 rounded up)
__global__ __launch_bounds__(NTHR) void k_con_g(int Rp, const double* __restrict__ Xt, const double* __restrict__ dv,
                                                double* __restrict__ g) {
  const int r = blockIdx.x * NTHR + threadIdx.x;
  if (r >= Rp) return;
  double a = 0.0;
  for (int k = 0; k <= r; ++k) a = a + Xt[(size_t)k * Rp + r] * dv[k];
  g[r] = a;
}

// The conditioned mean and standard deviation of the query points of one chunk, one thread per
// point: mu and 1 - sum v^2 from the row-tile partials (row_tile_sums, as k_predict_out), then
//   mu' = mu + sum_r E[q][r] g_r,   var' = (1 - sum v^2) - sum_r E[q][r]^2,   r ascending,
// clipped at 1e-12 (GP_func.py:39-40). R4: R rounded up to 4 (E's and g's padding is exact zeros).
// chi2 (nullptr on all chunks but the first): g . g, written by the first thread.
// grid: (ceil(m / 256))
__global__ __launch_bounds__(NTHR) void k_con_out(int nt, int m, const double* __restrict__ vz, int ldks,
                                                  const double* __restrict__ vsq, const double* __restrict__ E, int lde, int R4,
                                                  const double* __restrict__ g, double* __restrict__ mu,
                                                  double* __restrict__ sd, double* __restrict__ chi2) {
  const int q = blockIdx.x * NTHR + threadIdx.x;
  if (q >= m) return;
  double mq, s;
  row_tile_sums(nt, vz, vsq, ldks, q, mq, s);
  const d4* e4 = reinterpret_cast<const d4*>(E + (size_t)q * lde);
  double eg = 0.0, e2 = 0.0;
  for (int r = 0; r < R4; r += 4) {
    const d4 e = e4[r >> 2];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      eg = eg + e[j] * g[r + j];
      e2 = e2 + e[j] * e[j];
    }
  }
  double var = (1.0 - s) - e2;
  var = (var < 1e-12) ? 1e-12 : var;
  mu[q] = mq + eg;
  sd[q] = sqrt(var);
  if (chi2 && q == 0) {
    double x = 0.0;
    for (int r = 0; r < R4; ++r) x = x + g[r] * g[r];
    *chi2 = x;
  }
}

}  // namespace gpf
