// gpf_postcov.hip — joint posterior covariance of a set of query points (latent, noise-free):
//   Sigma = K_ss - K_s^T Kn^-1 K_s = K_ss - V^T V,  V = U K_s,  U = L^-1
// (GP_func.py:38-39 keeps only the diagonal of V^T V; here the whole matrix is formed). Three
// kernels behind the single-particle factorisation: k_predict_v stores V next to the per-column
// sums gpf_predict takes from it, k_post_cov forms the lower 128x128 tiles of K_ss - V^T V with
// FP64 MFMA, k_mirror_lower copies the lower triangle over the upper one.
#pragma once
#include "gpf_common.hip"
#include "gpf_predict.hip"

namespace gpf {

// k_predict_vsq (gpf_predict.hip) plus a store of every tile of V: V row-major Npad x ldks (the
// leading dimension of K_s). Both kernels are predict_tile, so vsq / vz — and the mean
// k_predict_out sums from vz — are bitwise gpf_predict's. The padded rows of U are identity rows
// over zero rows of K_s and the padded query columns of K_s are zero, so V's padding holds exact zeros.
// grid: (nqt, nt)
__global__ __launch_bounds__(Geo<T>::NTH, 4) void k_predict_v(int Npad, const double* __restrict__ U,
                                                       const double* __restrict__ Ks, int ldks,
                                                       double* __restrict__ vsq, const double* __restrict__ z,
                                                       double* __restrict__ vz, double* __restrict__ V) {
  // the deepest row tiles first
  predict_tile<true, false>(Npad, U, Ks, ldks, vsq, z, vz, V, blockIdx.x, (int)gridDim.y - 1 - (int)blockIdx.y);
}

// Lower tile (I, J <= I) of Sigma = K_ss - V^T V: acc = V[:, I]^T V[:, J] over depth Npad, both
// operands [k][c] panels of the row-major V (the TN flavour of the streaming core, as k_lml_grad
// uses it on U: nothing is transposed in memory). Every tile has the same depth, the chunks run
// in ascending k and each element's sum is one MFMA chain: fixed order, no atomics. The panels are
// re-read by the other tiles of the launch (default cache policy). On the diagonal tiles only
// the 16x16 blocks on and below the diagonal are formed (TRI_C_LOWER); what the epilogue writes
// above a tile's diagonal is overwritten by k_mirror_lower.
// Epilogue: C holds K_ss = kernel_func(queries, queries) from k_cross_cov (row-major, ld ldc);
// every element becomes K_ss - acc, and the diagonal elements use the prior variance 1.0 exactly
// (GP_func.py:34) instead of the builder's exp(-0.5 r2), whose r2 can round to a few ulp above 0.
// Tile order: the Mt (Mt - 1) / 2 tiles below the diagonal first (blockIdx.x = I (I - 1) / 2 + J), then
// the Mt diagonal tiles, which issue 36 of the 64 MFMA blocks per k-step: all depths are equal, so
// the lighter tiles go last and form the launch's tail (Mt = 32: 528 tiles on 512 resident
// workgroups, so 16 compute units get a third tile; profiles/predict_cov/tile_order_ab.txt).
// grid: (Mt (Mt + 1) / 2)
__global__ __launch_bounds__(Geo<T>::NTH, 4) void k_post_cov(int Npad, int Mt, const double* __restrict__ V, int ldv,
                                                             double* __restrict__ C, int64_t ldc) {
  __shared__ __attribute__((aligned(16))) double smem[DL_STAGE];
  const int idx = blockIdx.x, noff = Mt * (Mt - 1) / 2;
  int I, J;
  if (idx < noff) {
    I = (int)((sqrt(8.0 * idx + 1.0) + 1.0) * 0.5);
    while (I * (I + 1) / 2 <= idx) ++I;
    while (I * (I - 1) / 2 > idx) --I;
    J = idx - I * (I - 1) / 2;
  } else {
    I = J = idx - noff;
  }
  const Quad<T> qd;
  Acc<T> acc;
  acc.zero();
  if (I == J)
    gemm_stream_dl<true, false, TRI_C_LOWER, 2, false, true>(acc, V + (size_t)I * T, ldv, V + (size_t)J * T, ldv, Npad, smem, qd);
  else
    gemm_stream_dl<true, false, TRI_NONE, 2, false, true>(acc, V + (size_t)I * T, ldv, V + (size_t)J * T, ldv, Npad, smem, qd);
  double* Ct = C + (size_t)I * T * ldc + (size_t)J * T;
  if (I == J) {
    double* p0 = launder(Ct + (size_t)(qd.lane >> 4) * ldc + qd.cb + (qd.lane & 15));
#pragma unroll
    for (int mi = 0; mi < Acc<T>::MBR; ++mi)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        double* p = p0 + (size_t)(mi * 16 + 4 * r) * ldc;
        const double prior = (qd.row(mi, r) == qd.col(0)) ? 1.0 : *p;
        *p = prior - acc.v[mi][0][r];
      }
  } else {
    acc.visit(qd, Ct, (size_t)ldc, [](double& c, double a) { c = c - a; });
  }
}

// Sigma's upper triangle as a copy of the lower one: block (bi, bj <= bi) of 64x64 is read by
// rows, transposed through LDS (row stride 65: both passes conflict-free) and written by rows
// into block (bj, bi), so both sides move in 512-byte row segments; a diagonal block writes only
// its elements above the diagonal. Elements with row or column >= n (the padding) are left alone.
// The matrix is then exactly symmetric. Block index blockIdx.x = bi (bi + 1) / 2 + bj.
// grid: (nb (nb + 1) / 2), nb = ceil(n / 64)
constexpr int MIR_B = 64;
__global__ __launch_bounds__(NTHR) void k_mirror_lower(int n, double* __restrict__ C, int64_t ldc) {
  __shared__ double s[MIR_B][MIR_B + 1];
  const int idx = blockIdx.x, tid = threadIdx.x;
  int bi = (int)((sqrt(8.0 * idx + 1.0) - 1.0) * 0.5);
  while ((bi + 1) * (bi + 2) / 2 <= idx) ++bi;
  while (bi * (bi + 1) / 2 > idx) --bi;
  const int bj = idx - bi * (bi + 1) / 2;
  const int c = tid & (MIR_B - 1), r0 = tid >> 6;  // 4 rows per pass
  for (int r = r0; r < MIR_B; r += NTHR / MIR_B) {
    const int gi = bi * MIR_B + r, gj = bj * MIR_B + c;
    s[r][c] = (gi < n && gj < n) ? C[(size_t)gi * ldc + gj] : 0.0;
  }
  __syncthreads();
  for (int r = r0; r < MIR_B; r += NTHR / MIR_B) {
    const int gi = bj * MIR_B + r, gj = bi * MIR_B + c;  // element (gi, gj) of the upper triangle
    if (gi < n && gj < n && gj > gi) C[(size_t)gi * ldc + gj] = s[c][r];
  }
}

}  // namespace gpf
