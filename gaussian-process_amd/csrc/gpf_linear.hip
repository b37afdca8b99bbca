// gpf_linear.hip — linear functionals of the latent posterior (gpf_predict_linear): with weights
// A (R x M) over M query points,
//   mean = A mu,   cov = A K_ss A^T - V_A^T V_A,   V_A = U (K_s A^T),   U = L^-1,
// without anything of size M x M or Npad x M: the query axis is folded away chunk by chunk. The new
// work is three skinny FP64-MFMA products on the 128-tile streaming core (gemm_stream_dl), all with
// a small output and a deep contraction:
//   B = K_s Wt            Npad x Rpad, depth M   (NN: k_lin_nn on the K_s block of a query chunk)
//   G = K_ss Wt           Mpad x Rpad, depth M   (NN: k_lin_nn on one K_ss block of a chunk pair)
//   Q = Wt^T G, V_A^T V_A Rpad x Rpad, depth M / Npad (TN: k_lin_tn, nothing transposed in memory)
// with Wt = A^T (Mpad x Rpad, zero padded). The output has too few tiles to fill the chip (R <= 128:
// one tile column), so the parallelism comes from the depth: every workgroup takes one output tile
// and one depth piece and writes a partial tile; k_lin_reduce adds the partial tiles of an output
// tile in piece order (as the factorisation's split-K partials are combined: fixed order, no
// atomics) and adds the sum to, or subtracts it from, what the pass started with.
#pragma once
#include "gpf_common.hip"

namespace gpf {

constexpr int LIN_TT = T * T;  // doubles of one partial tile

// Depth pieces of a skinny product: `dt` depth tiles of 128 over `tiles` output tiles. As many pieces
// as bring the launch to LIN_WG workgroups (four per compute unit of a 256-CU device; a constant, so
// that the summation order depends on the shapes alone and not on the device), at least one depth
// tile each. per: depth tiles per piece; returns the number of pieces.
constexpr int LIN_WG = 1024;
__host__ __device__ inline int lin_pieces(int dt, int64_t tiles, int* per) {
  int64_t np = (LIN_WG + tiles - 1) / tiles;
  if (np > dt) np = dt;
  if (np < 1) np = 1;
  *per = (int)((dt + np - 1) / np);
  return (dt + *per - 1) / *per;
}

// Lower-triangular tile index -> (I, J <= I), idx = I (I + 1) / 2 + J
__device__ __forceinline__ void lin_tri(int idx, int& I, int& J) {
  I = (int)((sqrt(8.0 * idx + 1.0) - 1.0) * 0.5);
  while ((I + 1) * (I + 2) / 2 <= idx) ++I;
  while (I * (I + 1) / 2 > idx) --I;
  J = idx - I * (I + 1) / 2;
}

// Partial tile (piece p, row tile rt, column tile ct) of A W: A (rows x depth) a [r][k] row-major
// block of K_s or K_ss with leading dimension lda, W the [k][c] rows of Wt that go with A's columns
// (leading dimension ldw). Piece p covers the depth tiles [p per, min((p + 1) per, dt)). Both panels
// are read by other workgroups of the launch too (A by the other column tiles, W by every row
// tile): default cache policy.
// part: [piece][rt * nct + ct][128 x 128]
// grid: (nrt * nct, pieces)
__global__ __launch_bounds__(Geo<T>::NTH, 4) void k_lin_nn(int nct, int dt, int per, const double* __restrict__ A, int lda,
                                                           const double* __restrict__ W, int ldw,
                                                           double* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) double smem[DL_STAGE];
  const int tile = blockIdx.x, p = blockIdx.y;
  const int rt = tile / nct, ct = tile - rt * nct;
  const int k0 = p * per, k1 = min(k0 + per, dt);
  const Quad<T> qd;
  Acc<T> acc;
  acc.zero();
  gemm_stream_dl<true, false, TRI_NONE, 2, false>(acc, A + (size_t)rt * T * lda + (size_t)k0 * T, lda,
                                                  W + (size_t)k0 * T * ldw + (size_t)ct * T, ldw, (k1 - k0) * T, smem, qd);
  acc.store(qd, part + ((size_t)p * gridDim.x + tile) * LIN_TT, (size_t)T);
}

// Partial lower tile (piece p, I, J <= I) of X^T Y: both operands [k][c] row-major panels with the
// leading dimension ld (the TN flavour of the streaming core, as k_post_cov and k_lml_grad use it).
// part: [piece][I (I + 1) / 2 + J][128 x 128]
// grid: (nrt (nrt + 1) / 2, pieces)
__global__ __launch_bounds__(Geo<T>::NTH, 4) void k_lin_tn(int dt, int per, const double* __restrict__ X,
                                                           const double* __restrict__ Y, int ld,
                                                           double* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) double smem[DL_STAGE];
  const int tile = blockIdx.x, p = blockIdx.y;
  int I, J;
  lin_tri(tile, I, J);
  const int k0 = p * per, k1 = min(k0 + per, dt);
  const Quad<T> qd;
  Acc<T> acc;
  acc.zero();
  gemm_stream_dl<true, false, TRI_NONE, 2, false, true>(acc, X + (size_t)k0 * T * ld + (size_t)I * T, ld,
                                                        Y + (size_t)k0 * T * ld + (size_t)J * T, ld, (k1 - k0) * T, smem, qd);
  acc.store(qd, part + ((size_t)p * gridDim.x + tile) * LIN_TT, (size_t)T);
}

// out tile = base + sgn * (part[0] + part[1] + .. + part[pieces - 1]), the pieces added in order.
// base: nullptr (zero) or a matrix laid out like out (out itself to accumulate over passes).
// tri: the tiles are the lower ones of k_lin_tn (index -> (I, J)); else tile = rt * nct + ct.
// 16 rows x 128 columns per workgroup, a wave on 64 consecutive doubles of a row.
// grid: (tiles, 8)
__global__ __launch_bounds__(NTHR) void k_lin_reduce(int nct, int tri, int pieces, const double* __restrict__ part,
                                                     const double* base, double sgn, double* out, int64_t ldo) {
  const int tile = blockIdx.x, ntile = gridDim.x;
  int I, J;
  if (tri) {
    lin_tri(tile, I, J);
  } else {
    I = tile / nct;
    J = tile - I * nct;
  }
  const int c = threadIdx.x & (T - 1), r0 = blockIdx.y * 16 + (threadIdx.x >> 7);
  const double* pt = part + (size_t)tile * LIN_TT + c;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int r = r0 + 2 * j;
    double s = 0.0;
    for (int p = 0; p < pieces; ++p) s = s + pt[(size_t)p * ntile * LIN_TT + (size_t)r * T];
    const size_t o = ((size_t)I * T + r) * ldo + (size_t)J * T + c;
    out[o] = (base ? base[o] : 0.0) + sgn * s;
  }
}

// Wt = A^T, zero padded: w (R x M row-major, as the caller gave it) -> wt (Mpad x ldt row-major, ldt =
// Rpad). 64 x 64 blocks through LDS (row stride 65), so both sides move in 512-byte row segments.
// grid: (Mpad / 64, Rpad / 64)
__global__ __launch_bounds__(NTHR) void k_lin_wt(int R, int64_t M, const double* __restrict__ w, double* __restrict__ wt,
                                                 int ldt) {
  __shared__ double s[64][65];
  const int c = threadIdx.x & 63, r0 = threadIdx.x >> 6;
  const int64_t q0 = (int64_t)blockIdx.x * 64;
  const int f0 = blockIdx.y * 64;
  for (int r = r0; r < 64; r += NTHR / 64) {  // functional f0 + r, query q0 + c
    const int f = f0 + r;
    const int64_t q = q0 + c;
    s[r][c] = (f < R && q < M) ? w[(size_t)f * M + q] : 0.0;
  }
  __syncthreads();
  for (int r = r0; r < 64; r += NTHR / 64) wt[(size_t)(q0 + r) * ldt + f0 + c] = s[c][r];  // query q0 + r, functional f0 + c
}

// The diagonal of a K_ss block of a chunk with itself: the prior variance 1.0 exactly (GP_func.py:34)
// instead of the builder's exp(-0.5 r2), whose r2 can round to a few ulp above 0 (as k_post_cov does
// for Sigma's diagonal). grid: (ceil(m / 256))
__global__ __launch_bounds__(NTHR) void k_lin_unit_diag(int m, double* __restrict__ blk, int64_t ld) {
  const int i = blockIdx.x * NTHR + threadIdx.x;
  if (i < m) blk[(size_t)i * ld + i] = 1.0;
}

}  // namespace gpf
