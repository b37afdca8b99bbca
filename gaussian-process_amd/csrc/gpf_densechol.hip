// gpf_densechol.hip — blocked Cholesky factorisation of one dense symmetric matrix that is already
// on the device, and the draw product behind it (gpf_chol_dense, gpf_posterior_draws):
//   L L^T = A + jitter I        over 128-wide block columns, FP64 MFMA on 128-tiles
//   draws = mu + Z L^T          one streamed GEMM per (sample tile, query tile)
// (gpfit.posterior.draws_from takes the same factor with numpy.linalg.cholesky on the host.) The
// factorisation kernels of gpf_factor.hip build their matrix from coordinates; these read a dense
// A (row-major, leading dimension ld, npad = ceil(n / 128) 128 rows, lower triangle only) and work
// in a buffer of their own, so A survives a failed attempt and the next jitter of the ladder needs
// no recomputation.
//
// A's padding must be an identity block (diagonal 1, off-diagonals 0; k_post_cov leaves Sigma that
// way, k_dc_pad_diag does it for an uploaded matrix). The jitter is added to the first n diagonal
// elements only, so the padded rows factor to L = I, are zero off the diagonal all the way and add
// exact zeros to every sum they take part in.
//
// Schedule: k_dc_init copies A's lower tiles (+ jitter) into the L buffer, then per block column J
// three launches on one stream; the stream order is the only synchronisation (no workgroup waits
// for another one: no flags, no spinning):
//   k_dc_diag    (1 workgroup)            factor128 on tile (J, J) in place, U_JJ = L_JJ^-1 to the
//                                         scratch strip, info on a pivot that is not > 0
//   k_dc_finish  (nt - 1 - J workgroups)  L_IJ^T = U_JJ C_IJ^T (tri_to_lds + trmm_acc), in place
//   k_dc_trail   (m (m + 1) / 2 workgroups, m = nt - 1 - J)
//                                         C_IK -= L_IJ L_KJ^T for J < K <= I, depth 128, in place
//                                         (diagonal tiles: lower triangle, syrk_tile)
// The update of block column J is applied to the whole trailing matrix at once, so every launch but
// the diagonal one is as wide as the work that is left: a left-looking order (tile (I, J) formed in
// one pass of depth 128 J) puts at most nt - J workgroups on the chip per launch, 32 of 256 compute
// units at M = 4096 (measured: 8.9 ms there against 2.5 ms for this order).
// Every element's sum is seeded with the element of A and takes the block columns J = 0, 1, .. in
// ascending order, each as one MFMA chain over ascending k continued from the stored value: one fixed
// order whatever the schedule, no floating-point atomics, the same bits on every call.
// Behind the factorisation: the transposed inverse of the factor from the same strip (k_dc_inv_*,
// gpf_predict_conditioned; below, before k_draws).
#pragma once
#include "gpf_common.hip"
#include "gpf_diag.hip"

namespace gpf {

// Identity padding of an uploaded n x n matrix inside its zeroed npad x ld buffer.
// grid: (1), T threads (npad - n < T)
__global__ __launch_bounds__(T) void k_dc_pad_diag(int n, int npad, double* __restrict__ A, int64_t ld) {
  const int i = n + (int)threadIdx.x;
  if (i < npad) A[(size_t)i * ld + i] = 1.0;
}

// lower tile index -> (i, k <= i): the i (i - 1) / 2 + k tiles below the diagonal first, then the nd
// diagonal tiles (the lighter ones form the launch's tail, as in k_post_cov)
__device__ __forceinline__ void dc_tile(int idx, int nd, int& i, int& k) {
  const int noff = nd * (nd - 1) / 2;
  if (idx < noff) {
    i = (int)((sqrt(8.0 * idx + 1.0) + 1.0) * 0.5);
    while (i * (i + 1) / 2 <= idx) ++i;
    while (i * (i - 1) / 2 > idx) --i;
    k = idx - i * (i - 1) / 2;
  } else {
    i = k = idx - noff;
  }
}

// The working copy: lower tile (I, K) of A into L, the jitter added to the diagonal elements of the
// matrix proper. A diagonal tile is written whole, its upper half mirrored from the lower one (the
// 16 x 16 blocks on the diagonal are read in full by syrk_tile and factor128): A's upper triangle is
// never read.
// grid: (nt (nt + 1) / 2), DNTH threads
__global__ __launch_bounds__(DNTH) void k_dc_init(int nt, int n, double jitter, const double* __restrict__ A,
                                                  double* __restrict__ L, int ld) {
  int I, K;
  dc_tile(blockIdx.x, nt, I, K);
  const size_t l = (size_t)ld;
  const double* At = A + (size_t)I * T * l + (size_t)K * T;
  double* Lt = L + (size_t)I * T * l + (size_t)K * T;
  const int tid = threadIdx.x, c2 = 2 * (tid & 63), r0 = tid >> 6;
  for (int r = r0; r < T; r += DNTH / 64) {
    d2 v;
    if (I != K || c2 + 1 <= r) {
      v = *reinterpret_cast<const d2*>(At + (size_t)r * l + c2);
    } else {  // a pair on or right of the diagonal of a diagonal tile
      v.x = c2 <= r ? At[(size_t)r * l + c2] : At[(size_t)c2 * l + r];
      v.y = At[(size_t)(c2 + 1) * l + r];
    }
    if (I == K && I * T + r < n) {
      if (r == c2) v.x = v.x + jitter;
      if (r == c2 + 1) v.y = v.y + jitter;
    }
    *reinterpret_cast<d2*>(Lt + (size_t)r * l + c2) = v;
  }
}

// Words of throw-away scratch behind the U strip: factor128's y segment (read as y, written as z)
// and its two column-partial rows
constexpr int DC_JUNK = 3 * T;

// Block column J, the diagonal block: L's tile (J, J) holds the fully reduced C_JJ (lower 16 x 16
// blocks), becomes L_JJ; U_JJ goes to columns [128 J, 128 J + 128) of the 128 x ld strip Us
// (factor128 writes both tiles with one leading dimension). junk: DC_JUNK doubles, zero on entry of
// the first launch.
// grid: (1), DNTH threads
__global__ __launch_bounds__(DNTH) void k_dc_diag(int J, double* __restrict__ L, double* __restrict__ Us, int ld,
                                                  double* __restrict__ junk, int* __restrict__ info) {
  __shared__ __attribute__((aligned(16))) double lds[DB_LDS];
  const size_t l = (size_t)ld;
  factor128(L + (size_t)J * T * l + (size_t)J * T, Us + (size_t)J * T, l, junk, junk + T, junk + 2 * T, info, lds);
}

// Block column J, the finish of tile I = J + 1 + blockIdx.x: D = C_IJ^T into the accumulators by a
// transposed read (lane (g, c) of the wave with slab cb reads C(cb + c, 16 mi + 4 r + g): 32-byte runs
// of 16 rows per load, every row's 1 KiB used up by the wave's 32 loads), L_IJ^T = U_JJ D by row halves
// as in k_step's L-tile finish, and lane (g, c) gets L(cb + c, 16 jb + 4 e + g): the very elements it
// read, so the tile is finished in place with no hand-off between the waves.
// grid: (nt - 1 - J), DNTH threads
__global__ __launch_bounds__(DNTH) void k_dc_finish(int J, double* __restrict__ L, const double* __restrict__ Us, int ld) {
  __shared__ __attribute__((aligned(16))) double lds[TRI_LDS];
  const int I = J + 1 + (int)blockIdx.x;
  const size_t l = (size_t)ld;
  const Quad<T> qd;
  const int g = qd.lane >> 4, cl = qd.lane & 15;
  double* Lij = L + (size_t)I * T * l + (size_t)J * T;
  Acc<T> acc;
  {
    const double* p0 = launder(Lij + (size_t)(qd.cb + cl) * l + g);
#pragma unroll
    for (int mi = 0; mi < Acc<T>::MBR; ++mi)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc.v[mi][0][r] = p0[mi * 16 + 4 * r];
  }
  tri_to_lds(Us + (size_t)J * T, l, lds);
  double* lrow = launder(Lij + (size_t)(qd.cb + cl) * l + g);
#pragma unroll
  for (int P = 0; P < 4; ++P) {
    d4 o[2];
    switch (P) {
      case 0: trmm_acc<0, false>(o, acc, lds); break;
      case 1: trmm_acc<1, false>(o, acc, lds); break;
      case 2: trmm_acc<2, false>(o, acc, lds); break;
      default: trmm_acc<3, false>(o, acc, lds); break;
    }
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) lrow[16 * (2 * P + j) + 4 * e] = o[j][e];
  }
}

// Block column J, the trailing update: tile (I, K) = (J + 1 + i, J + 1 + k), k <= i < m = nt - 1 - J,
// C_IK -= L_IJ L_KJ^T over depth 128, seeded from the stored tile and stored back: both operands
// [r][k] row panels (the finished tiles of block column J), the A operand negated by the MFMA.
// Diagonal tiles update their lower triangle only (syrk_tile). The L tiles are re-read by the other
// tiles of the launch: default cache policy.
// grid: (m (m + 1) / 2), DNTH threads
__global__ __launch_bounds__(DNTH, 4) void k_dc_trail(int J, int m, double* __restrict__ L, int ld) {
  __shared__ __attribute__((aligned(16))) double smem[DL_STAGE];
  int i, k;
  dc_tile(blockIdx.x, m, i, k);
  const int I = J + 1 + i, K = J + 1 + k;
  const size_t l = (size_t)ld;
  const Quad<T> qd;
  const double* Lij = L + (size_t)I * T * l + (size_t)J * T;
  double* Cik = L + (size_t)I * T * l + (size_t)K * T;
  if (I == K) {
    syrk_tile<false>(Cik, l, Lij, ld, T, smem, qd);
  } else {
    Acc<T> acc;
    acc.load(qd, Cik, l);
    gemm_stream_dl<false, true, TRI_NONE, 2, false>(acc, Lij, ld, L + (size_t)K * T * l + (size_t)J * T, ld, T, smem, qd);
    acc.store(qd, Cik, l);
  }
}

// ---- the transposed inverse of a dense factor: Xt = L^-T (gpf_predict_conditioned's Lh^-T) ----
// Blocked forward substitution over the block rows I = 0, 1, .. of X = L^-1, written for the transpose
// (upper tiles (J, I), J <= I, of Xt; the tiles below the diagonal are not touched: the caller zeroes
// the buffer) so that a product with L^-T reads it as a [k][c] panel:
//   Xt_II = U_II^T                                       k_dc_inv_diag, every block row at once
//   Yt_JI = sum_{J <= K < I} Xt_JK L_IK^T   (J < I)      k_dc_inv_sum, into tile (J, I)
//   Xt_JI = - Yt_JI U_II^T                               k_dc_inv_fin, tile (J, I) in place
// with U_II = L_II^-1 from the strip the factorisation keeps. Two launches per block row I >= 1, ordered
// by the stream alone (block row I reads the finished tiles of the block rows before it); every sum is
// one MFMA chain over ascending k. L (nt 128 x ld, lower tiles), Xt (the same shape and ld), Us (128 x ld).

// grid: (nt), NTHR threads
__global__ __launch_bounds__(NTHR) void k_dc_inv_diag(const double* __restrict__ Us, double* __restrict__ Xt, int ld) {
  const int I = blockIdx.x;
  const size_t l = (size_t)ld;
  const double* u = Us + (size_t)I * T;
  double* x = Xt + (size_t)I * T * l + (size_t)I * T;
  for (int idx = threadIdx.x; idx < T * T; idx += NTHR) {
    const int r = idx >> 7, c = idx & (T - 1);
    x[(size_t)r * l + c] = u[(size_t)c * l + r];
  }
}

// grid: (I), DNTH threads: tile (J, I), J = blockIdx.x
__global__ __launch_bounds__(DNTH, 4) void k_dc_inv_sum(int I, const double* __restrict__ L, double* __restrict__ Xt, int ld) {
  __shared__ __attribute__((aligned(16))) double smem[DL_STAGE];
  const int J = blockIdx.x;
  const size_t l = (size_t)ld;
  const Quad<T> qd;
  Acc<T> acc;
  acc.zero();
  // A = row panel J of Xt from column 128 J ([r][k]); B^T = row panel I of L from the same column
  gemm_stream_dl<false, false, TRI_NONE, 2, false>(acc, Xt + (size_t)J * T * l + (size_t)J * T, ld,
                                                   L + (size_t)I * T * l + (size_t)J * T, ld, (I - J) * T, smem, qd);
  acc.store(qd, Xt + (size_t)J * T * l + (size_t)I * T, l);
}

// grid: (I), DNTH threads: tile (J, I), J = blockIdx.x, read whole by this workgroup alone before it
// is written (gemm_stream_dl ends behind its last transfer and a barrier)
__global__ __launch_bounds__(DNTH, 4) void k_dc_inv_fin(int I, const double* __restrict__ Us, double* __restrict__ Xt, int ld) {
  __shared__ __attribute__((aligned(16))) double smem[DL_STAGE];
  const int J = blockIdx.x;
  const size_t l = (size_t)ld;
  const Quad<T> qd;
  double* t = Xt + (size_t)J * T * l + (size_t)I * T;
  Acc<T> acc;
  acc.zero();
  gemm_stream_dl<false, true, TRI_NONE, 2, false>(acc, t, ld, Us + (size_t)I * T, ld, T, smem, qd);  // - Yt U_II^T
  acc.store(qd, t, l);
}

// draws[s, i] = mu[i] + sum_{j <= i} z[s, j] L[i, j]: tile (sample tile blockIdx.x, query tile I),
// acc = Z[:, 0 : 128 (I + 1)] L[I, 0 : 128 (I + 1)]^T, both operands [r][k] row panels (nothing is
// transposed in memory); L's diagonal tile carries exact zeros above its diagonal. The deepest query
// tiles start first. Z (Spad x ldz) has zero rows past S and zero columns past M; the padded columns
// of the result (mu's padding plus zeros) are never copied out.
// grid: (Spad / 128, Mt), DNTH threads
__global__ __launch_bounds__(DNTH, 4) void k_draws(int Mt, const double* __restrict__ Z, int ldz, const double* __restrict__ L,
                                                   int ldl, const double* __restrict__ mu, double* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) double smem[DL_STAGE];
  const int st = blockIdx.x, I = Mt - 1 - (int)blockIdx.y;
  const Quad<T> qd;
  Acc<T> acc;
  acc.zero();
  gemm_stream_dl<false, false>(acc, Z + (size_t)st * T * ldz, ldz, L + (size_t)I * T * ldl, ldl, (I + 1) * T, smem, qd);
  const double m = mu[(size_t)I * T + qd.col(0)];
  double* p0 = launder(out + ((size_t)st * T + (qd.lane >> 4)) * ldz + (size_t)I * T + qd.col(0));
#pragma unroll
  for (int mi = 0; mi < Acc<T>::MBR; ++mi)
#pragma unroll
    for (int r = 0; r < 4; ++r) p0[(size_t)(mi * 16 + 4 * r) * ldz] = m + acc.v[mi][0][r];
}

}  // namespace gpf
