// gpf_lmlgrad.hip — log marginal likelihood and its length-scale gradient for a batch of
// particles, from what a factorisation leaves on the device (L, U = L^-1, the szp partials of alpha).
//
// Fixed amplitude 1, fixed noise e^2, the context's ARD kernel (gpf_covfn.hip; se: GP_func.py:49-65). With
// Kn = K(x, x, l) + diag(e^2), W = Kn^-1 = U^T U and alpha = W y:
//   LML       = -1/2 y^T alpha - sum_i log L_ii - N/2 log(2 pi)
//   dLML/dl_k = sum_{i>j} (alpha_i alpha_j - W_ij) psi_ij (x_ik - x_jk)^2 / l_k^3
// (psi_ij = cov_dweight<KIND>(r2_ij): the noise-free kernel value K_ij itself under se; the diagonal
// terms vanish and the noise does not depend on l, so only the strict lower triangle is needed). W is never stored: every 128x128 tile of it is
// reduced in registers, as k_predict_vsq reduces V.
#pragma once
#include "gpf_common.hip"
#include "gpf_covfn.hip"

namespace gpf {

// The lower tile (I, J <= I) of index idx = I (I + 1) / 2 + J: the root in floating point, then
// corrected to the exact integers either way
__device__ __forceinline__ void tri_decode(int idx, int& I, int& J) {
  I = (int)((sqrt(8.0 * idx + 1.0) - 1.0) * 0.5);
  while ((I + 1) * (I + 2) / 2 <= idx) ++I;
  while (I * (I + 1) / 2 > idx) --I;
  J = idx - I * (I + 1) / 2;
}

// The same tiles with the nt (nt - 1) / 2 below the diagonal first (idx = I (I - 1) / 2 + J, J < I) and
// the nt diagonal tiles after them: for launches whose diagonal tiles are the lighter ones
__device__ __forceinline__ void tri_decode_offdiag_first(int idx, int nt, int& I, int& J) {
  const int noff = nt * (nt - 1) / 2;
  if (idx < noff) {
    tri_decode(idx, I, J);
    ++I;
  } else {
    I = J = idx - noff;
  }
}

// acc = A[:, I]^T A[:, J] over `depth` rows of the row-major A (leading dimension ld): both operands
// are [k][c] panels (the TN flavour of the streaming core: nothing is transposed in memory). On a
// diagonal tile only the lower triangle is formed (TRI_C_LOWER). Both panels are re-read by other
// tiles of the launch: default cache policy. Ends with a barrier: the stages are free afterwards.
__device__ __forceinline__ void gram_tile(Acc<T>& acc, const double* A, int ld, int I, int J, int depth, double* smem,
                                          const Quad<T>& qd) {
  acc.zero();
  if (I == J)
    gemm_stream_dl<true, false, TRI_C_LOWER, 2, false, true>(acc, A + (size_t)I * T, ld, A + (size_t)J * T, ld, depth, smem, qd);
  else
    gemm_stream_dl<true, false, TRI_NONE, 2, false, true>(acc, A + (size_t)I * T, ld, A + (size_t)J * T, ld, depth, smem, qd);
}

// Lower tile blockIdx.x = I (I + 1) / 2 + J of W = U^T U for particle blockIdx.y (ascending I, so the
// deepest tiles are dispatched first): W_IJ = sum_{K >= I} U_KI^T U_KJ, depth (nt - I) 128. Tiles K < I
// hold zeros (U is lower triangular) and the tiles above the diagonal of d_U are scratch: neither is
// read. U's diagonal blocks carry zeros above their diagonal (factor128) and the padded rows are
// identity rows (k_build_cov pads K with an identity block), so the padding adds exact zeros to every
// W_ij with i, j < N.
__device__ __forceinline__ void w_tile(Acc<T>& acc, int& I, int& J, int Npad, int nt, const double* U, double* smem,
                                       const Quad<T>& qd) {
  tri_decode(blockIdx.x, I, J);
  const double* Up = U + (size_t)blockIdx.y * Npad * Npad + (size_t)I * T * Npad;  // block row I: the first K
  gram_tile(acc, Up, Npad, I, J, (nt - I) * T, smem, qd);
}

// LDS of a gradient kernel with NV per-point vectors besides the squared norms (k_lml_grad: alpha;
// k_loo_grad: alpha, u): the GEMM's two stages, reused by the epilogue for the tile's coordinates
// ([d][T] rows | [d][T] columns, d <= DMAX: exactly DL_STAGE at d = 32), then n_i | n_j and the rows and
// columns of each vector (T each), then the waves' partial sums. In doubles.
template <int NV>
struct GradLds {
  static constexpr int VEC = DL_STAGE;
  static constexpr int RED = VEC + (2 + 2 * NV) * T;  // [8 waves][DMAX]
  static constexpr int LDS = RED + 8 * DMAX;          // NV = 1: 69.6 KiB, NV = 2: 71.6 KiB (two workgroups per CU)
};
static_assert(2 * DMAX * T <= DL_STAGE, "grad_epilogue: the tile's coordinates fit the GEMM stages");

// The epilogue of k_lml_grad and k_loo_grad: acc holds tile (I, J <= I) of a symmetric matrix M for
// particle p (after a GEMM that ended with a barrier), and for every element j < i < N
//   w_ij = weight(rows' vectors at i, columns' vectors at j, M_ij) psi_ij,
// psi_ij = cov_dweight<KIND>(r2_ij) (under se the noise-free kernel value K_ij) recomputed from x and the particle's length scales lp with
// k_build_cov's operation order (d_L holds L by now). Then per coordinate k
//   partial[p][tile][k] = sum_ij w_ij (x_ik - x_jk)^2
// summed in a fixed order: per lane over its 32 rows (ascending), over the 4 lane groups
// (sum_lane_groups), over the wave's 16 columns (xor 8, 4, 2, 1), over the 8 waves in wave order. No
// floating-point atomics: the same inputs give the same bits.
// load(v, g): vector v < NV at point g < N. weight(r, c, m): r[v] and c[v] the vectors at the row and
// at the column.
template <int NV, int KIND = COV_SE, typename Load, typename Weight>
__device__ __forceinline__ void grad_epilogue(Acc<T>& acc, const Quad<T>& qd, double* smem, int I, int J, int p, int N, int d,
                                              const double* __restrict__ x, const double* __restrict__ lp, Load load,
                                              Weight weight, double* __restrict__ partial) {
  const int tid = threadIdx.x;
  double* sa = smem;          // [d][T] rows (block I): scaled coordinates, then the raw ones
  double* sb = smem + d * T;  // [d][T] columns (block J)
  double* na = smem + GradLds<NV>::VEC;
  double* nb = na + T;
  double* vec = nb + T;  // vector v: rows at vec + 2 v T, columns T behind them
  double* red = smem + GradLds<NV>::RED;
  if (tid < 2 * T) {  // as cov_tile_acc: a = x / l, |a|^2 summed over the coordinates in order
    const int t = tid & (T - 1);
    const bool rows = tid < T;
    const int g = (rows ? I : J) * T + t;
    double* a = rows ? sa : sb;
    double nrm = 0.0;
    if (g < N) {
      for (int k = 0; k < d; ++k) {
        const double v = x[(size_t)k * N + g] / lp[k];
        a[k * T + t] = v;
        nrm = nrm + v * v;
      }
    } else {
      for (int k = 0; k < d; ++k) a[k * T + t] = 0.0;  // (padding: finite, masked below)
    }
    (rows ? na : nb)[t] = nrm;
#pragma unroll
    for (int v = 0; v < NV; ++v) vec[(2 * v + (rows ? 0 : 1)) * T + t] = g < N ? load(v, g) : 0.0;
  }
  __syncthreads();
  static_assert(Acc<T>::MBC == 1, "one column per lane");
  constexpr int MBR = Acc<T>::MBR;
  const int col = qd.col(0), gj = J * T + col;
  {
    const double nc = nb[col], b0 = sb[col];
    double cv[NV], rv[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) cv[v] = vec[(2 * v + 1) * T + col];
#pragma unroll
    for (int mi = 0; mi < MBR; ++mi) {
      double dot[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) dot[r] = sa[qd.row(mi, r)] * b0;
      for (int k = 1; k < d; ++k) {
        const double bk = sb[k * T + col];
#pragma unroll
        for (int r = 0; r < 4; ++r) dot[r] = fma(sa[k * T + qd.row(mi, r)], bk, dot[r]);
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = qd.row(mi, r), gi = I * T + row;
        double r2 = (na[row] + nc) - 2.0 * dot[r];
        r2 = r2 > 0.0 ? r2 : 0.0;  // np.maximum(sq_dist, 0)
#pragma unroll
        for (int v = 0; v < NV; ++v) rv[v] = vec[2 * v * T + row];
        const double w = weight(rv, cv, acc.v[mi][0][r]) * cov_dweight<KIND>(r2);
        double wm = (gj < gi && gi < N) ? w : 0.0;
        // (formed here: left to the optimiser, the 32 exponentials sink past the barriers below into the
        // coordinate loop's preheader, and their 32 arguments spill on the way)
        asm volatile("" : "+v"(wm));
        acc.v[mi][0][r] = wm;
        __builtin_amdgcn_sched_barrier(0);  // (one exp at a time, as cov_tile_acc)
      }
    }
  }
  __syncthreads();
  if (tid < 2 * T) {  // the raw coordinates replace the scaled ones
    const int t = tid & (T - 1);
    const bool rows = tid < T;
    const int g = (rows ? I : J) * T + t;
    double* a = rows ? sa : sb;
    for (int k = 0; k < d; ++k) a[k * T + t] = g < N ? x[(size_t)k * N + g] : 0.0;
  }
  __syncthreads();
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  for (int k = 0; k < d; ++k) {
    const double bk = sb[k * T + col];
    double s = 0.0;
#pragma unroll
    for (int mi = 0; mi < MBR; ++mi) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const double df = sa[k * T + qd.row(mi, r)] - bk;
        s = fma(acc.v[mi][0][r], df * df, s);
      }
      __builtin_amdgcn_sched_barrier(0);  // (the row reads in groups of 4: not all 32 in flight)
    }
    s = sum_lane_groups(s);
    s = s + __shfl_xor(s, 8);
    s = s + __shfl_xor(s, 4);
    s = s + __shfl_xor(s, 2);
    s = s + __shfl_xor(s, 1);
    if (qd.lane == 0) red[wave * DMAX + k] = s;
  }
  __syncthreads();
  if (tid < d) {
    double s = red[tid];
#pragma unroll
    for (int w = 1; w < 8; ++w) s = s + red[w * DMAX + tid];
    partial[((size_t)p * gridDim.x + blockIdx.x) * d + tid] = s;
  }
}

// GEMM: lower tile (I, J <= I) of W = U^T U for particle blockIdx.y (w_tile), never stored.
// Weight: (alpha_i alpha_j - W_ij) K_ij (grad_epilogue).
// Tile order: blockIdx.x = I (I + 1) / 2 + J, the deepest tiles first.
// grid: (nt (nt + 1) / 2, particles)
template <int KIND = COV_SE>
__global__ __launch_bounds__(Geo<T>::NTH, 4) void k_lml_grad(int N, int Npad, int nt, int d,
                                                             const double* __restrict__ x,
                                                             const double* __restrict__ ls,
                                                             const double* __restrict__ U,
                                                             const double* __restrict__ alpha,
                                                             double* __restrict__ partial) {
  __shared__ __attribute__((aligned(16))) double smem[GradLds<1>::LDS];
  const int p = blockIdx.y;
  int I, J;
  const Quad<T> qd;
  Acc<T> acc;
  w_tile(acc, I, J, Npad, nt, U, smem, qd);
  const double* ap = alpha + (size_t)p * Npad;
  grad_epilogue<1, KIND>(
      acc, qd, smem, I, J, p, N, d, x, ls + (size_t)p * d, [&](int, int g) { return ap[g]; },
      [](const double* ri, const double* cj, double w) { return ri[0] * cj[0] - w; }, partial);
}

// alpha_c = sum_t szp[p][t][c] over row tiles t >= c / 128, for every particle of the chunk
// (k_alpha: slot 0 only). alpha: [particles][Npad]. grid: (ceil(N/256), particles)
__global__ __launch_bounds__(NTHR) void k_alpha_batch(int N, int Npad, int nt, const double* __restrict__ szp,
                                                      double* __restrict__ alpha) {
  const int c = blockIdx.x * NTHR + threadIdx.x, p = blockIdx.y;
  if (c >= N) return;
  const double* sp = szp + (size_t)p * nt * Npad;
  double a = 0.0;
  for (int t = c / T; t < nt; ++t) a = a + sp[(size_t)t * Npad + c];
  alpha[(size_t)p * Npad + c] = a;
}

// lml[p] = -1/2 y^T alpha - sum_i log L_ii - N/2 log(2 pi). Thread t sums the points t, t + 256, ..
// in order; the 256 thread sums then fold in a fixed tree. grid: (particles)
__global__ __launch_bounds__(NTHR) void k_lml_value(int N, int Npad, const double* __restrict__ y,
                                                    const double* __restrict__ alpha, const double* __restrict__ L,
                                                    double* __restrict__ lml) {
  __shared__ double sy[NTHR], sl[NTHR];
  const int tid = threadIdx.x, p = blockIdx.x;
  const double* ap = alpha + (size_t)p * Npad;
  const double* Lp = L + (size_t)p * Npad * Npad;
  double ya = 0.0, ld = 0.0;
  for (int i = tid; i < N; i += NTHR) {
    ya = fma(y[i], ap[i], ya);
    ld = ld + log(Lp[(size_t)i * (Npad + 1)]);
  }
  sy[tid] = ya;
  sl[tid] = ld;
  __syncthreads();
  for (int h = NTHR / 2; h > 0; h >>= 1) {
    if (tid < h) {
      sy[tid] = sy[tid] + sy[tid + h];
      sl[tid] = sl[tid] + sl[tid + h];
    }
    __syncthreads();
  }
  if (tid == 0) lml[p] = (-0.5 * sy[0] - sl[0]) - 0.5 * (double)N * 1.8378770664093453;  // log(2 pi)
}

// grad[p][k] = (sum over the tiles, in tile order, of partial[p][tile][k]) / l_k^3.
// grid: (particles), DMAX threads
__global__ __launch_bounds__(DMAX) void k_lml_grad_sum(int ntile, int d, const double* __restrict__ partial,
                                                       const double* __restrict__ ls, double* __restrict__ grad) {
  const int k = threadIdx.x, p = blockIdx.x;
  if (k >= d) return;
  const double* pp = partial + (size_t)p * ntile * d + k;
  double s = 0.0;
  for (int t = 0; t < ntile; ++t) s = s + pp[(size_t)t * d];
  const double l = ls[(size_t)p * d + k];
  grad[(size_t)p * d + k] = s / (l * l * l);
}

}  // namespace gpf
