// gpf_loo.hip — leave-one-out (LOO) cross-validation for a batch of particles, and the length-scale
// gradient of the LOO log predictive density, from what a factorisation leaves on the device
// (U = L^-1, the s2p / szp partials of diag(Kn^-1) and alpha). Rasmussen & Williams, section 5.4.2.
//
// Fixed amplitude 1, fixed noise e^2, ARD squared-exponential (GP_func.py:49-65). With
// Kn = kernel_func(x, x, l) + diag(e^2), W = Kn^-1 = U^T U, alpha = W y, w_i = W_ii:
//   mu_i = y_i - alpha_i / w_i, sd_i = sqrt(1 / w_i)     (the prediction of the measured y_i from the others)
//   lpd  = sum_i [1/2 log w_i - 1/2 alpha_i^2 / w_i] - N/2 log(2 pi)
// and with c_i = alpha_i / w_i, g_i = 1/2 (1 + alpha_i^2 / w_i) / w_i, u = W c, G = W diag(g) W = B^T B,
// B = diag(sqrt g) W:
//   dlpd/dl_k = sum_{i>j} (u_i alpha_j + u_j alpha_i - 2 G_ij) K_ij (x_ik - x_jk)^2 / l_k^3
// (K_ij the noise-free kernel value). W is stored once per particle (k_loo_w), scaled and mirrored into
// the dense B (k_loo_scale_mirror); G is never stored: every 128x128 tile of it is reduced in
// registers against the kernel derivative (k_loo_grad), as k_lml_grad reduces W.
#pragma once
#include "gpf_common.hip"
#include "gpf_postcov.hip"  // MIR_B

namespace gpf {

// The per-particle vectors of a LOO call, Npad doubles each: [particles][LV_N][Npad]
enum LooVec : int {
  LV_ALPHA = 0,  // alpha = W y
  LV_MU,         // LOO mean
  LV_SD,         // LOO sd
  LV_CS,         // c_i / sqrt(g_i): u = W c = B^T (c / sqrt g)
  LV_SG,         // sqrt(g_i), 0 on the padding
  LV_U,          // u = W c
  LV_N
};

// w_i and alpha_i from the s2p / szp partials, summed over the row tiles t >= i / 128 in tile order
// (as k_points and k_alpha_batch sum them), then every per-point quantity and lpd[p]. Thread t takes
// the points t, t + 256, .. in order; the 256 thread sums of the density terms then fold in a fixed
// tree (as k_lml_value). The padded points get alpha = c = sqrt(g) = 0. grid: (particles)
__global__ __launch_bounds__(NTHR) void k_loo_points(int N, int Npad, int nt, const double* __restrict__ y,
                                                     const double* __restrict__ s2p, const double* __restrict__ szp,
                                                     double* __restrict__ vec, double* __restrict__ lpd) {
  __shared__ double sl[NTHR];
  const int tid = threadIdx.x, p = blockIdx.x;
  const double* a2 = s2p + (size_t)p * nt * Npad;
  const double* az = szp + (size_t)p * nt * Npad;
  double* vp = vec + (size_t)p * LV_N * Npad;
  double dens = 0.0;
  for (int i = tid; i < Npad; i += NTHR) {
    double al = 0.0, mu = 0.0, sd = 0.0, cs = 0.0, sg = 0.0;
    if (i < N) {
      double w = 0.0;
      for (int t = i / T; t < nt; ++t) {
        w = w + a2[(size_t)t * Npad + i];
        al = al + az[(size_t)t * Npad + i];
      }
      const double c = al / w;
      const double q = (al * al) / w;  // the squared pull
      mu = y[i] - c;
      sd = sqrt(1.0 / w);
      sg = sqrt((0.5 * (1.0 + q)) / w);
      cs = c / sg;
      dens = dens + (0.5 * log(w) - 0.5 * q);
    }
    vp[(size_t)LV_ALPHA * Npad + i] = al;
    vp[(size_t)LV_MU * Npad + i] = mu;
    vp[(size_t)LV_SD * Npad + i] = sd;
    vp[(size_t)LV_CS * Npad + i] = cs;
    vp[(size_t)LV_SG * Npad + i] = sg;
  }
  sl[tid] = dens;
  __syncthreads();
  for (int h = NTHR / 2; h > 0; h >>= 1) {
    if (tid < h) sl[tid] = sl[tid] + sl[tid + h];
    __syncthreads();
  }
  if (tid == 0) lpd[p] = sl[0] - 0.5 * (double)N * 1.8378770664093453;  // log(2 pi)
}

// Lower tile (I, J <= I) of W = U^T U for particle blockIdx.y, stored into the particle's Npad x Npad
// row-major matrix at Wm: k_lml_grad's GEMM call unchanged (depth (nt - I) 128, TRI_C_LOWER on the
// diagonal tiles, tile index I (I + 1) / 2 + J so the deepest tiles are dispatched first), with a
// store of the tile in place of the reduction. What a diagonal tile holds above its diagonal is not
// read (k_loo_scale_mirror takes the lower triangle only). grid: (nt (nt + 1) / 2, particles)
__global__ __launch_bounds__(Geo<T>::NTH, 4) void k_loo_w(int Npad, int nt, const double* __restrict__ U,
                                                          double* __restrict__ Wm) {
  __shared__ __attribute__((aligned(16))) double smem[DL_STAGE];
  const int idx = blockIdx.x, p = blockIdx.y;
  int I = (int)((sqrt(8.0 * idx + 1.0) - 1.0) * 0.5);
  while ((I + 1) * (I + 2) / 2 <= idx) ++I;
  while (I * (I + 1) / 2 > idx) --I;
  const int J = idx - I * (I + 1) / 2;
  const Quad<T> qd;
  Acc<T> acc;
  acc.zero();
  const double* Up = U + (size_t)p * Npad * Npad + (size_t)I * T * Npad;  // block row I: the first K
  const int depth = (nt - I) * T;
  if (I == J)
    gemm_stream_dl<true, false, TRI_C_LOWER, 2, false, true>(acc, Up + (size_t)I * T, Npad, Up + (size_t)J * T, Npad, depth,
                                                             smem, qd);
  else
    gemm_stream_dl<true, false, TRI_NONE, 2, false, true>(acc, Up + (size_t)I * T, Npad, Up + (size_t)J * T, Npad, depth,
                                                          smem, qd);
  acc.store(qd, Wm + (size_t)p * Npad * Npad + (size_t)I * T * Npad + (size_t)J * T, (size_t)Npad);
}

// B = diag(sqrt g) W, dense and in place: the 64x64 block (bi, bj <= bi) of the stored lower triangle
// of W is read by rows into LDS (row stride 65, as k_mirror_lower), then written back scaled by its
// rows' sqrt(g) and, transposed, into block (bj, bi) scaled by that block's rows. A diagonal block
// takes its elements above the diagonal from below it. Every element of the Npad x Npad matrix is
// written; rows and columns >= N get exact zeros. No block read here is written by another
// workgroup (the blocks above the diagonal are outputs only). Block index blockIdx.x = bi (bi + 1) / 2 + bj.
// grid: (nb (nb + 1) / 2, particles), nb = Npad / 64
__global__ __launch_bounds__(NTHR) void k_loo_scale_mirror(int N, int Npad, double* __restrict__ Bm,
                                                           const double* __restrict__ vec) {
  __shared__ double s[MIR_B][MIR_B + 1];
  const int idx = blockIdx.x, p = blockIdx.y, tid = threadIdx.x;
  int bi = (int)((sqrt(8.0 * idx + 1.0) - 1.0) * 0.5);
  while ((bi + 1) * (bi + 2) / 2 <= idx) ++bi;
  while (bi * (bi + 1) / 2 > idx) --bi;
  const int bj = idx - bi * (bi + 1) / 2;
  double* Bp = Bm + (size_t)p * Npad * Npad;
  const double* sg = vec + ((size_t)p * LV_N + LV_SG) * Npad;
  const int c = tid & (MIR_B - 1), r0 = tid >> 6;  // 4 rows per pass
  for (int r = r0; r < MIR_B; r += NTHR / MIR_B) {
    const int gi = bi * MIR_B + r, gj = bj * MIR_B + c;
    s[r][c] = (gi < N && gj <= gi) ? Bp[(size_t)gi * Npad + gj] : 0.0;
  }
  __syncthreads();
  for (int r = r0; r < MIR_B; r += NTHR / MIR_B) {
    {
      const int gi = bi * MIR_B + r, gj = bj * MIR_B + c;
      const double v = gj > gi ? s[c][r] : s[r][c];  // (gj > gi: a diagonal block's upper triangle)
      Bp[(size_t)gi * Npad + gj] = (gi < N && gj < N) ? sg[gi] * v : 0.0;
    }
    if (bi != bj) {
      const int gi = bj * MIR_B + r, gj = bi * MIR_B + c;  // element (gi, gj) of the upper triangle
      Bp[(size_t)gi * Npad + gj] = (gi < N && gj < N) ? sg[gi] * s[c][r] : 0.0;
    }
  }
}

// u_a = sum_i W_ia c_i = sum_i B_ia (c_i / sqrt g_i) from the dense B: 64 columns per workgroup, thread
// (q, c) sums the rows q, q + 4, .. of column c in ascending order, the four sums fold as
// (s0 + s1) + (s2 + s3). N^2 reads per particle in 512-byte row segments. grid: (Npad / 64, particles)
__global__ __launch_bounds__(NTHR) void k_loo_u(int N, int Npad, const double* __restrict__ Bm, double* __restrict__ vec) {
  __shared__ double sq[NTHR];
  const int p = blockIdx.y, tid = threadIdx.x;
  const int c = tid & 63, q = tid >> 6, a = blockIdx.x * 64 + c;
  const double* Bp = Bm + (size_t)p * Npad * Npad + a;
  double* vp = vec + (size_t)p * LV_N * Npad;
  const double* cs = vp + (size_t)LV_CS * Npad;
  double s = 0.0;
#pragma unroll 4
  for (int i = q; i < N; i += 4) s = fma(Bp[(size_t)i * Npad], cs[i], s);
  sq[tid] = s;
  __syncthreads();
  if (q == 0) vp[(size_t)LV_U * Npad + a] = a < N ? (sq[c] + sq[64 + c]) + (sq[128 + c] + sq[192 + c]) : 0.0;
}

// LDS of k_loo_grad: k_lml_grad's layout with six T-vectors (n, alpha and u of the rows and columns)
constexpr int LOO_VEC = DL_STAGE;            // n_i | n_j | alpha_i | alpha_j | u_i | u_j, T each
constexpr int LOO_RED = LOO_VEC + 6 * T;     // [8 waves][DMAX]
constexpr int LOO_LDS = LOO_RED + 8 * DMAX;  // doubles (71.6 KiB: two workgroups per CU)
static_assert(2 * DMAX * T <= DL_STAGE, "k_loo_grad: the tile's coordinates fit the GEMM stages");

// Lower tile (I, J <= I) of G = B^T B for particle blockIdx.y, reduced against the kernel derivative:
//   G_IJ = B[:, I]^T B[:, J] over the full depth Npad, both operands [k][c] panels of the row-major B
//   (the call k_post_cov makes on V). B's padding holds exact zeros.
// Epilogue: k_lml_grad's with the weight (u_i alpha_j + u_j alpha_i - 2 G_ij) K_ij: K_ij recomputed
// in k_build_cov's operation order, one exp in flight at a time, then per coordinate k
//   partial[p][tile][k] = sum_{j < i < N} w_ij (x_ik - x_jk)^2
// in k_lml_grad's fixed order (per lane over its 32 rows, the 4 lane groups, the wave's 16 columns,
// the 8 waves). No floating-point atomics. k_lml_grad_sum finishes the sum over the tiles.
// Tile order: all depths are equal, so the nt (nt - 1) / 2 tiles below the diagonal go first
// (blockIdx.x = I (I - 1) / 2 + J) and the lighter diagonal tiles last, as k_post_cov.
// grid: (nt (nt + 1) / 2, particles)
__global__ __launch_bounds__(Geo<T>::NTH, 4) void k_loo_grad(int N, int Npad, int nt, int d,
                                                             const double* __restrict__ x,
                                                             const double* __restrict__ ls,
                                                             const double* __restrict__ Bm,
                                                             const double* __restrict__ vec,
                                                             double* __restrict__ partial) {
  __shared__ __attribute__((aligned(16))) double smem[LOO_LDS];
  const int idx = blockIdx.x, p = blockIdx.y, noff = nt * (nt - 1) / 2;
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
  {
    const double* Bp = Bm + (size_t)p * Npad * Npad;
    if (I == J)
      gemm_stream_dl<true, false, TRI_C_LOWER, 2, false, true>(acc, Bp + (size_t)I * T, Npad, Bp + (size_t)J * T, Npad, Npad,
                                                               smem, qd);
    else
      gemm_stream_dl<true, false, TRI_NONE, 2, false, true>(acc, Bp + (size_t)I * T, Npad, Bp + (size_t)J * T, Npad, Npad,
                                                            smem, qd);
  }
  // (the GEMM ends with a barrier: the stages are free)
  const int tid = threadIdx.x;
  const double* lp = ls + (size_t)p * d;
  const double* vp = vec + (size_t)p * LV_N * Npad;
  double* sa = smem;          // [d][T] rows (block I): scaled coordinates, then the raw ones
  double* sb = smem + d * T;  // [d][T] columns (block J)
  double* na = smem + LOO_VEC;
  double* nb = na + T;
  double* ali = nb + T;
  double* alj = ali + T;
  double* ui = alj + T;
  double* uj = ui + T;
  double* red = smem + LOO_RED;
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
    (rows ? ali : alj)[t] = g < N ? vp[(size_t)LV_ALPHA * Npad + g] : 0.0;
    (rows ? ui : uj)[t] = g < N ? vp[(size_t)LV_U * Npad + g] : 0.0;
  }
  __syncthreads();
  static_assert(Acc<T>::MBC == 1, "one column per lane");
  constexpr int MBR = Acc<T>::MBR;
  const int col = qd.col(0), gj = J * T + col;
  {
    const double nc = nb[col], aj = alj[col], vj = uj[col], b0 = sb[col];
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
        const double w = ((ui[row] * aj + vj * ali[row]) - 2.0 * acc.v[mi][0][r]) * exp(-0.5 * r2);
        double wm = (gj < gi && gi < N) ? w : 0.0;
        // (formed here, as in k_lml_grad: left to the optimiser the exponentials sink into the
        // coordinate loop's preheader and their arguments spill)
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
    partial[((size_t)p * gridDim.x + idx) * d + tid] = s;
  }
}

}  // namespace gpf
