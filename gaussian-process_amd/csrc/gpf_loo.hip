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
#include "gpf_lmlgrad.hip"  // tri_decode, gram_tile, w_tile, grad_epilogue
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
// row-major matrix at Wm: k_lml_grad's GEMM and tile order (w_tile), with a store of the tile in place
// of the reduction. What a diagonal tile holds above its diagonal is not read (k_loo_scale_mirror takes
// the lower triangle only). grid: (nt (nt + 1) / 2, particles)
__global__ __launch_bounds__(Geo<T>::NTH, 4) void k_loo_w(int Npad, int nt, const double* __restrict__ U,
                                                          double* __restrict__ Wm) {
  __shared__ __attribute__((aligned(16))) double smem[DL_STAGE];
  int I, J;
  const Quad<T> qd;
  Acc<T> acc;
  w_tile(acc, I, J, Npad, nt, U, smem, qd);
  acc.store(qd, Wm + (size_t)blockIdx.y * Npad * Npad + (size_t)I * T * Npad + (size_t)J * T, (size_t)Npad);
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
  int bi, bj;
  tri_decode(idx, bi, bj);
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

// GEMM: lower tile (I, J <= I) of G = B^T B for particle blockIdx.y over the full depth Npad (the call
// k_post_cov makes on V; B's padding holds exact zeros), never stored.
// Weight: (u_i alpha_j + u_j alpha_i - 2 G_ij) K_ij (grad_epilogue; k_lml_grad_sum finishes the sum
// over the tiles).
// Tile order: all depths are equal, so the tiles below the diagonal go first and the lighter diagonal
// tiles last (tri_decode_offdiag_first), as k_post_cov.
// grid: (nt (nt + 1) / 2, particles)
template <int KIND = COV_SE>
__global__ __launch_bounds__(Geo<T>::NTH, 4) void k_loo_grad(int N, int Npad, int nt, int d,
                                                             const double* __restrict__ x,
                                                             const double* __restrict__ ls,
                                                             const double* __restrict__ Bm,
                                                             const double* __restrict__ vec,
                                                             double* __restrict__ partial) {
  __shared__ __attribute__((aligned(16))) double smem[GradLds<2>::LDS];
  const int p = blockIdx.y;
  int I, J;
  tri_decode_offdiag_first(blockIdx.x, nt, I, J);
  const Quad<T> qd;
  Acc<T> acc;
  gram_tile(acc, Bm + (size_t)p * Npad * Npad, Npad, I, J, Npad, smem, qd);
  const double* vp = vec + (size_t)p * LV_N * Npad;
  grad_epilogue<2, KIND>(
      acc, qd, smem, I, J, p, N, d, x, ls + (size_t)p * d,
      [&](int v, int g) { return vp[(size_t)(v == 0 ? LV_ALPHA : LV_U) * Npad + g]; },
      [](const double* ri, const double* cj, double m) { return (ri[1] * cj[0] + cj[1] * ri[0]) - 2.0 * m; }, partial);
}

}  // namespace gpf
