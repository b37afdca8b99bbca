// gpf_predbatch.hip — prediction at the query points for a batch of length-scale samples
// (gpf_predict_batch): the batched factorisation's U and z of every particle of a chunk stay
// resident, V = U K_s of all of them is reduced in one launch, and the particles' (mu, sd) are
// combined into the mixture's mean and sd on the device.
#pragma once
#include "gpf_common.hip"
#include "gpf_covariance.hip"
#include "gpf_predict.hip"

namespace gpf {

// k_predict_vsq (gpf_predict.hip) for the pc particles of a chunk in one launch: predict_tile on
// particle p's bases, so its partials are bitwise what k_predict_vsq gives for its U, K_s and z.
// Per-particle bases: U + p Npad^2, Ks + p ks_stride, z + p Npad, vsq / vz + p nt ldks.
// The dispatch order is x fastest, then y, then z:
//   order 0: grid (nqt, nt, pc) — one particle after the other, each deepest row tile first (a
//            particle's U row tile and K_s chunk meet in L2 and the Infinity Cache);
//   order 1: grid (nqt, pc, nt) — the deepest row tiles of all particles first (shortest tail).
// DESIGN.md §2h has the A/B.
__global__ __launch_bounds__(Geo<T>::NTH, 4) void k_predict_vsq_batch(int Npad, int nt, const double* __restrict__ U,
                                                               const double* __restrict__ Ks, int ldks,
                                                               size_t ks_stride, double* __restrict__ vsq,
                                                               const double* __restrict__ z,
                                                               double* __restrict__ vz, int order) {
  const int p = order ? (int)blockIdx.y : (int)blockIdx.z;
  const int t = nt - 1 - (order ? (int)blockIdx.z : (int)blockIdx.y);
  const size_t po = (size_t)p * nt * ldks;
  predict_tile<false, false>(Npad, U + (size_t)p * Npad * Npad, Ks + (size_t)p * ks_stride, ldks, vsq + po,
                             z + (size_t)p * Npad, vz + po, nullptr, blockIdx.x, t);
}

// k_cross_cov (gpf_covariance.hip) with the particle on grid axis z: cross_cov_block with particle
// p's length scales l + p d into out + p ostride, so every element is bitwise what launch_cross_cov
// gives for that particle (tests/test_predict_batch_gpu.py).
// grid: (ceil(C/256), ceil(R/CC_R), pc), dynamic LDS cross_cov_lds(d) bytes
template <int D, int KIND = COV_SE>
__global__ __launch_bounds__(NTHR) void k_cross_cov_batch(int N1, int N2, int R, int C, int dd,
                                                          const double* __restrict__ x1, int ld1,
                                                          const double* __restrict__ x2, int ld2,
                                                          const double* __restrict__ l, double* __restrict__ out,
                                                          int64_t ldo, size_t ostride) {
  cross_cov_block<D, KIND>(N1, N2, R, C, dd, x1, ld1, x2, ld2, l + (size_t)blockIdx.z * (D > 0 ? D : dd),
                     out + (size_t)blockIdx.z * ostride, ldo);
}

inline void launch_cross_cov_batch(hipStream_t stream, int kind, int pc, int N1, int N2, int R, int C, int d, const double* x1,
                                   int ld1, const double* x2, int ld2, const double* l, double* out, int64_t ldo,
                                   size_t ostride) {
  const dim3 grid((unsigned)((C + CC_C - 1) / CC_C), (unsigned)((R + CC_R - 1) / CC_R), (unsigned)pc);
  with_cov_kind(kind, [&](auto KIND) {
    with_cross_cov_dim(d, [&](auto D) {
      hipLaunchKernelGGL((k_cross_cov_batch<D(), KIND()>), grid, dim3(NTHR), cross_cov_lds(d), stream, N1, N2, R, C, d, x1, ld1, x2,
                         ld2, l, out, ldo, ostride);
    });
  });
}

// Every particle of the chunk at one chunk of query columns, one thread per (column, particle):
// mu_p and s from row_tile_sums and the variance clipped as in k_predict_out (bitwise its mu and sd
// for the same partials), into the (pc x lde) staging blocks st_mu / st_var
// and, where the caller wants every particle's own prediction, sd_p = sqrt(var_p) into each_sd.
// (Apart from k_predict_mix: one thread per column walking every particle's partials would run
// 2 nt pc loads one behind the other — 4096 at N=4096, P=64, over a millisecond per pass whatever
// the column count; here they spread over pc times as many threads.)
// grid: (ceil(m/256), pc)
__global__ __launch_bounds__(NTHR) void k_predict_each(int nt, int m, const double* __restrict__ vz,
                                                       const double* __restrict__ vsq, int ldks,
                                                       double* __restrict__ st_mu, double* __restrict__ st_var,
                                                       double* __restrict__ each_sd, int64_t lde) {
  const int q = blockIdx.x * NTHR + threadIdx.x, p = blockIdx.y;
  if (q >= m) return;
  double mu, s;
  row_tile_sums(nt, vz + (size_t)p * nt * ldks, vsq + (size_t)p * nt * ldks, ldks, q, mu, s);
  double var = 1.0 - s;
  var = (var < 1e-12) ? 1e-12 : var;
  st_mu[(size_t)p * lde + q] = mu;
  st_var[(size_t)p * lde + q] = var;
  if (each_sd) each_sd[(size_t)p * lde + q] = sqrt(var);
}

// One thread per query column walks the chunk's particles in order and folds their (mu_p, var_p)
// into the column's state (W, m, S, V), four rows of leading dimension ldst kept on the device
// across the particle chunks, by West's weighted update:
//   W += w, delta = mu_p - m, m += (w / W) delta, S += w delta (mu_p - m), V += w var_p.
// A particle with w = 0 is predicted but not folded in. Every column is independent of the others.
// grid: (ceil(m/256))
__global__ __launch_bounds__(NTHR) void k_predict_mix(int m, int pc, const double* __restrict__ st_mu,
                                                      const double* __restrict__ st_var, int64_t lde,
                                                      const double* __restrict__ w, double* __restrict__ state,
                                                      int64_t ldst) {
  const int q = blockIdx.x * NTHR + threadIdx.x;
  if (q >= m) return;
  double W = state[q], mean = state[ldst + q], S = state[2 * ldst + q], V = state[3 * ldst + q];
  for (int p = 0; p < pc; ++p) {
    const double mu = st_mu[(size_t)p * lde + q], var = st_var[(size_t)p * lde + q];
    const double wp = w[p];
    if (wp != 0.0) {
      W = W + wp;
      const double delta = mu - mean;
      mean = mean + (wp / W) * delta;
      S = S + wp * delta * (mu - mean);
      V = V + wp * var;
    }
  }
  state[q] = W;
  state[ldst + q] = mean;
  state[2 * ldst + q] = S;
  state[3 * ldst + q] = V;
}

// mix_mu = m, mix_sd = sqrt((V + S) / W): the law of total variance. grid: (ceil(M/256))
__global__ __launch_bounds__(NTHR) void k_predict_mix_out(int64_t M, const double* __restrict__ state, int64_t ldst,
                                                          double* __restrict__ mix_mu, double* __restrict__ mix_sd) {
  const int64_t q = (int64_t)blockIdx.x * NTHR + threadIdx.x;
  if (q >= M) return;
  mix_mu[q] = state[ldst + q];
  mix_sd[q] = sqrt((state[3 * ldst + q] + state[2 * ldst + q]) / state[q]);
}

}  // namespace gpf
