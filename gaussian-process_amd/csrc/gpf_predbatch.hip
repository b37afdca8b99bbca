// gpf_predbatch.hip — prediction at the query points for a batch of length-scale samples
// (gpf_predict_batch): the batched factorisation's U and z of every particle of a chunk stay
// resident, V = U K_s of all of them is reduced in one launch, and the particles' (mu, sd) are
// combined into the mixture's mean and sd on the device.
#pragma once
#include "gpf_common.hip"
#include "gpf_covariance.hip"
#include "gpf_predict.hip"

namespace gpf {

// k_predict_vsq (gpf_predict.hip) for the pc particles of a chunk in one launch: the same tile
// (gemm_stream_dl<true, false, TRI_A_LAST, 2, false>) and the same per-lane, lane-group and half sums
// in the same order, so particle p's partials are bitwise what k_predict_vsq gives for its U, K_s
// and z. Per-particle bases: U + p Npad^2, Ks + p ks_stride, z + p Npad, vsq / vz + p nt ldks.
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
  __shared__ __attribute__((aligned(16))) double smem[DL_STAGE];
  const int q = blockIdx.x;
  const int p = order ? (int)blockIdx.y : (int)blockIdx.z;
  const int t = nt - 1 - (order ? (int)blockIdx.z : (int)blockIdx.y);
  U += (size_t)p * Npad * Npad;
  Ks += (size_t)p * ks_stride;
  z += (size_t)p * Npad;
  vsq += (size_t)p * nt * ldks;
  vz += (size_t)p * nt * ldks;
  const Quad<T> qd;
  Acc<T> acc;
  acc.zero();
  gemm_stream_dl<true, false, TRI_A_LAST, 2, false>(acc, U + (size_t)t * T * Npad, Npad, Ks + (size_t)q * T, ldks, (t + 1) * T,
                                                    smem, qd);
  constexpr int MBR = Geo<T>::MBR;
  const double* zt = z + (size_t)t * T + (qd.lane >> 4);
  double half[2], zh[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    double a2 = 0.0, az = 0.0;
#pragma unroll
    for (int mi = h * MBR / 2; mi < (h + 1) * MBR / 2; ++mi)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        a2 = fma(acc.v[mi][0][r], acc.v[mi][0][r], a2);
        az = fma(acc.v[mi][0][r], zt[mi * 16 + 4 * r], az);
      }
    half[h] = sum_lane_groups(a2);
    zh[h] = sum_lane_groups(az);
  }
  if ((qd.lane >> 4) == 0) {
    const size_t o = (size_t)t * ldks + (size_t)q * T + qd.col(0);
    vsq[o] = half[0] + half[1];
    vz[o] = zh[0] + zh[1];
  }
}

// k_cross_cov (gpf_covariance.hip) with the particle on grid axis z: particle p's block with its length
// scales l + p d into out + p ostride. The body is k_cross_cov's, operation for operation, so every
// element is bitwise what launch_cross_cov gives for that particle (tests/test_predict_batch_gpu.py).
// grid: (ceil(C/256), ceil(R/CC_R), pc), dynamic LDS cross_cov_lds(d) bytes
template <int D>
__global__ __launch_bounds__(NTHR) void k_cross_cov_batch(int N1, int N2, int R, int C, int dd,
                                                          const double* __restrict__ x1, int ld1,
                                                          const double* __restrict__ x2, int ld2,
                                                          const double* __restrict__ l, double* __restrict__ out,
                                                          int64_t ldo, size_t ostride) {
  const int d = D > 0 ? D : dd;
  l += (size_t)blockIdx.z * d;
  out += (size_t)blockIdx.z * ostride;
  extern __shared__ double cc_lds[];
  double* ai = cc_lds;                  // [d][CC_R]
  double* aj = ai + (size_t)d * CC_R;   // [d][256]
  double* ni = aj + (size_t)d * CC_C;   // [CC_R]
  double* nj = ni + CC_R;               // [256]
  const int tid = threadIdx.x;
  const int bi = blockIdx.y, bj = blockIdx.x;
  for (int t = tid; t < CC_R + CC_C; t += NTHR) {
    const bool first = t < CC_R;
    const int tt = first ? t : t - CC_R;
    const int g = first ? bi * CC_R + tt : bj * CC_C + tt;
    const int lim = first ? N1 : N2;
    const double* xs = first ? x1 : x2;
    const int ldx = first ? ld1 : ld2;
    double* a = first ? ai : aj;
    const int lda = first ? CC_R : CC_C;
    double nrm = 0.0;
    if (g < lim) {
      for (int k = 0; k < d; ++k) {
        const double v = xs[(size_t)k * ldx + g] / l[k];
        a[k * lda + tt] = v;
        nrm = nrm + v * v;
      }
    }
    (first ? ni : nj)[tt] = nrm;
  }
  __syncthreads();
  const int c = tid & (CC_C - 1);
  const int gj = bj * CC_C + c;
  if (gj >= C) return;
  constexpr int DR = D > 0 ? D : DMAX;
  double bc[DR];
#pragma unroll
  for (int k = 0; k < DR; ++k) bc[k] = (k < d) ? aj[k * CC_C + c] : 0.0;
  const double nc = nj[c];
  const bool colok = gj < N2;
  double* op = out + gj;
  const int r0 = bi * CC_R;
  const int rmax = min(CC_R, R - r0);
#pragma unroll 4
  for (int r = 0; r < rmax; ++r) {
    const int gi = r0 + r;
    double v = 0.0;
    if (gi < N1 && colok) {
      double dot = ai[r] * bc[0];
#pragma unroll
      for (int k = 1; k < DR; ++k)
        if (k < d) dot = fma(ai[k * CC_R + r], bc[k], dot);
      double r2 = (ni[r] + nc) - 2.0 * dot;
      r2 = r2 > 0.0 ? r2 : 0.0;
      v = exp(-0.5 * r2);
    }
    __builtin_nontemporal_store(v, op + (size_t)gi * ldo);
  }
}

inline void launch_cross_cov_batch(hipStream_t stream, int pc, int N1, int N2, int R, int C, int d, const double* x1,
                                   int ld1, const double* x2, int ld2, const double* l, double* out, int64_t ldo,
                                   size_t ostride) {
  const dim3 grid((unsigned)((C + CC_C - 1) / CC_C), (unsigned)((R + CC_R - 1) / CC_R), (unsigned)pc);
  const size_t lds = cross_cov_lds(d);
  switch (d) {
    case 1: hipLaunchKernelGGL(k_cross_cov_batch<1>, grid, dim3(NTHR), lds, stream, N1, N2, R, C, d, x1, ld1, x2, ld2, l, out, ldo, ostride); break;
    case 2: hipLaunchKernelGGL(k_cross_cov_batch<2>, grid, dim3(NTHR), lds, stream, N1, N2, R, C, d, x1, ld1, x2, ld2, l, out, ldo, ostride); break;
    case 3: hipLaunchKernelGGL(k_cross_cov_batch<3>, grid, dim3(NTHR), lds, stream, N1, N2, R, C, d, x1, ld1, x2, ld2, l, out, ldo, ostride); break;
    case 4: hipLaunchKernelGGL(k_cross_cov_batch<4>, grid, dim3(NTHR), lds, stream, N1, N2, R, C, d, x1, ld1, x2, ld2, l, out, ldo, ostride); break;
    default: hipLaunchKernelGGL(k_cross_cov_batch<0>, grid, dim3(NTHR), lds, stream, N1, N2, R, C, d, x1, ld1, x2, ld2, l, out, ldo, ostride); break;
  }
}

// Every particle of the chunk at one chunk of query columns, one thread per (column, particle):
// mu_p = sum_t vz and s = sum_t vsq with t ascending and the variance clipped as in k_predict_out
// (bitwise its mu and sd for the same partials), into the (pc x lde) staging blocks st_mu / st_var
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
  const double* vzp = vz + (size_t)p * nt * ldks;
  const double* vsp = vsq + (size_t)p * nt * ldks;
  double mu = 0.0;
  for (int t = 0; t < nt; ++t) mu = mu + vzp[(size_t)t * ldks + q];
  double s = 0.0;
  for (int t = 0; t < nt; ++t) s = s + vsp[(size_t)t * ldks + q];
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
