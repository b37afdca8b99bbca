// gpf_hyperlml.hip — log marginal likelihood with a prior amplitude a and a noise scale s, and its
// gradient in (l, a, s), for a batch of particles (gpf_lml_hyper_batch).
//
// Model: Kn = a^2 K(l) + s^2 diag(e^2) = a^2 Kt, Kt = K(l) + r diag(e^2), r = (s / a)^2. The
// unit-amplitude Kt is what the factorisation factors (k_build_cov's per-particle noise factor r), so
// with Lt = chol(Kt), Wt = Kt^-1 = Ut^T Ut, alt = Wt y, wt_i = Wt_ii, Q = y^T alt and
// S = sum_i e_i^2 (alt_i^2 / a^2 - wt_i):
//   LML       = -Q / (2 a^2) - sum_i log Lt_ii - N log a - N/2 log(2 pi)
//   dLML/dl_k = sum_{i>j} (alt_i alt_j / a^2 - Wt_ij) K_ij (x_ik - x_jk)^2 / l_k^3
//   dLML/da   = (Q / a^2 - N) / a - (s^2 / a^3) S
//   dLML/ds   = (s / a^2) S
// The gradient in l is k_lml_grad (gpf_lmlgrad.hip) on the vector alt / a; the rest is O(N) per
// particle. At a = s = 1 every operation below that k_lml_value does not have is exact (a division
// by 1, a subtraction of 0), so the value and the l gradient are gpf_lml_batch's bits.
#pragma once
#include "gpf_common.hip"

namespace gpf {

// What k_hyper_value writes per particle: out[p][HV_*]
enum HyperVal : int { HV_LML = 0, HV_Q, HV_DA, HV_DS, HV_N };

// One workgroup per particle. Thread t takes the points t, t + 256, .. in order (k_lml_value's order
// for Q and sum log Lt_ii; wt_i summed over the row tiles t >= i / 128 in tile order, as k_loo_points
// sums it); the 256 thread sums of Q, sum log and S then fold in k_lml_value's fixed tree.
// as: [particles][2] = (a, s). grid: (particles)
__global__ __launch_bounds__(NTHR) void k_hyper_value(int N, int Npad, int nt, const double* __restrict__ y,
                                                      const double* __restrict__ e, const double* __restrict__ alpha,
                                                      const double* __restrict__ L, const double* __restrict__ s2p,
                                                      const double* __restrict__ as, double* __restrict__ out) {
  __shared__ double sy[NTHR], sl[NTHR], ss[NTHR];
  const int tid = threadIdx.x, p = blockIdx.x;
  const double* ap = alpha + (size_t)p * Npad;
  const double* Lp = L + (size_t)p * Npad * Npad;
  const double* a2 = s2p + (size_t)p * nt * Npad;
  const double a = as[2 * p], s = as[2 * p + 1];
  const double ia2 = 1.0 / (a * a);
  double ya = 0.0, ld = 0.0, sv = 0.0;
  for (int i = tid; i < N; i += NTHR) {
    const double al = ap[i];
    ya = fma(y[i], al, ya);
    ld = ld + log(Lp[(size_t)i * (Npad + 1)]);
    double w = 0.0;
    for (int t = i / T; t < nt; ++t) w = w + a2[(size_t)t * Npad + i];
    sv = sv + (e[i] * e[i]) * ((al * al) * ia2 - w);
  }
  sy[tid] = ya;
  sl[tid] = ld;
  ss[tid] = sv;
  __syncthreads();
  for (int h = NTHR / 2; h > 0; h >>= 1) {
    if (tid < h) {
      sy[tid] = sy[tid] + sy[tid + h];
      sl[tid] = sl[tid] + sl[tid + h];
      ss[tid] = ss[tid] + ss[tid + h];
    }
    __syncthreads();
  }
  if (tid == 0) {
    const double Q = sy[0], S = ss[0], n = (double)N;
    const double qa = Q / (a * a);
    double* o = out + (size_t)p * HV_N;
    o[HV_LML] = ((-0.5 * qa - sl[0]) - n * log(a)) - 0.5 * n * 1.8378770664093453;  // log(2 pi)
    o[HV_Q] = Q;
    o[HV_DA] = (qa - n) / a - ((s * s) / (a * a * a)) * S;
    o[HV_DS] = (s / (a * a)) * S;
  }
}

// scaled[p][i] = alpha[p][i] / a_p for i < N: the vector k_lml_grad takes in alpha's place.
// grid: (ceil(N/256), particles)
__global__ __launch_bounds__(NTHR) void k_hyper_scale(int N, int Npad, const double* __restrict__ alpha,
                                                      const double* __restrict__ as, double* __restrict__ scaled) {
  const int i = blockIdx.x * NTHR + threadIdx.x, p = blockIdx.y;
  if (i >= N) return;
  scaled[(size_t)p * Npad + i] = alpha[(size_t)p * Npad + i] / as[2 * p];
}

}  // namespace gpf
