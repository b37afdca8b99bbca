// gpf_covfn.hip — the covariance function family of a context (gpf_set_kernel).
//
// Every kind is a function of the clamped scaled squared distance r2 = sum_k (x_ik / l_k - x_jk / l_k)^2
// that the six evaluation sites compute with kernel_func's operation order (GP_func.py:56-63):
//   K_ij        = phi(r2)
//   dK_ij/dl_k  = psi(r2) (x_ik - x_jk)^2 / l_k^3,   psi = -2 phi'(r2)
//
//   kind          s            phi                          psi
//   se       (0)  -            exp(-r2 / 2)                 phi
//   matern32 (1)  sqrt(3 r2)   (1 + s) exp(-s)              3 exp(-s)
//   matern52 (2)  sqrt(5 r2)   (1 + s + s^2 / 3) exp(-s)    (5/3) (1 + s) exp(-s)
//
// phi(0) = 1 for all three (the "prior variance exactly 1.0 on the diagonal" rules of k_post_cov and
// gpf_linear.hip hold for every kind) and psi is finite at r2 = 0, so coincident points need no
// special case. The kind is a template constant of every kernel that reaches an evaluation site:
// the squared-exponential instantiations are textually the code they were before the family existed.
#pragma once
#include "gpf_common.hip"

#include <type_traits>

namespace gpf {

enum CovKind { COV_SE = 0, COV_MATERN32 = 1, COV_MATERN52 = 2 };
constexpr int COV_NKIND = 3;

// phi(r2), r2 >= 0. Plain C++ in a fixed operation order (gpfit/kernels.py has the same one); sqrt
// and exp are the device libm's.
template <int KIND>
__device__ __forceinline__ double cov_value(double r2) {
  if constexpr (KIND == COV_MATERN32) {
    const double s = sqrt(3.0 * r2);
    return (1.0 + s) * exp(-s);
  } else if constexpr (KIND == COV_MATERN52) {
    const double s = sqrt(5.0 * r2);
    return ((1.0 + s) + (s * s) / 3.0) * exp(-s);
  } else {
    static_assert(KIND == COV_SE, "unknown covariance kind");
    return exp(-0.5 * r2);
  }
}

// psi(r2) = -2 phi'(r2), r2 >= 0: the factor of (x_ik - x_jk)^2 / l_k^3 in dK_ij/dl_k.
template <int KIND>
__device__ __forceinline__ double cov_dweight(double r2) {
  if constexpr (KIND == COV_MATERN32) {
    const double s = sqrt(3.0 * r2);
    return 3.0 * exp(-s);
  } else if constexpr (KIND == COV_MATERN52) {
    const double s = sqrt(5.0 * r2);
    return ((5.0 / 3.0) * (1.0 + s)) * exp(-s);
  } else {
    static_assert(KIND == COV_SE, "unknown covariance kind");
    return exp(-0.5 * r2);
  }
}

inline bool cov_kind_known(int kind) { return kind >= 0 && kind < COV_NKIND; }

// The run-time kind as the kernels' template constant: f(std::integral_constant<int, KIND>()), as
// with_cross_cov_dim does for the dimension. An unknown kind (gpf_set_kernel admits none) runs se.
template <typename F>
inline void with_cov_kind(int kind, F f) {
  switch (kind) {
    case COV_MATERN32: f(std::integral_constant<int, COV_MATERN32>()); break;
    case COV_MATERN52: f(std::integral_constant<int, COV_MATERN52>()); break;
    default: f(std::integral_constant<int, COV_SE>()); break;
  }
}

}  // namespace gpf
