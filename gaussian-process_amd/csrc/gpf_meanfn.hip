// gpf_meanfn.hip — a polynomial mean function with its coefficients integrated out under a flat prior
// (Rasmussen & Williams 2.7): f(x) = h(x)^T beta + g(x), g the GP every other call models, h a few
// fixed basis functions. gpf_lml_mean_batch: the restricted log marginal likelihood (REML) and its
// gradient in (l, a, s) for a batch of particles; gpf_predict_mean: the prediction with the share of
// not knowing beta in its variance.
//
// Notation as gpf_hyperlml.hip (Kn = a^2 Kt, Kt = K(l) + r diag(e^2), r = (s / a)^2, Lt = chol(Kt),
// U = Lt^-1, z = U y, alt = U^T z, wt_i = (U^T U)_ii), and with H (m x N, 1 <= m <= 32) the basis at
// the training points:
//   Z  = U H^T (N x m),  At = Z^T Z = H Kt^-1 H^T = La La^T,  Zo = Z La^-T (orthonormal columns),
//   t  = Zo^T z,  beta = La^-T t,  zr = z - Zo t,  Q' = zr^T zr,
//   Bt = Zo^T U (m x N),  Pt = U^T U - Bt^T Bt,  at = Pt y = alt - Bt^T t,  pt_i = wt_i - sum_r Bt_ri^2,
//   S' = sum_i e_i^2 (at_i^2 / a^2 - pt_i)
//   LML       = -Q' / (2 a^2) - sum log Lt_ii - sum log La_rr - (N - m) log a - (N - m)/2 log(2 pi)
//   dLML/dl_k = sum_{i>j} (at_i at_j / a^2 - Pt_ij) K_ij (x_ik - x_jk)^2 / l_k^3
//   dLML/da   = (Q' / a^2 - (N - m)) / a - (s^2 / a^3) S'
//   dLML/ds   = (s / a^2) S'
// Q' is the sum of squares of the residual zr, never y^T alt - c^T beta: with an offset of 1e3 in y
// that difference loses what the residual keeps. No floating-point atomics; every sum runs in an
// order the shapes alone decide.
//
// mpad is m rounded up to 16 (16 or 32): the panels H (mpad x Npad), Z / Zo (Npad x mpad) and Bt
// (mpad x Npad) carry exact zeros in their padding.
#pragma once
#include "gpf_common.hip"
#include "gpf_lmlgrad.hip"
#include "gpf_predict.hip"

namespace gpf {

constexpr int MEAN_MAX = 32;           // basis functions at most
constexpr int MEAN_LD = MEAN_MAX + 1;  // La in LDS: row stride (odd: a column read spreads over the banks)

// What k_mean_small and k_mean_hyper write per particle: out[p][MV_*] (MV_SLA: sum log La_rr; an even
// count, so that the vectors behind it in the call's buffer keep their 16-byte alignment)
enum MeanVal : int { MV_LML = 0, MV_Q, MV_DA, MV_DS, MV_BAD, MV_SLA, MV_N };
static_assert(MV_N % 2 == 0, "MeanBufs: Z's 16-byte loads");

// ----------------------------------------------------------------------------
// The skinny triangular products with U, FP64 16x16x4 MFMA, every wave on a 16-row (NN) or
// 16-column (TN) slab of its 128-wide tile of U and NB = mpad / 16 accumulator blocks. U has no
// reuse inside a workgroup (every element feeds one MFMA per block), so it goes global -> VGPR
// directly, not through LDS; the narrow operand (H, Zo) is shared by the 8 waves through L1/L2.
// Both kernels read each lower tile of a particle's U exactly once and nothing above the block
// diagonal of d_U (scratch); the diagonal blocks hold zeros above their diagonal and the padded rows
// are identity rows, so with zero padding in H the padding of Z and Bt is exact zeros.
// ----------------------------------------------------------------------------

// Z = U H^T: row tile I = nt - 1 - blockIdx.x (the deepest first) of particle blockIdx.y sums the
// column tiles J <= I, depth (I + 1) 128 in ascending chunks of 16. Per chunk a lane (row r = lane & 15,
// group g = lane >> 4) fetches the pairs k0 + 2 g and k0 + 8 + 2 g of its row of U (64 contiguous
// bytes per row and instruction) and the same pairs of its row of H: MFMA step e then contracts the
// four depths the four groups hold in element e, the same for both operands.
// Hp: [16 NB][Npad]. Z: [particles][Npad][16 NB]. grid: (nt, particles), 512 threads
template <int NB>
__global__ __launch_bounds__(DNTH) void k_mean_nn(int Npad, int nt, const double* __restrict__ U,
                                                  const double* __restrict__ Hp, double* __restrict__ Z) {
  constexpr int MP = 16 * NB, UN = 4;  // UN chunks in flight per iteration (T is a multiple of 16 UN)
  const int I = nt - 1 - (int)blockIdx.x, p = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 15, g = lane >> 4;
  const int row0 = I * T + wave * 16;
  const double* ur = U + (size_t)p * Npad * Npad + (size_t)(row0 + r) * Npad + 2 * g;
  const double* hr = Hp + (size_t)r * Npad + 2 * g;
  d4 acc[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) acc[b] = d4{0.0, 0.0, 0.0, 0.0};
  const int depth = (I + 1) * T;
#pragma unroll 1
  for (int k0 = 0; k0 < depth; k0 += 16 * UN) {
    d2 u[UN][2], h[UN][NB][2];
#pragma unroll
    for (int c = 0; c < UN; ++c) {
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        u[c][j] = *reinterpret_cast<const d2*>(ur + k0 + 16 * c + 8 * j);
#pragma unroll
        for (int b = 0; b < NB; ++b) h[c][b][j] = *reinterpret_cast<const d2*>(hr + (size_t)(16 * b) * Npad + k0 + 16 * c + 8 * j);
      }
    }
#pragma unroll
    for (int c = 0; c < UN; ++c)
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int b = 0; b < NB; ++b) acc[b] = mfma(u[c][e >> 1][e & 1], h[c][b][e >> 1][e & 1], acc[b]);
  }
  double* zp = Z + (size_t)p * Npad * MP + (size_t)(row0 + g) * MP + r;
#pragma unroll
  for (int b = 0; b < NB; ++b)
#pragma unroll
    for (int e = 0; e < 4; ++e) zp[(size_t)(4 * e) * MP + 16 * b] = acc[b][e];
}

// X^T U for the narrow X = Zo (Npad x 16 NB): column tile J = blockIdx.x (the deepest first) of particle
// blockIdx.y sums the row tiles I >= J, depth (nt - J) 128 in ascending steps of 4: lane (index
// c = lane & 15, group g) holds X[k][16 b + c] as the A operand and U[k][its column] as the B operand
// at k = k0 + g. out(row i of X^T U, column j) goes to out[i * rs + j * cs] of the particle's block
// of `ostride` doubles: Bt as [16 NB][Npad] (rs = Npad, cs = 1), or its transpose in a wider panel.
// nout (nullable): the negated product, laid out like out (k_mean_grad's A panel).
// grid: (nt, particles), 512 threads
template <int NB>
__global__ __launch_bounds__(DNTH) void k_mean_tn(int Npad, int nt, const double* __restrict__ U,
                                                  const double* __restrict__ X, double* __restrict__ out,
                                                  double* __restrict__ nout, size_t ostride, int rs, int cs) {
  constexpr int MP = 16 * NB, UN = 4;
  const int J = blockIdx.x, p = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int c = lane & 15, g = lane >> 4;
  const int col0 = J * T + wave * 16;
  const double* uc = U + (size_t)p * Npad * Npad + (size_t)(J * T + g) * Npad + col0 + c;
  const double* xc = X + (size_t)p * Npad * MP + (size_t)(J * T + g) * MP + c;
  d4 acc[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) acc[b] = d4{0.0, 0.0, 0.0, 0.0};
  const int depth = (nt - J) * T;
#pragma unroll 1
  for (int k0 = 0; k0 < depth; k0 += 16 * UN) {
    double u[4 * UN], x[4 * UN][NB];
#pragma unroll
    for (int s = 0; s < 4 * UN; ++s) {
      u[s] = uc[(size_t)(k0 + 4 * s) * Npad];
#pragma unroll
      for (int b = 0; b < NB; ++b) x[s][b] = xc[(size_t)(k0 + 4 * s) * MP + 16 * b];
    }
#pragma unroll
    for (int s = 0; s < 4 * UN; ++s)
#pragma unroll
      for (int b = 0; b < NB; ++b) acc[b] = mfma(x[s][b], u[s], acc[b]);
  }
  double* op = out + (size_t)p * ostride + (size_t)g * rs + (size_t)(col0 + c) * cs;
#pragma unroll
  for (int b = 0; b < NB; ++b)
#pragma unroll
    for (int e = 0; e < 4; ++e) op[(size_t)(16 * b + 4 * e) * rs] = acc[b][e];
  if (nout) {
    double* np = nout + (op - out);
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
      for (int e = 0; e < 4; ++e) np[(size_t)(16 * b + 4 * e) * rs] = -acc[b][e];
  }
}

// The partials of At = Z^T Z: row tile blockIdx.x (128 points) of particle blockIdx.y, staged in LDS, gives
// part[p][tile][r][c] = sum over the tile's rows in order of Z[i][r] Z[i][c] for c <= r < m (k_mean_small
// adds the tiles in order). One workgroup per particle for the whole sum took 2 ms of the 64-particle
// batch at N = 4096: the sum is N m^2 / 2 long and 64 workgroups leave three quarters of the chip idle.
// part: [particles][nt][MP * MP]. grid: (nt, particles)
template <int MP>
__global__ __launch_bounds__(NTHR) void k_mean_gram(int Npad, int nt, int m, const double* __restrict__ Z,
                                                    double* __restrict__ part) {
  __shared__ double sz[T * MP];
  const int tid = threadIdx.x, tile = blockIdx.x, p = blockIdx.y;
  const double* Zt = Z + (size_t)p * Npad * MP + (size_t)tile * T * MP;
  for (int idx = tid; idx < T * MP; idx += NTHR) sz[idx] = Zt[idx];
  __syncthreads();
  double* out = part + ((size_t)p * nt + tile) * MP * MP;
  for (int idx = tid; idx < MP * MP; idx += NTHR) {
    const int r = idx / MP, c = idx - r * MP;
    if (c > r || r >= m) continue;
    double s = 0.0;
    for (int i = 0; i < T; ++i) s = fma(sz[i * MP + r], sz[i * MP + c], s);
    out[idx] = s;
  }
}

// ----------------------------------------------------------------------------
// One workgroup per particle, plain FP64: At = Z^T Z (k_mean_gram's partials, the row tiles in order),
// its Cholesky factor La (right-looking, in LDS; a pivot <= 0 or NaN sets the bad flag and is replaced
// by 1 so that the rest stays finite work), Zo = Z La^-T in place (row by row, forward substitution
// in registers), t = Zo^T z (per thread over its points t, t + 256, .. in order, then the lanes of a
// wave by xor 32 .. 1, then the 4 waves in order), beta = La^-T t, zr = z - Zo t, and with
// k_hyper_value's orders and tree Q' = zr^T zr and sum log Lt_ii, then the value. Also Lai = La^-1
// ([particles][32][32], lower triangular, zero padding).
// as: [particles][2] = (a, s). La's padding is the identity, so the padded columns of Zo stay zero.
// grid: (particles)
// ----------------------------------------------------------------------------
template <int MP>
__global__ __launch_bounds__(NTHR) void k_mean_small(int N, int Npad, int nt, int m, double* __restrict__ Z,
                                                     const double* __restrict__ gram,
                                                     const double* __restrict__ z, const double* __restrict__ L,
                                                     const double* __restrict__ as, double* __restrict__ out,
                                                     double* __restrict__ tvec, double* __restrict__ beta,
                                                     double* __restrict__ Lai, double* __restrict__ zr) {
  __shared__ double sA[MEAN_MAX * MEAN_LD], sI[MEAN_MAX * MEAN_LD], st[MEAN_MAX], sb[MEAN_MAX], sw[4 * MEAN_MAX], sy[NTHR],
      sl[NTHR];
  __shared__ int sbad;
  const int tid = threadIdx.x, p = blockIdx.x;
  double* Zp = Z + (size_t)p * Npad * MP;
  const double* gp = gram + (size_t)p * nt * MP * MP;
  const double* zp = z + (size_t)p * Npad;
  const double* Lp = L + (size_t)p * Npad * Npad;
  double* zrp = zr + (size_t)p * Npad;
  if (tid == 0) sbad = 0;
  for (int idx = tid; idx < MEAN_MAX * MEAN_LD; idx += NTHR) sA[idx] = 0.0;
  __syncthreads();
  // At, lower triangle; the identity on the padding's diagonal
  for (int idx = tid; idx < MP * MP; idx += NTHR) {
    const int r = idx / MP, c = idx - r * MP;
    if (c > r) continue;
    double s = 0.0;
    if (r < m) {
      for (int t = 0; t < nt; ++t) s = s + gp[(size_t)t * MP * MP + idx];
    } else {
      s = r == c ? 1.0 : 0.0;
    }
    sA[r * MEAN_LD + c] = s;
  }
  __syncthreads();
  for (int j = 0; j < m; ++j) {
    if (tid == 0) {
      double piv = sA[j * MEAN_LD + j];
      if (!(piv > 0.0)) {
        sbad = 1;
        piv = 1.0;
      }
      sA[j * MEAN_LD + j] = sqrt(piv);
    }
    __syncthreads();
    if (tid > j && tid < m) sA[tid * MEAN_LD + j] = sA[tid * MEAN_LD + j] / sA[j * MEAN_LD + j];
    __syncthreads();
    for (int idx = tid; idx < m * m; idx += NTHR) {
      const int i = idx / m, k = idx - i * m;
      if (k > j && k <= i) sA[i * MEAN_LD + k] = sA[i * MEAN_LD + k] - sA[i * MEAN_LD + j] * sA[k * MEAN_LD + j];
    }
    __syncthreads();
  }
  // Zo rows and the per-thread partials of t
  double tp[MP];
#pragma unroll
  for (int r = 0; r < MP; ++r) tp[r] = 0.0;
  for (int i = tid; i < N; i += NTHR) {
    double row[MP];
    const d2* src = reinterpret_cast<const d2*>(Zp + (size_t)i * MP);
#pragma unroll
    for (int r = 0; r < MP; r += 2) {
      const d2 v = src[r >> 1];
      row[r] = v.x;
      row[r + 1] = v.y;
    }
    const double zi = zp[i];
    // (La is re-read per point and row: hoisted out of the loops its 528 entries went to scratch)
    asm volatile("" ::: "memory");
#pragma unroll
    for (int r = 0; r < MP; ++r) {
      double v = row[r];
#pragma unroll
      for (int k = 0; k < r; ++k) v = v - sA[r * MEAN_LD + k] * row[k];
      v = v / sA[r * MEAN_LD + r];
      row[r] = v;
      tp[r] = fma(v, zi, tp[r]);
      __builtin_amdgcn_sched_barrier(0);
    }
    d2* dst = reinterpret_cast<d2*>(Zp + (size_t)i * MP);
#pragma unroll
    for (int r = 0; r < MP; r += 2) dst[r >> 1] = d2{row[r], row[r + 1]};
  }
#pragma unroll
  for (int r = 0; r < MP; ++r) {
    double v = tp[r];
    v = v + __shfl_xor(v, 32);
    v = v + __shfl_xor(v, 16);
    v = v + __shfl_xor(v, 8);
    v = v + __shfl_xor(v, 4);
    v = v + __shfl_xor(v, 2);
    v = v + __shfl_xor(v, 1);
    if ((tid & 63) == 0) sw[(tid >> 6) * MEAN_MAX + r] = v;
  }
  __syncthreads();
  if (tid < MP) st[tid] = ((sw[tid] + sw[MEAN_MAX + tid]) + sw[2 * MEAN_MAX + tid]) + sw[3 * MEAN_MAX + tid];
  __syncthreads();
  double sla = 0.0;
  if (tid == 0) {  // beta = La^-T t (back substitution, r descending), sum log La_rr (r ascending)
    for (int r = m - 1; r >= 0; --r) {
      double v = st[r];
      for (int k = r + 1; k < m; ++k) v = v - sA[k * MEAN_LD + r] * sb[k];
      sb[r] = v / sA[r * MEAN_LD + r];
    }
    for (int r = 0; r < m; ++r) sla = sla + log(sA[r * MEAN_LD + r]);
  }
  __syncthreads();
  if (tid < MEAN_MAX) {
    tvec[(size_t)p * MEAN_MAX + tid] = tid < m ? st[tid] : 0.0;
    beta[(size_t)p * MEAN_MAX + tid] = tid < m ? sb[tid] : 0.0;
  }
  // Lai = La^-1 (what gpf_predict_mean applies to h_q and cov(beta) = Lai^T Lai is made of): column j by
  // thread j, forward substitution, i ascending
  if (tid < m) {
    const int j = tid;
    for (int i = j; i < m; ++i) {
      double v = i == j ? 1.0 : 0.0;
      for (int k = j; k < i; ++k) v = v - sA[i * MEAN_LD + k] * sI[k * MEAN_LD + j];
      sI[i * MEAN_LD + j] = v / sA[i * MEAN_LD + i];
    }
  }
  __syncthreads();
  for (int idx = tid; idx < MEAN_MAX * MEAN_MAX; idx += NTHR) {
    const int r = idx / MEAN_MAX, c = idx - r * MEAN_MAX;
    Lai[(size_t)p * MEAN_MAX * MEAN_MAX + idx] = (c <= r && r < m) ? sI[r * MEAN_LD + c] : 0.0;
  }
  // zr and its sum of squares; sum log Lt_ii
  double qq = 0.0, ld = 0.0;
  for (int i = tid; i < N; i += NTHR) {
    const d2* src = reinterpret_cast<const d2*>(Zp + (size_t)i * MP);
    double f = 0.0;
#pragma unroll
    for (int r = 0; r < MP; r += 2) {
      const d2 v = src[r >> 1];
      f = fma(v.x, st[r], f);
      f = fma(v.y, st[r + 1], f);
    }
    const double res = zp[i] - f;
    zrp[i] = res;
    qq = fma(res, res, qq);
    ld = ld + log(Lp[(size_t)i * (Npad + 1)]);
  }
  for (int i = N + tid; i < Npad; i += NTHR) zrp[i] = 0.0;  // (k_predict_vsq reads whole tiles of it)
  sy[tid] = qq;
  sl[tid] = ld;
  __syncthreads();
  for (int h = NTHR / 2; h > 0; h >>= 1) {
    if (tid < h) {
      sy[tid] = sy[tid] + sy[tid + h];
      sl[tid] = sl[tid] + sl[tid + h];
    }
    __syncthreads();
  }
  if (tid == 0) {
    const double a = as[2 * p], Q = sy[0], nm = (double)(N - m);
    const double qa = Q / (a * a);
    double* o = out + (size_t)p * MV_N;
    o[MV_LML] = (((-0.5 * qa - sl[0]) - sla) - nm * log(a)) - 0.5 * nm * 1.8378770664093453;  // log(2 pi)
    o[MV_Q] = Q;
    o[MV_DA] = 0.0;
    o[MV_DS] = 0.0;
    o[MV_BAD] = sbad ? 1.0 : 0.0;
    o[MV_SLA] = sla;
  }
}

// The O(N m) rest of the gradient, one workgroup per particle, after Bt: per point (thread t takes
// t, t + 256, .. in order) at_i = alt_i - sum_r Bt_ri t_r and sum_r Bt_ri^2 (r ascending), wt_i from the
// s2p partials as k_hyper_value sums them, S' folded in its tree; then dLML/da, dLML/ds and
// scaled[p][i] = at_i / a, the vector grad_epilogue takes.
// grid: (particles)
__global__ __launch_bounds__(NTHR) void k_mean_hyper(int N, int Npad, int nt, int m, int MP, const double* __restrict__ e,
                                                     const double* __restrict__ alpha, const double* __restrict__ s2p,
                                                     const double* __restrict__ Bt, const double* __restrict__ tvec,
                                                     const double* __restrict__ as, double* __restrict__ out,
                                                     double* __restrict__ scaled) {
  __shared__ double ss[NTHR], st[MEAN_MAX];
  const int tid = threadIdx.x, p = blockIdx.x;
  const double* ap = alpha + (size_t)p * Npad;
  const double* a2 = s2p + (size_t)p * nt * Npad;
  const double* bp = Bt + (size_t)p * MP * Npad;
  const double a = as[2 * p], s = as[2 * p + 1];
  const double ia2 = 1.0 / (a * a);
  if (tid < MEAN_MAX) st[tid] = tvec[(size_t)p * MEAN_MAX + tid];
  __syncthreads();
  double sv = 0.0;
  for (int i = tid; i < N; i += NTHR) {
    double f = 0.0, b2 = 0.0;
    for (int r = 0; r < m; ++r) {
      const double b = bp[(size_t)r * Npad + i];
      f = fma(b, st[r], f);
      b2 = fma(b, b, b2);
    }
    const double at = ap[i] - f;
    double w = 0.0;
    for (int t = i / T; t < nt; ++t) w = w + a2[(size_t)t * Npad + i];
    sv = sv + (e[i] * e[i]) * ((at * at) * ia2 - (w - b2));
    scaled[(size_t)p * Npad + i] = at / a;
  }
  ss[tid] = sv;
  __syncthreads();
  for (int h = NTHR / 2; h > 0; h >>= 1) {
    if (tid < h) ss[tid] = ss[tid] + ss[tid + h];
    __syncthreads();
  }
  if (tid == 0) {
    double* o = out + (size_t)p * MV_N;
    const double S = ss[0], nm = (double)(N - m);
    const double qa = o[MV_Q] / (a * a);
    o[MV_DA] = (qa - nm) / a - ((s * s) / (a * a * a)) * S;
    o[MV_DS] = (s / (a * a)) * S;
  }
}

// gram_tile (gpf_lmlgrad.hip) continued: acc = A[:, I]^T A[:, J] over `depth` rows of A, then
// + N[:, I]^T B[:, J] over `depth2` rows of the panels N and B, all four [k][c] panels with the leading
// dimension ld. One DenseRun, so one set of per-lane offsets, serves both parts: as two
// gemm_stream_dl calls the chain kept two sets and copies of the accumulators live and spilled (as
// gemm_stream_dl_wait found). On a diagonal tile the first part forms the lower triangle only, the
// short second part the whole tile; what lies above the diagonal is never read.
template <int M0>
__device__ __forceinline__ void proj_run(Acc<T>& acc, const double* A1, const double* B1, int nch1, const double* A2,
                                         const double* B2, int nch2, int ld, double* smem, const Quad<T>& qd) {
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const DenseRun<true, false, 2, false, true> dr(qd, ld, ld, wave);
  // The second part continues the first one's chunk count, so the pipeline never drains: chunk nch1 of
  // the panels shifted back by nch1 chunks is chunk 0 of (A2, B2) (the shifted bases are never read
  // below it), and the last chunk of the first part, run with them, prefetches it behind its MFMAs.
  // (Restarted after a barrier, the second part's first transfer was exposed on every tile: 1.0 ms of
  // the 64-particle batch at N = 4096.)
  const int ntot = nch1 + nch2;
  const double* A2s = A2 - (size_t)nch1 * DL_KC * ld;
  const double* B2s = B2 - (size_t)nch1 * DL_KC * ld;
  dr.template issue<0>(A1, B1, ld, 0, smem);
  __builtin_amdgcn_s_waitcnt(0x0F70);  // (as gemm_stream_dl)
  dr.template run<M0>(acc, A1, B1, ld, 0, nch1 - 1, nch1, smem);
  dr.template run<M0>(acc, A2s, B2s, ld, nch1 - 1, nch1, ntot, smem);
  dr.template run<0>(acc, A2s, B2s, ld, nch1, ntot, ntot, smem);
  __syncthreads();
}
__device__ __forceinline__ void proj_tile(Acc<T>& acc, const double* A, const double* Nn, const double* B, int ld, int I, int J,
                                          int depth, int depth2, double* smem, const Quad<T>& qd) {
  acc.zero();
  const double* A1 = uniform_ptr(A + (size_t)I * T);
  const double* B1 = uniform_ptr(A + (size_t)J * T);
  const double* A2 = uniform_ptr(Nn + (size_t)I * T);
  const double* B2 = uniform_ptr(B + (size_t)J * T);
  const int n1 = depth / DL_KC, n2 = depth2 / DL_KC;
#define GPF_PROJ(m0) proj_run<m0>(acc, A1, B1, n1, A2, B2, n2, ld, smem, qd)
  if (I != J) {
    GPF_PROJ(0);
  } else {
    switch (qd.cb / 16) {  // TRI_C_LOWER: the row blocks mi >= slab (wave-uniform)
      case 0: GPF_PROJ(0); break;
      case 1: GPF_PROJ(1); break;
      case 2: GPF_PROJ(2); break;
      case 3: GPF_PROJ(3); break;
      case 4: GPF_PROJ(4); break;
      case 5: GPF_PROJ(5); break;
      case 6: GPF_PROJ(6); break;
      default: GPF_PROJ(7); break;
    }
  }
#undef GPF_PROJ
}

// k_lml_grad with the projected precision: w_tile's chain acc = U_.I^T U_.J, continued over the depth
// mpad on the panels (-Bt)_.I and Bt_.J ([k][c] panels like U's, their padding rows exact zeros), so
// acc holds the tile of Pt = U^T U - Bt^T Bt; then grad_epilogue on the vector at / a with k_lml_grad's
// weight.
// Bt, nBt = -Bt: [particles][mpad][Npad]. grid: (nt (nt + 1) / 2, particles), the deepest tiles first
template <int KIND = COV_SE>
__global__ __launch_bounds__(Geo<T>::NTH, 4) void k_mean_grad(int N, int Npad, int nt, int d, int mpad,
                                                              const double* __restrict__ x, const double* __restrict__ ls,
                                                              const double* __restrict__ U, const double* __restrict__ Bt,
                                                              const double* __restrict__ nBt,
                                                              const double* __restrict__ vec, double* __restrict__ partial) {
  __shared__ __attribute__((aligned(16))) double smem[GradLds<1>::LDS];
  const int p = blockIdx.y;
  int I, J;
  const Quad<T> qd;
  Acc<T> acc;
  tri_decode(blockIdx.x, I, J);
  const double* Up = U + (size_t)p * Npad * Npad + (size_t)I * T * Npad;
  const double* bn = nBt + (size_t)p * mpad * Npad;
  const double* bp = Bt + (size_t)p * mpad * Npad;
  proj_tile(acc, Up, bn, bp, Npad, I, J, (nt - I) * T, mpad, smem, qd);
  const double* vp = vec + (size_t)p * Npad;
  grad_epilogue<1, KIND>(
      acc, qd, smem, I, J, p, N, d, x, ls + (size_t)p * d, [&](int, int g) { return vp[g]; },
      [](const double* ri, const double* cj, double w) { return ri[0] * cj[0] - w; }, partial);
}

// gpf_predict_mean's outputs for the query points of one chunk, one thread per point: K_s^T at and
// 1 - sum v^2 from the row-tile partials (row_tile_sums; k_predict_vsq ran with zr in z's place)
// with k_predict_out's clip, then with w = Lai h_q (row r: k ascending)
//   mu_q = K_s[:, q]^T at + h_q^T beta,   var_q = max(1 - sum v^2, 1e-12) + sum_r (w_r - (Bt K_s[:, q])_r)^2,
// r ascending: the second term is |La^-1 R_q|^2 with R_q = h_q - G^T K_s[:, q], G^T = La Bt.
// hq: [m][ldks] the basis at the chunk's points. kb: [chunk][ldb] = K_s^T Bt^T. Lai: k_mean_small's La^-1.
// grid: (ceil(M / 256))
__global__ __launch_bounds__(NTHR) void k_mean_out(int nt, int M, int m, const double* __restrict__ vz, int ldks,
                                                   const double* __restrict__ vsq, const double* __restrict__ hq,
                                                   const double* __restrict__ kb, int ldb, const double* __restrict__ Lai,
                                                   const double* __restrict__ beta, double* __restrict__ mu,
                                                   double* __restrict__ sd) {
  __shared__ double sI[MEAN_MAX * MEAN_LD], sb[MEAN_MAX];
  for (int idx = threadIdx.x; idx < MEAN_MAX * MEAN_MAX; idx += NTHR) sI[(idx / MEAN_MAX) * MEAN_LD + idx % MEAN_MAX] = Lai[idx];
  if (threadIdx.x < MEAN_MAX) sb[threadIdx.x] = beta[threadIdx.x];
  __syncthreads();
  const int q = blockIdx.x * NTHR + threadIdx.x;
  if (q >= M) return;
  double mq, s;
  row_tile_sums(nt, vz, vsq, ldks, q, mq, s);
  double var = 1.0 - s;
  var = (var < 1e-12) ? 1e-12 : var;
  double hb = 0.0, e2 = 0.0;
  for (int r = 0; r < m; ++r) {
    hb = fma(hq[(size_t)r * ldks + q], sb[r], hb);
    double w = 0.0;
    for (int k = 0; k <= r; ++k) w = fma(sI[r * MEAN_LD + k], hq[(size_t)k * ldks + q], w);
    const double rr = w - kb[(size_t)q * ldb + r];
    e2 = fma(rr, rr, e2);
  }
  mu[q] = mq + hb;
  sd[q] = sqrt(var + e2);
}

}  // namespace gpf
