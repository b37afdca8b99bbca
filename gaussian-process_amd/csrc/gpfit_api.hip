// gpfit_api.hip — host side of libgpfit.so: the C-ABI declared in include/gpfit.h.
//
// One context = one HIP device + one stream + device-resident training data.
// gpf_eval_batch replaces the reference's process-pool fan-out over particles
// (find_len_scales.py:73-77,102-104,133-135): non-sentinel particles are packed
// into chunks that fit HBM and every chunk is one batched factorise+score.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cerrno>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "../../include/gpfit.h"
#include "gpf_common.hip"
#include "gpf_covariance.hip"
#include "gpf_factor.hip"
#include "gpf_persist.hip"
#include "gpf_objective.hip"
#include "gpf_predict.hip"
#include "gpf_predbatch.hip"
#include "gpf_postcov.hip"
#include "gpf_linear.hip"
#include "gpf_densechol.hip"
#include "gpf_conditioned.hip"
#include "gpf_lmlgrad.hip"
#include "gpf_loo.hip"
#include "gpf_hyperlml.hip"
#include "gpf_meanfn.hip"
#include "gpf_probsurf.hip"
#include "gpf_hull.hip"
#include "gpf_kmeans.hip"
#include "gpf_plan.hip"  // host only: Knobs, the schedule policies, plan_factor, plan_check

using gpf::BT;
using gpf::NTHR;
using gpf::T;

namespace {

enum ProfClass { PC_PANEL = 0, PC_DIAG = 1, PC_BUILD = 2, PC_LOSS = 3, PC_FACTOR = 4, PC_PRED = 5, PC_PREDK = 6, PC_PSURF = 7, PC_N = 8 };

constexpr int GRAPH_NT_MAX = 2;  // eval batches with N <= 256 run as a replayed HIP graph
// a captured batch must never reach Scratch::grow's hipMalloc/hipFree (every scratch user starts at nt = 4)
static_assert(GRAPH_NT_MAX < 4, "graph-captured batches must not use the factorisation's scratch buffers");

struct Pending {
  hipEvent_t a, b;
  int cls;
  double work;  // algorithmic flops or bytes of this launch
};

// One grow-only device scratch buffer of a context.
struct Scratch {
  void* p = nullptr;
  size_t cap = 0;
  // At least `bytes` (0: not needed). A regrow drops the captured graphs (they hold the old pointer),
  // waits for c->stream first when `sync` is set (the buffer's last user may still run) and, with
  // `zero`, queues the new buffer's zeroing on c->stream (the null stream would not order against it).
  int grow(gpf_ctx* c, size_t bytes, bool zero, bool sync = false);
  void release() {
    hipFree(p);
    p = nullptr;
    cap = 0;
  }
  template <typename V> V* as() const { return static_cast<V*>(p); }
};

// A kept set is given back after its call when it holds more device memory than GPF_PREDICT_KEEP_MB
// (default 2048): a one-off large call must not hold HBM that would starve the next factorisation's
// or hull's allocations
double keep_bytes(const Knobs& k) { return (k.predict_keep_mb.set ? k.predict_keep_mb.f : 2048.0) * 1048576.0; }

// The buffers one entry point keeps between its calls (gpf_ctx::kept): device buffers and pinned host
// staging, each with its capacity. A call plans the bytes of every buffer (its *_plan function), uses
// the set as it is when every buffer fits and otherwise gives the whole set back and allocates it at
// exactly the planned sizes. No captured graph holds a pointer into a set, so a regrow leaves the
// graphs alone (unlike Scratch::grow).
struct KeptSet {
  static constexpr int NMAX = 32;
  void* p[NMAX] = {};
  size_t cap[NMAX] = {};
  bool pinned[NMAX] = {};
  bool fits(const size_t* bytes, int n) const {
    for (int i = 0; i < n; ++i)
      if (bytes[i] > cap[i]) return false;
    return true;
  }
  // Waits for c->stream (the set's last user may still run), releases the set and allocates buffer i
  // at bytes[i] (0: none), as pinned host memory where bit i of pinned_mask is set. After a HIP error
  // the buffers allocated so far stay recorded for the next release().
  int regrow(gpf_ctx* c, const size_t* bytes, unsigned pinned_mask, int n);
  double held() const {  // device bytes (the pinned staging is not counted)
    double b = 0.0;
    for (int i = 0; i < NMAX; ++i)
      if (!pinned[i]) b += (double)cap[i];
    return b;
  }
  void release() {
    for (int i = 0; i < NMAX; ++i) {
      if (p[i]) pinned[i] ? hipHostFree(p[i]) : hipFree(p[i]);
      p[i] = nullptr;
      cap[i] = 0;
      pinned[i] = false;
    }
  }
  void trim(const Knobs& k) { if (held() > keep_bytes(k)) release(); }
  template <typename V = double> V* as(int i) const { return static_cast<V*>(p[i]); }
};

// What an entry point's *_plan function lays out from the call's sizes: the bytes of every buffer of
// its set and, where the call checks a budget, their device total (LinPlan and ConPlan carry more)
struct SetPlan {
  size_t bytes[KeptSet::NMAX];
  double total;
};

// The device bytes of a planned set: what counts against the memory budget and the keep rule
double device_bytes(const size_t* bytes, unsigned pinned_mask, int n) {
  double b = 0.0;
  for (int i = 0; i < n; ++i)
    if (!(pinned_mask >> i & 1)) b += (double)bytes[i];
  return b;
}

// The entry points that keep a set
enum KeptId { KEPT_PRED = 0, KEPT_PCOV, KEPT_PDRAW, KEPT_LIN, KEPT_CON, KEPT_PBATCH, KEPT_DCHOL, KEPT_PSURF, KEPT_PMEAN, KEPT_N };

}  // namespace

struct gpf_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  hipStream_t sub[MAX_GROUPS] = {};  // one stream per particle group (run_factor)
  hipEvent_t fork = nullptr, join[MAX_GROUPS] = {};
  std::string err;

  // training data
  int64_t N = 0, Npad = 0;
  int d = 0, nt = 0;
  int kind = gpf::COV_SE;  // the covariance function (gpf_set_kernel): a model choice, kept across gpf_set_data
  double* d_x = nullptr;
  double* d_y = nullptr;
  double* d_e = nullptr;
  std::vector<double> h_y;

  // objective grid / box
  int K = 0;
  double* d_sig = nullptr;
  double* d_exp = nullptr;
  double* d_lo = nullptr;
  double* d_hi = nullptr;
  std::vector<double> h_lo, h_hi;

  // per-chunk workspace
  int cap = 0;  // particles per chunk the workspace holds
  double* d_L = nullptr;
  double* d_U = nullptr;
  double* d_yb = nullptr;
  double* d_s2p = nullptr;
  // run_factor's scratch, sized by plan_factor (FactorPlan::*_bytes):
  Scratch part;    // split-K partial products (few tiles per launch)
  Scratch cnt;     // split-K arrival counters, one set per (particle, tile), kept zero
  Scratch la;      // look-ahead partials of the next critical tiles (gpf::la_item), two slots per particle
  Scratch pb;      // paired block columns: the lead launch's partials, nt-1 tiles per particle (gpf::pair_slot)
  Scratch pstart;  // ... and the partners' start words (gpf::pair_start_sync), PAIR_HMAX per tile
  Scratch lb;      // all-tile look-ahead pieces (gpf::lall_slot): two parities x particles x smax slots
  int fact_seq = 0;            // factorisations run (tags the start words)
  double* d_szp = nullptr;
  double* d_ls = nullptr;
  double* d_mu = nullptr;
  double* d_sd = nullptr;
  double* d_loss = nullptr;
  double* d_nfac = nullptr;  // per particle: the noise factor r of K = SE + r diag(e^2) (gpf_lml_hyper_batch)
  int* d_info = nullptr;
  int* d_flag = nullptr;  // per particle: last diagonal block published in the running launch (early_diag)
  int* d_cflag = nullptr;  // per particle: last diagonal block reduced by a SYRK workgroup (defer_syrk); reset by k_build_cov
  int* d_pst = nullptr;    // the persistent factorisation's counters (gpf::PState: 3 x cap x nt, heads, abort); reset by k_build_cov
  int ncu = 0;             // compute units of the device (the persistent launch's grid: two workgroups per CU)
  // the buffers the posterior entry points and gpf_prob_surface keep between calls, one set each
  // (PRED_*, PCOV_*, PDRAW_*, LIN_*, CON_*, PBATCH_*, DCHOL_*, PSURF_* below name a set's buffers):
  // a call touches its own set only; a regrow of the workspace (free_work) releases them all
  KeptSet kept[KEPT_N];
  int* d_hist = nullptr;
  // gpf_lml_batch: per-tile gradient partials [particles][tiles][d] and the gradient rows behind them,
  // grow-only and outside the chunk workspace (bytes_per_particle): the evaluation path's chunk
  // capacity does not depend on it
  Scratch gpart;
  // gpf_loo_batch: the chunk's per-particle vectors [particles][LV_N][Npad] and, with the gradient, the
  // dense B = diag(sqrt g) W [particles][Npad][Npad] behind them. Outside the chunk workspace like
  // gpart, but given back with it (free_work), so a regrown workspace is sized on all the free memory
  Scratch loo;
  // gpf_lml_hyper_batch: per particle (a, s), the four results of k_hyper_value, alt and alt / a
  // (Npad doubles each). Its own, like loo: no other call reads or writes it
  Scratch hyp;
  // the mean function's basis (gpf_set_basis): H zero-padded to [bmpad][Npad], bm rows (0: none);
  // every gpf_set_data discards it
  double* d_H = nullptr;
  int bm = 0, bmpad = 0;
  // gpf_lml_mean_batch: per particle (a, s), the results of k_mean_small / k_mean_hyper, t, beta, La^-1,
  // alt, at / a, zr, Z / Zo, Bt and -Bt (MeanBufs). Its own, like hyp
  Scratch mean;
  // pinned host staging for the per-batch transfers (async DMA, capturable in graphs)
  double* h_ls = nullptr;
  double* h_loss = nullptr;
  int* h_info = nullptr;
  // KMeans subsample (gpf_kmeans_set / gpf_kmeans_step): the centred points and the per-step buffers
  double *km_x = nullptr, *km_c = nullptr, *km_dist = nullptr, *km_sums = nullptr, *km_cnt = nullptr;
  int* km_lab = nullptr;
  int64_t km_n = 0;
  int km_d = 0, km_kcap = 0, km_cd = 0;  // km_cd: the d the centre buffers were sized for
  // last convex-hull grid (gpf_hull_fill -> gpf_hull_fetch)
  std::vector<double> hull_rows;
  int hull_d = 0;
  // small-problem path: one captured graph per batch size (launch-latency bound regime)
  std::vector<std::pair<int, hipGraphExec_t>> graphs;

  // profiling
  bool prof = false;
  unsigned long long* d_clk = nullptr;  // shader-clock probe of the factor kernels (gpf::ClockSpan), profiling only
  double bench_sclk = 0.0;              // shader clock (MHz) of the last gpf_mfma_peak / gpf_gemm_bench
  double acc[PC_N][3] = {};  // ms, launches, work
  double evals = 0;
  std::vector<Pending> pend;
  std::vector<hipEvent_t> pool;
};

#define GPF_HIP(ctx, expr)                                                                   \
  do {                                                                                       \
    hipError_t _e = (expr);                                                                  \
    if (_e != hipSuccess) {                                                                  \
      (ctx)->err = std::string(#expr) + ": " + hipGetErrorString(_e);                        \
      return GPF_HIP_ERROR;                                                                  \
    }                                                                                        \
  } while (0)

static int bad_arg(gpf_ctx* c, const char* m) {
  c->err = m;
  return GPF_BAD_ARG;
}

static hipEvent_t take_event(gpf_ctx* c) {
  if (!c->pool.empty()) {
    hipEvent_t e = c->pool.back();
    c->pool.pop_back();
    return e;
  }
  hipEvent_t e = nullptr;
  if (hipEventCreate(&e) != hipSuccess) return nullptr;
  return e;
}

// Launch helper: brackets the launch with events when profiling is on.
template <typename F>
static int launch_on(gpf_ctx* c, hipStream_t st, int cls, double work, F f) {
  hipEvent_t a = nullptr, b = nullptr;
  if (c->prof) {
    a = take_event(c);
    b = take_event(c);
    if (a && b) hipEventRecord(a, st);
  }
  f();
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    c->err = std::string("kernel launch: ") + hipGetErrorString(e);
    return GPF_HIP_ERROR;
  }
  if (c->prof && a && b) {
    hipEventRecord(b, st);
    c->pend.push_back({a, b, cls, work});
  }
  return GPF_OK;
}

template <typename F>
static int launch(gpf_ctx* c, int cls, double work, F f) {
  return launch_on(c, c->stream, cls, work, f);
}

static void harvest(gpf_ctx* c) {
  for (auto& p : c->pend) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) {
      c->acc[p.cls][0] += ms;
      c->acc[p.cls][1] += 1;
      c->acc[p.cls][2] += p.work;
    }
    c->pool.push_back(p.a);
    c->pool.push_back(p.b);
  }
  c->pend.clear();
}

static void clear_graphs(gpf_ctx* c) {
  for (auto& g : c->graphs) hipGraphExecDestroy(g.second);
  c->graphs.clear();
}

int Scratch::grow(gpf_ctx* c, size_t bytes, bool zero, bool sync) {
  if (bytes <= cap) return GPF_OK;
  if (sync) GPF_HIP(c, hipStreamSynchronize(c->stream));
  clear_graphs(c);
  release();
  GPF_HIP(c, hipMalloc(&p, bytes));
  cap = bytes;
  if (zero) GPF_HIP(c, hipMemsetAsync(p, 0, bytes, c->stream));
  return GPF_OK;
}

int KeptSet::regrow(gpf_ctx* c, const size_t* bytes, unsigned pinned_mask, int n) {
  GPF_HIP(c, hipStreamSynchronize(c->stream));
  release();
  for (int i = 0; i < n; ++i) {
    if (!bytes[i]) continue;
    GPF_HIP(c, (pinned_mask >> i & 1) ? hipHostMalloc(&p[i], bytes[i], hipHostMallocDefault) : hipMalloc(&p[i], bytes[i]));
    cap[i] = bytes[i];
    pinned[i] = pinned_mask >> i & 1;
  }
  return GPF_OK;
}

static void free_work(gpf_ctx* c) {
  clear_graphs(c);
  for (KeptSet& k : c->kept) k.release();
  hipHostFree(c->h_ls); hipHostFree(c->h_loss); hipHostFree(c->h_info);
  c->h_ls = c->h_loss = nullptr;
  c->h_info = nullptr;
  hipFree(c->d_L); hipFree(c->d_U); hipFree(c->d_yb); hipFree(c->d_s2p); hipFree(c->d_szp);
  hipFree(c->d_ls); hipFree(c->d_mu); hipFree(c->d_sd); hipFree(c->d_loss); hipFree(c->d_info);
  hipFree(c->d_hist);
  hipFree(c->d_nfac);
  c->d_nfac = nullptr;
  hipFree(c->d_flag);
  c->d_flag = nullptr;
  hipFree(c->d_cflag);
  c->d_cflag = nullptr;
  hipFree(c->d_pst);
  c->d_pst = nullptr;
  for (Scratch* s : {&c->part, &c->cnt, &c->la, &c->pb, &c->pstart, &c->lb, &c->loo, &c->hyp, &c->mean}) s->release();
  c->d_L = c->d_U = c->d_yb = c->d_s2p = c->d_szp = c->d_ls = c->d_mu = c->d_sd = c->d_loss = nullptr;
  c->d_info = nullptr;
  c->d_hist = nullptr;
  c->cap = 0;
}

static size_t bytes_per_particle(const gpf_ctx* c) {
  const size_t np = (size_t)c->Npad;
  // (+ the paired block columns' partial slots, nt-1 tiles, allocated when a factorisation pairs;
  // the noise factor's 8 bytes per particle are not counted, so no call's chunking changes)
  return 2 * np * np * 8 + (2 * (size_t)c->nt * np + 3 * np) * 8 + (size_t)(c->K + 1) * 4 + 64 * 8 + 8 +
         (size_t)std::max(c->nt - 1, 0) * T * T * 8;
}

// Chunk capacity from free HBM (GPF_MAX_CHUNK caps it, GPF_MEM_FRACTION scales the budget).
static int ensure_work(gpf_ctx* c, int want, const Knobs& k) {
  if (want <= c->cap) return GPF_OK;
  free_work(c);
  size_t fr = 0, tot = 0;
  GPF_HIP(c, hipMemGetInfo(&fr, &tot));
  const double frac = k.mem_fraction.set ? k.mem_fraction.f : 0.85;
  const size_t per = bytes_per_particle(c);
  long long fit = (long long)((double)fr * frac / (double)per);
  if (k.max_chunk.set) fit = std::min<long long>(fit, k.max_chunk.i);
  if (fit < 1) {
    c->err = "not enough device memory for one particle at N=" + std::to_string(c->N);
    return GPF_HIP_ERROR;
  }
  const int cap = (int)std::min<long long>(want, fit);
  const size_t np = (size_t)c->Npad;
  GPF_HIP(c, hipMalloc(&c->d_L, (size_t)cap * np * np * 8));
  GPF_HIP(c, hipMalloc(&c->d_U, (size_t)cap * np * np * 8));
  GPF_HIP(c, hipMalloc(&c->d_yb, (size_t)cap * np * 8));
  GPF_HIP(c, hipMalloc(&c->d_s2p, (size_t)cap * c->nt * np * 8));
  GPF_HIP(c, hipMalloc(&c->d_szp, (size_t)cap * c->nt * np * 8));
  GPF_HIP(c, hipMalloc(&c->d_ls, (size_t)cap * std::max(c->d, 1) * 8));
  GPF_HIP(c, hipMalloc(&c->d_mu, (size_t)cap * np * 8));
  GPF_HIP(c, hipMalloc(&c->d_sd, (size_t)cap * np * 8));
  GPF_HIP(c, hipMalloc(&c->d_loss, (size_t)cap * 8));
  GPF_HIP(c, hipMalloc(&c->d_nfac, (size_t)cap * 8));
  GPF_HIP(c, hipMalloc(&c->d_info, (size_t)cap * 4));
  GPF_HIP(c, hipMalloc(&c->d_flag, (size_t)cap * 4));  // reset by k_build_cov at every factorisation
  GPF_HIP(c, hipMalloc(&c->d_cflag, (size_t)cap * 4));  // likewise
  GPF_HIP(c, hipMalloc(&c->d_pst, ((size_t)3 * cap * c->nt + 16) * 4));  // likewise (persistent factorisation)
  GPF_HIP(c, hipMalloc(&c->d_hist, (size_t)cap * (c->K + 1) * 4));
  // on the library stream: the legacy null stream does not order against our non-blocking streams
  GPF_HIP(c, hipMemsetAsync(c->d_hist, 0, (size_t)cap * (c->K + 1) * 4, c->stream));  // k_score re-zeroes what it read
  GPF_HIP(c, hipHostMalloc((void**)&c->h_ls, (size_t)cap * std::max(c->d, 1) * 8, hipHostMallocDefault));
  GPF_HIP(c, hipHostMalloc((void**)&c->h_loss, (size_t)cap * 8, hipHostMallocDefault));
  GPF_HIP(c, hipHostMalloc((void**)&c->h_info, (size_t)cap * 4, hipHostMallocDefault));
  c->cap = cap;
  return GPF_OK;
}

// Factorise `pc` particles whose length scales are already in d_ls, as plan_factor (gpf_plan.hip)
// lays it out: in particle groups on their own streams, per group the K build (the 128-wide diagonal
// blocks), then one k_step per 128-wide block column. With the fused diagonal factor (plan.ed false)
// k_diag factors block 0 first and each launch J factors block J+1 at the end of its critical tile;
// with the early diagonal factor launch J itself starts with the factor of block J. Joins back
// into c->stream. nfac (device, nullable): the particles' noise factors, K = SE + r diag(e^2) (k_build_cov).
static int run_factor(gpf_ctx* c, int pc, const Knobs& knobs, const double* nfac = nullptr) {
  const int nt = c->nt, Np = (int)c->Npad, N = (int)c->N;
  const double Tf = (double)T, t3 = Tf * Tf * Tf;
  const int nb = Np / BT;
  const int ntri = nb * (nb + 1) / 2;
  const size_t ld = (size_t)Np;
  const FactorPlan plan = plan_factor(pc, nt, knobs);
  const int ng = plan.ng, spins = plan.spins;
  const bool persist = plan.persist, ed = plan.ed;
  // algorithmic flops of block-column launch J per particle, potrf + trtri (2/3 N^3) formulation:
  //   L tile: depth-128J GEMM 2 T^3 J + triangular multiply T^3 + look-ahead syrk share T^3
  //   U tile: depth-128(J-K) GEMM with a triangular factor 2 T^3 (J-K) - T^3 + triangular multiply T^3
  //   diagonal block: 2/3 T^3 (block J+1 fused at the end of launch J, or block J early in it)
  auto step_flops = [&](int J) {
    double fl = 0.0;
    for (int w = 0; w < nt - 1; ++w) {
      if (w < nt - 1 - J) fl += 2.0 * t3 * J + 2.0 * t3;
      else fl += 2.0 * t3 * (J - (w - (nt - 1 - J)));
    }
    if (ed || J + 1 < nt) fl += (2.0 / 3.0) * t3;
    return fl;
  };
  // paired block columns: the lead launch J also runs block column J+1's GEMMs over the columns < J
  // (L tiles I >= J+2: depth 128J; U tiles K < J: depth 128(J-K), first block triangular), which the
  // follow launch then does not
  auto pla_flops = [&](int J) {
    double fl = 0.0;
    for (int w = 1; w < nt - 1; ++w) {
      if (w < nt - 1 - J) fl += 2.0 * t3 * J;
      else fl += 2.0 * t3 * (J - (w - (nt - 1 - J))) - t3;
    }
    return fl;
  };
  // Scratch first (nt >= 4 only: never under a graph capture): a (re)allocation queues its zeroing
  // memset on c->stream, which must precede the fork event the group streams wait on (with ng > 1
  // the k_step launches run on the sub-streams, and an unordered memset could land after a piece
  // took its ticket, leaving a tile unfinished). The partners' start words start at zero (tags start at 1).
  if (int rc = c->part.grow(c, plan.part_bytes, false)) return rc;
  if (int rc = c->cnt.grow(c, plan.cnt_bytes, true)) return rc;
  if (int rc = c->la.grow(c, plan.la_bytes, false)) return rc;
  if (int rc = c->pb.grow(c, plan.pb_bytes, false)) return rc;
  if (int rc = c->pstart.grow(c, plan.pstart_bytes, true)) return rc;
  if (int rc = c->lb.grow(c, plan.lb_bytes, false)) return rc;
  // the split-K tickets and ready flags start at zero in every split factorisation: the
  // finishing pieces re-zero what they used, but a hand-off that timed out (info bit 2) leaves its
  // pair's ticket and flag set, and the next tree would elect the wrong finisher;
  // ~20 KB at N=4096 for one particle, on c->stream ahead of the fork
  if (plan.cnt_bytes) GPF_HIP(c, hipMemsetAsync(c->cnt.p, 0, plan.cnt_bytes, c->stream));
  hipEvent_t wa = nullptr, wb = nullptr;
  if (c->prof) {
    wa = take_event(c);
    wb = take_event(c);
    if (wa && wb) hipEventRecord(wa, c->stream);
  }
  if (ng > 1) {
    GPF_HIP(c, hipEventRecord(c->fork, c->stream));
    for (int g = 0; g < ng; ++g) GPF_HIP(c, hipStreamWaitEvent(c->sub[g], c->fork, 0));
  }
  double total = 0.0;
  for (int g = 0; g < ng; ++g) {
    const int p0 = (int)((long long)pc * g / ng), gc = (int)((long long)pc * (g + 1) / ng) - p0;
    hipStream_t st = (ng > 1) ? c->sub[g] : c->stream;
    double* Lg = c->d_L + (size_t)p0 * ld * ld;
    double* Ug = c->d_U + (size_t)p0 * ld * ld;
    double* yg = c->d_yb + (size_t)p0 * ld;
    double* s2g = c->d_s2p + (size_t)p0 * nt * ld;
    double* szg = c->d_szp + (size_t)p0 * nt * ld;
    int* ig = c->d_info + p0;
    const double* lsg = c->d_ls + (size_t)p0 * c->d;
    // only the diagonal blocks are built here; k_step computes the other tiles
    const int nbuild = nt > 1 ? 3 * nt : ntri;
    int rc = launch_on(c, st, PC_BUILD, 8.0 * nbuild * BT * BT * (double)gc, [&] {
      gpf::with_cov_kind(c->kind, [&](auto KIND) {
        hipLaunchKernelGGL(gpf::k_build_cov<KIND()>, dim3(nbuild, gc), dim3(NTHR), 0, st, N, Np, c->d, c->d_x, c->d_y, c->d_e,
                           lsg, Lg, yg, ig, (int)(nbuild != ntri), c->d_flag + p0, c->d_cflag + p0,
                           persist ? c->d_pst : nullptr, (long long)c->cap * nt, nt, nfac ? nfac + p0 : nullptr);
      });
    });
    if (rc) return rc;
    if (ed) continue;  // block 0 is factored by launch 0's diagonal workgroups
    // potrf + trtri of the first 128 block: 2/3 T^3 (later blocks are fused into k_step)
    rc = launch_on(c, st, PC_DIAG, (2.0 / 3.0) * t3 * gc, [&] {
      hipLaunchKernelGGL(gpf::k_diag, dim3(gc), dim3(gpf::DNTH), 0, st, 0, nt, N, Np, Lg, Ug, yg, s2g, szg, ig,
                         c->d_flag + p0);
    });
    if (rc) return rc;
    total += (2.0 / 3.0) * t3 * gc;
  }
  if (persist) {
    // one persistent launch: every block column of every particle (gpf_persist.hip)
    double fl = 0.0;
    for (int J = 0; J < nt; ++J) fl += step_flops(J);
    gpf::PItem a{nt, Np, N, c->d, spins, c->d_L, c->d_U, c->d_yb, c->d_s2p, c->d_szp, c->d_info, c->d_x, c->d_ls};
    const size_t ps = (size_t)c->cap * nt;
    gpf::PState ps_{c->d_pst, c->d_pst + ps, c->d_pst + 2 * ps, reinterpret_cast<unsigned*>(c->d_pst + 3 * ps),
                    c->d_pst + 3 * ps + gpf::PQ_MAX};
    const int rc = launch_on(c, c->stream, PC_PANEL, fl * pc, [&] {
      gpf::with_cov_kind(c->kind, [&](auto KIND) {
        hipLaunchKernelGGL(gpf::k_factor<KIND()>, dim3((unsigned)gpf::p_total_items(pc, nt)), dim3(gpf::STEP_NTH), 0, c->stream,
                           a, ps_, pc, c->prof ? c->d_clk : nullptr);
      });
    });
    if (rc) return rc;
    total += fl * pc;
    if (c->prof && wa && wb) {
      hipEventRecord(wb, c->stream);
      c->pend.push_back({wa, wb, PC_FACTOR, total});
    }
    return GPF_OK;
  }
  // block-column launches (split-K for launches with few tiles)
  const int seq = ++c->fact_seq & 0x7fffff;
  double *d_part = c->part.as<double>(), *d_la = c->la.as<double>(), *d_pb = c->pb.as<double>(), *d_lb = c->lb.as<double>();
  for (const StepLaunch& l : plan.steps) {
    // (paired columns: lead 1, follow 2; look-ahead pieces: bit 0 produces for J+1, bit 1 consumes J-1's —
    // either way the GEMMs over the columns < J of block column J+1's tiles move one launch earlier)
    const int ahead = l.pair | l.lall;
    const double fl = step_flops(l.J) + ((ahead & 1) ? pla_flops(l.J) : 0.0) - ((ahead & 2) ? pla_flops(l.J - 1) : 0.0);
    const int p0 = l.p0, gc = l.gc;
    hipStream_t st = (ng > 1) ? c->sub[l.g] : c->stream;
    // (every split launch gets its buffers: under SPLIT_ALL, l.S is chunks per piece, not a piece count)
    double* partg = l.split != gpf::SPLIT_NONE ? d_part + l.part_off : nullptr;
    unsigned* cntg = l.split != gpf::SPLIT_NONE ? c->cnt.as<unsigned>() + l.cnt_off : nullptr;
    if (l.split == gpf::SPLIT_ALL && !ed) return bad_arg(c, "internal: all-tile split without the early diagonal factor");
    auto kern = gpf::k_step<gpf::SPLIT_NONE, 0>;
    gpf::with_cov_kind(c->kind, [&](auto KIND) {
      kern = l.split == gpf::SPLIT_ALL ? gpf::k_step<gpf::SPLIT_ALL, 1, KIND()>
                                       : (ed ? gpf::k_step<gpf::SPLIT_NONE, 1, KIND()> : gpf::k_step<gpf::SPLIT_NONE, 0, KIND()>);
    });
    const int rc = launch_on(c, st, PC_PANEL, fl * gc, [&] {
      hipLaunchKernelGGL(kern, dim3(l.grid), dim3(gpf::STEP_NTH), l.lds, st, l.J, nt, Np, c->d_L + (size_t)p0 * ld * ld,
                         c->d_U + (size_t)p0 * ld * ld, c->d_yb + (size_t)p0 * ld, c->d_s2p + (size_t)p0 * nt * ld,
                         c->d_szp + (size_t)p0 * nt * ld, c->d_info + p0, gc, l.grp, N, c->d_x,
                         c->d_ls + (size_t)p0 * c->d, c->d, l.S, l.S2, partg, cntg, c->d_flag + p0, l.ed,
                         c->d_cflag + p0, l.defer, l.sy, spins,
                         step_la_arg(l, plan), l.la ? d_la + 2 * (size_t)p0 * T * T : nullptr, step_pair_arg(l),
                         l.lall ? d_lb + (size_t)2 * p0 * plan.lall_smax * T * T
                                : (l.pair ? d_pb + gpf::pair_slot(p0, 0, nt) : nullptr),
                         (l.pair == 1 && plan.psync) ? c->pstart.as<int>() + (size_t)p0 * (nt - 1) * gpf::PAIR_HMAX : nullptr,
                         step_tag(l, seq), c->prof ? c->d_clk : nullptr);
    });
    if (rc) return rc;
    total += fl * gc;
  }
  if (ng > 1) {
    for (int g = 0; g < ng; ++g) {
      GPF_HIP(c, hipEventRecord(c->join[g], c->sub[g]));
      GPF_HIP(c, hipStreamWaitEvent(c->stream, c->join[g], 0));
    }
  }
  if (c->prof && wa && wb) {
    hipEventRecord(wb, c->stream);
    c->pend.push_back({wa, wb, PC_FACTOR, total});
  }
  return GPF_OK;
}

// ---- convex-hull grid fill helpers (convex_hull.py:122-155,203-224) ----
namespace {
struct DevBuf {  // owning device allocation, stream-ordered (no device-wide sync on free)
  void* p = nullptr;
  hipStream_t st = nullptr;
  hipError_t alloc(size_t bytes, hipStream_t s) {
    st = s;
    return hipMallocAsync(&p, bytes, s);
  }
  ~DevBuf() { if (p) hipFreeAsync(p, st); }
  template <typename V> V* as() { return static_cast<V*>(p); }
};
inline unsigned blocks_for(int64_t n) { return (unsigned)std::max<int64_t>(1, (n + NTHR - 1) / NTHR); }
}  // namespace

// Sort rows (n x d, device) lexicographically by columns order[0], order[1], ... (stable LSD
// sequence of radix sorts) and drop repeated rows; rows/n are replaced by the result.
static int hull_sort_unique(gpf_ctx* c, DevBuf& rows, int64_t& n, int d, const int* order) {
  hipStream_t st = c->stream;
  DevBuf perm, perm2, key, key2, flag, pos, temp, out;
  GPF_HIP(c, perm.alloc(std::max<int64_t>(n, 1) * 8, st));
  GPF_HIP(c, perm2.alloc(std::max<int64_t>(n, 1) * 8, st));
  GPF_HIP(c, key.alloc(std::max<int64_t>(n, 1) * 8, st));
  GPF_HIP(c, key2.alloc(std::max<int64_t>(n, 1) * 8, st));
  hipLaunchKernelGGL(gpf::k_hull_iota, dim3(blocks_for(n)), dim3(NTHR), 0, st, perm.as<int64_t>(), n);
  size_t tb = 0, tb2 = 0;
  GPF_HIP(c, hipcub::DeviceRadixSort::SortPairs(nullptr, tb, key.as<uint64_t>(), key2.as<uint64_t>(),
                                                perm.as<int64_t>(), perm2.as<int64_t>(), n, 0, 64, st));
  GPF_HIP(c, hipcub::DeviceScan::ExclusiveSum(nullptr, tb2, perm.as<int64_t>(), perm2.as<int64_t>(), n, st));
  GPF_HIP(c, temp.alloc(std::max<size_t>(std::max(tb, tb2), 16), st));
  for (int q = d - 1; q >= 0; --q) {
    hipLaunchKernelGGL(gpf::k_hull_key, dim3(blocks_for(n)), dim3(NTHR), 0, st, rows.as<double>(),
                       perm.as<int64_t>(), n, d, order[q], key.as<uint64_t>());
    GPF_HIP(c, hipcub::DeviceRadixSort::SortPairs(temp.p, tb, key.as<uint64_t>(), key2.as<uint64_t>(),
                                                  perm.as<int64_t>(), perm2.as<int64_t>(), n, 0, 64, st));
    std::swap(perm.p, perm2.p);
  }
  GPF_HIP(c, flag.alloc(std::max<int64_t>(n, 1) * 8, st));
  GPF_HIP(c, pos.alloc(std::max<int64_t>(n, 1) * 8, st));
  hipLaunchKernelGGL(gpf::k_hull_flag, dim3(blocks_for(n)), dim3(NTHR), 0, st, rows.as<double>(), perm.as<int64_t>(),
                     n, d, flag.as<int64_t>());
  GPF_HIP(c, hipcub::DeviceScan::ExclusiveSum(temp.p, tb2, flag.as<int64_t>(), pos.as<int64_t>(), n, st));
  int64_t last[2] = {0, 0};
  GPF_HIP(c, hipMemcpyAsync(&last[0], pos.as<int64_t>() + (n - 1), 8, hipMemcpyDeviceToHost, st));
  GPF_HIP(c, hipMemcpyAsync(&last[1], flag.as<int64_t>() + (n - 1), 8, hipMemcpyDeviceToHost, st));
  GPF_HIP(c, hipStreamSynchronize(st));
  const int64_t m = last[0] + last[1];
  GPF_HIP(c, out.alloc(std::max<int64_t>(m, 1) * d * 8, st));
  hipLaunchKernelGGL(gpf::k_hull_compact, dim3(blocks_for(n)), dim3(NTHR), 0, st, rows.as<double>(),
                     perm.as<int64_t>(), flag.as<int64_t>(), pos.as<int64_t>(), n, d, out.as<double>());
  GPF_HIP(c, hipGetLastError());
  GPF_HIP(c, hipStreamSynchronize(st));
  std::swap(rows.p, out.p);
  n = m;
  return GPF_OK;
}

// Status of particle slot q of the last chunk, from its factor's info word in the pinned c->h_info
// (valid once c->stream has been synchronised behind the copy).
static int particle_status(gpf_ctx* c, int q) {
  if (c->h_info[q] & 2) {
    c->err = "k_step: diagonal-block hand-off timed out";
    return GPF_HIP_ERROR;
  }
  if (c->h_info[q] != 0) {
    c->err = "Matrix is not positive definite";
    return GPF_NOT_PD;
  }
  return GPF_OK;
}

// ---- around the kept sets: what every posterior entry point checks before it allocates ----
// n length scales, finite and > 0 (fn: the entry point, for the message)
static int check_ls(gpf_ctx* c, const char* fn, const double* ls, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (!(ls[i] > 0.0) || !std::isfinite(ls[i])) {
      c->err = std::string(fn) + ": length scales must be finite and > 0";
      return GPF_BAD_ARG;
    }
  return GPF_OK;
}

// The memory budget of a call's own buffers, half of the free device memory (fr, for the message):
// queried with `set` given back first (null: as things stand), so what the set held counts as free
struct Budget {
  double half = 0.0;
  size_t fr = 0;
};
static int half_free(gpf_ctx* c, KeptSet* set, Budget* b) {
  if (set) {
    GPF_HIP(c, hipStreamSynchronize(c->stream));
    set->release();
  }
  size_t tot = 0;
  GPF_HIP(c, hipMemGetInfo(&b->fr, &tot));
  b->half = 0.5 * (double)b->fr;
  return GPF_OK;
}

// The largest multiple of the tile up to hi for which ok(multiple) holds (ok holds up to some size
// and not beyond), 0 if none: the "largest M that fits" of the budget messages
template <typename F>
static int64_t largest_tiled(int64_t hi, F ok) {
  int64_t fit = 0;
  for (int64_t lo = 0, h = hi / T; lo < h;) {
    const int64_t mid = (lo + h + 1) / 2;
    if (ok(mid * T)) fit = mid * T, lo = mid; else h = mid - 1;
  }
  return fit;
}

// "... need X MiB<at>, more than half of the free Y MiB of device memory; <largest> <fit>": the end of
// every budget message of the two acquisition helpers below
static int over_budget(gpf_ctx* c, const std::string& what, double total, const char* at, const Budget& bg,
                       const char* largest, int64_t fit) {
  c->err = what + " need " + std::to_string((long long)(total / 1048576.0)) + " MiB" + at + ", more than half of the free " +
           std::to_string((long long)(bg.fr / 1048576)) + " MiB of device memory; " + largest + std::to_string(fit);
  return GPF_BAD_ARG;
}

// The kept set of a call that does not chunk over M (gpf_predict_cov, gpf_posterior_draws): the set
// plan(Cp) lays out must fit half of the free memory whole, the set's own given back first.
// what: the message's "<entry point>: <buffers> for M=.. at N=..".
template <typename F>
static int acquire_whole(gpf_ctx* c, KeptSet& ks, int64_t Cp, int nbuf, unsigned pinned, F plan, const std::string& what) {
  const SetPlan p = plan(Cp);
  if (ks.fits(p.bytes, nbuf)) return GPF_OK;
  Budget bg;
  if (int rb = half_free(c, &ks, &bg)) return rb;
  if (p.total > bg.half)
    return over_budget(c, what, p.total, "", bg, "the largest M that fits is ",
                       largest_tiled(Cp, [&](int64_t cols) { return plan(cols).total <= bg.half; }));
  return ks.regrow(c, p.bytes, pinned, nbuf);
}

// The kept set of a call that folds the query axis away `chunk` points per pass (gpf_predict_linear,
// gpf_predict_conditioned): the caller's chunk, or gpf_predict's default, in whole tiles (the block's
// leading dimension and the byte offsets of the streamed panels stay well inside 32 bits); where
// the set plan(M, Cc) lays out does not fit half of the free memory (the set's own given back first)
// the chunk is halved down to one tile, and then the call fails. *out: the plan the set now fits.
template <typename F, typename P>
static int acquire_chunked(gpf_ctx* c, KeptSet& ks, int nbuf, const char* fn, int64_t M, int R, int64_t chunk, F plan,
                           P* out) {
  const int64_t Mp = ((M + T - 1) / T) * T;
  int64_t Cc = std::min<int64_t>(chunk > 0 ? chunk : 16384, 65536);
  Cc = std::min(((Cc + T - 1) / T) * T, Mp);
  P p = plan(M, Cc);
  if (!ks.fits(p.bytes, nbuf)) {
    Budget bg;
    if (int rb = half_free(c, &ks, &bg)) return rb;
    while (p.total > bg.half && Cc > T) {  // fewer query points per pass
      Cc = std::max<int64_t>(T, ((Cc / 2 + T - 1) / T) * T);
      p = plan(M, Cc);
    }
    if (p.total > bg.half)
      return over_budget(c, std::string(fn) + ": the weights, the coordinates and the operands for M=" + std::to_string(M) +
                                ", R=" + std::to_string(R) + " at N=" + std::to_string(c->N),
                         p.total, " at 128 query points per pass", bg, "the largest M that fits at this R is ",
                         largest_tiled(Mp, [&](int64_t m) { return plan(m, T).total <= bg.half; }));
    if (int rg = ks.regrow(c, p.bytes, 0, nbuf)) return rg;
  }
  *out = p;
  return GPF_OK;
}

// What every posterior entry point does between its argument checks and its own work: the device, a
// minimal histogram (the objective grid is not needed), the knobs and, with slots > 0, a factorisation
// workspace of that many particles (first: a (re)allocation there frees the kept sets too)
static int posterior_open(gpf_ctx* c, int slots, Knobs* knobs) {
  hipSetDevice(c->device);
  if (c->K <= 0) c->K = 2;
  *knobs = Knobs::from_env();
  return slots > 0 ? ensure_work(c, slots, *knobs) : GPF_OK;
}

// ... and at its end: the stream drained, the profile folded in, and the set kept for the next call
// only while it is modest (a huge batch_size can size it up to half of free HBM; see keep_bytes)
static int posterior_close(gpf_ctx* c, KeptSet& ks, const Knobs& knobs, int rc) {
  hipStreamSynchronize(c->stream);
  if (c->prof) harvest(c);
  ks.trim(knobs);
  return rc;
}

// The flops of V = U K_s over every row tile of U at `cols` padded columns (row tile t has t+1
// column tiles, the last triangular)
static double v_flops(int nt, int64_t cols) {
  return 2.0 * T * T * (double)cols * ((double)nt * (nt + 1) / 2) - (double)T * T * cols * nt;
}

// K_s of the m query points xq (coordinates with the leading dimension ldx) into ks (Np x ceil(m / 128)
// tiles, leading dimension ldks), then the row-tile partials of V = U K_s and V^T z (k_predict_vsq)
static int queue_ks_vsq(gpf_ctx* c, int64_t m, const double* xq, int64_t ldx, double* ks, int64_t ldks, const double* z,
                        double* vsq, double* vz) {
  const int64_t Np = c->Npad;
  const int nqt = (int)((m + T - 1) / T), Cm = nqt * T;
  int rc = launch(c, PC_PREDK, 8.0 * Np * Cm, [&] {
    gpf::launch_cross_cov(c->stream, c->kind, (int)c->N, (int)m, (int)Np, Cm, c->d, c->d_x, (int)c->N, xq, (int)ldx, c->d_ls, ks, ldks);
  });
  if (rc) return rc;
  return launch(c, PC_PRED, v_flops(c->nt, Cm), [&] {
    hipLaunchKernelGGL(gpf::k_predict_vsq, dim3(nqt, c->nt), dim3(gpf::Geo<T>::NTH), 0, c->stream, (int)Np, c->d_U, ks, (int)ldks,
                       vsq, z, vz, 0);
  });
}

extern "C" {

#ifndef GPF_BUILD_INFO
#define GPF_BUILD_INFO "unknown"
#endif
int gpf_version(void) { return GPF_ABI_VERSION; }
const char* gpf_build_info(void) { return GPF_BUILD_INFO; }
int gpf_tile(void) { return T; }

int gpf_open(int device, gpf_ctx** out) {
  if (!out) return GPF_BAD_ARG;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return GPF_HIP_ERROR;
  if (device < 0 || device >= n) return GPF_BAD_ARG;
  if (hipSetDevice(device) != hipSuccess) return GPF_HIP_ERROR;
  gpf_ctx* c = new gpf_ctx();
  c->device = device;
  if (hipDeviceGetAttribute(&c->ncu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || c->ncu <= 0) c->ncu = 256;
  bool ok = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) == hipSuccess &&
            hipEventCreateWithFlags(&c->fork, hipEventDisableTiming) == hipSuccess;
  for (int g = 0; ok && g < MAX_GROUPS; ++g)
    ok = hipStreamCreateWithFlags(&c->sub[g], hipStreamNonBlocking) == hipSuccess &&
         hipEventCreateWithFlags(&c->join[g], hipEventDisableTiming) == hipSuccess;
  if (!ok) {
    gpf_close(c);
    return GPF_HIP_ERROR;
  }
  *out = c;
  return GPF_OK;
}

void gpf_close(gpf_ctx* c) {
  if (!c) return;
  hipSetDevice(c->device);
  hipStreamSynchronize(c->stream);
  harvest(c);
  free_work(c);
  hipFree(c->d_x); hipFree(c->d_y); hipFree(c->d_e);
  hipFree(c->d_H);
  hipFree(c->d_clk);
  c->gpart.release();
  hipFree(c->d_sig); hipFree(c->d_exp); hipFree(c->d_lo); hipFree(c->d_hi);
  hipFree(c->km_x); hipFree(c->km_c); hipFree(c->km_dist); hipFree(c->km_sums); hipFree(c->km_cnt); hipFree(c->km_lab);
  for (auto e : c->pool) hipEventDestroy(e);
  for (int g = 0; g < MAX_GROUPS; ++g) {
    if (c->sub[g]) hipStreamDestroy(c->sub[g]);
    if (c->join[g]) hipEventDestroy(c->join[g]);
  }
  if (c->fork) hipEventDestroy(c->fork);
  if (c->stream) hipStreamDestroy(c->stream);
  delete c;
}

const char* gpf_last_error(gpf_ctx* c) { return c ? c->err.c_str() : "null context"; }

int gpf_set_data(gpf_ctx* c, const double* x, const double* y, const double* e, int64_t N, int d) {
  if (!c) return GPF_BAD_ARG;
  if (N <= 0 || d <= 0 || !x || !y || !e) return bad_arg(c, "gpf_set_data: empty or null input");
  if (d > gpf::DMAX) return bad_arg(c, "gpf_set_data: d exceeds DMAX (32)");
  if (N > (int64_t)1 << 20) return bad_arg(c, "gpf_set_data: N too large");
  hipSetDevice(c->device);
  GPF_HIP(c, hipStreamSynchronize(c->stream));
  free_work(c);
  hipFree(c->d_x); hipFree(c->d_y); hipFree(c->d_e);
  c->d_x = c->d_y = c->d_e = nullptr;
  hipFree(c->d_H);  // the basis belongs to the training points it was evaluated at
  c->d_H = nullptr;
  c->bm = c->bmpad = 0;
  if (d != c->d) {  // the search box is per dimension: a new d discards it (gpf_eval_batch asks for a new gpf_set_grid)
    c->h_lo.clear();
    c->h_hi.clear();
  }
  c->N = N;
  c->d = d;
  c->nt = (int)((N + T - 1) / T);
  c->Npad = (int64_t)c->nt * T;
  GPF_HIP(c, hipMalloc(&c->d_x, (size_t)N * d * 8));
  GPF_HIP(c, hipMalloc(&c->d_y, (size_t)N * 8));
  GPF_HIP(c, hipMalloc(&c->d_e, (size_t)N * 8));
  GPF_HIP(c, hipMemcpy(c->d_x, x, (size_t)N * d * 8, hipMemcpyHostToDevice));
  GPF_HIP(c, hipMemcpy(c->d_y, y, (size_t)N * 8, hipMemcpyHostToDevice));
  GPF_HIP(c, hipMemcpy(c->d_e, e, (size_t)N * 8, hipMemcpyHostToDevice));
  c->h_y.assign(y, y + N);
  return GPF_OK;
}

int gpf_set_kernel(gpf_ctx* c, int kind) {
  if (!c) return GPF_BAD_ARG;
  if (!gpf::cov_kind_known(kind)) return bad_arg(c, "gpf_set_kernel: unknown kind (0 se, 1 matern32, 2 matern52)");
  if (kind == c->kind) return GPF_OK;
  hipSetDevice(c->device);
  GPF_HIP(c, hipStreamSynchronize(c->stream));
  clear_graphs(c);  // a replay would launch the other kind's kernels
  c->kind = kind;
  return GPF_OK;
}

int gpf_get_kernel(gpf_ctx* c, int* kind) {
  if (!c || !kind) return GPF_BAD_ARG;
  *kind = c->kind;
  return GPF_OK;
}

int gpf_set_grid(gpf_ctx* c, const double* sig, const double* expct, int K, const double* lo, const double* hi) {
  if (!c) return GPF_BAD_ARG;
  if (c->d <= 0) return bad_arg(c, "gpf_set_grid: call gpf_set_data first");
  if (K < 2 || K > gpf::KGRID_MAX || !sig || !expct || !lo || !hi) return bad_arg(c, "gpf_set_grid: bad grid");
  // k_points bisects |pull_k| <= 1 over k, which is the reference's K comparisons only on a finite,
  // non-decreasing grid (the reference computes something for any order: a deliberate deviation).
  // Checked before the context or the device is touched, so a rejected grid leaves the old one whole.
  for (int k = 0; k < K; ++k) {
    char m[128];
    if (!std::isfinite(sig[k])) {
      std::snprintf(m, sizeof m, "gpf_set_grid: sigma_vals[%d] is not finite", k);
      return bad_arg(c, m);
    }
    if (k > 0 && sig[k] < sig[k - 1]) {
      std::snprintf(m, sizeof m, "gpf_set_grid: sigma_vals must be non-decreasing, sigma_vals[%d] < sigma_vals[%d]", k, k - 1);
      return bad_arg(c, m);
    }
  }
  for (int k = 0; k < K; ++k)
    if (!std::isfinite(expct[k])) {
      char m[128];
      std::snprintf(m, sizeof m, "gpf_set_grid: expected[%d] is not finite", k);
      return bad_arg(c, m);
    }
  hipSetDevice(c->device);
  GPF_HIP(c, hipStreamSynchronize(c->stream));
  if (K != c->K || !c->d_sig) {  // (no d_sig: K is the placeholder of a call that needs no grid)
    free_work(c);  // histogram size depends on K
    hipFree(c->d_sig); hipFree(c->d_exp);
    c->d_sig = c->d_exp = nullptr;
    GPF_HIP(c, hipMalloc(&c->d_sig, (size_t)K * 8));
    GPF_HIP(c, hipMalloc(&c->d_exp, (size_t)K * 8));
  }
  if (!c->d_lo) {
    GPF_HIP(c, hipMalloc(&c->d_lo, gpf::DMAX * 8));
    GPF_HIP(c, hipMalloc(&c->d_hi, gpf::DMAX * 8));
  }
  c->K = K;
  GPF_HIP(c, hipMemcpy(c->d_sig, sig, (size_t)K * 8, hipMemcpyHostToDevice));
  GPF_HIP(c, hipMemcpy(c->d_exp, expct, (size_t)K * 8, hipMemcpyHostToDevice));
  GPF_HIP(c, hipMemcpy(c->d_lo, lo, (size_t)c->d * 8, hipMemcpyHostToDevice));
  GPF_HIP(c, hipMemcpy(c->d_hi, hi, (size_t)c->d * 8, hipMemcpyHostToDevice));
  c->h_lo.assign(lo, lo + c->d);
  c->h_hi.assign(hi, hi + c->d);
  return GPF_OK;
}

int gpf_eval_batch(gpf_ctx* c, const double* ls, int P, double* loss, double* mu, double* sd, int* bad_idx) {
  if (!c) return GPF_BAD_ARG;
  if (bad_idx) *bad_idx = -1;
  if (P < 0 || (P > 0 && (!ls || !loss))) return bad_arg(c, "gpf_eval_batch: bad arguments");
  if (c->N <= 0 || c->K <= 0) return bad_arg(c, "gpf_eval_batch: call gpf_set_data and gpf_set_grid first");
  // the box is read per dimension below (h_lo[k], k < d) and on the device (k_score): it must be the one of
  // this d. It is missing after a gpf_set_data that changed d, and when only gpf_log_marginal_likelihood or
  // gpf_debug_factor gave K a value
  if ((int)c->h_lo.size() != c->d || (int)c->h_hi.size() != c->d || !c->d_sig)
    return bad_arg(c, "gpf_eval_batch: no grid for this dimension: call gpf_set_grid after gpf_set_data");
  hipSetDevice(c->device);
  const Knobs knobs = Knobs::from_env();
  const int d = c->d;
  const int64_t N = c->N, Np = c->Npad;
  // sentinel particles (find_len_scales.py:156-157) never reach the GPU
  std::vector<int> act;
  act.reserve(P);
  for (int p = 0; p < P; ++p) {
    bool out = false;
    for (int k = 0; k < d; ++k) {
      const double v = ls[(size_t)p * d + k];
      if (v <= c->h_lo[k] || v >= c->h_hi[k]) out = true;
    }
    if (out) {
      loss[p] = 1e13;
      if (mu) for (int64_t i = 0; i < N; ++i) mu[(size_t)p * N + i] = NAN;
      if (sd) for (int64_t i = 0; i < N; ++i) sd[(size_t)p * N + i] = NAN;
    } else {
      act.push_back(p);
    }
  }
  if (act.empty()) return GPF_OK;
  // Enqueue one chunk of pc particles whose length scales are staged in c->h_ls.
  auto enqueue = [&](int pc) -> int {
    GPF_HIP(c, hipMemcpyAsync(c->d_ls, c->h_ls, (size_t)pc * d * 8, hipMemcpyHostToDevice, c->stream));
    int r = run_factor(c, pc, knobs);
    if (r) return r;
    r = launch(c, PC_LOSS, 0.0, [&] {
      hipLaunchKernelGGL(gpf::k_points, dim3((unsigned)((N + NTHR - 1) / NTHR), pc), dim3(NTHR), 0, c->stream,
                         (int)N, (int)Np, c->nt, c->K, c->d_y, c->d_e, c->d_sig, c->d_s2p, c->d_szp, c->d_mu,
                         c->d_sd, c->d_hist);
      hipLaunchKernelGGL(gpf::k_score, dim3(pc), dim3(NTHR), 0, c->stream, (int)N, c->K, d, c->d_sig, c->d_exp,
                         c->d_hist, c->d_ls, c->d_lo, c->d_hi, c->d_loss);
    });
    if (r) return r;
    GPF_HIP(c, hipMemcpyAsync(c->h_loss, c->d_loss, (size_t)pc * 8, hipMemcpyDeviceToHost, c->stream));
    GPF_HIP(c, hipMemcpyAsync(c->h_info, c->d_info, (size_t)pc * 4, hipMemcpyDeviceToHost, c->stream));
    return GPF_OK;
  };
  // Small problems are launch-latency bound: the whole batch (copies + ~5 kernels) is
  // captured once per batch size as a HIP graph and replayed. The batch is padded to all P
  // slots (spare slots repeat an active particle) so one graph serves every PSO iteration.
  // (Replaying graphs of the live particles up to N = 1920 measured no gain at N = 1024: the
  // ~10 us between dependent k_step launches is not launch overhead; profiles/r1/split_crit_ab.txt.)
  const bool graph = !c->prof && !mu && !sd && c->nt <= GRAPH_NT_MAX && !knobs.no_graph.set;
  if (graph) {
    int rc = ensure_work(c, P, knobs);
    if (rc) return rc;
    if (c->cap >= P) {
      for (int q = 0; q < P; ++q) {
        const int src = act[q < (int)act.size() ? q : 0];
        for (int k = 0; k < d; ++k) c->h_ls[(size_t)q * d + k] = ls[(size_t)src * d + k];
      }
      hipGraphExec_t ge = nullptr;
      for (auto& g : c->graphs)
        if (g.first == P) ge = g.second;
      if (!ge) {
        GPF_HIP(c, hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
        const int rq = enqueue(P);
        hipGraph_t gr = nullptr;
        const hipError_t ec = hipStreamEndCapture(c->stream, &gr);
        if (rq) {
          if (gr) hipGraphDestroy(gr);
          return rq;
        }
        GPF_HIP(c, ec);
        const hipError_t ei = hipGraphInstantiate(&ge, gr, nullptr, nullptr, 0);
        hipGraphDestroy(gr);
        GPF_HIP(c, ei);
        if (c->graphs.size() >= 8) {  // bounded cache: drop the oldest batch size
          hipGraphExecDestroy(c->graphs.front().second);
          c->graphs.erase(c->graphs.begin());
        }
        c->graphs.push_back({P, ge});
      }
      GPF_HIP(c, hipGraphLaunch(ge, c->stream));
      GPF_HIP(c, hipStreamSynchronize(c->stream));
      c->evals += (double)act.size();
      for (size_t q = 0; q < act.size(); ++q) {
        if (const int st = particle_status(c, (int)q)) {
          if (st == GPF_NOT_PD && bad_idx) *bad_idx = act[q];
          return st;
        }
        loss[act[q]] = c->h_loss[q];
      }
      return GPF_OK;
    }
  }
  int rc = ensure_work(c, (int)act.size(), knobs);
  if (rc) return rc;
  const int cap = c->cap;
  std::vector<double> hmu, hsd;
  if (mu) hmu.resize((size_t)cap * Np);
  if (sd) hsd.resize((size_t)cap * Np);
  for (size_t s = 0; s < act.size(); s += cap) {
    const int pc = (int)std::min<size_t>(cap, act.size() - s);
    for (int q = 0; q < pc; ++q)
      for (int k = 0; k < d; ++k) c->h_ls[(size_t)q * d + k] = ls[(size_t)act[s + q] * d + k];
    rc = enqueue(pc);
    if (rc) return rc;
    if (mu) GPF_HIP(c, hipMemcpyAsync(hmu.data(), c->d_mu, (size_t)pc * Np * 8, hipMemcpyDeviceToHost, c->stream));
    if (sd) GPF_HIP(c, hipMemcpyAsync(hsd.data(), c->d_sd, (size_t)pc * Np * 8, hipMemcpyDeviceToHost, c->stream));
    GPF_HIP(c, hipStreamSynchronize(c->stream));
    if (c->prof) harvest(c);
    c->evals += pc;
    for (int q = 0; q < pc; ++q) {
      const int p = act[s + q];
      if (const int st = particle_status(c, q)) {
        if (st == GPF_NOT_PD && bad_idx) *bad_idx = p;
        return st;
      }
      loss[p] = c->h_loss[q];
      if (mu) std::memcpy(mu + (size_t)p * N, hmu.data() + (size_t)q * Np, (size_t)N * 8);
      if (sd) std::memcpy(sd + (size_t)p * N, hsd.data() + (size_t)q * Np, (size_t)N * 8);
    }
  }
  return GPF_OK;
}

// Factorise one particle (slot 0 of the workspace) without waiting: the factor's status word is
// copied to the pinned c->h_info[0] behind it on c->stream, and the caller checks it (particle_status)
// after its next synchronisation — gpf_predict queues the query kernels right behind the
// factorisation instead of idling the GPU for a host round trip. ls == nullptr: the length scales
// are already in d_ls (queued on c->stream by the caller). alpha_out (nullable): alpha = K^-1 y
// into the mu slot of particle 0 (gpf_predict forms its mean from V^T z and does not need it).
static int factor_single_async(gpf_ctx* c, const double* ls, double** alpha_out, const Knobs& knobs) {
  int rc = ensure_work(c, 1, knobs);
  if (rc) return rc;
  if (ls) {
    std::memcpy(c->h_ls, ls, (size_t)c->d * 8);
    GPF_HIP(c, hipMemcpyAsync(c->d_ls, c->h_ls, (size_t)c->d * 8, hipMemcpyHostToDevice, c->stream));
  }
  GPF_HIP(c, hipMemsetAsync(c->d_info, 0, 4, c->stream));
  rc = run_factor(c, 1, knobs);
  if (rc) return rc;
  if (alpha_out) {
    rc = launch(c, PC_LOSS, 0.0, [&] {
      hipLaunchKernelGGL(gpf::k_alpha, dim3((unsigned)((c->N + NTHR - 1) / NTHR)), dim3(NTHR), 0, c->stream,
                         (int)c->N, (int)c->Npad, c->nt, c->d_szp, c->d_mu);
    });
    if (rc) return rc;
    *alpha_out = c->d_mu;
  }
  GPF_HIP(c, hipMemcpyAsync(c->h_info, c->d_info, 4, hipMemcpyDeviceToHost, c->stream));
  return GPF_OK;
}

static int factor_single(gpf_ctx* c, const double* ls, double** alpha_out, const Knobs& knobs) {
  int rc = factor_single_async(c, ls, alpha_out, knobs);
  if (rc) return rc;
  GPF_HIP(c, hipStreamSynchronize(c->stream));
  rc = particle_status(c, 0);
  if (rc) *alpha_out = nullptr;
  return rc;
}

// gpf_predict's kept buffers
enum PredBuf {
  PRED_XF = 0,  // the chunk's query coordinates, d x Cp
  PRED_KS,      // K_s, Np x Cp
  PRED_VSQ,     // per row tile of V = U K_s: the partials of sd and of mu = V^T z (gpf::k_predict_vsq), nt x Cp each
  PRED_VZ,
  PRED_MU,      // Cp each
  PRED_SD,
  PRED_HX,      // pinned staging: the coordinates, (mu | sd)
  PRED_HOUT,
  PRED_NBUF
};
constexpr unsigned PRED_PINNED = 1u << PRED_HX | 1u << PRED_HOUT;

static SetPlan pred_plan(const gpf_ctx* c, int64_t Cp) {
  SetPlan p{};
  const size_t C = (size_t)Cp;
  p.bytes[PRED_XF] = p.bytes[PRED_HX] = (size_t)c->d * C * 8;
  p.bytes[PRED_KS] = (size_t)c->Npad * C * 8;
  p.bytes[PRED_VSQ] = p.bytes[PRED_VZ] = (size_t)c->nt * C * 8;
  p.bytes[PRED_MU] = p.bytes[PRED_SD] = C * 8;
  p.bytes[PRED_HOUT] = 2 * C * 8;
  return p;
}

// One prediction call that walks the query points in chunks (gpf_predict, gpf_predict_mean): what
// predict_chunks needs from its entry point. The set's first PRED_NBUF buffers are gpf_predict's
// (`plan` starts from pred_plan). The hooks run once the set is acquired, and queue on c->stream.
struct Prediction {
  const char* fn;  // the entry point, for the messages
  KeptId set;
  SetPlan (*plan)(const gpf_ctx*, int64_t Cp);
  int nbuf;
  unsigned pinned;
  int64_t col_bytes;  // device bytes per query column that grow with the chunk (the chunk that fits half of free memory)
  const double *ls, *xfit;
  int64_t M, batch;
  double *mu, *sd;
  // optional: nrows more rows of M values per query point, staged beside the coordinates through the
  // pinned buffer rows_host into the device buffer rows_dev (leading dimension Cp)
  const double* rows = nullptr;
  int nrows = 0, rows_host = 0, rows_dev = 0;
  std::function<int()> before_factor, after_factor;  // optional: the call's own uploads and kernels around the factorisation
  std::function<const double*()> z;                  // optional: k_predict_vsq's z (default: z = U y of slot 0)
  // the chunk's launches behind k_predict_vsq: (mu, sd) of the m points from query point s on into PRED_MU / PRED_SD
  std::function<int(int64_t s, int64_t m, int64_t Cp)> out;
  // optional: a failure of the call's own, from what `out` copied back at s = 0 (it sets c->err); asked
  // after the factorisation's status
  std::function<int()> first_check;
};

// The chunks of a prediction: the chunk sized and the set acquired, the length scales and chunk 0's
// coordinates queued ahead of the factorisation, then per chunk K_s, k_predict_vsq, the call's
// kernels and the copy back. Nothing reaches q.mu / q.sd before the factorisation's status and the
// call's own check have passed on chunk 0.
static int predict_chunks(gpf_ctx* c, const Prediction& q) {
  Knobs knobs;
  if (int ro = posterior_open(c, 1, &knobs)) return ro;
  KeptSet& ks = c->kept[q.set];
  const int64_t M = q.M;
  // Query chunk: as large as memory allows (the reference's batch_size only bounds its
  // own host memory, GP_func.py:28-30; results do not depend on it). Sized before the
  // factorisation is queued, so that a (re)allocation never waits for it; free memory is only
  // queried when the kept buffers are too small.
  int64_t chunk = std::min<int64_t>(std::max<int64_t>(std::max<int64_t>(q.batch, 1), 16384), M);
  int64_t Cp = ((chunk + T - 1) / T) * T;
  // buffers kept from the previous call when they are large enough (a hipMalloc/hipFree of the
  // Np x Cp cross-covariance per call cost ~1 ms of the call's wall time); pinned host staging
  // for the query coordinates and the outputs (pageable copies stage through a bounce buffer)
  SetPlan p = q.plan(c, Cp);
  if (!ks.fits(p.bytes, q.nbuf)) {
    Budget bg;
    if (int rb = half_free(c, nullptr, &bg)) return rb;
    const int64_t maxcols = std::max<int64_t>(T, (int64_t)(bg.half / (double)q.col_bytes));
    chunk = std::min<int64_t>(chunk, maxcols);
    Cp = ((chunk + T - 1) / T) * T;
    p = q.plan(c, Cp);
    if (!ks.fits(p.bytes, q.nbuf))
      if (int rg = ks.regrow(c, p.bytes, q.pinned, q.nbuf)) return rg;
  }
  // (Two overlaps of V = U K_s with the single-particle factorisation were built and measured in
  // round 4 — V's row tiles on a low-priority side stream behind each factor launch, and the same
  // with the CUs partitioned by stream CU masks — and removed: the factorisation's latency-bound
  // chain needs the whole chip, profiles/r4/ab_r4g_summary.txt, ab_pred_cumask.txt.)
  double *d_xf = ks.as(PRED_XF), *d_mu = ks.as(PRED_MU), *d_sd = ks.as(PRED_SD), *hx = ks.as(PRED_HX), *hout = ks.as(PRED_HOUT);
  auto stage_chunk = [&](int64_t s0, int64_t m) -> int {
    for (int k = 0; k < c->d; ++k) std::memcpy(hx + (size_t)k * Cp, q.xfit + (size_t)k * M + s0, (size_t)m * 8);
    for (int r = 0; r < q.nrows; ++r) std::memcpy(ks.as(q.rows_host) + (size_t)r * Cp, q.rows + (size_t)r * M + s0, (size_t)m * 8);
    GPF_HIP(c, hipMemcpyAsync(d_xf, hx, (size_t)c->d * Cp * 8, hipMemcpyHostToDevice, c->stream));
    if (q.nrows)
      GPF_HIP(c, hipMemcpyAsync(ks.as(q.rows_dev), ks.as(q.rows_host), (size_t)q.nrows * Cp * 8, hipMemcpyHostToDevice, c->stream));
    return GPF_OK;
  };
  // the length scales and chunk 0's coordinates first, then the factorisation
  std::memcpy(c->h_ls, q.ls, (size_t)c->d * 8);
  GPF_HIP(c, hipMemcpyAsync(c->d_ls, c->h_ls, (size_t)c->d * 8, hipMemcpyHostToDevice, c->stream));
  int rc = stage_chunk(0, std::min<int64_t>(chunk, M));
  if (!rc && q.before_factor) rc = q.before_factor();
  if (!rc) rc = factor_single_async(c, nullptr, nullptr, knobs);
  if (!rc && q.after_factor) rc = q.after_factor();
  if (rc) return rc;
  const double* d_z = q.z ? q.z() : c->d_yb;
  for (int64_t s = 0; s < M && rc == GPF_OK; s += chunk) {
    const int64_t m = std::min<int64_t>(chunk, M - s);
    if (s > 0) {
      if (hipStreamSynchronize(c->stream) != hipSuccess) {  // the staging buffers are reused
        rc = GPF_HIP_ERROR;
        break;
      }
      if ((rc = stage_chunk(s, m))) break;
    }
    if ((rc = queue_ks_vsq(c, m, d_xf, Cp, ks.as(PRED_KS), Cp, d_z, ks.as(PRED_VSQ), ks.as(PRED_VZ)))) break;
    if ((rc = q.out(s, m, Cp))) break;
    if (hipMemcpyAsync(hout, d_mu, (size_t)m * 8, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        hipMemcpyAsync(hout + Cp, d_sd, (size_t)m * 8, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess) {
      rc = GPF_HIP_ERROR;
      c->err = std::string(q.fn) + ": copy back failed";
      break;
    }
    if (s == 0) {  // the factorisation's status (its copy preceded this synchronisation), then the call's own
      rc = particle_status(c, 0);
      if (!rc && q.first_check) rc = q.first_check();
      if (rc) break;
    }
    std::memcpy(q.mu + s, hout, (size_t)m * 8);
    std::memcpy(q.sd + s, hout + Cp, (size_t)m * 8);
  }
  return posterior_close(c, ks, knobs, rc);
}

int gpf_predict(gpf_ctx* c, const double* ls, const double* xfit, int64_t M, int64_t batch, double* mu,
                double* sd) {
  if (!c) return GPF_BAD_ARG;
  if (c->N <= 0) return bad_arg(c, "gpf_predict: call gpf_set_data first");
  if (M < 0 || (M > 0 && (!xfit || !mu || !sd)) || !ls) return bad_arg(c, "gpf_predict: bad arguments");
  if (M == 0) return GPF_OK;
  KeptSet& ks = c->kept[KEPT_PRED];
  Prediction q{"gpf_predict", KEPT_PRED, pred_plan, PRED_NBUF, PRED_PINNED, (c->Npad + 2 * c->nt) * 8, ls, xfit, M, batch, mu, sd};
  q.out = [&](int64_t, int64_t m, int64_t Cp) {
    return launch(c, PC_LOSS, 0.0, [&] {
      hipLaunchKernelGGL(gpf::k_predict_out, dim3((unsigned)((m + NTHR - 1) / NTHR)), dim3(NTHR), 0, c->stream, c->nt, (int)m,
                         ks.as(PRED_VZ), (int)Cp, ks.as(PRED_VSQ), ks.as(PRED_MU), ks.as(PRED_SD));
    });
  };
  return predict_chunks(c, q);
}


// gpf_predict_cov's kept buffers, and gpf_posterior_draws': a set like it with its own behind
enum PcovBuf {
  PCOV_XF = 0,  // the query coordinates, d x Cp
  PCOV_KS,      // K_s and V = U K_s, Np x Cp each
  PCOV_V,
  PCOV_COV,     // Sigma, Cp x Cp
  PCOV_VSQ,     // k_predict_v's partials, nt x Cp each
  PCOV_VZ,
  PCOV_MU,      // (mu | sd), 2 Cp
  PCOV_HX,      // pinned staging: the coordinates, the mean
  PCOV_HMU,
  PCOV_NBUF
};
enum PdrawBuf {
  PDRAW_L = PCOV_NBUF,  // Sigma's factor L, Cp x Cp
  PDRAW_Z,              // the normals and the draws, Sp x Cp each
  PDRAW_DR,
  PDRAW_U,              // the dense factorisation's U_JJ strip (dense_chol_strip_bytes)
  PDRAW_NBUF
};
constexpr unsigned PCOV_PINNED = 1u << PCOV_HX | 1u << PCOV_HMU;

static SetPlan pcov_plan(const gpf_ctx* c, int64_t Cp) {
  SetPlan p{};
  const size_t C = (size_t)Cp;
  p.bytes[PCOV_XF] = p.bytes[PCOV_HX] = (size_t)c->d * C * 8;
  p.bytes[PCOV_KS] = p.bytes[PCOV_V] = (size_t)c->Npad * C * 8;
  p.bytes[PCOV_COV] = C * C * 8;
  p.bytes[PCOV_VSQ] = p.bytes[PCOV_VZ] = (size_t)c->nt * C * 8;
  p.bytes[PCOV_MU] = 2 * C * 8;
  p.bytes[PCOV_HMU] = C * 8;
  p.total = device_bytes(p.bytes, PCOV_PINNED, PCOV_NBUF);
  return p;
}

// gpf_predict_cov's device pipeline, queued on the context's stream over the buffer set bufs (PCOV_*):
// the single-particle factorisation, K_s and K_ss, V = U K_s with the mean's partials, the mean, Sigma's
// lower tiles and the mirror copy. Leaves mu in PCOV_MU and Sigma in PCOV_COV (leading dimension Cp: symmetric, padded
// diagonal 1, padding 0). gpf_posterior_draws runs the same launches in the same order, so its mean
// is bitwise gpf_predict_cov's.
static int pcov_enqueue(gpf_ctx* c, const Knobs& knobs, const double* ls, const double* xfit, int64_t M, int64_t Cp,
                        void* const* bufs) {
  auto buf = [&](int i) { return (double*)bufs[i]; };
  double *xf = buf(PCOV_XF), *ks = buf(PCOV_KS), *v = buf(PCOV_V), *cov = buf(PCOV_COV), *vsq = buf(PCOV_VSQ);
  double *vz = buf(PCOV_VZ), *mu = buf(PCOV_MU), *hx = buf(PCOV_HX);
  const int64_t Np = c->Npad;
  const int nqt = (int)(Cp / T);
  // the kept buffers may be wider than this call needs: every matrix of the call uses the leading
  // dimension Cp of this call's padded M, so the results do not depend on what an earlier call left
  std::memcpy(c->h_ls, ls, (size_t)c->d * 8);
  GPF_HIP(c, hipMemcpyAsync(c->d_ls, c->h_ls, (size_t)c->d * 8, hipMemcpyHostToDevice, c->stream));
  for (int k = 0; k < c->d; ++k) std::memcpy(hx + (size_t)k * Cp, xfit + (size_t)k * M, (size_t)M * 8);
  GPF_HIP(c, hipMemcpyAsync(xf, hx, (size_t)c->d * Cp * 8, hipMemcpyHostToDevice, c->stream));
  int rc = factor_single_async(c, nullptr, nullptr, knobs);
  if (rc) return rc;
  // K_s (Np x Cp, zero rows / columns past N / M) and K_ss into Sigma's buffer (zero past M)
  rc = launch(c, PC_PREDK, 8.0 * Np * Cp + 8.0 * Cp * Cp, [&] {
    gpf::launch_cross_cov(c->stream, c->kind, (int)c->N, (int)M, (int)Np, (int)Cp, c->d, c->d_x, (int)c->N, xf, (int)Cp, c->d_ls,
                          ks, Cp);
    gpf::launch_cross_cov(c->stream, c->kind, (int)M, (int)M, (int)Cp, (int)Cp, c->d, xf, (int)Cp, xf, (int)Cp, c->d_ls,
                          cov, Cp);
  });
  // V = U K_s, stored, and its per-column partials
  if (!rc)
    rc = launch(c, PC_PRED, v_flops(c->nt, Cp), [&] {
      hipLaunchKernelGGL(gpf::k_predict_v, dim3(nqt, c->nt), dim3(gpf::Geo<T>::NTH), 0, c->stream, (int)Np, c->d_U, ks,
                         (int)Cp, vsq, c->d_yb, vz, v);
    });
  if (!rc)
    rc = launch(c, PC_LOSS, 0.0, [&] {
      hipLaunchKernelGGL(gpf::k_predict_out, dim3((unsigned)((M + NTHR - 1) / NTHR)), dim3(NTHR), 0, c->stream, c->nt, (int)M,
                         vz, (int)Cp, vsq, mu, mu + Cp);
    });
  // Sigma's lower tiles, 2 T^2 Np flops each (the diagonal tiles counted in full, as k_lml_grad's):
  // Np Cp^2 for the lower half plus Np Cp T for the diagonal tiles
  const int ntile = nqt * (nqt + 1) / 2;
  if (!rc)
    rc = launch(c, PC_PRED, 2.0 * T * T * (double)Np * ntile, [&] {
      hipLaunchKernelGGL(gpf::k_post_cov, dim3((unsigned)ntile), dim3(gpf::Geo<T>::NTH), 0, c->stream, (int)Np, nqt, v,
                         (int)Cp, cov, Cp);
    });
  const int nmb = (int)((M + gpf::MIR_B - 1) / gpf::MIR_B);
  if (!rc)
    rc = launch(c, PC_PREDK, 8.0 * (double)M * M, [&] {
      hipLaunchKernelGGL(gpf::k_mirror_lower, dim3((unsigned)(nmb * (nmb + 1) / 2)), dim3(NTHR), 0, c->stream, (int)M, cov,
                         Cp);
    });
  return rc;
}

int gpf_predict_cov(gpf_ctx* c, const double* ls, const double* xfit, int64_t M, double* mu, double* cov) {
  if (!c) return GPF_BAD_ARG;
  if (c->N <= 0) return bad_arg(c, "gpf_predict_cov: call gpf_set_data first");
  if (M < 0) return bad_arg(c, "gpf_predict_cov: M < 0");
  if (!ls) return bad_arg(c, "gpf_predict_cov: null length scales");
  if (M > 0 && (!xfit || !mu || !cov)) return bad_arg(c, "gpf_predict_cov: null buffer");
  if (int rl = check_ls(c, "gpf_predict_cov", ls, (size_t)c->d)) return rl;
  if (M > (int64_t)1 << 24) return bad_arg(c, "gpf_predict_cov: M > 2^24 (Sigma is dense: M x M doubles)");
  if (M == 0) return GPF_OK;
  Knobs knobs;
  if (int ro = posterior_open(c, 1, &knobs)) return ro;
  KeptSet& ks = c->kept[KEPT_PCOV];
  const int64_t Cp = ((M + T - 1) / T) * T;
  if (int ra = acquire_whole(c, ks, Cp, PCOV_NBUF, PCOV_PINNED, [&](int64_t cols) { return pcov_plan(c, cols); },
                             "gpf_predict_cov: K_s, V and Sigma for M=" + std::to_string(M) + " at N=" + std::to_string(c->N)))
    return ra;
  double *d_mu = ks.as(PCOV_MU), *hmu = ks.as(PCOV_HMU);
  int rc = pcov_enqueue(c, knobs, ls, xfit, M, Cp, ks.p);
  if (!rc && hipMemcpyAsync(hmu, d_mu, (size_t)M * 8, hipMemcpyDeviceToHost, c->stream) != hipSuccess) {
    rc = GPF_HIP_ERROR;
    c->err = "gpf_predict_cov: copy back failed";
  }
  if (hipStreamSynchronize(c->stream) != hipSuccess && !rc) {
    rc = GPF_HIP_ERROR;
    c->err = "gpf_predict_cov: synchronisation failed";
  }
  // the factorisation's status before anything reaches the caller's buffers
  if (!rc) rc = particle_status(c, 0);
  if (!rc) {
    std::memcpy(mu, hmu, (size_t)M * 8);
    if (hipMemcpy2DAsync(cov, (size_t)M * 8, ks.as(PCOV_COV), (size_t)Cp * 8, (size_t)M * 8, (size_t)M, hipMemcpyDeviceToHost,
                         c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess) {
      rc = GPF_HIP_ERROR;
      c->err = "gpf_predict_cov: copy back failed";
    }
  }
  return posterior_close(c, ks, knobs, rc);
}

// ---- linear functionals of the posterior (gpf_linear.hip) ----
// gpf_predict_linear's kept buffers
enum LinBuf {
  LIN_WRAW = 0,  // the weights as given, R x M
  LIN_WT,        // Wt = A^T, Mp x Rp, zero padded
  LIN_G,         // G = K_ss Wt, Mp x Rp
  LIN_XF,        // the query coordinates, d x Mp
  LIN_BLK,       // one kernel block: K_s[:, c] (Np x Cc) or K_ss[c1, c2] (Cc x Cc)
  LIN_B,         // B = K_s Wt, Np x Rp
  LIN_V,         // V_A = U B, Np x Rp
  LIN_Q,         // Q = Wt^T G = A K_ss A^T, Rp x Rp
  LIN_COV,       // Q - V_A^T V_A, Rp x Rp
  LIN_VSQ,       // k_predict_v's partials, nt x Rp each
  LIN_VZ,
  LIN_MU,        // (mean | k_predict_out's sd slot), 2 Rp
  LIN_PART,      // the partial tiles of the product in flight
  LIN_NBUF
};

// The shape of one gpf_predict_linear call: the padded sizes, the query points per pass and the bytes
// of every buffer
struct LinPlan {
  int64_t Mp, Cc, Np;
  int Rp, Rt, nt, d;
  size_t bytes[LIN_NBUF];
  double total;
};

static LinPlan lin_plan(const gpf_ctx* c, int64_t M, int R, int64_t Cc) {
  LinPlan p{};
  p.Np = c->Npad;
  p.nt = c->nt;
  p.d = c->d;
  p.Mp = ((M + T - 1) / T) * T;
  p.Rp = ((R + T - 1) / T) * T;
  p.Rt = p.Rp / T;
  p.Cc = std::min(Cc, p.Mp);
  const size_t Mp = (size_t)p.Mp, Rp = (size_t)p.Rp, Np = (size_t)p.Np, C = (size_t)p.Cc;
  const int ct = (int)(p.Cc / T), ntri = p.Rt * (p.Rt + 1) / 2;
  // the partial tiles of the largest launch. A launch over `tiles` output tiles and dt depth tiles has
  // at most min(dt, ceil(LIN_WG / tiles)) pieces (lin_pieces), so fewer than min(tiles dt, tiles +
  // LIN_WG) partial tiles, which grows with both: bound each product at its largest pass (B's and G's
  // at a full chunk, Q over Mp, V_A^T V_A over Np); a ragged last chunk needs no more
  auto bound = [](size_t tiles, size_t dt) { return std::min(tiles * dt, tiles + (size_t)gpf::LIN_WG); };
  size_t ptiles = bound((size_t)p.nt * p.Rt, ct);
  ptiles = std::max(ptiles, bound((size_t)ct * p.Rt, ct));
  ptiles = std::max(ptiles, bound(ntri, (size_t)(p.Mp / T)));
  ptiles = std::max(ptiles, bound(ntri, p.nt));
  p.bytes[LIN_WRAW] = (size_t)R * (size_t)M * 8;
  p.bytes[LIN_WT] = p.bytes[LIN_G] = Mp * Rp * 8;
  p.bytes[LIN_XF] = (size_t)p.d * Mp * 8;
  p.bytes[LIN_BLK] = std::max(Np, C) * C * 8;
  p.bytes[LIN_B] = p.bytes[LIN_V] = Np * Rp * 8;
  p.bytes[LIN_Q] = p.bytes[LIN_COV] = Rp * Rp * 8;
  p.bytes[LIN_VSQ] = p.bytes[LIN_VZ] = (size_t)p.nt * Rp * 8;
  p.bytes[LIN_MU] = 2 * Rp * 8;
  p.bytes[LIN_PART] = ptiles * gpf::LIN_TT * 8;
  p.total = device_bytes(p.bytes, 0, LIN_NBUF);
  return p;
}

// One skinny product behind the stream: the partial tiles of `tiles` output tiles over dt depth
// tiles (launch_parts queues k_lin_nn, k_lin_tn or k_con_tn with the piece size it is given) into
// part (the call's LIN_PART buffer), then their ordered sum into out (+ base, or base - sum with
// sgn = -1).
extern "C++" template <typename F>
static int lin_product(gpf_ctx* c, double* part, int tiles, int nct, bool tri, int dt, double flops, const double* base,
                       double sgn, double* out, int64_t ldo, F launch_parts) {
  int per;
  const int pieces = gpf::lin_pieces(dt, tiles, &per);
  int rc = launch(c, PC_PRED, flops, [&] { launch_parts(dim3((unsigned)tiles, (unsigned)pieces), per, part); });
  if (!rc)
    rc = launch(c, PC_PRED, 0.0, [&] {
      hipLaunchKernelGGL(gpf::k_lin_reduce, dim3((unsigned)tiles, 8), dim3(NTHR), 0, c->stream, nct, tri ? 1 : 0, pieces, part,
                         base, sgn, out, ldo);
    });
  return rc;
}

// gpf_predict_linear's device pipeline for the plan p, queued on the context's stream over the buffer
// set bufs (LIN_*; sized by p): the uploads, Wt, the single-particle factorisation, B = K_s Wt, V_A
// with the mean, G = K_ss Wt, Q and S = Q - V_A^T V_A and the two mirror copies. Leaves A mu in
// LIN_MU, S in LIN_COV, Q in LIN_Q and B, V_A, G, Wt and the coordinates where they are.
// gpf_predict_conditioned runs the same launches in the same order over its own buffers, so its
// functionals are bitwise gpf_predict_linear's.
static int lin_enqueue(gpf_ctx* c, const Knobs& knobs, void* const* bufs, const LinPlan& p, const double* ls,
                       const double* xfit, int64_t M, const double* w, int R) {
  const int64_t Cc = p.Cc, Np = p.Np, Mp = p.Mp;
  const int Rp = p.Rp, Rt = p.Rt, nt = p.nt, d = p.d;
  auto buf = [&](int i) { return (double*)bufs[i]; };
  double *wt = buf(LIN_WT), *G = buf(LIN_G), *xf = buf(LIN_XF), *blk = buf(LIN_BLK), *B = buf(LIN_B), *V = buf(LIN_V);
  double *Q = buf(LIN_Q), *S = buf(LIN_COV), *mu = buf(LIN_MU), *pt = buf(LIN_PART);
  hipStream_t st = c->stream;

  // the length scales, the coordinates (leading dimension Mp) and the weights, then the factorisation
  std::memcpy(c->h_ls, ls, (size_t)d * 8);
  GPF_HIP(c, hipMemcpyAsync(c->d_ls, c->h_ls, (size_t)d * 8, hipMemcpyHostToDevice, st));
  GPF_HIP(c, hipMemcpy2DAsync(xf, (size_t)Mp * 8, xfit, (size_t)M * 8, (size_t)M * 8, (size_t)d, hipMemcpyHostToDevice, st));
  GPF_HIP(c, hipMemcpyAsync(buf(LIN_WRAW), w, (size_t)R * (size_t)M * 8, hipMemcpyHostToDevice, st));
  int rc = launch(c, PC_PREDK, 8.0 * (double)Mp * Rp, [&] {
    hipLaunchKernelGGL(gpf::k_lin_wt, dim3((unsigned)(Mp / 64), (unsigned)(Rp / 64)), dim3(NTHR), 0, st, R, M, buf(LIN_WRAW), wt, Rp);
  });
  if (!rc) rc = factor_single_async(c, nullptr, nullptr, knobs);

  // B = K_s Wt, a chunk of query points per pass
  for (int64_t s = 0; s < M && !rc; s += Cc) {
    const int64_t m = std::min<int64_t>(Cc, M - s);
    const int Cm = (int)(((m + T - 1) / T) * T);
    rc = launch(c, PC_PREDK, 8.0 * (double)Np * Cm, [&] {
      gpf::launch_cross_cov(st, c->kind, (int)c->N, (int)m, (int)Np, Cm, d, c->d_x, (int)c->N, xf + s, (int)Mp, c->d_ls, blk, Cc);
    });
    if (rc) break;
    const double* ws = wt + (size_t)s * Rp;
    rc = lin_product(c, pt, nt * Rt, Rt, false, Cm / T, 2.0 * (double)Np * Cm * Rp, s ? B : nullptr, 1.0, B, Rp,
                     [&](dim3 grid, int per, double* part) {
                       hipLaunchKernelGGL(gpf::k_lin_nn, grid, dim3(gpf::Geo<T>::NTH), 0, st, Rt, Cm / T, per, blk, (int)Cc, ws,
                                          Rp, part);
                     });
  }
  // V_A = U B with the mean's partials (sum over the row tiles of V_A^T z = B^T alpha = A mu)
  if (!rc)
    rc = launch(c, PC_PRED, v_flops(nt, Rp), [&] {
      hipLaunchKernelGGL(gpf::k_predict_v, dim3(Rt, nt), dim3(gpf::Geo<T>::NTH), 0, st, (int)Np, c->d_U, B, Rp, buf(LIN_VSQ),
                         c->d_yb, buf(LIN_VZ), V);
    });
  if (!rc)
    rc = launch(c, PC_LOSS, 0.0, [&] {
      hipLaunchKernelGGL(gpf::k_predict_out, dim3((unsigned)((R + NTHR - 1) / NTHR)), dim3(NTHR), 0, st, nt, R, buf(LIN_VZ), Rp,
                         buf(LIN_VSQ), mu, mu + Rp);
    });
  // G = K_ss Wt: the rows of chunk c1 over every chunk c2, one K_ss block at a time
  for (int64_t s1 = 0; s1 < M && !rc; s1 += Cc) {
    const int64_t m1 = std::min<int64_t>(Cc, M - s1);
    const int C1 = (int)(((m1 + T - 1) / T) * T);
    double* G1 = G + (size_t)s1 * Rp;
    for (int64_t s2 = 0; s2 < M && !rc; s2 += Cc) {
      const int64_t m2 = std::min<int64_t>(Cc, M - s2);
      const int C2 = (int)(((m2 + T - 1) / T) * T);
      rc = launch(c, PC_PREDK, 8.0 * (double)C1 * C2, [&] {
        gpf::launch_cross_cov(st, c->kind, (int)m1, (int)m2, C1, C2, d, xf + s1, (int)Mp, xf + s2, (int)Mp, c->d_ls, blk, Cc);
        if (s1 == s2)
          hipLaunchKernelGGL(gpf::k_lin_unit_diag, dim3((unsigned)((m1 + NTHR - 1) / NTHR)), dim3(NTHR), 0, st, (int)m1, blk, Cc);
      });
      if (rc) break;
      const double* ws = wt + (size_t)s2 * Rp;
      rc = lin_product(c, pt, (C1 / T) * Rt, Rt, false, C2 / T, 2.0 * (double)C1 * C2 * Rp, s2 ? G1 : nullptr, 1.0, G1, Rp,
                       [&](dim3 grid, int per, double* part) {
                         hipLaunchKernelGGL(gpf::k_lin_nn, grid, dim3(gpf::Geo<T>::NTH), 0, st, Rt, C2 / T, per, blk, (int)Cc, ws,
                                            Rp, part);
                       });
    }
  }
  // Q = Wt^T G (the prior covariance of the functionals) and Q - V_A^T V_A, lower tiles, then the mirror
  // copies. (k_post_cov is not used on Q: it pins the diagonal to K_ss's 1.0, which is not Q's.)
  const int ntri = Rt * (Rt + 1) / 2;
  if (!rc)
    rc = lin_product(c, pt, ntri, Rt, true, (int)(Mp / T), 2.0 * T * T * (double)Mp * ntri, nullptr, 1.0, Q, Rp,
                     [&](dim3 grid, int per, double* part) {
                       hipLaunchKernelGGL(gpf::k_lin_tn, grid, dim3(gpf::Geo<T>::NTH), 0, st, (int)(Mp / T), per, wt, G, Rp, part);
                     });
  if (!rc)
    rc = lin_product(c, pt, ntri, Rt, true, nt, 2.0 * T * T * (double)Np * ntri, Q, -1.0, S, Rp,
                     [&](dim3 grid, int per, double* part) {
                       hipLaunchKernelGGL(gpf::k_lin_tn, grid, dim3(gpf::Geo<T>::NTH), 0, st, nt, per, V, V, Rp, part);
                     });
  const int nmb = (R + gpf::MIR_B - 1) / gpf::MIR_B;
  if (!rc)
    rc = launch(c, PC_PREDK, 16.0 * (double)R * R, [&] {
      hipLaunchKernelGGL(gpf::k_mirror_lower, dim3((unsigned)(nmb * (nmb + 1) / 2)), dim3(NTHR), 0, st, R, Q, (int64_t)Rp);
      hipLaunchKernelGGL(gpf::k_mirror_lower, dim3((unsigned)(nmb * (nmb + 1) / 2)), dim3(NTHR), 0, st, R, S, (int64_t)Rp);
    });
  return rc;
}

int gpf_predict_linear(gpf_ctx* c, const double* ls, const double* xfit, int64_t M, const double* w, int R, int64_t chunk,
                       double* mean, double* cov, double* prior) {
  if (!c) return GPF_BAD_ARG;
  if (c->N <= 0) return bad_arg(c, "gpf_predict_linear: call gpf_set_data first");
  if (M < 0 || R < 0 || chunk < 0) return bad_arg(c, "gpf_predict_linear: M, R and chunk must be >= 0");
  if (!ls) return bad_arg(c, "gpf_predict_linear: null length scales");
  if (M > 0 && R > 0 && (!xfit || !w || !mean || !cov)) return bad_arg(c, "gpf_predict_linear: null buffer");
  if (int rl = check_ls(c, "gpf_predict_linear", ls, (size_t)c->d)) return rl;
  if (M > (int64_t)1 << 30) return bad_arg(c, "gpf_predict_linear: M > 2^30");
  if (R > 1 << 14) return bad_arg(c, "gpf_predict_linear: R > 16384");
  if (M == 0 || R == 0) return GPF_OK;
  for (size_t i = 0, n = (size_t)R * (size_t)M; i < n; ++i)
    if (!std::isfinite(w[i])) return bad_arg(c, "gpf_predict_linear: weights must be finite");
  Knobs knobs;
  if (int ro = posterior_open(c, 1, &knobs)) return ro;
  KeptSet& ks = c->kept[KEPT_LIN];
  LinPlan p;
  if (int ra = acquire_chunked(c, ks, LIN_NBUF, "gpf_predict_linear", M, R, chunk,
                               [&](int64_t m, int64_t cc) { return lin_plan(c, m, R, cc); }, &p))
    return ra;
  const int Rp = p.Rp;
  double *Q = ks.as(LIN_Q), *S = ks.as(LIN_COV), *mu = ks.as(LIN_MU);
  hipStream_t st = c->stream;
  int rc = lin_enqueue(c, knobs, ks.p, p, ls, xfit, M, w, R);
  if (hipStreamSynchronize(st) != hipSuccess && !rc) {
    rc = GPF_HIP_ERROR;
    c->err = "gpf_predict_linear: synchronisation failed";
  }
  // the factorisation's status before anything reaches the caller's buffers
  if (!rc) rc = particle_status(c, 0);
  if (!rc) {
    const size_t row = (size_t)R * 8, pitch = (size_t)Rp * 8;
    if (hipMemcpyAsync(mean, mu, row, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipMemcpy2DAsync(cov, row, S, pitch, row, (size_t)R, hipMemcpyDeviceToHost, st) != hipSuccess ||
        (prior && hipMemcpy2DAsync(prior, row, Q, pitch, row, (size_t)R, hipMemcpyDeviceToHost, st) != hipSuccess) ||
        hipStreamSynchronize(st) != hipSuccess) {
      rc = GPF_HIP_ERROR;
      c->err = "gpf_predict_linear: copy back failed";
    }
  }
  return posterior_close(c, ks, knobs, rc);
}

// ---- dense Cholesky on the device and posterior draws (gpf_densechol.hip) ----
// The U_JJ strip of a dense factorisation with leading dimension ld: 128 x ld doubles, factor128's
// throw-away outputs (gpf::DC_JUNK doubles) and the status word (one int in a double's slot)
static size_t dense_chol_strip_bytes(int64_t ld) { return ((size_t)T * (size_t)ld + gpf::DC_JUNK + 1) * 8; }

// The jitter ladder over a device matrix, the one place it lives (gpf_chol_dense and
// gpf_posterior_draws both end here): A (npad x ld, lower triangle read, identity padding; not
// modified) -> L (npad x ld, lower tiles) with L L^T = A + jitters[t] I for the first t that
// factorises: the working copy, then three launches per block column on the context's stream
// (gpf_densechol.hip). strip: dense_chol_strip_bytes(ld), zeroed here. Every attempt runs to its end
// and is judged by one status word read back afterwards.
// Returns GPF_OK with *jitter_used / *tries set, or GPF_NOT_PD with *tries = nj.
static int dense_chol_ladder(gpf_ctx* c, const double* dA, double* dL, double* strip, int64_t n, int64_t ld,
                             const double* jitters, int nj, double* jitter_used, int* tries) {
  const int nt = (int)((n + T - 1) / T);
  double* junk = strip + (size_t)T * ld;
  int* dinfo = reinterpret_cast<int*>(junk + gpf::DC_JUNK);
  GPF_HIP(c, hipMemsetAsync(junk, 0, (gpf::DC_JUNK + 1) * 8, c->stream));
  for (int t = 0; t < nj; ++t) {
    if (t > 0) GPF_HIP(c, hipMemsetAsync(dinfo, 0, 4, c->stream));
    const double jit = jitters[t];
    const int ntile = nt * (nt + 1) / 2;
    int rc = launch(c, PC_PREDK, 16.0 * T * T * ntile, [&] {
      hipLaunchKernelGGL(gpf::k_dc_init, dim3(ntile), dim3(gpf::DNTH), 0, c->stream, nt, (int)n, jit, dA, dL, (int)ld);
    });
    for (int J = 0; J < nt && !rc; ++J) {
      const int m = nt - 1 - J;
      rc = launch(c, PC_PRED, 2.0 / 3.0 * T * T * (double)T, [&] {  // potrf + trtri of the block
        hipLaunchKernelGGL(gpf::k_dc_diag, dim3(1), dim3(gpf::DNTH), 0, c->stream, J, dL, strip, (int)ld, junk, dinfo);
      });
      if (!rc && m > 0)
        rc = launch(c, PC_PRED, (double)T * T * T * m, [&] {
          hipLaunchKernelGGL(gpf::k_dc_finish, dim3(m), dim3(gpf::DNTH), 0, c->stream, J, dL, strip, (int)ld);
        });
      if (!rc && m > 0)  // 2 T^3 per tile below the diagonal, T^3 per diagonal tile
        rc = launch(c, PC_PRED, (double)T * T * T * m * m, [&] {
          hipLaunchKernelGGL(gpf::k_dc_trail, dim3(m * (m + 1) / 2), dim3(gpf::DNTH), 0, c->stream, J, m, dL, (int)ld);
        });
    }
    if (rc) return rc;
    int info = 0;
    GPF_HIP(c, hipMemcpyAsync(&info, dinfo, 4, hipMemcpyDeviceToHost, c->stream));
    GPF_HIP(c, hipStreamSynchronize(c->stream));
    if (info == 0) {
      *jitter_used = jit;
      *tries = t + 1;
      return GPF_OK;
    }
  }
  *tries = nj;
  c->err = "Matrix is not positive definite";
  return GPF_NOT_PD;
}

static const char* ladder_arg_error(const double* jitters, int nj) {
  if (!jitters || nj < 1) return "needs at least one jitter";
  for (int t = 0; t < nj; ++t)
    if (!std::isfinite(jitters[t])) return "jitters must be finite";
  return nullptr;
}

// gpf_chol_dense's kept buffers
enum DcholBuf {
  DCHOL_A = 0,  // the matrix and its factor, np x np each
  DCHOL_L,
  DCHOL_U,      // the U_JJ strip (dense_chol_strip_bytes)
  DCHOL_NBUF
};

static SetPlan dchol_plan(int64_t np) {
  SetPlan p{};
  p.bytes[DCHOL_A] = p.bytes[DCHOL_L] = (size_t)np * np * 8;
  p.bytes[DCHOL_U] = dense_chol_strip_bytes(np);
  p.total = device_bytes(p.bytes, 0, DCHOL_NBUF);
  return p;
}

int gpf_chol_dense(gpf_ctx* c, const double* A, int64_t n, const double* jitters, int nj, double* L, double* jitter_used,
                   int* tries) {
  if (!c) return GPF_BAD_ARG;
  if (n < 0) return bad_arg(c, "gpf_chol_dense: n < 0");
  if (!jitter_used || !tries) return bad_arg(c, "gpf_chol_dense: null buffer");
  if (const char* m = ladder_arg_error(jitters, nj)) {
    c->err = std::string("gpf_chol_dense: ") + m;
    return GPF_BAD_ARG;
  }
  if (n > 0 && (!A || !L)) return bad_arg(c, "gpf_chol_dense: null buffer");
  if (n > (int64_t)1 << 24) return bad_arg(c, "gpf_chol_dense: n > 2^24");
  if (n == 0) return GPF_OK;
  hipSetDevice(c->device);
  const Knobs knobs = Knobs::from_env();
  const int64_t np = ((n + T - 1) / T) * T;  // rows and leading dimension of this call's matrices
  KeptSet& ks = c->kept[KEPT_DCHOL];
  const SetPlan p = dchol_plan(np);
  if (!ks.fits(p.bytes, DCHOL_NBUF)) {
    Budget bg;
    if (int rb = half_free(c, &ks, &bg)) return rb;
    if (p.total > bg.half) {
      const int64_t fit = (int64_t)(std::sqrt(bg.half / 16.0) / T) * T - T;
      c->err = "gpf_chol_dense: the matrix and its factor for n=" + std::to_string(n) + " need " +
               std::to_string((long long)(p.total / 1048576.0)) + " MiB, more than half of the free " +
               std::to_string((long long)(bg.fr / 1048576)) + " MiB of device memory; the largest n that fits is " +
               std::to_string(std::max<int64_t>(fit, 0));
      return GPF_BAD_ARG;
    }
    if (int rg = ks.regrow(c, p.bytes, 0, DCHOL_NBUF)) return rg;
  }
  double *dA = ks.as(DCHOL_A), *dL = ks.as(DCHOL_L);
  // A zero-padded with an identity block; L's tiles above the diagonal are never written by the
  // factorisation: zero for the copy back
  GPF_HIP(c, hipMemsetAsync(dA, 0, (size_t)np * np * 8, c->stream));
  GPF_HIP(c, hipMemsetAsync(dL, 0, (size_t)np * np * 8, c->stream));
  GPF_HIP(c, hipMemcpy2DAsync(dA, (size_t)np * 8, A, (size_t)n * 8, (size_t)n * 8, (size_t)n, hipMemcpyHostToDevice, c->stream));
  int rc = launch(c, PC_PREDK, 8.0 * (double)n * n, [&] {
    hipLaunchKernelGGL(gpf::k_dc_pad_diag, dim3(1), dim3(T), 0, c->stream, (int)n, (int)np, dA, np);
  });
  double jit = 0.0;
  int tr = 0;
  if (!rc) rc = dense_chol_ladder(c, dA, dL, ks.as(DCHOL_U), n, np, jitters, nj, &jit, &tr);
  if (rc == GPF_OK) {
    if (hipMemcpy2DAsync(L, (size_t)n * 8, dL, (size_t)np * 8, (size_t)n * 8, (size_t)n, hipMemcpyDeviceToHost, c->stream) !=
            hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess) {
      rc = GPF_HIP_ERROR;
      c->err = "gpf_chol_dense: copy back failed";
    }
  }
  if (rc == GPF_OK) *jitter_used = jit;
  if (rc == GPF_OK || rc == GPF_NOT_PD) *tries = tr;
  hipStreamSynchronize(c->stream);
  if (c->prof) harvest(c);
  ks.trim(knobs);
  return rc;
}

static SetPlan pdraw_plan(const gpf_ctx* c, int64_t Cp, int64_t Sp) {
  SetPlan p = pcov_plan(c, Cp);
  p.bytes[PDRAW_L] = (size_t)Cp * Cp * 8;
  p.bytes[PDRAW_Z] = p.bytes[PDRAW_DR] = (size_t)Sp * Cp * 8;
  p.bytes[PDRAW_U] = dense_chol_strip_bytes(Cp);
  p.total = device_bytes(p.bytes, PCOV_PINNED, PDRAW_NBUF);
  return p;
}

int gpf_posterior_draws(gpf_ctx* c, const double* ls, const double* xfit, int64_t M, const double* z, int64_t S,
                        const double* jitters, int nj, double* mu, double* draws, double* chol, double* jitter_used,
                        int* tries) {
  if (!c) return GPF_BAD_ARG;
  if (c->N <= 0) return bad_arg(c, "gpf_posterior_draws: call gpf_set_data first");
  if (M < 0 || S < 0) return bad_arg(c, "gpf_posterior_draws: M < 0 or S < 0");
  if (!ls) return bad_arg(c, "gpf_posterior_draws: null length scales");
  if (!jitter_used || !tries) return bad_arg(c, "gpf_posterior_draws: null buffer");
  if (const char* m = ladder_arg_error(jitters, nj)) {
    c->err = std::string("gpf_posterior_draws: ") + m;
    return GPF_BAD_ARG;
  }
  if (M > 0 && (!xfit || !mu)) return bad_arg(c, "gpf_posterior_draws: null buffer");
  if (M > 0 && S > 0 && (!z || !draws)) return bad_arg(c, "gpf_posterior_draws: null buffer");
  if (int rl = check_ls(c, "gpf_posterior_draws", ls, (size_t)c->d)) return rl;
  if (M > (int64_t)1 << 24 || S > (int64_t)1 << 24) return bad_arg(c, "gpf_posterior_draws: M or S > 2^24");
  if (M == 0 || S == 0) return GPF_OK;
  Knobs knobs;
  if (int ro = posterior_open(c, 1, &knobs)) return ro;
  KeptSet& ks = c->kept[KEPT_PDRAW];
  const int nqt = (int)((M + T - 1) / T), nst = (int)((S + T - 1) / T);
  const int64_t Cp = (int64_t)nqt * T, Sp = (int64_t)nst * T;
  if (int ra = acquire_whole(c, ks, Cp, PDRAW_NBUF, PCOV_PINNED, [&](int64_t cols) { return pdraw_plan(c, cols, Sp); },
                             "gpf_posterior_draws: K_s, V, Sigma, its factor and the draws for M=" + std::to_string(M) +
                                 ", S=" + std::to_string(S) + " at N=" + std::to_string(c->N)))
    return ra;
  double *d_mu = ks.as(PCOV_MU), *hmu = ks.as(PCOV_HMU), *d_cov = ks.as(PCOV_COV);
  double *d_L = ks.as(PDRAW_L), *d_z = ks.as(PDRAW_Z), *d_dr = ks.as(PDRAW_DR);
  // (as in gpf_predict_cov, every matrix of the call uses this call's Cp as its leading dimension)
  // the mean's padding is read by k_draws for the padded columns only: finite, not uninitialised
  GPF_HIP(c, hipMemsetAsync(d_mu, 0, (size_t)Cp * 8, c->stream));
  int rc = pcov_enqueue(c, knobs, ls, xfit, M, Cp, ks.p);
  if (!rc && hipMemcpyAsync(hmu, d_mu, (size_t)M * 8, hipMemcpyDeviceToHost, c->stream) != hipSuccess) {
    rc = GPF_HIP_ERROR;
    c->err = "gpf_posterior_draws: copy back failed";
  }
  // the normals, zero-padded to Sp x Cp (behind the pipeline's launches on the stream; pageable source)
  if (!rc && (hipMemsetAsync(d_z, 0, (size_t)Sp * Cp * 8, c->stream) != hipSuccess ||
              hipMemcpy2DAsync(d_z, (size_t)Cp * 8, z, (size_t)M * 8, (size_t)M * 8, (size_t)S, hipMemcpyHostToDevice,
                               c->stream) != hipSuccess)) {
    rc = GPF_HIP_ERROR;
    c->err = "gpf_posterior_draws: upload of the normals failed";
  }
  if (hipStreamSynchronize(c->stream) != hipSuccess && !rc) {
    rc = GPF_HIP_ERROR;
    c->err = "gpf_posterior_draws: synchronisation failed";
  }
  // the training factorisation's status before the dense one starts
  if (!rc) rc = particle_status(c, 0);
  double jit = 0.0;
  int tr = 0;
  if (!rc && chol) rc = hipMemsetAsync(d_L, 0, (size_t)Cp * Cp * 8, c->stream) == hipSuccess ? GPF_OK : GPF_HIP_ERROR;
  const bool laddered = !rc;
  if (!rc) rc = dense_chol_ladder(c, d_cov, d_L, ks.as(PDRAW_U), M, Cp, jitters, nj, &jit, &tr);
  if (!rc)  // 2 T^2 flops per 128-deep step of a tile, depth 128 (I + 1)
    rc = launch(c, PC_PRED, 2.0 * T * T * (double)T * nst * ((double)nqt * (nqt + 1) / 2), [&] {
      hipLaunchKernelGGL(gpf::k_draws, dim3(nst, nqt), dim3(gpf::DNTH), 0, c->stream, nqt, d_z, (int)Cp, d_L, (int)Cp,
                         d_mu, d_dr);
    });
  if (!rc) {
    // nothing of size M x M leaves the device unless the caller asks for the factor
    bool ok = hipMemcpy2DAsync(draws, (size_t)M * 8, d_dr, (size_t)Cp * 8, (size_t)M * 8, (size_t)S, hipMemcpyDeviceToHost,
                               c->stream) == hipSuccess;
    if (ok && chol)
      ok = hipMemcpy2DAsync(chol, (size_t)M * 8, d_L, (size_t)Cp * 8, (size_t)M * 8, (size_t)M, hipMemcpyDeviceToHost,
                            c->stream) == hipSuccess;
    if (!ok || hipStreamSynchronize(c->stream) != hipSuccess) {
      rc = GPF_HIP_ERROR;
      c->err = "gpf_posterior_draws: copy back failed";
    }
  }
  if (!rc) {
    std::memcpy(mu, hmu, (size_t)M * 8);
    *jitter_used = jit;
  }
  if (laddered && (rc == GPF_OK || rc == GPF_NOT_PD)) *tries = tr;
  return posterior_close(c, ks, knobs, rc);
}

// ---- the posterior conditioned on measured linear functionals (gpf_conditioned.hip) ----
// gpf_predict_conditioned's kept buffers: the LIN_* set first, then its own
enum ConBuf {
  CON_W2 = LIN_NBUF,  // W2 = U^T V_A = Kn^-1 K_s A^T, Np x Rp
  CON_H,              // H = A Sigma A^T + diag(s^2), Rp x Rp, identity padding
  CON_LH,             // its factor Lh, lower tiles
  CON_STRIP,          // the dense factorisation's U_JJ strip (dense_chol_strip_bytes)
  CON_XT,             // Lh^-T, upper tiles, zero below
  CON_C,              // C = Sigma A^T of the chunk in flight, Cc x Rp
  CON_E,              // E = C Lh^-T of the chunk in flight, Cc x Rp
  CON_G,              // (d = b - A mu | g = Lh^-1 d | chi2), 2 Rp + 1
  CON_BS,             // (b | s), 2 Rp
  CON_VSQ,            // k_predict_vsq's partials of the chunk in flight, nt x Cc each
  CON_VZ,
  CON_OUT,            // (mu' | sd'), Mp each
  CON_NBUF
};
static_assert(CON_NBUF <= KeptSet::NMAX && PDRAW_NBUF <= KeptSet::NMAX, "KeptSet holds up to NMAX buffers");

struct ConPlan {
  LinPlan lin;  // (its LIN_PART also holds the partial tiles of this call's own products)
  size_t bytes[CON_NBUF];
  double total;
};

static ConPlan con_plan(const gpf_ctx* c, int64_t M, int R, int64_t Cc) {
  ConPlan q{};
  q.lin = lin_plan(c, M, R, Cc);
  const LinPlan& p = q.lin;
  const size_t Mp = (size_t)p.Mp, Rp = (size_t)p.Rp, Np = (size_t)p.Np, C = (size_t)p.Cc;
  const size_t ct = C / T;
  // the partial tiles of W2 (nt Rt tiles, depth nt), C (ct Rt tiles, depth nt) and E (ct Rt tiles, depth Rt)
  auto bound = [](size_t tiles, size_t dt) { return std::min(tiles * dt, tiles + (size_t)gpf::LIN_WG); };
  size_t ptiles = std::max(bound((size_t)p.nt * p.Rt, p.nt), std::max(bound(ct * p.Rt, p.nt), bound(ct * p.Rt, p.Rt)));
  for (int i = 0; i < LIN_NBUF; ++i) q.bytes[i] = p.bytes[i];
  q.bytes[LIN_PART] = std::max(q.bytes[LIN_PART], ptiles * gpf::LIN_TT * 8);
  q.bytes[CON_W2] = Np * Rp * 8;
  q.bytes[CON_H] = q.bytes[CON_LH] = q.bytes[CON_XT] = Rp * Rp * 8;
  q.bytes[CON_STRIP] = dense_chol_strip_bytes((int64_t)Rp);
  q.bytes[CON_C] = q.bytes[CON_E] = C * Rp * 8;
  q.bytes[CON_G] = (2 * Rp + 1) * 8;
  q.bytes[CON_BS] = 2 * Rp * 8;
  q.bytes[CON_VSQ] = q.bytes[CON_VZ] = (size_t)p.nt * C * 8;
  q.bytes[CON_OUT] = 2 * Mp * 8;
  q.total = device_bytes(q.bytes, 0, CON_NBUF);
  return q;
}

int gpf_predict_conditioned(gpf_ctx* c, const double* ls, const double* xfit, int64_t M, const double* w, int R,
                            const double* b, const double* sv, int64_t chunk, double* mu_out, double* sd_out, double* fmean,
                            double* fcov, double* chi2) {
  if (!c) return GPF_BAD_ARG;
  // (gpf_predict_linear's checks, then this call's own)
  if (c->N <= 0) return bad_arg(c, "gpf_predict_conditioned: call gpf_set_data first");
  if (M < 0 || R < 0 || chunk < 0) return bad_arg(c, "gpf_predict_conditioned: M, R and chunk must be >= 0");
  if (!ls) return bad_arg(c, "gpf_predict_conditioned: null length scales");
  if (M > 0 && R > 0 && (!xfit || !w || !b || !sv || !mu_out || !sd_out)) return bad_arg(c, "gpf_predict_conditioned: null buffer");
  if (int rl = check_ls(c, "gpf_predict_conditioned", ls, (size_t)c->d)) return rl;
  if (M > (int64_t)1 << 30) return bad_arg(c, "gpf_predict_conditioned: M > 2^30");
  if (R > 1024) return bad_arg(c, "gpf_predict_conditioned: R > 1024 (larger R is not built yet)");
  if (M == 0 || R == 0) return GPF_OK;
  for (size_t i = 0, n = (size_t)R * (size_t)M; i < n; ++i)
    if (!std::isfinite(w[i])) return bad_arg(c, "gpf_predict_conditioned: weights must be finite");
  for (int r = 0; r < R; ++r) {
    if (!std::isfinite(b[r])) return bad_arg(c, "gpf_predict_conditioned: the measured values must be finite");
    if (!(sv[r] >= 0.0) || !std::isfinite(sv[r]))
      return bad_arg(c, "gpf_predict_conditioned: the standard errors must be finite and >= 0");
  }
  Knobs knobs;
  if (int ro = posterior_open(c, 1, &knobs)) return ro;
  KeptSet& ks = c->kept[KEPT_CON];
  ConPlan q;
  if (int ra = acquire_chunked(c, ks, CON_NBUF, "gpf_predict_conditioned", M, R, chunk,
                               [&](int64_t m, int64_t cc) { return con_plan(c, m, R, cc); }, &q))
    return ra;
  const LinPlan& p = q.lin;
  const int64_t Cc = p.Cc, Np = p.Np, Mp = p.Mp;
  const int Rp = p.Rp, Rt = p.Rt, nt = p.nt, d = p.d;
  auto buf = [&](int i) { return ks.as(i); };
  double *G = buf(LIN_G), *xf = buf(LIN_XF), *blk = buf(LIN_BLK), *V = buf(LIN_V), *S = buf(LIN_COV), *amu = buf(LIN_MU);
  double *pt = buf(LIN_PART), *W2 = buf(CON_W2), *H = buf(CON_H), *Lh = buf(CON_LH), *strip = buf(CON_STRIP), *Xt = buf(CON_XT);
  double *Cq = buf(CON_C), *E = buf(CON_E), *dv = buf(CON_G), *g = dv + Rp, *dchi = dv + 2 * Rp, *bs = buf(CON_BS);
  double *vsq = buf(CON_VSQ), *vz = buf(CON_VZ), *omu = buf(CON_OUT), *osd = omu + Mp;
  hipStream_t st = c->stream;

  // pass 1: gpf_predict_linear's pipeline (B, V_A, G, Q, S = A Sigma A^T and A mu stay on the device)
  int rc = lin_enqueue(c, knobs, ks.p, p, ls, xfit, M, w, R);
  // b and s, then H and d = b - A mu, W2 = U^T V_A (U lower triangular: the depth tiles k < i are zeros)
  if (!rc && (hipMemcpyAsync(bs, b, (size_t)R * 8, hipMemcpyHostToDevice, st) != hipSuccess ||
              hipMemcpyAsync(bs + Rp, sv, (size_t)R * 8, hipMemcpyHostToDevice, st) != hipSuccess ||
              hipMemsetAsync(Xt, 0, (size_t)Rp * Rp * 8, st) != hipSuccess)) {
    rc = GPF_HIP_ERROR;
    c->err = "gpf_predict_conditioned: upload of the measurements failed";
  }
  if (!rc)
    rc = launch(c, PC_PREDK, 16.0 * (double)Rp * Rp, [&] {
      hipLaunchKernelGGL(gpf::k_con_h, dim3((unsigned)Rp), dim3(NTHR), 0, st, R, Rp, S, bs, bs + Rp, amu, H, dv);
    });
  if (!rc)
    rc = lin_product(c, pt, nt * Rt, Rt, false, nt, (double)Np * Np * Rp, nullptr, 1.0, W2, Rp,
                     [&](dim3 grid, int per, double* part) {
                       hipLaunchKernelGGL(gpf::k_con_tn, grid, dim3(gpf::Geo<T>::NTH), 0, st, Rt, nt, per, 1, c->d_U, (int)Np, V,
                                          Rp, part);
                     });
  // the training factorisation's status before the dense one starts (as gpf_posterior_draws), then
  // H = Lh Lh^T without jitter; the ladder waits for its status word, so both are known before the
  // first chunk: nothing reaches the caller's buffers after a failure
  if (hipStreamSynchronize(st) != hipSuccess && !rc) {
    rc = GPF_HIP_ERROR;
    c->err = "gpf_predict_conditioned: synchronisation failed";
  }
  if (!rc && (rc = particle_status(c, 0)) == GPF_NOT_PD)
    c->err = "gpf_predict_conditioned: the covariance of the training points is not positive definite";
  const double jit0 = 0.0;
  double jit = 0.0;
  int tr = 0;
  if (!rc && (rc = dense_chol_ladder(c, H, Lh, strip, R, Rp, &jit0, 1, &jit, &tr)) == GPF_NOT_PD)
    c->err = "gpf_predict_conditioned: H = A Sigma A^T + diag(s^2) is not positive definite (redundant functionals "
             "with zero error?)";
  // Xt = Lh^-T and g = Lh^-1 d
  if (!rc)
    rc = launch(c, PC_PREDK, 16.0 * T * T * Rt, [&] {
      hipLaunchKernelGGL(gpf::k_dc_inv_diag, dim3((unsigned)Rt), dim3(NTHR), 0, st, strip, Xt, Rp);
    });
  for (int I = 1; I < Rt && !rc; ++I) {
    rc = launch(c, PC_PRED, (double)T * T * T * I * (I + 1), [&] {  // 2 T^3 per 128-deep step, I - J of them for tile J
      hipLaunchKernelGGL(gpf::k_dc_inv_sum, dim3((unsigned)I), dim3(gpf::DNTH), 0, st, I, Lh, Xt, Rp);
    });
    if (!rc)
      rc = launch(c, PC_PRED, 2.0 * T * T * T * I, [&] {
        hipLaunchKernelGGL(gpf::k_dc_inv_fin, dim3((unsigned)I), dim3(gpf::DNTH), 0, st, I, strip, Xt, Rp);
      });
  }
  if (!rc)
    rc = launch(c, PC_LOSS, 0.0, [&] {
      hipLaunchKernelGGL(gpf::k_con_g, dim3((unsigned)((Rp + NTHR - 1) / NTHR)), dim3(NTHR), 0, st, Rp, Xt, dv, g);
    });
  // pass 2: a chunk of query points per pass
  const int R4 = (R + 3) / 4 * 4;
  for (int64_t s = 0; s < M && !rc; s += Cc) {
    const int64_t m = std::min<int64_t>(Cc, M - s);
    const int nqt = (int)((m + T - 1) / T);
    const int Cm = nqt * T;
    if ((rc = queue_ks_vsq(c, m, xf + s, Mp, blk, Cc, c->d_yb, vsq, vz))) break;  // (as gpf_predict)
    // C = G - K_s^T W2 over the chunk's rows, then E = C Lh^-T
    const double* G1 = G + (size_t)s * Rp;
    rc = lin_product(c, pt, nqt * Rt, Rt, false, nt, 2.0 * (double)Np * Cm * Rp, G1, -1.0, Cq, Rp,
                     [&](dim3 grid, int per, double* part) {
                       hipLaunchKernelGGL(gpf::k_con_tn, grid, dim3(gpf::Geo<T>::NTH), 0, st, Rt, nt, per, 0, blk, (int)Cc, W2, Rp,
                                          part);
                     });
    if (rc) break;
    rc = lin_product(c, pt, nqt * Rt, Rt, false, Rt, 2.0 * (double)Cm * Rp * Rp, nullptr, 1.0, E, Rp,
                     [&](dim3 grid, int per, double* part) {
                       hipLaunchKernelGGL(gpf::k_lin_nn, grid, dim3(gpf::Geo<T>::NTH), 0, st, Rt, Rt, per, Cq, Rp, Xt, Rp, part);
                     });
    if (rc) break;
    rc = launch(c, PC_LOSS, 0.0, [&] {
      hipLaunchKernelGGL(gpf::k_con_out, dim3((unsigned)((m + NTHR - 1) / NTHR)), dim3(NTHR), 0, st, nt, (int)m, vz, (int)Cc, vsq,
                         E, Rp, R4, g, omu + s, osd + s, s == 0 ? dchi : nullptr);
    });
  }
  if (!rc) {
    const size_t row = (size_t)R * 8, pitch = (size_t)Rp * 8;
    double hchi = 0.0;
    if (hipMemcpyAsync(mu_out, omu, (size_t)M * 8, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipMemcpyAsync(sd_out, osd, (size_t)M * 8, hipMemcpyDeviceToHost, st) != hipSuccess ||
        (fmean && hipMemcpyAsync(fmean, amu, row, hipMemcpyDeviceToHost, st) != hipSuccess) ||
        (fcov && hipMemcpy2DAsync(fcov, row, S, pitch, row, (size_t)R, hipMemcpyDeviceToHost, st) != hipSuccess) ||
        (chi2 && hipMemcpyAsync(&hchi, dchi, 8, hipMemcpyDeviceToHost, st) != hipSuccess) ||
        hipStreamSynchronize(st) != hipSuccess) {
      rc = GPF_HIP_ERROR;
      c->err = "gpf_predict_conditioned: copy back failed";
    }
    if (!rc && chi2) *chi2 = hchi;
  }
  return posterior_close(c, ks, knobs, rc);
}

// ---- KMeans subsample (find_len_scales.py:25-47; gpf_kmeans.hip) ----
int gpf_kmeans_set(gpf_ctx* c, const double* X, int64_t n, int d) {
  if (!c) return GPF_BAD_ARG;
  if (n <= 0 || d <= 0 || d > gpf::DMAX || !X) return bad_arg(c, "gpf_kmeans_set: bad arguments");
  hipSetDevice(c->device);
  GPF_HIP(c, hipStreamSynchronize(c->stream));
  if (n != c->km_n || d != c->km_d) {
    hipFree(c->km_x); hipFree(c->km_dist); hipFree(c->km_lab);
    c->km_x = c->km_dist = nullptr;
    c->km_lab = nullptr;
    c->km_n = 0;
    GPF_HIP(c, hipMalloc(&c->km_x, (size_t)n * d * 8));
    GPF_HIP(c, hipMalloc(&c->km_dist, (size_t)n * 8));
    GPF_HIP(c, hipMalloc(&c->km_lab, (size_t)n * 4));
    c->km_n = n;
    c->km_d = d;
  }
  GPF_HIP(c, hipMemcpyAsync(c->km_x, X, (size_t)n * d * 8, hipMemcpyHostToDevice, c->stream));
  GPF_HIP(c, hipStreamSynchronize(c->stream));
  return GPF_OK;
}

int gpf_kmeans_step(gpf_ctx* c, const double* centers, int k, int update, int* labels, double* sums,
                    double* counts, double* dist) {
  if (!c) return GPF_BAD_ARG;
  if (c->km_n <= 0) return bad_arg(c, "gpf_kmeans_step: call gpf_kmeans_set first");
  const int d = c->km_d;
  if (k <= 0 || !centers || !labels || (update && (!sums || !counts))) return bad_arg(c, "gpf_kmeans_step: bad arguments");
  if ((int64_t)k * (d + 1) > gpf::KM_MAXKD)  // centres + norms in LDS (gpfit.kmeans falls back to the host fit)
    return bad_arg(c, "gpf_kmeans_step: k x (d + 1) exceeds KM_MAXKD (8192)");
  hipSetDevice(c->device);
  if (k > c->km_kcap || d != c->km_cd) {  // the centre buffers are k x d: both sizes matter
    GPF_HIP(c, hipStreamSynchronize(c->stream));
    hipFree(c->km_c); hipFree(c->km_sums); hipFree(c->km_cnt);
    c->km_c = c->km_sums = c->km_cnt = nullptr;
    c->km_kcap = 0;
    GPF_HIP(c, hipMalloc(&c->km_c, (size_t)k * d * 8));
    GPF_HIP(c, hipMalloc(&c->km_sums, (size_t)k * d * 8));
    GPF_HIP(c, hipMalloc(&c->km_cnt, (size_t)k * 8));
    c->km_kcap = k;
    c->km_cd = d;
  }
  const int64_t n = c->km_n;
  GPF_HIP(c, hipMemcpyAsync(c->km_c, centers, (size_t)k * d * 8, hipMemcpyHostToDevice, c->stream));
  gpf::launch_km_assign(c->stream, n, d, k, c->km_x, c->km_c, c->km_lab, c->km_dist);
  GPF_HIP(c, hipGetLastError());
  if (update) {
    hipLaunchKernelGGL(gpf::k_km_sums, dim3((unsigned)k), dim3(NTHR), 0, c->stream, n, d, c->km_x, c->km_lab, c->km_sums,
                       c->km_cnt);
    GPF_HIP(c, hipGetLastError());
    GPF_HIP(c, hipMemcpyAsync(sums, c->km_sums, (size_t)k * d * 8, hipMemcpyDeviceToHost, c->stream));
    GPF_HIP(c, hipMemcpyAsync(counts, c->km_cnt, (size_t)k * 8, hipMemcpyDeviceToHost, c->stream));
  }
  GPF_HIP(c, hipMemcpyAsync(labels, c->km_lab, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
  if (dist) GPF_HIP(c, hipMemcpyAsync(dist, c->km_dist, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
  GPF_HIP(c, hipStreamSynchronize(c->stream));
  return GPF_OK;
}

int gpf_kernel(gpf_ctx* c, const double* x1, int64_t N1, const double* x2, int64_t N2, int d, const double* l,
               double* out) {
  if (!c) return GPF_BAD_ARG;
  if (N1 < 0 || N2 < 0 || d <= 0 || d > gpf::DMAX || !l) return bad_arg(c, "gpf_kernel: bad arguments");
  if (N1 == 0 || N2 == 0) return GPF_OK;
  if (!x1 || !x2 || !out) return bad_arg(c, "gpf_kernel: null buffer");
  hipSetDevice(c->device);
  double *dx1 = nullptr, *dx2 = nullptr, *dl = nullptr, *dout = nullptr;
  GPF_HIP(c, hipMalloc(&dx1, (size_t)N1 * d * 8));
  GPF_HIP(c, hipMalloc(&dx2, (size_t)N2 * d * 8));
  GPF_HIP(c, hipMalloc(&dl, (size_t)d * 8));
  GPF_HIP(c, hipMalloc(&dout, (size_t)N1 * N2 * 8));
  GPF_HIP(c, hipMemcpyAsync(dx1, x1, (size_t)N1 * d * 8, hipMemcpyHostToDevice, c->stream));
  GPF_HIP(c, hipMemcpyAsync(dx2, x2, (size_t)N2 * d * 8, hipMemcpyHostToDevice, c->stream));
  GPF_HIP(c, hipMemcpyAsync(dl, l, (size_t)d * 8, hipMemcpyHostToDevice, c->stream));
  int rc = launch(c, PC_BUILD, 8.0 * N1 * N2, [&] {
    gpf::launch_cross_cov(c->stream, c->kind, (int)N1, (int)N2, (int)N1, (int)N2, d, dx1, (int)N1, dx2, (int)N2, dl, dout, (int64_t)N2);
  });
  if (rc == GPF_OK) {
    if (hipMemcpyAsync(out, dout, (size_t)N1 * N2 * 8, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess) {
      rc = GPF_HIP_ERROR;
      c->err = "gpf_kernel: copy back failed";
    }
  }
  if (c->prof) harvest(c);
  hipFree(dx1); hipFree(dx2); hipFree(dl); hipFree(dout);
  return rc;
}

int gpf_log_marginal_likelihood(gpf_ctx* c, const double* ls, double* out) {
  if (!c || !ls || !out) return GPF_BAD_ARG;
  if (c->N <= 0) return bad_arg(c, "gpf_log_marginal_likelihood: call gpf_set_data first");
  hipSetDevice(c->device);
  if (c->K <= 0) c->K = 2;
  double* alpha = nullptr;
  int rc = factor_single(c, ls, &alpha, Knobs::from_env());
  if (rc) return rc;
  const int64_t N = c->N, Np = c->Npad;
  std::vector<double> a(N), dg(N);
  GPF_HIP(c, hipMemcpy(a.data(), alpha, (size_t)N * 8, hipMemcpyDeviceToHost));
  GPF_HIP(c, hipMemcpy2D(dg.data(), 8, c->d_L, (size_t)(Np + 1) * 8, 8, (size_t)N, hipMemcpyDeviceToHost));
  double ya = 0.0, ld = 0.0;
  for (int64_t i = 0; i < N; ++i) ya += c->h_y[i] * a[i];
  for (int64_t i = 0; i < N; ++i) ld += std::log(dg[i]);
  *out = -0.5 * ya - ld - 0.5 * (double)N * std::log(2.0 * M_PI);
  return GPF_OK;
}

// ---- the batched objectives over the chunk workspace: gpf_lml_batch, gpf_loo_batch, gpf_lml_hyper_batch,
// gpf_lml_mean_batch ----

// The flops of W = U^T U on the lower tiles, the same N^3/3 as the factorisation: the sum over the
// tiles (I, J <= I) of 2 T^3 (nt - I) (k_lml_grad, k_loo_w)
static double tri_gemm_flops(int nt) {
  double fl = 0.0;
  for (int I = 0; I < nt; ++I) fl += 2.0 * (double)T * T * T * (double)(nt - I) * (I + 1);
  return fl;
}

// One batched objective call: what objective_batch needs from its entry point. The hooks run once
// per pass of pc particles starting at particle s, on c->stream; q is a particle's slot in its pass.
struct Objective {
  const double* rows;  // particle p's d length scales at rows + p * stride
  int stride;
  int P, pass;                   // particles, and particles per pass (<= c->cap)
  const double* nfac = nullptr;  // run_factor's per-slot noise factors (filled by `upload`), or none
  double* value;                 // [P]: -inf for a particle whose matrix is not positive definite
  const double* hval;            // where `fetch` leaves slot q's value on the host: hval[q * hstride]
  int hstride;
  double* grad = nullptr;  // null: no gradient. Particle p's d length-scale derivatives at grad + p * gstride
  int gstride = 0;
  double grad_flops = 0.0;  // per particle, of `tiles`
  int* status;
  int* bad_idx;
  std::function<int(int s, int pc)> upload;  // optional: what the pass needs on the device before its factorisation
  std::function<int(int pc)> enqueue;        // the value kernels and, with the gradient, what precedes `tiles`
  // the kernel that reduces every lower tile to partial[pc][nt (nt + 1) / 2][d] (a bare launch:
  // objective_batch brackets it together with k_lml_grad_sum)
  std::function<void(int pc, double* partial)> tiles;
  std::function<int(int s, int pc)> fetch;              // the pass's results to the host (hval and the call's own outputs)
  std::function<void(int p, int q, bool bad)> outputs;  // optional: the call's own per-particle outputs
  // optional: a failure of the call's own in slot q whose factorisation succeeded (from what `fetch`
  // brought back); it sets c->err and the particle is GPF_NOT_PD like one whose matrix failed
  std::function<bool(int q)> failed;
};

// The passes of a batched objective: stage the length scales, factorise, run the call's kernels, finish
// the gradient (the sum over the tiles and 1 / l^3: k_lml_grad_sum), bring the results and the factors'
// info words back, and fold them particle by particle. A particle whose matrix is not positive definite
// gets status GPF_NOT_PD, value -inf and a NaN gradient row; the first one sets the return value and
// *bad_idx, and the batch goes on. The caller has sized the workspace (ensure_work).
static int objective_batch(gpf_ctx* c, const Knobs& knobs, const Objective& o) {
  const int d = c->d, ntile = c->nt * (c->nt + 1) / 2;
  double* d_grad = nullptr;
  std::vector<double> hg;
  if (o.grad) {
    // per-tile partials, then the gradient rows
    // (synchronised regrow: the previous call's gradient pass may still be reading it)
    if (int rc = c->gpart.grow(c, ((size_t)o.pass * ntile * d + (size_t)o.pass * d) * 8, false, true)) return rc;
    d_grad = c->gpart.as<double>() + (size_t)o.pass * ntile * d;
    hg.resize((size_t)o.pass * d);
  }
  int ret = GPF_OK, rc;
  std::string first_err;
  for (int s = 0; s < o.P; s += o.pass) {
    const int pc = std::min(o.pass, o.P - s);
    for (int q = 0; q < pc; ++q) std::memcpy(c->h_ls + (size_t)q * d, o.rows + (size_t)(s + q) * o.stride, (size_t)d * 8);
    GPF_HIP(c, hipMemcpyAsync(c->d_ls, c->h_ls, (size_t)pc * d * 8, hipMemcpyHostToDevice, c->stream));
    if (o.upload && (rc = o.upload(s, pc))) return rc;
    if ((rc = run_factor(c, pc, knobs, o.nfac))) return rc;
    if ((rc = o.enqueue(pc))) return rc;
    if (o.grad) {
      rc = launch(c, PC_LOSS, o.grad_flops * pc, [&] {
        o.tiles(pc, c->gpart.as<double>());
        hipLaunchKernelGGL(gpf::k_lml_grad_sum, dim3(pc), dim3(gpf::DMAX), 0, c->stream, ntile, d, c->gpart.as<double>(), c->d_ls,
                           d_grad);
      });
      if (rc) return rc;
      GPF_HIP(c, hipMemcpyAsync(hg.data(), d_grad, (size_t)pc * d * 8, hipMemcpyDeviceToHost, c->stream));
    }
    if ((rc = o.fetch(s, pc))) return rc;
    GPF_HIP(c, hipMemcpyAsync(c->h_info, c->d_info, (size_t)pc * 4, hipMemcpyDeviceToHost, c->stream));
    GPF_HIP(c, hipStreamSynchronize(c->stream));
    if (c->prof) harvest(c);
    for (int q = 0; q < pc; ++q) {
      const int p = s + q;
      const int st = particle_status(c, q);
      if (st == GPF_HIP_ERROR) return st;
      const bool bad = st != GPF_OK || (o.failed && o.failed(q));
      if (bad && ret == GPF_OK) {
        ret = GPF_NOT_PD;
        first_err = c->err;
        if (o.bad_idx) *o.bad_idx = p;
      }
      if (o.status) o.status[p] = bad ? GPF_NOT_PD : GPF_OK;
      o.value[p] = bad ? -INFINITY : o.hval[(size_t)q * o.hstride];
      if (o.grad)
        for (int k = 0; k < d; ++k) o.grad[(size_t)p * o.gstride + k] = bad ? NAN : hg[(size_t)q * d + k];
      if (o.outputs) o.outputs(p, q, bad);
    }
  }
  if (ret != GPF_OK) c->err = first_err;  // the message of the particle *bad_idx names
  return ret;
}

int gpf_lml_batch(gpf_ctx* c, const double* ls, int P, double* lml, double* grad, int* status, int* bad_idx) {
  if (!c) return GPF_BAD_ARG;
  if (bad_idx) *bad_idx = -1;
  if (P < 0 || (P > 0 && (!ls || !lml))) return bad_arg(c, "gpf_lml_batch: bad arguments");
  if (c->N <= 0) return bad_arg(c, "gpf_lml_batch: call gpf_set_data first");
  const int d = c->d, nt = c->nt;
  if (int rl = check_ls(c, "gpf_lml_batch", ls, (size_t)P * d)) return rl;
  if (P == 0) return GPF_OK;
  hipSetDevice(c->device);
  const int64_t N = c->N, Np = c->Npad;
  const Knobs knobs = Knobs::from_env();
  if (int rc = ensure_work(c, P, knobs)) return rc;
  Objective o;
  o.rows = ls, o.stride = d, o.P = P, o.pass = std::min(c->cap, P);
  o.value = lml, o.hval = c->h_loss, o.hstride = 1;
  o.grad = grad, o.gstride = d, o.grad_flops = tri_gemm_flops(nt);
  o.status = status, o.bad_idx = bad_idx;
  // alpha into the mu slots, the value into the loss slots of the chunk workspace
  o.enqueue = [&](int pc) {
    return launch(c, PC_LOSS, 0.0, [&] {
      hipLaunchKernelGGL(gpf::k_alpha_batch, dim3((unsigned)((N + NTHR - 1) / NTHR), pc), dim3(NTHR), 0, c->stream, (int)N,
                         (int)Np, nt, c->d_szp, c->d_mu);
      hipLaunchKernelGGL(gpf::k_lml_value, dim3(pc), dim3(NTHR), 0, c->stream, (int)N, (int)Np, c->d_y, c->d_mu, c->d_L,
                         c->d_loss);
    });
  };
  o.tiles = [&](int pc, double* partial) {
    gpf::with_cov_kind(c->kind, [&](auto KIND) {
      hipLaunchKernelGGL(gpf::k_lml_grad<KIND()>, dim3((unsigned)(nt * (nt + 1) / 2), pc), dim3(gpf::Geo<T>::NTH), 0, c->stream,
                         (int)N, (int)Np, nt, d, c->d_x, c->d_ls, c->d_U, c->d_mu, partial);
    });
  };
  o.fetch = [&](int, int pc) -> int {
    GPF_HIP(c, hipMemcpyAsync(c->h_loss, c->d_loss, (size_t)pc * 8, hipMemcpyDeviceToHost, c->stream));
    return GPF_OK;
  };
  return objective_batch(c, knobs, o);
}

// ---- gpf_loo_batch: leave-one-out predictions, their log predictive density and its gradient ----
int gpf_loo_batch(gpf_ctx* c, const double* ls, int P, double* lpd, double* grad, double* mu, double* sd, int* status,
                  int* bad_idx) {
  if (!c) return GPF_BAD_ARG;
  if (bad_idx) *bad_idx = -1;
  if (P < 0 || (P > 0 && (!ls || !lpd))) return bad_arg(c, "gpf_loo_batch: bad arguments");
  if (c->N <= 0) return bad_arg(c, "gpf_loo_batch: call gpf_set_data first");
  const int d = c->d, nt = c->nt;
  if (int rl = check_ls(c, "gpf_loo_batch", ls, (size_t)P * d)) return rl;
  if (P == 0) return GPF_OK;
  hipSetDevice(c->device);
  const int64_t N = c->N, Np = c->Npad;
  const Knobs knobs = Knobs::from_env();
  int rc = ensure_work(c, P, knobs);
  if (rc) return rc;
  const int ntile = nt * (nt + 1) / 2;
  // particles per pass: the workspace's capacity, lowered to what the call's own buffer (the vectors
  // and, with the gradient, B) fits in the memory that is free beside the workspace
  const size_t per = ((size_t)gpf::LV_N * Np + (grad ? (size_t)Np * Np : 0)) * 8;
  int pcm = std::min(c->cap, P);
  if ((size_t)pcm * per > c->loo.cap) {
    size_t fr = 0, tot = 0;
    GPF_HIP(c, hipStreamSynchronize(c->stream));
    GPF_HIP(c, hipMemGetInfo(&fr, &tot));
    const double frac = knobs.mem_fraction.set ? knobs.mem_fraction.f : 0.85;
    const long long fit = (long long)(((double)fr + (double)c->loo.cap) * frac / (double)per);
    if (fit < 1) {
      c->err = "gpf_loo_batch: not enough device memory for one particle at N=" + std::to_string(c->N);
      return GPF_HIP_ERROR;
    }
    pcm = (int)std::min<long long>(pcm, fit);
  }
  if ((rc = c->loo.grow(c, (size_t)pcm * per, false, true))) return rc;
  double* d_vec = c->loo.as<double>();
  double* d_B = d_vec + (size_t)pcm * gpf::LV_N * Np;
  const size_t vpitch = (size_t)gpf::LV_N * Np * 8;
  Objective o;
  o.rows = ls, o.stride = d, o.P = P, o.pass = pcm;
  o.value = lpd, o.hval = c->h_loss, o.hstride = 1;
  // G = B^T B reduced against the kernel derivative: every lower tile over the full depth, 2 T^3 nt
  o.grad = grad, o.gstride = d, o.grad_flops = 2.0 * (double)T * T * T * nt * (double)ntile;
  o.status = status, o.bad_idx = bad_idx;
  o.enqueue = [&](int pc) {
    // the per-point quantities into the call's vectors, the density into the loss slots of the workspace
    int rc = launch(c, PC_LOSS, 0.0, [&] {
      hipLaunchKernelGGL(gpf::k_loo_points, dim3(pc), dim3(NTHR), 0, c->stream, (int)N, (int)Np, nt, c->d_y, c->d_s2p, c->d_szp,
                         d_vec, c->d_loss);
    });
    if (rc || !grad) return rc;
    // W = U^T U, then B = diag(sqrt g) W mirrored to the full matrix and u = W c
    rc = launch(c, PC_LOSS, tri_gemm_flops(nt) * pc, [&] {
      hipLaunchKernelGGL(gpf::k_loo_w, dim3((unsigned)ntile, pc), dim3(gpf::Geo<T>::NTH), 0, c->stream, (int)Np, nt, c->d_U, d_B);
    });
    if (rc) return rc;
    const int nmb = (int)(Np / gpf::MIR_B);
    return launch(c, PC_LOSS, 0.0, [&] {
      hipLaunchKernelGGL(gpf::k_loo_scale_mirror, dim3((unsigned)(nmb * (nmb + 1) / 2), pc), dim3(NTHR), 0, c->stream, (int)N,
                         (int)Np, d_B, d_vec);
      hipLaunchKernelGGL(gpf::k_loo_u, dim3((unsigned)nmb, pc), dim3(NTHR), 0, c->stream, (int)N, (int)Np, d_B, d_vec);
    });
  };
  o.tiles = [&](int pc, double* partial) {
    gpf::with_cov_kind(c->kind, [&](auto KIND) {
      hipLaunchKernelGGL(gpf::k_loo_grad<KIND()>, dim3((unsigned)ntile, pc), dim3(gpf::Geo<T>::NTH), 0, c->stream, (int)N, (int)Np,
                         nt, d, c->d_x, c->d_ls, d_B, d_vec, partial);
    });
  };
  o.fetch = [&](int s, int pc) -> int {
    if (mu)
      GPF_HIP(c, hipMemcpy2DAsync(mu + (size_t)s * N, (size_t)N * 8, d_vec + (size_t)gpf::LV_MU * Np, vpitch, (size_t)N * 8,
                                  (size_t)pc, hipMemcpyDeviceToHost, c->stream));
    if (sd)
      GPF_HIP(c, hipMemcpy2DAsync(sd + (size_t)s * N, (size_t)N * 8, d_vec + (size_t)gpf::LV_SD * Np, vpitch, (size_t)N * 8,
                                  (size_t)pc, hipMemcpyDeviceToHost, c->stream));
    GPF_HIP(c, hipMemcpyAsync(c->h_loss, c->d_loss, (size_t)pc * 8, hipMemcpyDeviceToHost, c->stream));
    return GPF_OK;
  };
  o.outputs = [&](int p, int, bool bad) {
    if (bad && mu) std::fill(mu + (size_t)p * N, mu + (size_t)(p + 1) * N, (double)NAN);
    if (bad && sd) std::fill(sd + (size_t)p * N, sd + (size_t)(p + 1) * N, (double)NAN);
  };
  return objective_batch(c, knobs, o);
}

// ---- gpf_lml_hyper_batch: log marginal likelihood and its gradient in (l, a, s) ----
int gpf_lml_hyper_batch(gpf_ctx* c, const double* th, int P, double* lml, double* grad, double* qout, int* status,
                        int* bad_idx) {
  if (!c) return GPF_BAD_ARG;
  if (bad_idx) *bad_idx = -1;
  if (P < 0 || (P > 0 && (!th || !lml))) return bad_arg(c, "gpf_lml_hyper_batch: bad arguments");
  if (c->N <= 0) return bad_arg(c, "gpf_lml_hyper_batch: call gpf_set_data first");
  const int d = c->d, nt = c->nt, dh = d + 2;
  // (a, s) and the noise factor r = (s / a)^2 of every particle: they outlive the passes' copies
  std::vector<double> has((size_t)P * 2), hr((size_t)P);
  for (int p = 0; p < P; ++p) {
    const double* row = th + (size_t)p * dh;
    if (int rl = check_ls(c, "gpf_lml_hyper_batch", row, (size_t)d)) return rl;
    const double a = row[d], s = row[d + 1];
    if (!(a > 0.0) || !std::isfinite(a) || !(s > 0.0) || !std::isfinite(s))
      return bad_arg(c, "gpf_lml_hyper_batch: amplitude and noise scale must be finite and > 0");
    const double q = s / a, r = q * q;
    if (!(r > 0.0) || !std::isfinite(r))
      return bad_arg(c, "gpf_lml_hyper_batch: the noise factor (s / a)^2 must be finite and > 0");
    has[(size_t)2 * p] = a;
    has[(size_t)2 * p + 1] = s;
    hr[p] = r;
  }
  if (P == 0) return GPF_OK;
  hipSetDevice(c->device);
  const int64_t N = c->N, Np = c->Npad;
  const Knobs knobs = Knobs::from_env();
  int rc = ensure_work(c, P, knobs);
  if (rc) return rc;
  const int pcm = std::min(c->cap, P);
  // the call's own vectors: (a, s) | k_hyper_value's results | alt | alt / a
  // (synchronised regrow: the previous call's kernels may still be reading it)
  if ((rc = c->hyp.grow(c, ((size_t)pcm * (2 + gpf::HV_N) + 2 * (size_t)pcm * Np) * 8, false, true))) return rc;
  double* d_as = c->hyp.as<double>();
  double* d_out = d_as + (size_t)pcm * 2;
  double* d_al = d_out + (size_t)pcm * gpf::HV_N;
  double* d_sc = d_al + (size_t)pcm * Np;
  std::vector<double> ho((size_t)pcm * gpf::HV_N);
  Objective o;
  o.rows = th, o.stride = dh, o.P = P, o.pass = pcm, o.nfac = c->d_nfac;
  o.value = lml, o.hval = ho.data() + gpf::HV_LML, o.hstride = gpf::HV_N;
  o.grad = grad, o.gstride = dh, o.grad_flops = tri_gemm_flops(nt);  // k_lml_grad on alt / a
  o.status = status, o.bad_idx = bad_idx;
  o.upload = [&](int s, int pc) -> int {
    GPF_HIP(c, hipMemcpyAsync(c->d_nfac, hr.data() + s, (size_t)pc * 8, hipMemcpyHostToDevice, c->stream));
    GPF_HIP(c, hipMemcpyAsync(d_as, has.data() + (size_t)2 * s, (size_t)pc * 2 * 8, hipMemcpyHostToDevice, c->stream));
    return GPF_OK;
  };
  o.enqueue = [&](int pc) {
    return launch(c, PC_LOSS, 0.0, [&] {
      hipLaunchKernelGGL(gpf::k_alpha_batch, dim3((unsigned)((N + NTHR - 1) / NTHR), pc), dim3(NTHR), 0, c->stream, (int)N,
                         (int)Np, nt, c->d_szp, d_al);
      hipLaunchKernelGGL(gpf::k_hyper_value, dim3(pc), dim3(NTHR), 0, c->stream, (int)N, (int)Np, nt, c->d_y, c->d_e, d_al,
                         c->d_L, c->d_s2p, d_as, d_out);
    });
  };
  o.tiles = [&](int pc, double* partial) {
    hipLaunchKernelGGL(gpf::k_hyper_scale, dim3((unsigned)((N + NTHR - 1) / NTHR), pc), dim3(NTHR), 0, c->stream, (int)N,
                       (int)Np, d_al, d_as, d_sc);
    gpf::with_cov_kind(c->kind, [&](auto KIND) {
      hipLaunchKernelGGL(gpf::k_lml_grad<KIND()>, dim3((unsigned)(nt * (nt + 1) / 2), pc), dim3(gpf::Geo<T>::NTH), 0, c->stream,
                         (int)N, (int)Np, nt, d, c->d_x, c->d_ls, c->d_U, d_sc, partial);
    });
  };
  o.fetch = [&](int, int pc) -> int {
    GPF_HIP(c, hipMemcpyAsync(ho.data(), d_out, (size_t)pc * gpf::HV_N * 8, hipMemcpyDeviceToHost, c->stream));
    return GPF_OK;
  };
  o.outputs = [&](int p, int q, bool bad) {
    const double* r = ho.data() + (size_t)q * gpf::HV_N;
    if (qout) qout[p] = bad ? NAN : r[gpf::HV_Q];
    if (grad) {
      grad[(size_t)p * dh + d] = bad ? NAN : r[gpf::HV_DA];
      grad[(size_t)p * dh + d + 1] = bad ? NAN : r[gpf::HV_DS];
    }
  };
  return objective_batch(c, knobs, o);
}

// ---- the marginalised polynomial mean: gpf_set_basis, gpf_lml_mean_batch, gpf_predict_mean ----
int gpf_set_basis(gpf_ctx* c, const double* H, int m) {
  if (!c) return GPF_BAD_ARG;
  if (c->N <= 0) return bad_arg(c, "gpf_set_basis: call gpf_set_data first");
  if (!H || m < 1 || m > gpf::MEAN_MAX) return bad_arg(c, "gpf_set_basis: the basis needs 1 to 32 rows");
  if ((int64_t)m >= c->N) return bad_arg(c, "gpf_set_basis: the basis needs fewer rows than there are points");
  const int64_t N = c->N, Np = c->Npad;
  for (int64_t i = 0; i < (int64_t)m * N; ++i)
    if (!std::isfinite(H[i])) return bad_arg(c, "gpf_set_basis: the basis must be finite");
  const int mp = (m + 15) / 16 * 16;
  std::vector<double> hp((size_t)mp * Np, 0.0);
  for (int r = 0; r < m; ++r) std::memcpy(hp.data() + (size_t)r * Np, H + (size_t)r * N, (size_t)N * 8);
  hipSetDevice(c->device);
  GPF_HIP(c, hipStreamSynchronize(c->stream));  // (the last mean call may still read the old basis)
  hipFree(c->d_H);
  c->d_H = nullptr;
  c->bm = c->bmpad = 0;
  GPF_HIP(c, hipMalloc(&c->d_H, hp.size() * 8));
  GPF_HIP(c, hipMemcpy(c->d_H, hp.data(), hp.size() * 8, hipMemcpyHostToDevice));
  c->bm = m;
  c->bmpad = mp;
  return GPF_OK;
}

namespace {
// The per-particle buffers of a mean call inside one allocation for `pc` slots
struct MeanBufs {
  double *as, *out, *t, *beta, *La, *al, *sc, *zr, *Z, *Bt, *nBt;
  static size_t doubles(size_t pc, size_t Np, size_t mp) {
    return pc * (2 + gpf::MV_N + 2 * gpf::MEAN_MAX + gpf::MEAN_MAX * gpf::MEAN_MAX + 3 * Np + 3 * Np * mp);
  }
  MeanBufs(double* base, size_t pc, size_t Np, size_t mp) {
    as = base;
    out = as + pc * 2;
    t = out + pc * gpf::MV_N;
    beta = t + pc * gpf::MEAN_MAX;
    La = beta + pc * gpf::MEAN_MAX;                // k_mean_small's Lai = La^-1, 32 x 32 per slot
    al = La + pc * gpf::MEAN_MAX * gpf::MEAN_MAX;  // (an even offset: Z's 16-byte loads stay aligned)
    sc = al + pc * Np;
    zr = sc + pc * Np;
    Z = zr + pc * Np;
    Bt = Z + pc * Np * mp;
    nBt = Bt + pc * Np * mp;  // -Bt: k_mean_grad's A panel
  }
};
}  // namespace

// Z = U H^T, then k_mean_small, for the first pc slots of the workspace on c->stream
static int mean_enqueue_small(gpf_ctx* c, int pc, const MeanBufs& b) {
  const int Np = (int)c->Npad, nt = c->nt, N = (int)c->N, m = c->bm, mp = c->bmpad;
  const double bytes = 8.0 * T * T * (double)(nt * (nt + 1) / 2) * pc;
  int rc = launch(c, PC_LOSS, bytes, [&] {
    if (mp == 16)
      hipLaunchKernelGGL(gpf::k_mean_nn<1>, dim3(nt, pc), dim3(gpf::DNTH), 0, c->stream, Np, nt, c->d_U, c->d_H, b.Z);
    else
      hipLaunchKernelGGL(gpf::k_mean_nn<2>, dim3(nt, pc), dim3(gpf::DNTH), 0, c->stream, Np, nt, c->d_U, c->d_H, b.Z);
  });
  if (rc) return rc;
  // (the partials of Z^T Z wait in Bt's place, nt mp^2 of its 128 nt mp doubles per slot: Bt is formed
  // after k_mean_small has added them up)
  return launch(c, PC_LOSS, 0.0, [&] {
    if (mp == 16) {
      hipLaunchKernelGGL(gpf::k_mean_gram<16>, dim3(nt, pc), dim3(NTHR), 0, c->stream, Np, nt, m, b.Z, b.Bt);
      hipLaunchKernelGGL(gpf::k_mean_small<16>, dim3(pc), dim3(NTHR), 0, c->stream, N, Np, nt, m, b.Z, b.Bt, c->d_yb, c->d_L,
                         b.as, b.out, b.t, b.beta, b.La, b.zr);
    } else {
      hipLaunchKernelGGL(gpf::k_mean_gram<32>, dim3(nt, pc), dim3(NTHR), 0, c->stream, Np, nt, m, b.Z, b.Bt);
      hipLaunchKernelGGL(gpf::k_mean_small<32>, dim3(pc), dim3(NTHR), 0, c->stream, N, Np, nt, m, b.Z, b.Bt, c->d_yb, c->d_L,
                         b.as, b.out, b.t, b.beta, b.La, b.zr);
    }
  });
}

// Zo^T U for the first pc slots into out[slot * ostride + row * rs + column * cs], and its negative
// into nout (nullable) likewise (k_mean_tn)
static int mean_enqueue_tn(gpf_ctx* c, int pc, const MeanBufs& b, double* out, double* nout, size_t ostride, int rs, int cs) {
  const int Np = (int)c->Npad, nt = c->nt;
  const double bytes = 8.0 * T * T * (double)(nt * (nt + 1) / 2) * pc;
  return launch(c, PC_LOSS, bytes, [&] {
    if (c->bmpad == 16)
      hipLaunchKernelGGL(gpf::k_mean_tn<1>, dim3(nt, pc), dim3(gpf::DNTH), 0, c->stream, Np, nt, c->d_U, b.Z, out, nout, ostride,
                         rs, cs);
    else
      hipLaunchKernelGGL(gpf::k_mean_tn<2>, dim3(nt, pc), dim3(gpf::DNTH), 0, c->stream, Np, nt, c->d_U, b.Z, out, nout, ostride,
                         rs, cs);
  });
}

int gpf_lml_mean_batch(gpf_ctx* c, const double* th, int P, double* lml, double* grad, double* beta, double* qout,
                       int* status, int* bad_idx) {
  if (!c) return GPF_BAD_ARG;
  if (bad_idx) *bad_idx = -1;
  if (P < 0 || (P > 0 && (!th || !lml))) return bad_arg(c, "gpf_lml_mean_batch: bad arguments");
  if (c->N <= 0) return bad_arg(c, "gpf_lml_mean_batch: call gpf_set_data first");
  if (c->bm <= 0) return bad_arg(c, "gpf_lml_mean_batch: no basis for this data: call gpf_set_basis after gpf_set_data");
  const int d = c->d, nt = c->nt, dh = d + 2, m = c->bm, mp = c->bmpad;
  std::vector<double> has((size_t)P * 2), hr((size_t)P);
  for (int p = 0; p < P; ++p) {
    const double* row = th + (size_t)p * dh;
    if (int rl = check_ls(c, "gpf_lml_mean_batch", row, (size_t)d)) return rl;
    const double a = row[d], s = row[d + 1];
    if (!(a > 0.0) || !std::isfinite(a) || !(s > 0.0) || !std::isfinite(s))
      return bad_arg(c, "gpf_lml_mean_batch: amplitude and noise scale must be finite and > 0");
    const double q = s / a, r = q * q;
    if (!(r > 0.0) || !std::isfinite(r))
      return bad_arg(c, "gpf_lml_mean_batch: the noise factor (s / a)^2 must be finite and > 0");
    has[(size_t)2 * p] = a;
    has[(size_t)2 * p + 1] = s;
    hr[p] = r;
  }
  if (P == 0) return GPF_OK;
  hipSetDevice(c->device);
  const int64_t N = c->N, Np = c->Npad;
  const Knobs knobs = Knobs::from_env();
  int rc = ensure_work(c, P, knobs);
  if (rc) return rc;
  const int pcm = std::min(c->cap, P);
  // (synchronised regrow: the previous call's kernels may still be reading it)
  if ((rc = c->mean.grow(c, MeanBufs::doubles((size_t)pcm, (size_t)Np, (size_t)mp) * 8, false, true))) return rc;
  const MeanBufs b(c->mean.as<double>(), (size_t)pcm, (size_t)Np, (size_t)mp);
  const int ntile = nt * (nt + 1) / 2;
  std::vector<double> ho((size_t)pcm * gpf::MV_N), hb((size_t)pcm * gpf::MEAN_MAX);
  Objective o;
  o.rows = th, o.stride = dh, o.P = P, o.pass = pcm, o.nfac = c->d_nfac;
  o.value = lml, o.hval = ho.data() + gpf::MV_LML, o.hstride = gpf::MV_N;
  // k_mean_grad: k_lml_grad's chain and mpad more of depth on every lower tile
  o.grad = grad, o.gstride = dh, o.grad_flops = tri_gemm_flops(nt) + 2.0 * (double)T * T * mp * (double)ntile;
  o.status = status, o.bad_idx = bad_idx;
  o.upload = [&](int s, int pc) -> int {
    GPF_HIP(c, hipMemcpyAsync(c->d_nfac, hr.data() + s, (size_t)pc * 8, hipMemcpyHostToDevice, c->stream));
    GPF_HIP(c, hipMemcpyAsync(b.as, has.data() + (size_t)2 * s, (size_t)pc * 2 * 8, hipMemcpyHostToDevice, c->stream));
    return GPF_OK;
  };
  o.enqueue = [&](int pc) -> int {
    if (int r1 = mean_enqueue_small(c, pc, b)) return r1;
    if (!grad) return GPF_OK;
    // Bt = Zo^T U, then alt, at / a and the derivatives in a and s
    if (int r2 = mean_enqueue_tn(c, pc, b, b.Bt, b.nBt, (size_t)mp * Np, (int)Np, 1)) return r2;
    return launch(c, PC_LOSS, 0.0, [&] {
      hipLaunchKernelGGL(gpf::k_alpha_batch, dim3((unsigned)((N + NTHR - 1) / NTHR), pc), dim3(NTHR), 0, c->stream, (int)N,
                         (int)Np, nt, c->d_szp, b.al);
      hipLaunchKernelGGL(gpf::k_mean_hyper, dim3(pc), dim3(NTHR), 0, c->stream, (int)N, (int)Np, nt, m, mp, c->d_e, b.al,
                         c->d_s2p, b.Bt, b.t, b.as, b.out, b.sc);
    });
  };
  o.tiles = [&](int pc, double* partial) {
    gpf::with_cov_kind(c->kind, [&](auto KIND) {
      hipLaunchKernelGGL(gpf::k_mean_grad<KIND()>, dim3((unsigned)ntile, pc), dim3(gpf::Geo<T>::NTH), 0, c->stream, (int)N, (int)Np,
                         nt, d, mp, c->d_x, c->d_ls, c->d_U, b.Bt, b.nBt, b.sc, partial);
    });
  };
  o.fetch = [&](int, int pc) -> int {
    GPF_HIP(c, hipMemcpyAsync(ho.data(), b.out, (size_t)pc * gpf::MV_N * 8, hipMemcpyDeviceToHost, c->stream));
    if (beta) GPF_HIP(c, hipMemcpyAsync(hb.data(), b.beta, (size_t)pc * gpf::MEAN_MAX * 8, hipMemcpyDeviceToHost, c->stream));
    return GPF_OK;
  };
  o.failed = [&](int q) {
    if (ho[(size_t)q * gpf::MV_N + gpf::MV_BAD] == 0.0) return false;
    c->err = "H Kt^-1 H^T is not positive definite (the basis is rank-deficient for this particle)";
    return true;
  };
  o.outputs = [&](int p, int q, bool bad) {
    const double* r = ho.data() + (size_t)q * gpf::MV_N;
    if (qout) qout[p] = bad ? NAN : r[gpf::MV_Q];
    if (beta)
      for (int k = 0; k < m; ++k) beta[(size_t)p * m + k] = bad ? NAN : hb[(size_t)q * gpf::MEAN_MAX + k];
    if (grad) {
      grad[(size_t)p * dh + d] = bad ? NAN : r[gpf::MV_DA];
      grad[(size_t)p * dh + d + 1] = bad ? NAN : r[gpf::MV_DS];
    }
  };
  return objective_batch(c, knobs, o);
}

// gpf_predict_mean's kept buffers: gpf_predict's, then its own
enum PmeanBuf {
  PMEAN_HF = PRED_NBUF,  // the basis at the chunk's query points, mpad x Cp
  PMEAN_W,               // the single particle's MeanBufs
  PMEAN_BT,              // Bt^T zero-padded to a 128-wide operand, Np x 128
  PMEAN_KB,              // K_s^T Bt^T of the chunk, Cp x 128
  PMEAN_PART,            // k_con_tn's partial tiles
  PMEAN_HH,              // pinned staging of the basis
  PMEAN_NBUF
};
constexpr unsigned PMEAN_PINNED = PRED_PINNED | 1u << PMEAN_HH;
// depth tiles per piece of K_s^T Bt^T: a constant, so that the pieces (and with them every bit of the
// result) do not depend on the query chunk
constexpr int PMEAN_PER = 4;

static SetPlan pmean_plan(const gpf_ctx* c, int64_t Cp) {
  SetPlan p = pred_plan(c, Cp);
  const size_t C = (size_t)Cp, Np = (size_t)c->Npad;
  p.bytes[PMEAN_HF] = p.bytes[PMEAN_HH] = (size_t)c->bmpad * C * 8;
  p.bytes[PMEAN_W] = MeanBufs::doubles(1, Np, (size_t)c->bmpad) * 8;
  p.bytes[PMEAN_BT] = Np * T * 8;
  p.bytes[PMEAN_KB] = C * T * 8;
  p.bytes[PMEAN_PART] = (size_t)((c->nt + PMEAN_PER - 1) / PMEAN_PER) * (C / T) * gpf::LIN_TT * 8;
  return p;
}

int gpf_predict_mean(gpf_ctx* c, const double* ls, const double* xfit, const double* hfit, int64_t M, int64_t batch,
                     double* mu, double* sd, double* beta, double* bcov) {
  if (!c) return GPF_BAD_ARG;
  if (c->N <= 0) return bad_arg(c, "gpf_predict_mean: call gpf_set_data first");
  if (c->bm <= 0) return bad_arg(c, "gpf_predict_mean: no basis for this data: call gpf_set_basis after gpf_set_data");
  if (M < 0 || (M > 0 && (!xfit || !hfit || !mu || !sd)) || !ls) return bad_arg(c, "gpf_predict_mean: bad arguments");
  if (int rl = check_ls(c, "gpf_predict_mean", ls, (size_t)c->d)) return rl;
  if (M == 0) return GPF_OK;
  KeptSet& ks = c->kept[KEPT_PMEAN];
  const int64_t Np = c->Npad;
  const int nt = c->nt, m = c->bm, mp = c->bmpad;
  const int pieces = (nt + PMEAN_PER - 1) / PMEAN_PER;
  auto bufs = [&] { return MeanBufs(ks.as(PMEAN_W), 1, (size_t)Np, (size_t)mp); };
  std::vector<double> hsmall(gpf::MV_N + 2 * gpf::MEAN_MAX);               // out | t | beta of slot 0
  std::vector<double> inv(bcov ? (size_t)gpf::MEAN_MAX * gpf::MEAN_MAX : 0);  // k_mean_small's Lai = La^-1
  Prediction q{"gpf_predict_mean", KEPT_PMEAN, pmean_plan, PMEAN_NBUF, PMEAN_PINNED,
               (Np + 2 * nt + T + mp + (int64_t)pieces * T) * 8, ls, xfit, M, batch, mu, sd};
  q.rows = hfit;
  q.nrows = m;
  q.rows_host = PMEAN_HH;
  q.rows_dev = PMEAN_HF;
  q.before_factor = [&]() -> int {
    const double ones[2] = {1.0, 1.0};  // the unit model: (a, s) go through the data (gpfit.amplitude.scaled_data)
    GPF_HIP(c, hipMemcpyAsync(bufs().as, ones, 16, hipMemcpyHostToDevice, c->stream));
    GPF_HIP(c, hipMemsetAsync(ks.as(PMEAN_BT), 0, (size_t)Np * T * 8, c->stream));
    return GPF_OK;
  };
  // Zo, t, beta, La and zr of slot 0, then Bt^T into the 128-wide operand
  q.after_factor = [&] {
    const int rc = mean_enqueue_small(c, 1, bufs());
    return rc ? rc : mean_enqueue_tn(c, 1, bufs(), ks.as(PMEAN_BT), nullptr, 0, 1, T);
  };
  q.z = [&] { return (const double*)bufs().zr; };  // K_s^T at and sum v^2: gpf_predict's kernel with zr in z's place
  q.out = [&](int64_t s, int64_t mq, int64_t Cp) -> int {
    const int nqt = (int)((mq + T - 1) / T);
    const MeanBufs b = bufs();
    // K_s^T Bt^T over fixed depth pieces, added in piece order
    int rc = launch(c, PC_PRED, 2.0 * (double)Np * nqt * T * T, [&] {
      hipLaunchKernelGGL(gpf::k_con_tn, dim3((unsigned)nqt, (unsigned)pieces), dim3(gpf::Geo<T>::NTH), 0, c->stream, 1, nt,
                         PMEAN_PER, 0, ks.as(PRED_KS), (int)Cp, ks.as(PMEAN_BT), T, ks.as(PMEAN_PART));
      hipLaunchKernelGGL(gpf::k_lin_reduce, dim3((unsigned)nqt, 8), dim3(NTHR), 0, c->stream, 1, 0, pieces, ks.as(PMEAN_PART),
                         (const double*)nullptr, 1.0, ks.as(PMEAN_KB), (int64_t)T);
    });
    if (rc) return rc;
    rc = launch(c, PC_LOSS, 0.0, [&] {
      hipLaunchKernelGGL(gpf::k_mean_out, dim3((unsigned)((mq + NTHR - 1) / NTHR)), dim3(NTHR), 0, c->stream, nt, (int)mq, m,
                         ks.as(PRED_VZ), (int)Cp, ks.as(PRED_VSQ), ks.as(PMEAN_HF), ks.as(PMEAN_KB), T, b.La, b.beta,
                         ks.as(PRED_MU), ks.as(PRED_SD));
    });
    if (!rc && s == 0 && hipMemcpyAsync(hsmall.data(), b.out, hsmall.size() * 8, hipMemcpyDeviceToHost, c->stream) != hipSuccess) {
      rc = GPF_HIP_ERROR;
      c->err = "gpf_predict_mean: copy back failed";
    }
    return rc;
  };
  q.first_check = [&]() -> int {  // At's status; the stream is idle: La for cov(beta) while the set is held
    if (hsmall[gpf::MV_BAD] != 0.0) {
      c->err = "H Kt^-1 H^T is not positive definite (the basis is rank-deficient at these length scales)";
      return GPF_NOT_PD;
    }
    if (bcov) GPF_HIP(c, hipMemcpy(inv.data(), bufs().La, inv.size() * 8, hipMemcpyDeviceToHost));
    return GPF_OK;
  };
  const int rc = predict_chunks(c, q);
  if (rc) return rc;
  // out | t | beta lie behind one another in MeanBufs: beta from the copy of chunk 0
  if (beta) std::memcpy(beta, hsmall.data() + gpf::MV_N + gpf::MEAN_MAX, (size_t)m * 8);
  if (bcov)  // cov(beta) = At^-1 = Lai^T Lai (m <= 32: on the host)
    for (int i = 0; i < m; ++i)
      for (int j = 0; j < m; ++j) {
        double v = 0.0;
        for (int k = std::max(i, j); k < m; ++k) v += inv[(size_t)k * gpf::MEAN_MAX + i] * inv[(size_t)k * gpf::MEAN_MAX + j];
        bcov[(size_t)i * m + j] = v;
      }
  return GPF_OK;
}

// ---- gpf_predict_batch: prediction for a batch of length-scale samples and their mixture ----

// Device bytes of a gpf_predict_batch pass per particle and padded query column (the K_s column, the
// vsq / vz partials, the staging of mu_p, sd_p and var_p) ...
static double pbatch_col_bytes(const gpf_ctx* c) { return 8.0 * ((double)c->Npad + 2.0 * c->nt + 3.0); }
// ... and of the call whatever the chunks: the coordinates, the mixture state, (mix_mu | mix_sd), the weights
static double pbatch_fixed_bytes(const gpf_ctx* c, int64_t Mp, int P) { return 8.0 * ((c->d + 6.0) * (double)Mp + P); }

// gpf_predict_batch's kept buffers
enum PbatchBuf {
  PBATCH_XF = 0,  // the query coordinates, d x Mp
  PBATCH_KS,      // the chunk's K_s blocks, pc x Np x Cq
  PBATCH_VSQ,     // the vsq / vz partials, pc x nt x Cq each
  PBATCH_VZ,
  PBATCH_W,       // the weights, P
  PBATCH_STATE,   // the mixture state, 4 x Mp
  PBATCH_MIX,     // (mix_mu | mix_sd), 2 x Mp
  PBATCH_EACH,    // (mu_p | sd_p | var_p) of the pass, pc x Cq each
  PBATCH_HEACH,   // pinned host copy of (mu_p | sd_p), when the caller asks for per-particle output
  PBATCH_NBUF
};
constexpr unsigned PBATCH_PINNED = 1u << PBATCH_HEACH;

// npc: particles per chunk x padded query columns per pass, as pbatch_plan sized them (on
// pbatch_col_bytes / pbatch_fixed_bytes: the same bytes per column and per call)
static SetPlan pbatch_bytes(const gpf_ctx* c, int64_t Mp, int P, size_t npc, bool each) {
  SetPlan p{};
  p.bytes[PBATCH_XF] = (size_t)c->d * Mp * 8;
  p.bytes[PBATCH_KS] = npc * (size_t)c->Npad * 8;
  p.bytes[PBATCH_VSQ] = p.bytes[PBATCH_VZ] = npc * c->nt * 8;
  p.bytes[PBATCH_W] = (size_t)P * 8;
  p.bytes[PBATCH_STATE] = (size_t)4 * Mp * 8;
  p.bytes[PBATCH_MIX] = (size_t)2 * Mp * 8;
  p.bytes[PBATCH_EACH] = 3 * npc * 8;
  p.bytes[PBATCH_HEACH] = each ? 2 * npc * 8 : 0;
  return p;
}

// The particle-chunk capacity pc and the query chunk cq (padded columns per pass) of a
// gpf_predict_batch call, planned together: ensure_work alone sizes the factorisation workspace to
// GPF_MEM_FRACTION (0.85) of the free memory, which at large N leaves no room for the particles'
// K_s blocks. The workspace of pc particles is taken first; the call's own buffers (fixed +
// pc col cq bytes) must then fit half of what is left. A workspace the context already holds with
// at least pc slots is kept if the buffers fit beside it; if they do not (an earlier batch took
// most of the memory) it is given back and regrown to pc slots (regrow). The query chunk is halved
// down to 128 before the particle chunk shrinks (by a quarter per step): a smaller query chunk costs
// launches, a smaller particle chunk changes the factorisation's schedule. keep > 0 (chunk = 0, the
// default): the chunk also stays within GPF_PREDICT_KEEP_MB while that leaves at least 512 columns per
// pass, so that the next call finds the buffers (DESIGN.md 2h has the measurement).
// Pure: free_b = free device bytes, held_b = this call's kept buffers, cap slots of per bytes held.
struct PbatchPlan {
  int pc = 0;
  int64_t cq = 0;
  bool regrow = false;
  double left = 0.0;  // what the last candidate had for the call's buffers (for the error message)
};
static bool pbatch_plan_pure(double free_b, double held_b, int cap, double per, double col, double fixed, int pc0, int64_t cq0,
                             double keep, double frac, PbatchPlan* out) {
  // what a regrown workspace starts from: free_work returns the old one and this call's kept buffers
  const double avail = free_b + held_b, avail_regrown = avail + (double)cap * per;
  int pc = std::max(1, pc0);
  if (cap < pc) pc = (int)std::max(1.0, std::min((double)pc, std::floor(avail_regrown * frac / per)));
  for (;;) {
    for (int regrow = cap >= pc ? 0 : 1; regrow < 2; ++regrow) {
      if (regrow && (double)pc * per > avail_regrown * frac) continue;  // (ensure_work would give fewer slots)
      const double left = regrow ? avail_regrown - (double)pc * per : avail;
      out->left = left;
      int64_t cq = cq0;
      while (cq > T && fixed + (double)pc * col * (double)cq > 0.5 * left) cq = ((cq / 2 + T - 1) / T) * T;
      if (keep > 0.0 && fixed + (double)pc * col * (double)cq > keep) {
        const int64_t kq = (int64_t)((keep - fixed) / ((double)pc * col)) / T * T;
        if (kq >= 512) cq = std::min(cq, kq);
      }
      if (fixed + (double)pc * col * (double)cq <= 0.5 * left) {
        out->pc = pc;
        out->cq = cq;
        out->regrow = regrow && cap >= pc;  // (cap < pc: ensure_work regrows anyway)
        return true;
      }
    }
    if (pc == 1) return false;
    pc -= std::max(1, pc / 4);
  }
}

static int pbatch_plan(gpf_ctx* c, const Knobs& k, int P, int64_t M, int64_t chunk, PbatchPlan* plan) {
  const int64_t Mp = ((M + T - 1) / T) * T;
  int64_t cq0 = chunk > 0 ? std::min<int64_t>(chunk, 65536) : 16384;
  cq0 = std::min<int64_t>(((cq0 + T - 1) / T) * T, Mp);
  size_t fr = 0, tot = 0;
  GPF_HIP(c, hipMemGetInfo(&fr, &tot));
  const double per = (double)bytes_per_particle(c), col = pbatch_col_bytes(c), fixed = pbatch_fixed_bytes(c, Mp, P);
  int pc = std::min(P, 65535);  // (the particle is a grid axis of k_predict_vsq_batch)
  if (k.max_chunk.set) pc = (int)std::max<long long>(1, std::min<long long>(pc, k.max_chunk.i));
  if (pbatch_plan_pure((double)fr, c->kept[KEPT_PBATCH].held(), c->cap, per, col, fixed, pc, cq0, chunk == 0 ? keep_bytes(k) : 0.0,
                       k.mem_fraction.set ? k.mem_fraction.f : 0.85, plan))
    return GPF_OK;
  const double mfit = (0.5 * plan->left - col * T) / (8.0 * (c->d + 6.0));
  const double all = (double)fr + c->kept[KEPT_PBATCH].held() + (double)c->cap * per;
  c->err = "gpf_predict_batch: N=" + std::to_string(c->N) + ", M=" + std::to_string(M) +
           " do not fit half of the free device memory with one particle at chunk 128: " +
           (mfit >= 1.0 ? "the largest M that fits at this N is about " + std::to_string((long long)mfit)
                        : "the largest N that fits is about " +
                              std::to_string((long long)std::max(0.0, std::sqrt(std::max(0.0, 0.5 * all) / 16.0))));
  return GPF_BAD_ARG;
}

int gpf_predict_batch(gpf_ctx* c, const double* ls, int P, const double* w, const double* xfit, int64_t M, int64_t chunk,
                      double* mix_mu, double* mix_sd, double* mu_PM, double* sd_PM, int* bad_idx) {
  if (!c) return GPF_BAD_ARG;
  if (bad_idx) *bad_idx = -1;
  if (c->N <= 0) return bad_arg(c, "gpf_predict_batch: call gpf_set_data first");
  if (P < 0 || M < 0 || chunk < 0) return bad_arg(c, "gpf_predict_batch: P, M and chunk must be >= 0");
  if (M > (int64_t)1 << 30) return bad_arg(c, "gpf_predict_batch: M too large");
  if (P > 0 && M > 0 && (!ls || !xfit || !mix_mu || !mix_sd)) return bad_arg(c, "gpf_predict_batch: null buffer");
  const int d = c->d, nt = c->nt;
  if (ls)
    if (int rl = check_ls(c, "gpf_predict_batch", ls, (size_t)P * d)) return rl;
  // the weights, normalised to sum 1 (null: equal)
  std::vector<double> wn((size_t)P, P > 0 ? 1.0 / (double)P : 0.0);
  if (w && P > 0) {
    double sum = 0.0;
    for (int p = 0; p < P; ++p) {
      if (!(w[p] >= 0.0) || !std::isfinite(w[p])) return bad_arg(c, "gpf_predict_batch: weights must be finite and >= 0");
      sum += w[p];
    }
    if (!(sum > 0.0) || !std::isfinite(sum)) return bad_arg(c, "gpf_predict_batch: the weights must have a finite sum > 0");
    for (int p = 0; p < P; ++p) wn[p] = w[p] / sum;
  }
  if (P == 0 || M == 0) return GPF_OK;
  Knobs knobs;
  posterior_open(c, 0, &knobs);  // (the workspace below, once the plan has sized it)
  const int64_t N = c->N, Np = c->Npad, Mp = ((M + T - 1) / T) * T;
  const bool each = mu_PM || sd_PM;
  PbatchPlan plan;
  int rc = pbatch_plan(c, knobs, P, M, chunk, &plan);
  if (rc) return rc;
  int cap = plan.pc;
  const int64_t Cq = plan.cq;
  // the factorisation workspace first: a (re)allocation there frees this call's buffers too
  if (plan.regrow) {  // the workspace an earlier, larger batch left would not leave room: back to cap slots
    GPF_HIP(c, hipStreamSynchronize(c->stream));
    free_work(c);
  }
  if ((rc = ensure_work(c, cap, knobs))) return rc;
  cap = std::min(cap, c->cap);
  const size_t npc = (size_t)cap * (size_t)Cq;
  // (the budget check was the plan's: it counted what the set holds as free, and the regrow gives it back first)
  KeptSet& ks = c->kept[KEPT_PBATCH];
  const SetPlan need = pbatch_bytes(c, Mp, P, npc, each);
  if (!ks.fits(need.bytes, PBATCH_NBUF))
    if ((rc = ks.regrow(c, need.bytes, PBATCH_PINNED, PBATCH_NBUF))) return rc;
  double *d_xf = ks.as(PBATCH_XF), *d_ks = ks.as(PBATCH_KS), *d_vsq = ks.as(PBATCH_VSQ), *d_vz = ks.as(PBATCH_VZ);
  double *d_w = ks.as(PBATCH_W), *d_st = ks.as(PBATCH_STATE), *d_mix = ks.as(PBATCH_MIX), *d_emu = ks.as(PBATCH_EACH);
  double *d_evar = d_emu + 2 * npc, *heach = ks.as(PBATCH_HEACH);
  double* d_esd = each ? d_emu + npc : nullptr;
  // the query coordinates (leading dimension Mp), the weights and the zeroed mixture state, once
  GPF_HIP(c, hipMemcpy2DAsync(d_xf, (size_t)Mp * 8, xfit, (size_t)M * 8, (size_t)M * 8, (size_t)d, hipMemcpyHostToDevice,
                              c->stream));
  GPF_HIP(c, hipMemcpyAsync(d_w, wn.data(), (size_t)P * 8, hipMemcpyHostToDevice, c->stream));
  GPF_HIP(c, hipMemsetAsync(d_st, 0, (size_t)4 * Mp * 8, c->stream));
  // 0: one particle after the other; 1: the deepest row tiles of all particles first (k_predict_vsq_batch)
  // (default by pass: where one particle's tiles of a full pass fill the 512 resident workgroup slots its
  // operands are shared while it runs, order 0; where they do not, several particles are resident either way
  // and the shorter tail wins, order 1 — at N=4096, P=64: 0.97-0.98x the time at 79 column tiles, 1.05-1.08x
  // at 7)
  const int nqt_full = (int)(std::min<int64_t>(Cq, Mp) / T);
  const int order = knobs.predbatch_order.num((long long)nqt_full * nt < 512 ? 1 : 0) != 0;
  // the K_s blocks: 1: k_cross_cov_batch, one launch per pass; 0: k_cross_cov once per particle (bitwise equal)
  const bool ks_batched = knobs.predbatch_ks.flag(true);
  for (int s = 0; s < P && rc == GPF_OK; s += cap) {
    const int pc = std::min(cap, P - s);
    std::memcpy(c->h_ls, ls + (size_t)s * d, (size_t)pc * d * 8);
    GPF_HIP(c, hipMemcpyAsync(c->d_ls, c->h_ls, (size_t)pc * d * 8, hipMemcpyHostToDevice, c->stream));
    GPF_HIP(c, hipMemsetAsync(c->d_info, 0, (size_t)pc * 4, c->stream));
    if ((rc = run_factor(c, pc, knobs))) break;
    GPF_HIP(c, hipMemcpyAsync(c->h_info, c->d_info, (size_t)pc * 4, hipMemcpyDeviceToHost, c->stream));
    for (int64_t s0 = 0; s0 < M && rc == GPF_OK; s0 += Cq) {
      const int64_t m = std::min<int64_t>(Cq, M - s0);
      const int nqt = (int)((m + T - 1) / T);
      const int Cm = nqt * T;
      // the particles' K_s blocks (Np x Cm, leading dimension Cq), every element bitwise gpf_predict's: one
      // k_cross_cov_batch launch (at N=100, P=64 the 64 launches of k_cross_cov took 0.51 of the call's 1.2 ms,
      // the one launch 0.13; profiles/predict_batch/bench.json)
      rc = launch(c, PC_PREDK, 8.0 * Np * Cm * (double)pc, [&] {
        if (ks_batched) {
          gpf::launch_cross_cov_batch(c->stream, c->kind, pc, (int)N, (int)m, (int)Np, Cm, d, c->d_x, (int)N, d_xf + s0, (int)Mp,
                                      c->d_ls, d_ks, Cq, (size_t)Np * Cq);
          return;
        }
        for (int q = 0; q < pc; ++q)
          gpf::launch_cross_cov(c->stream, c->kind, (int)N, (int)m, (int)Np, Cm, d, c->d_x, (int)N, d_xf + s0, (int)Mp,
                                c->d_ls + (size_t)q * d, d_ks + (size_t)q * Np * Cq, Cq);
      });
      if (rc) break;
      rc = launch(c, PC_PRED, v_flops(nt, Cm) * pc, [&] {
        hipLaunchKernelGGL(gpf::k_predict_vsq_batch, order ? dim3(nqt, pc, nt) : dim3(nqt, nt, pc), dim3(gpf::Geo<T>::NTH), 0,
                           c->stream, (int)Np, nt, c->d_U, d_ks, (int)Cq, (size_t)Np * Cq, d_vsq, c->d_yb, d_vz, order);
      });
      if (rc) break;
      rc = launch(c, PC_LOSS, 0.0, [&] {
        hipLaunchKernelGGL(gpf::k_predict_each, dim3((unsigned)((m + NTHR - 1) / NTHR), pc), dim3(NTHR), 0, c->stream, nt,
                           (int)m, d_vz, d_vsq, (int)Cq, d_emu, d_evar, d_esd, Cq);
        hipLaunchKernelGGL(gpf::k_predict_mix, dim3((unsigned)((m + NTHR - 1) / NTHR)), dim3(NTHR), 0, c->stream, (int)m, pc,
                           d_emu, d_evar, Cq, d_w + s, d_st + s0, Mp);
      });
      if (rc) break;
      if (each) {
        if (hipMemcpyAsync(heach, d_emu, 2 * npc * 8, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
            hipStreamSynchronize(c->stream) != hipSuccess) {
          rc = GPF_HIP_ERROR;
          c->err = "gpf_predict_batch: copy back failed";
          break;
        }
        for (int q = 0; q < pc; ++q) {
          if (mu_PM) std::memcpy(mu_PM + (size_t)(s + q) * M + s0, heach + (size_t)q * Cq, (size_t)m * 8);
          if (sd_PM) std::memcpy(sd_PM + (size_t)(s + q) * M + s0, heach + npc + (size_t)q * Cq, (size_t)m * 8);
        }
      }
    }
    if (rc) break;
    if (hipStreamSynchronize(c->stream) != hipSuccess) {
      rc = GPF_HIP_ERROR;
      c->err = "gpf_predict_batch: synchronisation failed";
      break;
    }
    if (c->prof) harvest(c);
    for (int q = 0; q < pc && rc == GPF_OK; ++q) {
      rc = particle_status(c, q);
      if (rc == GPF_NOT_PD && bad_idx) *bad_idx = s + q;
    }
  }
  if (rc == GPF_OK) {
    rc = launch(c, PC_LOSS, 0.0, [&] {
      hipLaunchKernelGGL(gpf::k_predict_mix_out, dim3((unsigned)((M + NTHR - 1) / NTHR)), dim3(NTHR), 0, c->stream, M, d_st, Mp,
                         d_mix, d_mix + Mp);
    });
    if (rc == GPF_OK && (hipMemcpyAsync(mix_mu, d_mix, (size_t)M * 8, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
                         hipMemcpyAsync(mix_sd, d_mix + Mp, (size_t)M * 8, hipMemcpyDeviceToHost, c->stream) != hipSuccess)) {
      rc = GPF_HIP_ERROR;
      c->err = "gpf_predict_batch: copy back failed";
    }
  }
  return posterior_close(c, ks, knobs, rc);
}

// Host-only: gpf_predict_batch's memory plan for given byte counts (no device, no context): see gpfit.h.
int gpf_predict_batch_plan(double free_b, double held_b, int cap_slots, double per_particle_b, double per_col_b, double fixed_b,
                           int P, int64_t Mpad, int64_t chunk, double keep_b, double mem_fraction, int* pc, int64_t* cq,
                           int* regrow) {
  if (!pc || !cq || !regrow || P < 1 || Mpad < T || Mpad % T || chunk < 0 || !(per_particle_b > 0.0) || !(per_col_b > 0.0))
    return GPF_BAD_ARG;
  int64_t cq0 = chunk > 0 ? std::min<int64_t>(chunk, 65536) : 16384;
  cq0 = std::min<int64_t>(((cq0 + T - 1) / T) * T, Mpad);
  PbatchPlan plan;
  if (!pbatch_plan_pure(free_b, held_b, cap_slots, per_particle_b, per_col_b, fixed_b, std::min(P, 65535), cq0,
                        chunk == 0 ? keep_b : 0.0, mem_fraction, &plan))
    return GPF_BAD_ARG;
  *pc = plan.pc;
  *cq = plan.cq;
  *regrow = plan.regrow ? 1 : 0;
  return GPF_OK;
}

// Host-only structural check of the k_step dispatch plan (no device, no context): see gpfit.h.
int gpf_plan_check(int pc, int nt, long long* stats, char* msg, int msg_len) {
  return plan_check(pc, nt, Knobs::from_env(), stats, msg, msg_len);
}

int gpf_sync(gpf_ctx* c) {
  if (!c) return GPF_BAD_ARG;
  GPF_HIP(c, hipSetDevice(c->device));
  GPF_HIP(c, hipDeviceSynchronize());
  return GPF_OK;
}

int gpf_set_profiling(gpf_ctx* c, int on) {
  if (!c) return GPF_BAD_ARG;
  c->prof = on != 0;  // (profiled batches take the plain launch path, never a graph)
  if (c->prof && !c->d_clk) {
    hipSetDevice(c->device);
    GPF_HIP(c, hipMalloc(&c->d_clk, 2 * sizeof(unsigned long long)));
    GPF_HIP(c, hipMemsetAsync(c->d_clk, 0, 2 * sizeof(unsigned long long), c->stream));
  }
  return GPF_OK;
}

int gpf_reset_profile(gpf_ctx* c) {
  if (!c) return GPF_BAD_ARG;
  hipSetDevice(c->device);
  hipStreamSynchronize(c->stream);
  harvest(c);
  std::memset(c->acc, 0, sizeof(c->acc));
  c->evals = 0;
  if (!c->d_clk) GPF_HIP(c, hipMalloc(&c->d_clk, 2 * sizeof(unsigned long long)));
  GPF_HIP(c, hipMemsetAsync(c->d_clk, 0, 2 * sizeof(unsigned long long), c->stream));
  return GPF_OK;
}

int gpf_get_profile(gpf_ctx* c, double* out, int n) {
  if (!c || !out) return 0;
  hipStreamSynchronize(c->stream);
  harvest(c);
  double v[24] = {c->acc[PC_PANEL][0],  c->acc[PC_PANEL][1],  c->acc[PC_PANEL][2], c->acc[PC_DIAG][0],
                  c->acc[PC_DIAG][1],   c->acc[PC_DIAG][2],   c->acc[PC_BUILD][0], c->acc[PC_BUILD][1],
                  c->acc[PC_BUILD][2],  c->acc[PC_LOSS][0],   c->acc[PC_LOSS][1],  c->evals,
                  c->acc[PC_FACTOR][0], c->acc[PC_FACTOR][1], c->acc[PC_FACTOR][2],
                  c->acc[PC_PRED][0],   c->acc[PC_PRED][1],   c->acc[PC_PRED][2],
                  c->acc[PC_PREDK][0],  c->acc[PC_PREDK][1],  c->acc[PC_PREDK][2],
                  c->acc[PC_PSURF][0],  c->acc[PC_PSURF][1],  c->acc[PC_PSURF][2]};
  // [24] shader clock (MHz) the factor kernels held while they ran (gpf::ClockSpan), [25] the
  // device's compute units, [26] the FP64 matrix ceiling at that clock (TFLOP/s, 128 flop per CU
  // per clock)
  unsigned long long clk[2] = {0, 0};
  if (c->d_clk) hipMemcpy(clk, c->d_clk, sizeof(clk), hipMemcpyDeviceToHost);
  const double mhz = clk[1] > 0 ? 100.0 * (double)clk[0] / (double)clk[1] : 0.0;
  const double w[27 - 24] = {mhz, (double)c->ncu, 128.0 * c->ncu * mhz * 1e6 / 1e12};
  const int m = std::min(n, 27);
  for (int i = 0; i < m; ++i) out[i] = i < 24 ? v[i] : w[i - 24];
  return m;
}

int gpf_selftest_mfma(gpf_ctx* c, const double* a, const double* b, double* out) {
  if (!c || !a || !b || !out) return GPF_BAD_ARG;
  hipSetDevice(c->device);
  double *da = nullptr, *db = nullptr, *dc = nullptr;
  GPF_HIP(c, hipMalloc(&da, 64 * 8));
  GPF_HIP(c, hipMalloc(&db, 64 * 8));
  GPF_HIP(c, hipMalloc(&dc, 256 * 8));
  GPF_HIP(c, hipMemcpy(da, a, 64 * 8, hipMemcpyHostToDevice));
  GPF_HIP(c, hipMemcpy(db, b, 64 * 8, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(gpf::k_selftest_mfma, dim3(1), dim3(64), 0, c->stream, da, db, dc);
  GPF_HIP(c, hipGetLastError());
  GPF_HIP(c, hipStreamSynchronize(c->stream));
  GPF_HIP(c, hipMemcpy(out, dc, 256 * 8, hipMemcpyDeviceToHost));
  hipFree(da); hipFree(db); hipFree(dc);
  return GPF_OK;
}

int gpf_debug_factor(gpf_ctx* c, const double* ls, double* L, double* U, double* z, double* alpha) {
  if (!c || !ls || !L || !U || !z || !alpha) return GPF_BAD_ARG;
  if (c->N <= 0) return bad_arg(c, "gpf_debug_factor: call gpf_set_data first");
  hipSetDevice(c->device);
  if (c->K <= 0) c->K = 2;
  double* al = nullptr;
  int rc = factor_single(c, ls, &al, Knobs::from_env());
  if (rc && rc != GPF_NOT_PD) return rc;
  const size_t np = (size_t)c->Npad;
  GPF_HIP(c, hipMemcpy(L, c->d_L, np * np * 8, hipMemcpyDeviceToHost));
  GPF_HIP(c, hipMemcpy(U, c->d_U, np * np * 8, hipMemcpyDeviceToHost));
  GPF_HIP(c, hipMemcpy(z, c->d_yb, np * 8, hipMemcpyDeviceToHost));
  if (al) GPF_HIP(c, hipMemcpy(alpha, al, (size_t)c->N * 8, hipMemcpyDeviceToHost));
  return rc;
}

// Shader clock (MHz) from a ClockSpan buffer: shader clocks over 100 MHz reference clocks.
static double read_clock(const unsigned long long* dclk) {
  unsigned long long h[2] = {0, 0};
  if (hipMemcpy(h, dclk, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess || h[1] == 0) return 0.0;
  return 100.0 * (double)h[0] / (double)h[1];
}

int gpf_bench_clock(gpf_ctx* c, double* mhz) {
  if (!c || !mhz) return GPF_BAD_ARG;
  *mhz = c->bench_sclk;
  return GPF_OK;
}

int gpf_mfma_peak(gpf_ctx* c, int blocks, int iters, double* tflops) {
  if (!c || !tflops || blocks <= 0 || iters <= 0) return GPF_BAD_ARG;
  hipSetDevice(c->device);
  double* out = nullptr;
  GPF_HIP(c, hipMalloc(&out, (size_t)blocks * 8));
  hipEvent_t a, b;
  GPF_HIP(c, hipEventCreate(&a));
  GPF_HIP(c, hipEventCreate(&b));
  unsigned long long* clk = nullptr;
  GPF_HIP(c, hipMalloc(&clk, 2 * sizeof(unsigned long long)));
  GPF_HIP(c, hipMemsetAsync(clk, 0, 2 * sizeof(unsigned long long), c->stream));
  hipLaunchKernelGGL(gpf::k_mfma_rate, dim3(blocks), dim3(NTHR), 0, c->stream, iters, 1.0, out, nullptr);  // warm-up
  GPF_HIP(c, hipEventRecord(a, c->stream));
  hipLaunchKernelGGL(gpf::k_mfma_rate, dim3(blocks), dim3(NTHR), 0, c->stream, iters, 1.0, out, clk);
  GPF_HIP(c, hipEventRecord(b, c->stream));
  GPF_HIP(c, hipEventSynchronize(b));
  c->bench_sclk = read_clock(clk);
  hipFree(clk);
  float ms = 0.f;
  GPF_HIP(c, hipEventElapsedTime(&ms, a, b));
  *tflops = (double)blocks * 4.0 * iters * 8.0 * 2048.0 / (ms * 1e-3) / 1e12;
  hipEventDestroy(a);
  hipEventDestroy(b);
  hipFree(out);
  return GPF_OK;
}

// gpf_prob_surface's kept row-chunk buffers
enum PsurfBuf {
  PSURF_T = 0,  // the tails as given and compacted, rows x E each
  PSURF_CMP,
  PSURF_INFO,   // one double4 per row (gpf::k_prob_prep)
  PSURF_Y,      // the surface, rows x PS_POINTS each
  PSURF_P,
  PSURF_OK,     // the row flags
  PSURF_NBUF
};

static SetPlan psurf_plan(int64_t rows, int Ea) {
  SetPlan p{};
  p.bytes[PSURF_T] = p.bytes[PSURF_CMP] = (size_t)rows * Ea * 8;
  p.bytes[PSURF_INFO] = (size_t)rows * sizeof(double4);
  p.bytes[PSURF_Y] = p.bytes[PSURF_P] = (size_t)rows * gpf::PS_POINTS * 8;
  p.bytes[PSURF_OK] = (size_t)rows * 4;
  return p;
}

// Probability surface (calc_prob_surf.py:15-30,67-81) of M rows of E tail entries each.
int gpf_prob_surface(gpf_ctx* c, const double* tails, int64_t M, int E, double* y, double* p, int* ok) {
  if (!c) return GPF_BAD_ARG;
  if (M < 0 || E < 0 || E > gpf::PS_EMAX || (M > 0 && (!tails || !y || !p || !ok)))
    return bad_arg(c, "gpf_prob_surface: bad arguments");
  if (M == 0) return GPF_OK;
  hipSetDevice(c->device);
  const int64_t chunk = std::min<int64_t>(M, 1 << 20);
  const int Ea = std::max(E, 1);
  // (no budget check: a chunk is at most 2^20 rows)
  KeptSet& ks = c->kept[KEPT_PSURF];
  const SetPlan need = psurf_plan(chunk, Ea);
  if (!ks.fits(need.bytes, PSURF_NBUF))
    if (int rg = ks.regrow(c, need.bytes, 0, PSURF_NBUF)) return rg;
  double *dt = ks.as(PSURF_T), *dcmp = ks.as(PSURF_CMP), *dy = ks.as(PSURF_Y), *dp = ks.as(PSURF_P);
  double4* dinfo = ks.as<double4>(PSURF_INFO);
  int* dok = ks.as<int>(PSURF_OK);
  int rc = GPF_OK;
  for (int64_t s = 0; s < M && rc == GPF_OK; s += chunk) {
    const int64_t m = std::min<int64_t>(chunk, M - s);
    if (hipMemcpyAsync(dt, tails + s * E, (size_t)m * E * 8, hipMemcpyHostToDevice, c->stream) != hipSuccess) {
      rc = GPF_HIP_ERROR;
      break;
    }
    // algorithmic bytes: the tails read, y and p written, the row flags
    const double bytes = (double)m * (E * 8.0 + 2.0 * gpf::PS_POINTS * 8.0 + 4.0);
    rc = launch(c, PC_PSURF, bytes, [&] {
      hipLaunchKernelGGL(gpf::k_prob_prep, dim3(blocks_for(m)), dim3(NTHR), 0, c->stream, dt, m, E, dcmp, dinfo);
      hipLaunchKernelGGL(gpf::k_prob_surf, dim3(blocks_for(m * gpf::PS_POINTS)), dim3(NTHR), 0, c->stream, dcmp, dinfo, m, E,
                         dy, dp, dok);
    });
    if (rc) break;
    if (hipMemcpyAsync(y + s * gpf::PS_POINTS, dy, (size_t)m * gpf::PS_POINTS * 8, hipMemcpyDeviceToHost, c->stream) !=
            hipSuccess ||
        hipMemcpyAsync(p + s * gpf::PS_POINTS, dp, (size_t)m * gpf::PS_POINTS * 8, hipMemcpyDeviceToHost, c->stream) !=
            hipSuccess ||
        hipMemcpyAsync(ok + s, dok, (size_t)m * 4, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess) {
      rc = GPF_HIP_ERROR;
      c->err = "gpf_prob_surface: copy failed";
    }
  }
  if (rc == GPF_HIP_ERROR && c->err.empty()) c->err = "gpf_prob_surface: HIP error";
  hipStreamSynchronize(c->stream);
  ks.trim(Knobs::from_env());
  return rc;
}

// ---- convex-hull grid fill (convex_hull.py:122-155,203-224; helpers above the C-ABI block) ----
int gpf_hull_fill(gpf_ctx* c, const double* shell, int64_t n, int d, const double* res, const int* decimals,
                  int64_t* m_out) {
  if (!c) return GPF_BAD_ARG;
  if (n <= 0 || d <= 0 || d > gpf::DMAX || !shell || !res || !decimals || !m_out)
    return bad_arg(c, "gpf_hull_fill: bad arguments");
  hipSetDevice(c->device);
  gpf::HullDims hd{};
  hd.d = d;
  for (int j = 0; j < d; ++j) {
    if (!(res[j] > 0.0)) return bad_arg(c, "gpf_hull_fill: resolution must be > 0");
    hd.res[j] = res[j];
    hd.p10[j] = (res[j] < 1.0 && decimals[j] >= 0) ? std::pow(10.0, decimals[j]) : 0.0;
  }
  hipStream_t st = c->stream;
  DevBuf rows;
  GPF_HIP(c, rows.alloc((size_t)n * d * 8, st));
  GPF_HIP(c, hipMemcpyAsync(rows.p, shell, (size_t)n * d * 8, hipMemcpyHostToDevice, st));
  std::vector<int> order(d);
  for (int j = 0; j < d; ++j) order[j] = j;
  int rc = hull_sort_unique(c, rows, n, d, order.data());
  if (rc) return rc;
  for (int i = 0; i < d; ++i) {
    // pass i: the grid is sorted by columns i, i+1, .., i-1 (mod d); fill along the last of them
    hd.axis = (d - 1 + i) % d;
    DevBuf cnt, off, temp, grown;
    GPF_HIP(c, cnt.alloc((size_t)n * 8, st));
    GPF_HIP(c, off.alloc((size_t)n * 8, st));
    hipLaunchKernelGGL(gpf::k_hull_count, dim3(blocks_for(n)), dim3(NTHR), 0, st, rows.as<double>(), n, hd,
                       cnt.as<int64_t>());
    size_t tb = 0;
    GPF_HIP(c, hipcub::DeviceScan::ExclusiveSum(nullptr, tb, cnt.as<int64_t>(), off.as<int64_t>(), n, st));
    GPF_HIP(c, temp.alloc(std::max<size_t>(tb, 16), st));
    GPF_HIP(c, hipcub::DeviceScan::ExclusiveSum(temp.p, tb, cnt.as<int64_t>(), off.as<int64_t>(), n, st));
    int64_t last[2] = {0, 0};
    GPF_HIP(c, hipMemcpyAsync(&last[0], off.as<int64_t>() + (n - 1), 8, hipMemcpyDeviceToHost, st));
    GPF_HIP(c, hipMemcpyAsync(&last[1], cnt.as<int64_t>() + (n - 1), 8, hipMemcpyDeviceToHost, st));
    GPF_HIP(c, hipStreamSynchronize(st));
    const int64_t add = last[0] + last[1];
    GPF_HIP(c, grown.alloc((size_t)(n + add) * d * 8, st));
    GPF_HIP(c, hipMemcpyAsync(grown.p, rows.p, (size_t)n * d * 8, hipMemcpyDeviceToDevice, st));
    hipLaunchKernelGGL(gpf::k_hull_emit, dim3(blocks_for(n)), dim3(NTHR), 0, st, rows.as<double>(), n, hd,
                       off.as<int64_t>(), grown.as<double>() + (size_t)n * d);
    GPF_HIP(c, hipGetLastError());
    std::swap(rows.p, grown.p);
    n += add;
    for (int j = 0; j < d; ++j) order[j] = (i + 1 + j) % d;
    rc = hull_sort_unique(c, rows, n, d, order.data());
    if (rc) return rc;
  }
  c->hull_rows.resize((size_t)n * d);
  GPF_HIP(c, hipMemcpy(c->hull_rows.data(), rows.p, (size_t)n * d * 8, hipMemcpyDeviceToHost));
  c->hull_d = d;
  *m_out = n;
  return GPF_OK;
}

int gpf_hull_fetch(gpf_ctx* c, double* out) {
  if (!c || !out) return GPF_BAD_ARG;
  if (!c->hull_rows.empty()) std::memcpy(out, c->hull_rows.data(), c->hull_rows.size() * 8);
  return GPF_OK;
}

// Measurement hook: TF/s of the k_step L-tile GEMM core alone (k_gemm_bench) on
// P random Npad x Npad matrices, tiles = workgroups per particle, depth D.
int gpf_gemm_bench(gpf_ctx* c, int mode, int Npad, int P, int tiles, int D, int iters, double* tflops) {
  if (!c || !tflops || Npad % T || D % T || P <= 0 || tiles <= 0 || iters <= 0) return GPF_BAD_ARG;
  if ((D / T + 1 + tiles) * T > Npad) return bad_arg(c, "gpf_gemm_bench: tiles do not fit");
  hipSetDevice(c->device);
  double *L = nullptr, *C = nullptr;
  const size_t n = (size_t)P * Npad * Npad;
  GPF_HIP(c, hipMalloc(&L, n * 8));
  GPF_HIP(c, hipMalloc(&C, (size_t)P * tiles * T * T * 8));
  // mode bit 8: zero operands (rounds 1-3); otherwise hashed values in [-1, 1) (gpf::k_fill_hash);
  // bit 16 / 32: the 3- / 4-stage LDS pipeline (gpf::DenseRun NS) instead of 2
  const auto kb = (mode & 32) ? gpf::k_gemm_bench<4> : (mode & 16) ? gpf::k_gemm_bench<3> : gpf::k_gemm_bench<2>;
  if (mode & 8)
    GPF_HIP(c, hipMemsetAsync(L, 0, n * 8, c->stream));
  else
    hipLaunchKernelGGL(gpf::k_fill_hash, dim3(4096), dim3(NTHR), 0, c->stream, L, (long long)n);
  hipEvent_t a, b;
  GPF_HIP(c, hipEventCreate(&a));
  GPF_HIP(c, hipEventCreate(&b));
  const int W = P * tiles;
  unsigned long long* clk = nullptr;
  GPF_HIP(c, hipMalloc(&clk, 2 * sizeof(unsigned long long)));
  GPF_HIP(c, hipMemsetAsync(clk, 0, 2 * sizeof(unsigned long long), c->stream));
  hipLaunchKernelGGL(kb, dim3(W), dim3(gpf::STEP_NTH), 0, c->stream, mode, D, Npad, P, L, C, nullptr);
  GPF_HIP(c, hipEventRecord(a, c->stream));
  for (int i = 0; i < iters; ++i)
    hipLaunchKernelGGL(kb, dim3(W), dim3(gpf::STEP_NTH), 0, c->stream, mode, D, Npad, P, L, C, clk);
  GPF_HIP(c, hipEventRecord(b, c->stream));
  GPF_HIP(c, hipEventSynchronize(b));
  c->bench_sclk = read_clock(clk);
  hipFree(clk);
  float ms = 0.f;
  GPF_HIP(c, hipEventElapsedTime(&ms, a, b));
  *tflops = 2.0 * T * T * (double)D * W * iters / (ms * 1e-3) / 1e12;
  hipEventDestroy(a);
  hipEventDestroy(b);
  hipFree(L);
  hipFree(C);
  return GPF_OK;
}

// Debug / measurement hook: the diagonal-block factor (gpf::factor128) on n 128x128 blocks.
int gpf_debug_factor128(gpf_ctx* c, const double* A, const double* y, int n, double* L, double* U, double* z, double* s2,
                        double* sz, int* bad, double* cycles) {
  if (!c || !A || !y || n <= 0 || !L || !U || !z || !s2 || !sz || !bad) return GPF_BAD_ARG;
  hipSetDevice(c->device);
  const size_t nb = (size_t)n * T * T, nv = (size_t)n * T;
  DevBuf dL, dU, dy, ds2, dsz, db, dc;
  GPF_HIP(c, dL.alloc(nb * 8, c->stream));
  GPF_HIP(c, dU.alloc(nb * 8, c->stream));
  GPF_HIP(c, dy.alloc(nv * 8, c->stream));
  GPF_HIP(c, ds2.alloc(nv * 8, c->stream));
  GPF_HIP(c, dsz.alloc(nv * 8, c->stream));
  GPF_HIP(c, db.alloc((size_t)n * 4, c->stream));
  GPF_HIP(c, dc.alloc((size_t)n * 8, c->stream));
  GPF_HIP(c, hipMemcpyAsync(dL.p, A, nb * 8, hipMemcpyHostToDevice, c->stream));
  GPF_HIP(c, hipMemsetAsync(dU.p, 0x7f, nb * 8, c->stream));  // (every entry must be written)
  GPF_HIP(c, hipMemcpyAsync(dy.p, y, nv * 8, hipMemcpyHostToDevice, c->stream));
  GPF_HIP(c, hipMemsetAsync(db.p, 0, (size_t)n * 4, c->stream));
  hipLaunchKernelGGL(gpf::k_debug_factor128, dim3(n), dim3(gpf::DNTH), 0, c->stream, dL.as<double>(), dU.as<double>(),
                     dy.as<double>(), ds2.as<double>(), dsz.as<double>(), db.as<int>(), dc.as<unsigned long long>());
  GPF_HIP(c, hipGetLastError());
  GPF_HIP(c, hipMemcpyAsync(L, dL.p, nb * 8, hipMemcpyDeviceToHost, c->stream));
  GPF_HIP(c, hipMemcpyAsync(U, dU.p, nb * 8, hipMemcpyDeviceToHost, c->stream));
  GPF_HIP(c, hipMemcpyAsync(z, dy.p, nv * 8, hipMemcpyDeviceToHost, c->stream));
  GPF_HIP(c, hipMemcpyAsync(s2, ds2.p, nv * 8, hipMemcpyDeviceToHost, c->stream));
  GPF_HIP(c, hipMemcpyAsync(sz, dsz.p, nv * 8, hipMemcpyDeviceToHost, c->stream));
  GPF_HIP(c, hipMemcpyAsync(bad, db.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
  std::vector<unsigned long long> cyc(n);
  GPF_HIP(c, hipMemcpyAsync(cyc.data(), dc.p, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
  GPF_HIP(c, hipStreamSynchronize(c->stream));
  if (cycles)
    for (int i = 0; i < n; ++i) cycles[i] = (double)cyc[i];
  return GPF_OK;
}

#ifdef GPF_WG_TRACE
// diagnostic builds only: per-workgroup (start, end, placement) of k_step, [J][wg][3]
int gpf_debug_wg_trace(unsigned long long* out, int nj, int nwg) {
  if (!out || nj <= 0 || nwg <= 0 || nj > gpf::WG_TRACE_J || nwg > gpf::WG_TRACE_N) return GPF_BAD_ARG;
  hipDeviceSynchronize();
  std::vector<unsigned long long> h((size_t)gpf::WG_TRACE_J * gpf::WG_TRACE_N * 3);
  if (hipMemcpyFromSymbol(h.data(), HIP_SYMBOL(gpf::g_wg_trace), h.size() * 8) != hipSuccess) return GPF_HIP_ERROR;
  for (int j = 0; j < nj; ++j)
    std::memcpy(out + (size_t)j * nwg * 3, h.data() + (size_t)j * gpf::WG_TRACE_N * 3, (size_t)nwg * 3 * 8);
  return GPF_OK;
}
// diagnostic builds only: wave-0 phase-end stamps of k_step workgroups, [J][wg][4] (see step_item)
int gpf_debug_wg_phase(unsigned long long* out, int nj, int nwg) {
  if (!out || nj <= 0 || nwg <= 0 || nj > gpf::WG_TRACE_J || nwg > gpf::WG_TRACE_N) return GPF_BAD_ARG;
  hipDeviceSynchronize();
  std::vector<unsigned long long> h((size_t)gpf::WG_TRACE_J * gpf::WG_TRACE_N * 4);
  if (hipMemcpyFromSymbol(h.data(), HIP_SYMBOL(gpf::g_wg_phase), h.size() * 8) != hipSuccess) return GPF_HIP_ERROR;
  for (int j = 0; j < nj; ++j)
    std::memcpy(out + (size_t)j * nwg * 4, h.data() + (size_t)j * gpf::WG_TRACE_N * 4, (size_t)nwg * 4 * 8);
  return GPF_OK;
}
#endif


}  // extern "C"

// swarm exchange across ranks (after the C-ABI above: it calls gpf_eval_batch)
#include "gpf_comm.hip"
