// gpf_plan.hip — host-only planning of one factorisation (included by gpfit_api.hip behind the kernel
// sources): the tuning environment as one snapshot per API call (Knobs), the schedule policies as pure
// functions of (particles, block columns, Knobs), the planner (plan_factor -> FactorPlan: everything
// run_factor launches and allocates) and its structural check on the host (plan_check, persist_check).
#pragma once

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

namespace {

using gpf::T;

constexpr int MAX_GROUPS = 4;  // particle groups factorised on concurrent streams

// One GPF_* variable as read at the top of an API call: set or not, and its value both ways (the
// defaults stay with the policies below, next to the measurements behind them).
struct Knob {
  bool set = false;
  long long i = 0;
  double f = 0.0;
  int num(int dflt) const { return set ? (int)i : dflt; }
  bool flag(bool dflt) const { return set ? i != 0 : dflt; }
};

// Every tuning variable the host reads, read once per C-ABI call (never cached on the context: a
// caller may change the environment between calls) and passed down by const reference, so that every
// policy of one factorisation sees the same values.
struct Knobs {
  Knob persist, groups, step_group, split_k, split_k_slots, split_k_minch, early_diag, defer_syrk, lookahead, reorder,
      pair, pair_sync, la_all, la_all_pb, la_all_from, la_all_first, wait_spins, step_1percu, la_delay_test,
      no_graph, mem_fraction, max_chunk, predict_keep_mb, predbatch_order, predbatch_ks;
  static Knobs from_env() {
    auto rd = [](const char* name) {
      Knob k;
      if (const char* s = getenv(name)) k = {true, atoll(s), atof(s)};
      return k;
    };
    Knobs k;
    k.persist = rd("GPF_PERSIST");
    k.groups = rd("GPF_GROUPS");
    k.step_group = rd("GPF_STEP_GROUP");
    k.split_k = rd("GPF_SPLIT_K");
    k.split_k_slots = rd("GPF_SPLIT_K_SLOTS");
    k.split_k_minch = rd("GPF_SPLIT_K_MINCH");
    k.early_diag = rd("GPF_EARLY_DIAG");
    k.defer_syrk = rd("GPF_DEFER_SYRK");
    k.lookahead = rd("GPF_LOOKAHEAD");
    k.reorder = rd("GPF_REORDER");
    k.pair = rd("GPF_PAIR");
    k.pair_sync = rd("GPF_PAIR_SYNC");
    k.la_all = rd("GPF_LA_ALL");
    k.la_all_pb = rd("GPF_LA_ALL_PB");
    k.la_all_from = rd("GPF_LA_ALL_FROM");
    k.la_all_first = rd("GPF_LA_ALL_FIRST");
    k.wait_spins = rd("GPF_WAIT_SPINS");
    k.step_1percu = rd("GPF_STEP_1PERCU");
    k.la_delay_test = rd("GPF_LA_DELAY_TEST");
    k.no_graph = rd("GPF_NO_GRAPH");
    k.mem_fraction = rd("GPF_MEM_FRACTION");
    k.max_chunk = rd("GPF_MAX_CHUNK");
    k.predict_keep_mb = rd("GPF_PREDICT_KEEP_MB");
    k.predbatch_order = rd("GPF_PREDBATCH_ORDER");
    k.predbatch_ks = rd("GPF_PREDBATCH_KS");
    return k;
  }
};

// Particle groups factorised on concurrent streams (GPF_GROUPS overrides): they fill the tail
// of each dependent block-column launch with another group's tiles. Measured on MI355X
// (profiles/r1/groups_ab.txt, profiles/r2/groups_stagger_ab.txt): 2 groups +4.6% at N=4096 P=32
// (config D's share of one GPU), +1.7% at N=4096 P=64 (config C, round 2: 1303 -> 1324
// evals/s, same box), -19% at N=1024 P=32, 4 groups worse everywhere. Default: 2 groups for
// chunks with at least 16 block columns, else 1. (With concurrent groups the per-launch times
// overlap, so bench.py rates the whole factorisation phase instead: no gaps or overlap counted.)
// Persistent factorisation (gpf::k_factor, gpf_persist.hip) for slot-bound schedules with many
// block columns: more tiles per block column than the 512 workgroup slots and nt >= 64 (config
// E's per-GPU share: 22.2-22.3 vs 22.0 evals/s, 0.945 vs 0.937 of the FP64 ceiling at the clock
// the chip held). At nt = 32 (configs C, D) the per-block-column launches on two group streams
// stay faster: 1344-1368 vs 1310-1331 evals/s — per clock the two are within 0.5%, but the chip
// holds ~40 MHz less under the persistent launch (profiles/r4/ab_persist_clock.txt,
// ab_r4g_summary.txt). B-like launches (fewer tiles than slots) lose 24% (no early diagonal
// factor in it). GPF_PERSIST = 0/1 overrides.
bool persist_on(int pc, int nt, const Knobs& k) {
  const bool on = k.persist.flag((long long)pc * (nt - 1) > 512 && nt >= 64);
  return on && nt >= 3 && pc >= 2;  // (a single particle — the prediction — keeps its split launches)
}

int num_groups(int pc, int nt, const Knobs& k) {
  if (persist_on(pc, nt, k)) return 1;  // one launch over every particle
  int g = std::max(1, std::min(k.groups.num(nt >= 16 ? 2 : 1), MAX_GROUPS));
  while (g > 1 && pc / g < 8) --g;  // keep >= 8 particles (one per XCD) per group
  return g;
}

// Particles per XCD dispatch group of k_step (see gpf::step_tile); GPF_STEP_GROUP
// overrides, 0 = particle fastest over the whole launch.
int step_group(int pc, const Knobs& k) { return std::max(0, std::min(k.step_group.num(0), pc / 8)); }

// Split-K factor of the block-column launches: launches with at most 64 tiles (a single
// particle: the prediction path) cut every tile's GEMM into S depth ranges (gpf::flat_piece), S
// filling ~512 workgroup slots. Measured (profiles/r1/split_k_ab.txt): single-particle factor at
// N=4096 11.3 -> 9.9 ms with S=16 (7.4 ms since the partials are stored write-through, with no
// release fence); config B (224 tiles, S=2) 21.3k -> 14.3k evals/s with the fence, hence the
// threshold. At most 8 pieces since round 2 (with the split-K reduction tree and the early
// diagonal factor): an L tile's depth is 8J 16-deep chunks, so 8 pieces are always even while
// 16 leave odd-J tiles uneven and J = 1 tiles with empty pieces — single-particle factor at
// N=4096 4.17 -> 3.90 ms, N=2048 equal, N=8192 already 8 (512/63), S=16 there 16.4 vs 13.5 ms
// (profiles/r2/predict_splitk_ab.txt). GPF_SPLIT_K overrides (1 = off). Not for tiny problems (nt < 4).
int split_k(int tiles, int nt, const Knobs& k) {
  int S = (nt >= 4 && tiles <= 64) ? std::max(1, std::min(8, 512 / std::max(1, tiles))) : 1;
  if (k.split_k.set) S = std::max(1, std::min(32, k.split_k.num(0)));
  return nt < 4 ? 1 : S;
}

// Chunk target of launch J under the all-tile split (gpf::split_all_pieces): the launch's GEMM
// depth (pc particles, every tile) spread over `slots` workgroups of about equal work, one per CU
// (a slot per particle is kept for the diagonal workgroups — also without the early diagonal
// factor, so that both schedules sum the same pieces and stay bitwise equal: a piece that shares
// the diagonal factor's CU slows its dependent chain; two pieces per CU run at half rate each),
// with pieces of at least
// GPF_SPLIT_K_MINCH (4) 16-deep chunks. A fixed S pieces per tile (rounds 1-2) gave every tile
// the same piece count, so the deepest tiles — the critical tile I = J+1 among them — had the
// longest pieces and, from J ~ 10 on, ended the launch after the diagonal factor.
// GPF_SPLIT_K_SLOTS overrides the workgroup budget (256).
int split_all_target(int pc, int nt, int J, const Knobs& k) {
  const int slots = std::max(1, k.split_k_slots.num(256)), minch = std::max(1, k.split_k_minch.num(4));
  const int budget = std::max(1, slots - pc);
  long long tot = 0;
  for (int w = 0; w < nt - 1; ++w) tot += gpf::split_all_chunks(J, w, nt);
  const int cap = std::max(1, J * T / gpf::DL_KC);  // every tile in one piece from here on
  auto wgs = [&](int tgt) {
    long long n = 0;
    for (int w = 0; w < nt - 1; ++w) n += gpf::split_all_pieces(J, w, nt, tgt);
    return pc * n;
  };
  // smallest target >= the even share whose pieces fit the budget (the count falls with tgt)
  int lo = (int)std::min<long long>(cap, std::max<long long>(minch, (pc * tot + budget - 1) / budget)), hi = cap;
  while (lo < hi) {
    const int mid = (lo + hi) / 2;
    if (wgs(mid) <= budget) hi = mid;
    else lo = mid + 1;
  }
  return std::min(lo, cap);
}

// Early diagonal factor (gpf::k_step<SPLIT, 1>, gpf_factor.hip) for factorisations whose launches
// leave workgroup slots idle: there the launch time is the critical tile's chain, and moving the
// diagonal factor of block J to the start of launch J, beside the GEMMs, takes it off that chain
// (same-box A/B, gpurun_out r2i: config B, N=1024 P=32, 23.1k -> 29.2k evals/s; N=2048 P=32
// +5%; the single-particle prediction factor 7.1 -> 6.0 ms). Launches with more tiles than
// slots are bound by the slot load instead, and their tiles would wait for the flag in the first
// block columns (config C -0.7%, config D's 32-particle share -0.3%, E neutral), so they keep the
// fused factor. pc: the particles of all concurrent groups. GPF_EARLY_DIAG = 0/1 overrides.
// The all-tile split always runs it (its flat finish, gpf::flat_piece, waits for the diagonal block
// inside the launch): GPF_EARLY_DIAG=0 does not apply there.
bool split_all_on(int pc, int nt, const Knobs& k) {
  const int ng = num_groups(pc, nt, k);
  return split_k(((pc + ng - 1) / ng) * (nt - 1), nt, k) > 1;
}
bool early_diag(int pc, int nt, const Knobs& k) {
  return (k.early_diag.flag((long long)pc * (nt - 1) <= 512) || split_all_on(pc, nt, k)) && nt > 1;
}

// Deferred diagonal update (gpf::syrk_item; see gpf::step_decode) for every factorisation without
// the all-tile split. GPF_DEFER_SYRK = 0 restores the per-tile look-ahead (A/B knob).
bool defer_syrk(const Knobs& k) { return k.defer_syrk.flag(true); }

// Look-ahead of the critical tile (gpf::la_item) for launches with the early diagonal factor and
// no split: launch J (1 <= J <= nt-3) also runs the first ~7/16 of the next critical tile's GEMM
// (on its SYRK workgroups), and launch J+1's critical tile continues from there. There the
// launch's chain was that tile's depth-128J GEMM once it outgrew the diagonal factor (config B
// from J = 4): same box, B 33.8k -> 36.1k evals/s, launch spans 743 -> 687 us
// (profiles/r3s2/ab_lookahead_B.txt).
// Slot-bound launches (config C, the fused factor) gain nothing from moving work between launches.
// GPF_LOOKAHEAD = 0/1 overrides.
bool look_ahead(int pc, int nt, const Knobs& k) { return k.lookahead.flag(early_diag(pc, nt, k)) && nt >= 4; }

// Reordered dispatch of early-diagonal launches with SYRK workgroups (gpf::step_decode ro): the
// diagonal factors get their CUs alone. GPF_REORDER = 0/1 overrides.
bool reorder_on(const Knobs& k) { return k.reorder.flag(true); }

// Paired block columns (gpf::pair_decode; lead launch J streams each tile's panel once for block
// columns J and J+1, the follow launch J+1 finishes from the partials) for the fused-diagonal
// schedule without split: slot-bound launches (configs C, D) whose particle groups are multiples of 8
// (one particle per XCD in every group of 8, so a tile and its partner share an XCD) and nt >= 4.
// GPF_PAIR = 0/1 overrides; GPF_PAIR_SYNC = 0 drops the partners' start synchronisation
// (gpf::pair_start_sync).
bool pair_on(const Knobs& k) { return k.pair.flag(false); }

// All-tile look-ahead in pieces (gpf::lall_decode) for the early-diagonal launches without split
// (config B: fewer tiles than workgroup slots, launches bound by their deepest tile), from launch
// GPF_LA_ALL_FROM on (default nt-2: the last launch, whose deepest U tile is the factorisation's
// longest item, consumes them: config B 41.5-41.7k -> 42.4k evals/s; from launch 1 on, or nt-3, the
// producing launches grow by more than the consumers shrink: 35-39k; profiles/r6/
// ab_B_lookahead_pieces.txt). GPF_LA_ALL = 0/1 overrides. In the launches it covers it replaces the
// critical-tile look-ahead (GPF_LOOKAHEAD) and the reordered dispatch.
bool lall_on(const Knobs& k) { return k.la_all.flag(true); }
// piece size in 128-blocks (GPF_LA_ALL_PB, 1..4) and the pieces ahead of the tiles (GPF_LA_ALL_FIRST)
int lall_pb(const Knobs& k) { return std::max(1, std::min(4, k.la_all_pb.num(1))); }
bool lall_first(const Knobs& k) { return k.la_all_first.flag(true); }
// the first launch that produces pieces (GPF_LA_ALL_FROM; default nt-2: only the last launch, whose
// deepest U tile is the longest item of the factorisation, consumes them; negative: counted from nt)
int lall_from(int nt, const Knobs& k) {
  const int j = k.la_all_from.num(-2);
  return std::max(1, j < 0 ? nt + j : j);
}
// (the pieces per particle and launch grow as nt J / 2: the look-ahead is for short factorisations;
// gpf::lall_tag carries the group's particle count in 12 bits)
constexpr int LALL_NT_MAX = 32, LALL_GC_MAX = 0xfff;
int lall_smax(int nt, int pb) {
  int m = 1;
  for (int J = 0; J < nt; ++J) m = std::max(m, gpf::lall_total(J, nt, pb));
  return m;
}

// Bound of the early-diagonal hand-off spin (gpf::wait_diag, polls of ~1 us): ~2 s by default;
// GPF_WAIT_SPINS lowers it to exercise the timeout report (tests/test_gpu.py).
int wait_spins(const Knobs& k) { return k.wait_spins.set ? std::max(0, k.wait_spins.num(0)) : 1 << 21; }

// One k_step launch of a factorisation: block column J of particle group g (particles
// [p0, p0+gc) of the chunk, on that group's stream), its kernel variant, grid, pieces per split
// tile, and where its split-K partial slots and arrival counters start (element offsets into
// the split buffers). run_factor launches exactly this list; plan_check verifies it on the host.
struct StepLaunch {
  int J, g, p0, gc, split, S, S2, grp, ed;  // S: pieces per split tile (SPLIT_ALL: chunks per piece); S2: partial
                                            // slots per tile; ed: the launch starts with gc diagonal workgroups
  int defer, sy;                        // deferred diagonal update; sy: gc SYRK workgroups follow
  int ro;  // reordered dispatch (gpf::step_decode ro): light U tiles, diagonal, other tiles, SYRK workgroups
  int la;  // look-ahead: bit 0: gc LA workgroups follow (gpf::la_item); bit 1: the critical tiles seed from launch J-1's
  int pair;  // paired block columns: 1 lead launch (gpf::pair_decode), 2 follow launch (its tiles seed from the lead's partials)
  int lall;  // look-ahead pieces: bit 0 produces for J+1, bit 1 consumes launch J-1's, bit 2 pieces ahead of the tiles
  int tag;   // early-diagonal launches: gpf::lall_tag of the group (the fused ones tag per factorisation, step_tag)
  unsigned grid, lds;  // lds: dynamic LDS (GPF_STEP_1PERCU)
  size_t part_off, cnt_off;
};

// Everything decided about one factorisation of pc particles over nt block columns: run_factor
// grows the scratch buffers to the sizes given here (bytes; 0: not used) ahead of the fork and then
// walks `steps`; plan_check verifies this same object.
struct FactorPlan {
  bool persist = false, ed = false, psync = true;
  int ng = 1, S = 1, Smax = 1;  // S > 1: the all-tile split; Smax: partial slots per tile
  int lall_pb = 1, lall_smax = 1, lall_from = 1;
  int spins = 0, la_delay = 0;  // la_delay: test hook, the seeded critical tiles wait ~0.3 ms first (gpf::step_item)
  std::vector<StepLaunch> steps;
  size_t part_bytes = 0, cnt_bytes = 0, la_bytes = 0, pb_bytes = 0, pstart_bytes = 0, lb_bytes = 0;
};

// The integers k_step takes as `la`, `pair` and `ptag` (seq: the factorisation's number, which makes the
// paired columns' start words unique per factorisation and launch).
int step_la_arg(const StepLaunch& l, const FactorPlan& f) { return l.la | ((l.la & 2) ? f.la_delay : 0) | (l.ro ? 32 : 0); }
int step_pair_arg(const StepLaunch& l) { return l.ed ? l.lall : l.pair; }
int step_tag(const StepLaunch& l, int seq) { return l.ed ? l.tag : (seq << 8) | l.J; }

FactorPlan plan_factor(int pc, int nt, const Knobs& k) {
  FactorPlan f;
  f.persist = persist_on(pc, nt, k);
  f.ng = num_groups(pc, nt, k);
  f.spins = wait_spins(k);
  if (f.persist) return f;  // one launch over every particle and block column (gpf_persist.hip)
  const int ng = f.ng;
  f.ed = early_diag(pc, nt, k);
  f.psync = k.pair_sync.flag(true);
  f.la_delay = k.la_delay_test.flag(false) ? 4 : 0;
  f.lall_pb = lall_pb(k);
  f.lall_smax = lall_smax(nt, f.lall_pb);
  f.lall_from = lall_from(nt, k);
  auto group_p0 = [&](int g) { return (int)((long long)pc * g / ng); };
  // Split-K: S (all tiles) and the largest factor any launch uses; the partial buffers are sized for
  // it. split_k never splits below nt = 4, so a graph-captured batch (nt <= 2) needs no scratch.
  const int S = f.S = split_k(((pc + ng - 1) / ng) * (nt - 1), nt, k);
  if (S > 1) {  // the all-tile split: slots for the most pieces any tile gets
    for (int g = 0; g < ng; ++g)  // (the target depends on the group's particle count)
      for (int J = 1; J < nt; ++J) {
        const int tgt = split_all_target(group_p0(g + 1) - group_p0(g), nt, J, k);
        for (int w = 0; w < nt - 1; ++w) f.Smax = std::max(f.Smax, gpf::split_all_pieces(J, w, nt, tgt));
      }
    f.Smax = std::max(f.Smax, 2);
  }
  const int Smax = f.Smax;
  const bool la_on = look_ahead(pc, nt, k), defer = S == 1 && defer_syrk(k);  // the all-tile split keeps the per-tile look-ahead
  bool any_la = false, any_pair = false, any_lall = false;
  // block columns interleaved across groups so every stream has work queued early
  for (int J = 0; nt > 1 && J < nt; ++J) {
    for (int g = 0; g < ng; ++g) {
      StepLaunch l{};
      l.J = J;
      l.g = g;
      l.p0 = group_p0(g);
      l.gc = group_p0(g + 1) - l.p0;
      l.grp = step_group(l.gc, k);
      l.S = S > 1 ? split_all_target(l.gc, nt, J, k) : 1;
      l.S2 = S > 1 ? Smax : 1;
      l.split = S > 1 ? gpf::SPLIT_ALL : gpf::SPLIT_NONE;
      l.ed = f.ed ? 1 : 0;
      l.defer = defer ? 1 : 0;
      l.sy = (l.defer && J >= 1 && J <= nt - 2) ? 1 : 0;
      // look-ahead: launch J-1 of this group must have run unsplit too (its LA workgroups)
      const bool la_ok = la_on && l.ed && S == 1;
      l.la = ((la_ok && J >= 1 && J <= nt - 3) ? 1 : 0) | ((la_ok && J >= 2 && J <= nt - 2) ? 2 : 0);
      // reordered dispatch: only where the first 3 gc workgroups (the light U tiles, which wait for
      // the diagonal workgroups behind them, and the SYRK workgroups) fit the chip's CUs at once
      // and one group (a concurrent group's launch could hold the slots the waiters need)
      l.ro = (reorder_on(k) && ng == 1 && l.ed && l.sy && S == 1 && l.grp == 0 && J >= 1 && 3 * l.gc <= 256) ? 1 : 0;
      // paired block columns: leads at odd J with a block column behind them, each followed by J+1
      const bool pairs = pair_on(k) && !l.ed && l.defer && l.grp == 0 && l.gc % 8 == 0 && nt >= 4;
      l.pair = pairs && (J & 1) && J + 1 <= nt - 1 ? 1 : (pairs && J >= 2 && !(J & 1) ? 2 : 0);
      if (l.pair == 2) l.sy = 0;  // (the lead's partial SYRK and the critical tile reduce the diagonal block)
      int nall = 0;
      for (int w = 0; S > 1 && w < nt - 1; ++w) nall += gpf::split_all_pieces(J, w, nt, l.S);
      l.grid = (S > 1 ? l.gc * nall : l.gc * (nt - 1)) + (l.ed ? l.gc : 0) + (l.sy ? l.gc : 0) +
               ((l.la & 1) && !l.sy ? l.gc : 0);  // (with SYRK workgroups the look-ahead rides on them)
      if (l.pair == 1) l.grid = (unsigned)(l.gc * gpf::pair_grid_per_particle(J, nt));
      // look-ahead pieces (early-diagonal launches), for groups whose particle count fits the tag
      if (lall_on(k) && l.ed && l.defer && nt >= 4 && nt <= LALL_NT_MAX && J >= f.lall_from && l.gc <= LALL_GC_MAX) {
        // launches J >= from produce pieces for J+1, launches J > from consume them (and run no
        // critical-tile look-ahead: the pieces carry the next critical tile too); launch `from` may still
        // seed its critical tile from the launch before it
        l.lall = (gpf::lall_items(J, nt) > 0 ? 1 : 0) | (J >= 2 && J > f.lall_from ? 2 : 0);
        if ((l.lall & 1) && lall_first(k)) l.lall |= 4;
        l.la = J > f.lall_from ? 0 : (l.la & 2);
        l.ro = 0;
        l.grid = (unsigned)(l.gc * (nt - 1) + l.gc + (l.sy ? l.gc : 0) + l.gc * gpf::lall_total(J, nt, f.lall_pb));
      }
      if (l.ed) l.tag = gpf::lall_tag(l.gc, f.lall_pb, f.lall_smax);
      // Dynamic LDS that keeps a k_step launch at one workgroup per CU (its static LDS plus this exceeds
      // half of the CU's 160 KiB): GPF_STEP_1PERCU = 1 for every unsplit early-diagonal launch (A/B knob).
      if (k.step_1percu.flag(false) && l.ed && S == 1) l.lds = (unsigned)(82 * 1024 - gpf::STEP_LDS * 8);
      // one set of partial slots per group: groups run concurrently
      l.part_off = (size_t)l.p0 * (nt - 1) * Smax * T * T;
      l.cnt_off = (size_t)l.p0 * (nt - 1) * gpf::split_cnt_stride(nt);
      any_la = any_la || l.la != 0;
      any_pair = any_pair || l.pair != 0;
      any_lall = any_lall || l.lall != 0;
      f.steps.push_back(l);
    }
  }
  const size_t tiles = (size_t)pc * (nt - 1);
  if (Smax > 1) {
    f.part_bytes = tiles * Smax * T * T * 8;
    f.cnt_bytes = tiles * gpf::split_cnt_stride(nt) * 4;  // arrival counters, one set per (particle, tile)
  }
  if (any_la) f.la_bytes = 2 * (size_t)pc * T * T * 8;  // two slots per particle (gpf::la_slot)
  if (any_pair) {
    f.pb_bytes = tiles * T * T * 8;                  // the lead launch's partials (gpf::pair_slot)
    f.pstart_bytes = tiles * gpf::PAIR_HMAX * 4;     // the partners' start words (gpf::pair_start_sync)
  }
  if (any_lall) f.lb_bytes = (size_t)2 * pc * f.lall_smax * T * T * 8;  // two parities (gpf::lall_slot)
  return f;
}

int plan_fail(char* msg, int len, const char* fmt, ...) {
  if (msg && len > 0) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(msg, (size_t)len, fmt, ap);
    va_end(ap);
  }
  return GPF_BAD_ARG;
}

// Host-only structural check of the k_step dispatch plan (no device, no context): see gpfit.h.
// The persistent factorisation's queues (gpf::p_decode, as k_factor decodes its tickets): every
// (block column, particle, tile) exactly once, one SYRK item per particle for 1 <= J <= nt-2, every
// particle in one queue, and each item's inputs (the counters it waits for) produced by items
// earlier in that queue — the deadlock-freedom argument of gpf_persist.hip.
int persist_check(int pc, int nt, long long* stats, char* msg, int msg_len) {
  const int nq = gpf::p_nq(pc);
  // done[p][...]: the ticket position at which each counter value first becomes available
  std::vector<long long> seen((size_t)pc * nt * nt, 0), syrk((size_t)pc * nt, 0);
  std::vector<int> lcol((size_t)pc * nt, 0), ucol((size_t)pc * nt, 0), sdone((size_t)pc * nt, 0);
  for (int p = 0; p < pc; ++p) ucol[(size_t)p * nt] = 1;  // k_diag before the launch
  long long items = 0, tiles = 0, syrks = 0;
  for (int q = 0; q < nq; ++q) {
    const long long n = gpf::p_queue_items(pc, nt, q);
    int Jc = 0;
    long long bc = 0;
    for (long long t = 0; t < n; ++t) {
      int p = -1, w = -2;
      const int kind = gpf::p_decode(t, pc, nt, q, Jc, bc, p, w);
      const int J = Jc;
      if (p < 0 || p >= pc || p % nq != q || J < 0 || J >= nt)
        return plan_fail(msg, msg_len, "persistent queue %d ticket %lld decodes out of range (J=%d p=%d)", q, t, J, p);
      int* lc = &lcol[(size_t)p * nt];
      int* uc = &ucol[(size_t)p * nt];
      int* sd = &sdone[(size_t)p * nt];
      // items run in ticket order here: a wait that is not yet satisfied would wait for a later item
      if (kind == gpf::PK_SYRK) {
        if (!gpf::p_sy(J, nt) || syrk[(size_t)p * nt + J]++)
          return plan_fail(msg, msg_len, "persistent: misplaced or duplicate SYRK item J=%d p=%d", J, p);
        if (lc[J + 1] < J) return plan_fail(msg, msg_len, "persistent: SYRK J=%d p=%d before its row", J, p);
        sd[J + 1] = 1;
        ++syrks;
      } else {
        if (w < 0 || w >= nt - 1) return plan_fail(msg, msg_len, "persistent: tile %d out of range (J=%d)", w, J);
        long long& cnt = seen[((size_t)p * nt + J) * nt + w];
        if (cnt++) return plan_fail(msg, msg_len, "persistent: tile J=%d p=%d w=%d twice", J, p, w);
        if (kind == gpf::PK_LTILE) {
          const int I = J + 1 + w;
          if ((J > 0 && (lc[I] < J || lc[J] < J)) || uc[J] < J + 1 || (I == J + 1 && J > 0 && !sd[I]))
            return plan_fail(msg, msg_len, "persistent: L tile (%d, %d) of p=%d ahead of its inputs", J, I, p);
          if (lc[I] != J) return plan_fail(msg, msg_len, "persistent: row %d of p=%d out of order", I, p);
          lc[I] = J + 1;
          if (I == J + 1) uc[I] = I + 1;  // the critical tile factors block I
        } else {
          const int K = w - (nt - 1 - J);
          if (K < 0 || K >= J || lc[J] < J || uc[K] < J || uc[J] < J + 1)
            return plan_fail(msg, msg_len, "persistent: U tile (%d, %d) of p=%d ahead of its inputs", J, K, p);
          if (uc[K] != J) return plan_fail(msg, msg_len, "persistent: U column %d of p=%d out of order", K, p);
          uc[K] = J + 1;
        }
        ++tiles;
      }
      ++items;
    }
  }
  for (int p = 0; p < pc; ++p)
    for (int J = 0; J < nt; ++J) {
      if (syrk[(size_t)p * nt + J] != gpf::p_sy(J, nt))
        return plan_fail(msg, msg_len, "persistent: particle %d column %d has %lld SYRK items", p, J, syrk[(size_t)p * nt + J]);
      for (int w = 0; w < nt - 1; ++w)
        if (seen[((size_t)p * nt + J) * nt + w] != 1)
          return plan_fail(msg, msg_len, "persistent: tile J=%d p=%d w=%d run %lld times", J, p, w,
                           seen[((size_t)p * nt + J) * nt + w]);
    }
  if (stats) {
    const long long st[11] = {1, items, tiles, 0, 1, 1, 1, 0, syrks, 1, 0};
    std::copy(st, st + 11, stats);
  }
  return GPF_OK;
}

// The check behind gpf_plan_check: the plan run_factor would walk under these knobs.
int plan_check(int pc, int nt, const Knobs& knobs, long long* stats, char* msg, int msg_len) {
  if (msg && msg_len > 0) msg[0] = 0;
  if (pc <= 0 || nt <= 0) return plan_fail(msg, msg_len, "bad arguments pc=%d nt=%d", pc, nt);
  const FactorPlan fp = plan_factor(pc, nt, knobs);
  if (fp.persist) return persist_check(pc, nt, stats, msg, msg_len);
  const std::vector<StepLaunch>& plan = fp.steps;
  const int ntl = nt - 1, ng = fp.ng, Smax = fp.Smax, lsmax = fp.lall_smax, lpb = fp.lall_pb;
  const size_t part_cap = fp.part_bytes / 8, cnt_cap = fp.cnt_bytes / 4, cstride = (size_t)gpf::split_cnt_stride(nt);
  // partial-slot and counter ranges each group touches: groups run concurrently, so they must
  // be disjoint (within a group the launches are ordered on its stream)
  std::vector<size_t> plo(MAX_GROUPS, SIZE_MAX), phi(MAX_GROUPS, 0), clo(MAX_GROUPS, SIZE_MAX), chi(MAX_GROUPS, 0);
  long long wgs = 0, whole_tiles = 0, split_tiles = 0, pairs = 0;
  std::vector<int> whole, piece, diag, syrk;
  long long diag_wgs = 0, syrk_wgs = 0;
  std::vector<int> la_prev(MAX_GROUPS, 0), pair_prev(MAX_GROUPS, 0), pairJ(MAX_GROUPS, -1), lall_prev(MAX_GROUPS, 0);
  if ((int)plan.size() != (nt > 1 ? nt * ng : 0)) return plan_fail(msg, msg_len, "plan has %d launches, want %d",
                                                              (int)plan.size(), nt * ng);
  for (const StepLaunch& l : plan) {
    if (l.gc <= 0 || l.p0 < 0 || l.p0 + l.gc > pc || l.g < 0 || l.g >= ng)
      return plan_fail(msg, msg_len, "J=%d: bad group range p0=%d gc=%d g=%d", l.J, l.p0, l.gc, l.g);
    if (l.ed != (fp.ed ? 1 : 0) || (l.pair && l.lall))
      return plan_fail(msg, msg_len, "J=%d g=%d: launch kind ed=%d pair=%d pieces=%d", l.J, l.g, l.ed, l.pair, l.lall);
    if (l.S < 1 || (l.split == gpf::SPLIT_NONE && (l.S != 1 || l.S2 != 1)) || (l.split == gpf::SPLIT_ALL && l.S2 != Smax))
      return plan_fail(msg, msg_len, "J=%d g=%d: split kind %d with S=%d S2=%d", l.J, l.g, l.split, l.S, l.S2);
    if (l.split != gpf::SPLIT_NONE && Smax < 2)
      return plan_fail(msg, msg_len, "J=%d g=%d: split launch without split-K buffers (Smax=%d)", l.J, l.g, Smax);
    // the look-ahead partial a seeded launch reads (slot of J-1) is never the one it writes (slot of J)
    if ((l.la & 2) && (l.la & 1) && gpf::la_slot(0, l.J - 1) == gpf::la_slot(0, l.J))
      return plan_fail(msg, msg_len, "J=%d g=%d: look-ahead reads and writes the same slot", l.J, l.g);
    if (l.la && fp.la_bytes < 2 * (size_t)(l.p0 + l.gc) * T * T * 8)
      return plan_fail(msg, msg_len, "J=%d g=%d: look-ahead slots outside the buffer", l.J, l.g);
    const int tiles = l.gc * ntl;
    auto pieces_of = [&](int w) { return l.split == gpf::SPLIT_ALL ? gpf::split_all_pieces(l.J, w, nt, l.S) : l.S; };
    for (int w = 0; w < ntl; ++w)
      if (pieces_of(w) > l.S2) return plan_fail(msg, msg_len, "J=%d tile %d: %d pieces but %d slots", l.J, w, pieces_of(w), l.S2);
    whole.assign((size_t)tiles, 0);
    piece.assign((size_t)tiles * l.S2, 0);
    diag.assign((size_t)l.gc, 0);
    syrk.assign((size_t)l.gc, 0);
    if (l.sy && (!l.defer || l.J < 1 || l.J > nt - 2 || l.split == gpf::SPLIT_ALL))
      return plan_fail(msg, msg_len, "J=%d: SYRK workgroups without a diagonal block to reduce", l.J);
    if (l.defer && l.split == gpf::SPLIT_ALL)
      return plan_fail(msg, msg_len, "J=%d: deferred diagonal update under the all-tile split", l.J);
    // the flat finish waits for the diagonal block inside the launch (gpf::flat_piece)
    if (l.split == gpf::SPLIT_ALL && !l.ed)
      return plan_fail(msg, msg_len, "J=%d: all-tile split launch without the early diagonal factor", l.J);
    // look-ahead: LA workgroups only where a next critical tile exists, no split, early diagonal
    // factor; a seeded launch follows a launch of the same group that ran them
    if (l.la && (l.split != gpf::SPLIT_NONE || !l.ed || ((l.la & 1) && (l.J < 1 || l.J > nt - 3)) ||
                 ((l.la & 2) && (l.J < 2 || l.J > nt - 2 || !(la_prev[l.g] & 1)))))
      return plan_fail(msg, msg_len, "J=%d g=%d: look-ahead bits %d out of place", l.J, l.g, l.la);
    if ((la_prev[l.g] & 1) && !(l.la & 2))
      return plan_fail(msg, msg_len, "J=%d g=%d: look-ahead partials of launch J-1 left unused", l.J, l.g);
    la_prev[l.g] = l.la;
    if (l.ro && (ng != 1 || !l.ed || !l.sy || l.split != gpf::SPLIT_NONE || l.grp != 0 || l.J < 1 || 3 * l.gc > 256 ||
                 l.grid != (unsigned)(l.gc * (nt - 1) + 2 * l.gc)))
      return plan_fail(msg, msg_len, "J=%d g=%d: reordered dispatch out of place", l.J, l.g);
    // look-ahead pieces (early-diagonal launches): pieces only from J >= 1 with a block column behind,
    // consumed by the next launch of the same group (which reads the other parity); the tag the kernel
    // decodes the group's particle count from must carry it whole
    if (l.lall) {
      if (!l.ed || l.split != gpf::SPLIT_NONE || !l.defer || (l.la & 1) || ((l.la & 2) && (l.lall & 2)) || l.ro || nt < 4 ||
          ((l.lall & 1) && gpf::lall_items(l.J, nt) == 0) ||
          ((l.lall & 2) && (l.J < 2 || !(lall_prev[l.g] & 1) || pairJ[l.g] != l.J - 1)))
        return plan_fail(msg, msg_len, "J=%d g=%d: look-ahead pieces %d out of place", l.J, l.g, l.lall);
      if (gpf::P_of(l.tag) != l.gc || gpf::pb_of(l.tag) != lpb || gpf::smax_of(l.tag) != lsmax ||
          fp.lb_bytes < (size_t)2 * (l.p0 + l.gc) * lsmax * T * T * 8)
        return plan_fail(msg, msg_len, "J=%d g=%d: look-ahead tag %#x does not carry gc=%d pb=%d smax=%d", l.J, l.g,
                         (unsigned)l.tag, l.gc, lpb, lsmax);
    }
    if ((lall_prev[l.g] & 1) && !(l.lall & 2))
      return plan_fail(msg, msg_len, "J=%d g=%d: launch J-1's look-ahead pieces left unused", l.J, l.g);
    lall_prev[l.g] = l.lall;
    // paired block columns: a lead launch (J odd, with a block column behind it, fused diagonal factor,
    // deferred update, no split, groups of 8 particles) is followed on its stream by the follow
    // launch J+1, and only there
    if (l.pair && (l.ed || l.split != gpf::SPLIT_NONE || !l.defer || l.grp != 0 || l.gc % 8 != 0 || nt < 4 ||
                   fp.pb_bytes < gpf::pair_slot(l.p0 + l.gc, 0, nt) * 8 ||
                   fp.pstart_bytes < (size_t)(l.p0 + l.gc) * ntl * gpf::PAIR_HMAX * 4 ||
                   (l.pair == 1 && (!(l.J & 1) || l.J + 1 > nt - 1 || !l.sy)) ||
                   (l.pair == 2 && (l.sy || pair_prev[l.g] != 1 || pairJ[l.g] != l.J - 1))))
      return plan_fail(msg, msg_len, "J=%d g=%d: paired block column %d out of place", l.J, l.g, l.pair);
    if (pair_prev[l.g] == 1 && l.pair != 2)
      return plan_fail(msg, msg_len, "J=%d g=%d: the lead launch's partials left unused", l.J, l.g);
    pair_prev[l.g] = l.pair;
    pairJ[l.g] = l.J;
    if (l.pair == 1) {
      ++pairs;
      if (l.grid != (unsigned)(l.gc * gpf::pair_grid_per_particle(l.J, nt)))
        return plan_fail(msg, msg_len, "J=%d g=%d: lead launch grid %u", l.J, l.g, l.grid);
      std::vector<int> pla((size_t)tiles, 0), syp((size_t)l.gc, 0);
      for (unsigned b = 0; b < l.grid; ++b) {
        int p = -1, w = -1;
        const int role = gpf::pair_decode((int)b, l.J, l.gc, nt, p, w);
        if (p < 0 || p >= l.gc || (int)(b & 7) != (p & 7))
          return plan_fail(msg, msg_len, "J=%d block %u: pair decode p=%d (its XCD is not the particle's)", l.J, b, p);
        if (role != gpf::ROLE_WHOLE) {  // a partner: its tile's workgroup of the same particle 8 or 16 ids
          // earlier (a SYRK workgroup: its critical tile, which waits for it, 8 ids later)
          int p2 = -1, w2 = -1, ok = 0;
          for (int k = 1; k <= 2 && !ok; ++k) {
            const int b2 = role == gpf::ROLE_SYRK ? (int)b + 8 * k : (int)b - 8 * k;
            ok = b2 >= 0 && b2 < (int)l.grid && gpf::pair_decode(b2, l.J, l.gc, nt, p2, w2) == gpf::ROLE_WHOLE &&
                 p2 == p && w2 == (role == gpf::ROLE_SYRK ? 0 : w) && (role != gpf::ROLE_SYRK || k == 1);
          }
          if (!ok) return plan_fail(msg, msg_len, "J=%d block %u: partner (role %d) not beside its tile", l.J, b, role);
        }
        if (role == gpf::ROLE_SYRK) {
          if (syrk[p]++) return plan_fail(msg, msg_len, "J=%d: duplicate SYRK workgroup p=%d", l.J, p);
        } else if (role == gpf::ROLE_SYRKP) {
          if (w != 1 || l.J + 2 > nt - 1 || syp[p]++)
            return plan_fail(msg, msg_len, "J=%d: misplaced or duplicate partial SYRK p=%d", l.J, p);
        } else if (role == gpf::ROLE_PLA) {
          if (w < 1 || w >= ntl || pla[(size_t)p * ntl + w]++)
            return plan_fail(msg, msg_len, "J=%d: misplaced or duplicate look-ahead partial p=%d w=%d", l.J, p, w);
          if (gpf::pair_slot(p, w - 1, nt) + (size_t)T * T > (size_t)l.gc * ntl * T * T)
            return plan_fail(msg, msg_len, "J=%d: partial slot outside the group's buffer", l.J);
        } else if (role == gpf::ROLE_WHOLE) {
          if (w < 0 || w >= ntl) return plan_fail(msg, msg_len, "J=%d block %u decodes out of range", l.J, b);
          ++whole[(size_t)p * ntl + w];
        } else {
          return plan_fail(msg, msg_len, "J=%d block %u: role %d in a lead launch", l.J, b, role);
        }
        ++wgs;
      }
      for (int q = 0; q < l.gc; ++q) {
        if (syrk[q] != 1 || syp[q] != (l.J + 2 <= nt - 1 ? 1 : 0))
          return plan_fail(msg, msg_len, "J=%d particle %d: %d SYRK, %d partial SYRK workgroups", l.J, q, syrk[q], syp[q]);
        syrk_wgs += 1;
        for (int w = 0; w < ntl; ++w) {
          if (whole[(size_t)q * ntl + w] != 1 || pla[(size_t)q * ntl + w] != (w >= 1 ? 1 : 0))
            return plan_fail(msg, msg_len, "J=%d particle %d tile %d: %d runs, %d partials", l.J, q, w,
                             whole[(size_t)q * ntl + w], pla[(size_t)q * ntl + w]);
          ++whole_tiles;
        }
      }
      continue;
    }
    std::vector<int> lawg((size_t)l.gc, 0);
    const int nstd = (l.ed ? l.gc : 0) + (l.sy ? l.gc : 0) + l.gc * ntl;
    std::vector<int> lpc;
    if (l.lall & 1) {
      if (l.grid != (unsigned)(nstd + l.gc * gpf::lall_total(l.J, nt, lpb)))
        return plan_fail(msg, msg_len, "J=%d g=%d: look-ahead launch grid %u", l.J, l.g, l.grid);
      lpc.assign((size_t)l.gc * lsmax, 0);
    }
    for (unsigned b = 0; b < l.grid; ++b) {
      int p = -1, w = -1, sidx = -1;
      if ((l.lall & 1) && gpf::lall_is_piece((int)b, l.J, l.gc, nt, nstd, l.lall, l.tag)) {
        // a look-ahead piece: every (particle, item, piece) once
        int it = -1;
        gpf::lall_decode(gpf::lall_piece_index((int)b, l.gc, nt, nstd, l.lall), l.J, l.gc, nt, lpb, p, it, sidx);
        if (p < 0 || p >= l.gc || it < 0 || it >= gpf::lall_items(l.J, nt) || sidx < 0 || sidx >= gpf::lall_np(l.J, it, nt, lpb))
          return plan_fail(msg, msg_len, "J=%d block %u: look-ahead piece decodes out of range", l.J, b);
        const int o = gpf::lall_off(l.J, it, nt, lpb) + sidx;
        if (o >= lsmax || gpf::lall_slot(l.J, it, sidx, p, l.gc, nt, lsmax, lpb) + (size_t)T * T > (size_t)2 * l.gc * lsmax * T * T ||
            lpc[(size_t)p * lsmax + o]++)
          return plan_fail(msg, msg_len, "J=%d block %u: look-ahead piece slot %d duplicate or outside", l.J, b, o);
        ++wgs;
        continue;
      }
      // (pieces ahead of the tiles: the block index the kernel hands step_decode)
      const unsigned bt = (l.lall & 5) == 5 ? (unsigned)gpf::lall_tile_block((int)b, l.J, l.gc, nt, nstd, l.tag) : b;
      const int role =
          l.split == gpf::SPLIT_ALL ? gpf::step_decode<gpf::SPLIT_ALL>(bt, l.J, l.gc, nt, l.grp, l.S, l.ed, 0, 0, p, w, sidx)
                                    : gpf::step_decode<gpf::SPLIT_NONE>(bt, l.J, l.gc, nt, l.grp, l.S, l.ed, l.sy,
                                                                        (l.la & 1) && !l.sy, p, w, sidx, l.ro);
      if (role == gpf::ROLE_DIAG) {  // one diagonal workgroup per particle, ahead of every tile of the launch
        // (reordered: right behind the particles' light U tiles, which wait for it, and the SYRK workgroups)
        if (!l.ed || p < 0 || p >= l.gc || (unsigned)p + (l.ro ? 2 * l.gc : 0) != bt || diag[p]++)
          return plan_fail(msg, msg_len, "J=%d block %u: misplaced or duplicate diagonal workgroup (p=%d)", l.J, b, p);
        ++wgs;
        continue;
      }
      if (role == gpf::ROLE_LA) {  // one per particle, right behind the diagonal and SYRK workgroups
        if (!(l.la & 1) || l.sy || p < 0 || p >= l.gc || (unsigned)p + (l.ed ? l.gc : 0) != bt || lawg[p]++)
          return plan_fail(msg, msg_len, "J=%d block %u: misplaced or duplicate look-ahead workgroup (p=%d)", l.J, b, p);
        ++wgs;
        continue;
      }
      if (role == gpf::ROLE_SYRK) {  // one per particle, right behind the diagonal workgroups (reordered: the light U tiles)
        if (!l.sy || p < 0 || p >= l.gc || (unsigned)p + (l.ro || l.ed ? l.gc : 0) != bt || syrk[p]++)
          return plan_fail(msg, msg_len, "J=%d block %u: misplaced or duplicate SYRK workgroup (p=%d)", l.J, b, p);
        ++wgs;
        continue;
      }
      if (p < 0 || p >= l.gc || w < 0 || w >= ntl || sidx < 0 || sidx >= pieces_of(w))
        return plan_fail(msg, msg_len, "J=%d block %u decodes out of range (p=%d w=%d)", l.J, b, p, w);
      const int t = p * ntl + w;
      if (role == gpf::ROLE_WHOLE) {
        ++whole[t];
      } else if (role == gpf::ROLE_PIECE) {
        if (pieces_of(w) < 2) return plan_fail(msg, msg_len, "J=%d block %u is a piece of an unsplit tile", l.J, b);
        ++piece[(size_t)t * l.S2 + sidx];
        // slots as k_step addresses them: S2 per tile
        // counters: the flat finish's FLAT_CNT words of (particle, launch, tile) inside the
        // particle's ntl * cstride (gpf::flat_piece)
        const size_t off = l.part_off + ((size_t)t * l.S2 + sidx) * T * T;
        const size_t ci = l.cnt_off + (size_t)p * ntl * cstride + ((size_t)l.J * ntl + w) * gpf::FLAT_CNT;
        const size_t cn = gpf::FLAT_CNT;
        if (off + (size_t)T * T > part_cap || ci + cn > cnt_cap || l.S2 > gpf::SPLIT_MAXS ||
            ci + cn > l.cnt_off + (size_t)(p + 1) * ntl * cstride)
          return plan_fail(msg, msg_len, "J=%d tile %d piece %d outside the split buffers (S=%d S2=%d)", l.J, t, sidx, l.S,
                           l.S2);
        plo[l.g] = std::min(plo[l.g], off);
        phi[l.g] = std::max(phi[l.g], off + (size_t)T * T);
        clo[l.g] = std::min(clo[l.g], ci);
        chi[l.g] = std::max(chi[l.g], ci + cn);
      }
      ++wgs;
    }
    for (size_t i = 0; i < lpc.size(); ++i)
      if ((int)(i % lsmax) < gpf::lall_total(l.J, nt, lpb) && lpc[i] != 1)
        return plan_fail(msg, msg_len, "J=%d particle %d: look-ahead piece %d run %d times", l.J, (int)(i / lsmax),
                         (int)(i % lsmax), lpc[i]);
    for (int q = 0; q < l.gc; ++q) {
      if (diag[q] != l.ed) return plan_fail(msg, msg_len, "J=%d particle %d: %d diagonal workgroups", l.J, q, diag[q]);
      diag_wgs += diag[q];
      if (syrk[q] != l.sy) return plan_fail(msg, msg_len, "J=%d particle %d: %d SYRK workgroups", l.J, q, syrk[q]);
      if (lawg[q] != ((l.la & 1) && !l.sy ? 1 : 0))
        return plan_fail(msg, msg_len, "J=%d particle %d: %d look-ahead workgroups", l.J, q, lawg[q]);
      syrk_wgs += syrk[q];
    }
    for (int t = 0; t < tiles; ++t) {
      int np = 0;
      for (int s = 0; s < l.S2; ++s) {
        if (piece[(size_t)t * l.S2 + s] > 1) return plan_fail(msg, msg_len, "J=%d tile %d: piece %d run %d times", l.J, t, s, piece[(size_t)t * l.S2 + s]);
        np += piece[(size_t)t * l.S2 + s];
      }
      if (whole[t] == 1 && np == 0) ++whole_tiles;
      else if (whole[t] == 0 && np == pieces_of(t % ntl)) ++split_tiles;  // S arrivals on a zeroed counter: one finisher
      else return plan_fail(msg, msg_len, "J=%d tile %d: %d whole runs and %d pieces", l.J, t, whole[t], np);
    }
  }
  for (int g = 0; g < ng; ++g)
    if (pair_prev[g] == 1 || (lall_prev[g] & 1)) return plan_fail(msg, msg_len, "group %d ends with unused partials", g);
  for (int a = 0; a < ng; ++a)
    for (int b2 = a + 1; b2 < ng; ++b2) {
      if (plo[a] < phi[a] && plo[b2] < phi[b2] && plo[a] < phi[b2] && plo[b2] < phi[a])
        return plan_fail(msg, msg_len, "groups %d and %d share split-K partial slots", a, b2);
      if (clo[a] < chi[a] && clo[b2] < chi[b2] && clo[a] < chi[b2] && clo[b2] < chi[a])
        return plan_fail(msg, msg_len, "groups %d and %d share split-K counters", a, b2);
    }
  if (stats) {  // (entry 9: not persistent; entry 10: lead launches of paired block columns)
    const long long st[11] = {(long long)plan.size(), wgs, whole_tiles, split_tiles, fp.S, Smax, ng, diag_wgs, syrk_wgs, 0, pairs};
    std::copy(st, st + 11, stats);
  }
  return GPF_OK;
}

}  // namespace
