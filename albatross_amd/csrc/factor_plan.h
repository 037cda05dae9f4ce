// factor_plan.h — the schedule of the dense factorisation as plain C++ (no HIP; g++ -std=c++17 compiles it): which outer
// steps a factorisation of n rows takes and what each does, how the panels of an outer block are launched, how a step
// launch is shaped.  Integer arithmetic on n, the remaining rows and FactorSwitches only.  chol.hip fills the switches
// from the context and the call's FactorRequest and carries the plan out (factor_lower, panel_phase);
// agp_debug_factor_plan (debug_api.hip) shows the same plan to tests/test_fit_schedule_host.py without a device.  Every
// switch point of the schedule lives HERE.
#pragma once

namespace agp {

// ---- the schedule's switch points (measured on one MI355X; DESIGN.md sections 3 and 8 hold the sweeps) ------------
// The switches a caller can set - AGP_PANEL_FUSED=0 (POTRF and TRSM as two launches), AGP_STEP_BELOW=<rows> (0: no step
// launches), ... - are read ONCE, at agp_context_create, into ctx->tune (api.hip); everything else is a constant.
constexpr long long FUSED_BELOW = 4608;     // remaining rows at or below which POTRF + TRSM are one fused launch (2048 .. 4608 best)
constexpr long long INNER_LEFT_ABOVE = 6144;  // left-looking inside an outer block while more rows than this remain
constexpr long long NBO_512_ABOVE = 2048, NBO_256_ABOVE = 1024;  // outer block width 512 / 256 / 128 by remaining rows
constexpr long long NBO_WIDE_ABOVE = 8192;  // ... and FactorRequest::nbo_wide (mixed precision) above this
constexpr long long THROTTLE_BELOW = 8192;  // bulk updates handed to their stream by the host once their panel is done
constexpr long long U1_F32_ABOVE = 4096;    // mixed precision: U1 on the fp32 MFMA path while the block column is this tall
constexpr long long SINGLE_BELOW = 1536;    // the very end on one stream (when the step launches are off)
constexpr long long MASK_BELOW = 8704;      // bulk updates on the CU-masked stream from here on
constexpr long long HANDOVER_BULK_ABOVE = 1536;  // hand-over to a step tail with more rows than this: the bulk kernel
// (chol.hip asserts that these three equal NB, 1 + UPD_BLOCKS and agp_context::HEADCNT_WORDS)
constexpr long long PLAN_NB = 128;          // panel width
constexpr long long STEP_FIXED_CRITICAL = 10;  // step launch: the factoring workgroup and the nine that update its block
constexpr long long MERGED_STEPS_MAX = 256;    // counters of the merged bulk updates, one per outer step

// What the bulk updates of a factorisation multiply: the fp64 panels themselves, or - the mixed-precision fit - a
// low-precision copy of each step's panel in one of three formats.  The values are what agp_debug_factor_plan receives
// in switches[5].
enum class BulkProducts : int { Fp64 = -1, Fp32 = 3, Bf16x3 = 4, F16x2 = 5 };
inline bool uses_planes(BulkProducts p) { return p == BulkProducts::Bf16x3 || p == BulkProducts::F16x2; }  // split 16-bit planes
inline bool is_mixed(BulkProducts p) { return p == BulkProducts::Fp32 || uses_planes(p); }

// Everything the decisions read, as plain values (chol.hip: factor_switches fills it from the context's tuning and
// buffers and from the FactorRequest of the call).
struct FactorSwitches {
  bool panel_fused = true;                     // ctx->tune
  long long step_below = 4608, merge_above = 8704;
  long long nbo_override = 0, nbo_wide = 0;    // nbo_wide: FactorRequest::nbo_wide (split planes) or AGP_FP64_NBO, already resolved
  BulkProducts products = BulkProducts::Fp64;  // of the bulk updates (FactorRequest::products, or what it fell back to)
  long long step_slots = 0, cus = 256;         // workgroups of the step kernel the device holds at once / its CUs
  bool have_masked_stream = false;
  bool headcnt_ready = false;                  // the merged updates' counters are zeroed
  bool step_buffers_ready = false;             // second image + row counters + what the fused kernel needs, for all n rows
  bool fused_buffers_ready = false;            // z slots and tile images sentinel-filled for the columns in question
  // inversion of the wide diagonal blocks for the fit's back substitution under the factorisation (FactorRequest::inv_W)
  bool inv_requested = false;                  // asked for, and ev_inv and the second stream exist
  long long bs_BW = 0, bs_done = 0;            // block width / blocks already inverted on entry
};

// ---- what ONE factorisation is asked to do and what it reports: arguments of factor_lower (chol.hip), never kept --
// The sentinel fills panel_fused_plan planned for the fused panel kernels: a value, used by the one factorisation it
// was made for.
struct FusedPrep {
  const double *img = nullptr;  // tile images the fills were planned for (nullptr: nothing planned, two-launch path)
  long long upto = 0;           // columns [.., upto) are covered
  bool headcnt = false;         // the merged updates' counters are zeroed in the same launch
  bool covers(const double *images, long long columns) const { return img && img == images && upto >= columns; }
};
struct FactorTimers;  // common.h (HIP events)
struct FactorRequest {
  BulkProducts products = BulkProducts::Fp64;  // of the bulk updates
  long long nbo_wide = 0;       // mixed precision, split planes: outer block width while many rows remain (0 / 512: default schedule)
  // Early inversion of the wide diagonal blocks for the back substitution of a fit: factor_lower inverts the blocks that
  // are final on its (then idle) second stream while the chain-bound tail runs, and records ev_inv behind them.
  double *inv_W = nullptr;      // where the inverses go (nullptr: not requested)
  long long inv_BW = 0;         // ... and their width
  FusedPrep prep;               // fills the caller has already launched with its own (default: factor_lower prepares)
  FactorTimers *timers = nullptr;
};
struct FactorOutcome { long long inv_done = 0; };  // wide blocks inverted under the factorisation

// The request's part of the switches (the context's part: chol.hip, factor_switches).  products: req.products, or what
// factor_lower fell back to; prep: the fills in force for the tile images `img` up to column `upto`; fp64_nbo:
// AGP_FP64_NBO (measurement switch); can_invert: the event and the stream of the inversion exist.  Every factorisation
// enters with no wide block inverted: bs_done stays 0 (only agp_debug_factor_plan sets it, like nbo_override).
inline void apply_request(FactorSwitches &sw, const FactorRequest &req, BulkProducts products, const FusedPrep &prep, const double *img,
                          long long upto, long long fp64_nbo, bool can_invert) {
  sw.products = products;
  sw.nbo_wide = uses_planes(products) ? req.nbo_wide : fp64_nbo;
  sw.fused_buffers_ready = prep.covers(img, upto);
  sw.headcnt_ready = sw.fused_buffers_ready && prep.headcnt;
  sw.inv_requested = req.inv_W && can_invert;
  sw.bs_BW = req.inv_BW;
}

// bits of an outer step and of the inversions: the values of agp_context::ScheduleRecord (chol.hip asserts it)
constexpr unsigned STEP_BIT_MERGED = 1, STEP_BIT_STEP = 2, STEP_BIT_THROTTLED = 4, STEP_BIT_MASKED = 8, STEP_BIT_SINGLE = 16;
constexpr unsigned INV_BIT_EARLY = 1, INV_BIT_LAST_STEP = 2, INV_BIT_TAIL = 4;

// One outer step: apply the factored panel block [k0, kend) to what is right of it, factor the block [kend, next_end).
// The first step has k0 == kend == 0 and nothing to apply.
struct OuterStep {
  long long k0 = 0, kend = 0, next_end = 0;
  long long index = 0;         // of the steps with an update, from 0: the counter word of a merged launch
  unsigned bits = 0;           // STEP_BIT_*: what ScheduleRecord shows
  bool step_mode = false;      // the panels of [kend, next_end) as step launches
  bool masked = false;         // bulk stream of this step: the CU-masked one
  bool mixed_tall = false;     // mixed precision and >= U1_F32_ABOVE rows: operand copy of the panel, U1 on the low-precision path
  bool handover_whole_trailing = false;  // U1 is the hand-over to the step tail: the whole trailing matrix, bulk kernel
  // Wide diagonal blocks to invert on the idle second stream.  At the last step: blocks [0, inv_last_step), all final
  // when the step begins.  Under the panels: blocks [inv_first, inv_first + inv_count) become final after panel
  // mark_after - the host marks that panel, waits for the mark and hands the inversion over while the last four panels
  // run.  inv_bit: INV_BIT_EARLY (an all-step fit, which never reaches a last step) or INV_BIT_TAIL (the step tail).
  long long inv_last_step = 0;
  long long inv_first = 0, inv_count = 0, mark_after = -1;
  unsigned inv_bit = 0;
};

// May `rows` remaining rows be factored with step launches?  The row workgroups of a step launch wait for trailing
// workgroups that are dispatched AFTER them: all critical workgroups (10 + one per 64 rows) and at least 64 trailing ones
// must be resident at once, or the waiters would sit out their 2 s time-out.  Fewer slots than that (a small partition,
// a CU mask): the two-launch schedule.  Should the hand-over time out all the same (flags[2]), agp_fit_create repeats
// the fit without step launches (api.hip).
inline bool step_fits(long long step_below, long long step_slots, long long rows) {
  return step_below > 0 && rows <= step_below && step_slots >= STEP_FIXED_CRITICAL + rows / 64 + 64;
}

// Outer block width as a function of the remaining (trailing) size.  Wide blocks (K = 512) keep
// the bulk update's C traffic off the HBM roofline and its MFMA efficiency up; narrow blocks
// shorten the serial panel chain per step.  With the current panel kernels the choice barely
// matters at N = 16384 (scripts/sweep_nbo.sh: every split at or below 4096 within 1 %).
inline long long pick_nbo(long long remaining, long long override_nbo, long long wide) {
  if (override_nbo > 0) return override_nbo;
  // (mixed precision, bf16 x 3: at 150 TFLOP/s the fp64 C read-modify-write of a K = 512 update is 2.3 TB/s next to
  // 2.6 TB/s of operand strips beyond the L2 - a deeper outer block halves the former while many rows remain)
  if (wide > 512 && remaining > NBO_WIDE_ABOVE) return wide;
  if (remaining > NBO_512_ABOVE) return 512;
  if (remaining > NBO_256_ABOVE) return 256;
  return PLAN_NB;
}

// Yields the outer steps of one factorisation in order: FactorPlanner p(n, sw); OuterStep s; while (p.next(s)) ...
class FactorPlanner {
 public:
  FactorPlanner(long long n, const FactorSwitches &sw) : n_(n), sw_(sw), bs_done_(sw.bs_done) {}

  bool next(OuterStep &s) {
    if (started_ && kend_ >= n_) return false;
    s = OuterStep();
    const long long bw = sw_.bs_BW, last_wide = invertible() && n_ % bw == 0 ? n_ / bw - 1 : 0;  // all but the last wide block
    if (!started_) {
      started_ = true;
      // a small matrix: every panel a step launch.  Such a fit never reaches the two-stream tail where the wide blocks
      // get inverted at the last step: all but the last one are inverted under its last four panels instead.
      s.step_mode = step_ok(n_);
      s.next_end = s.step_mode ? n_ : clip(pick_nbo(n_, sw_.nbo_override, sw_.nbo_wide));
      s.bits = s.step_mode ? STEP_BIT_STEP : 0u;
      if (s.step_mode && bs_done_ == 0 && last_wide >= 1) under_panels(s, 0, last_wide, INV_BIT_EARLY);
      kend_ = s.next_end;
      return true;
    }
    const long long rows = n_ - kend_;
    s.k0 = k0_; s.kend = kend_; s.index = index_++;
    s.next_end = clip(kend_ + pick_nbo(rows, sw_.nbo_override, sw_.nbo_wide));
    // The very end runs on ONE stream: the last outer block spans all remaining columns - as step launches (U1
    // becomes the hand-over update of the whole trailing matrix), or, where those are off, with <= SINGLE_BELOW rows left:
    // there the bulk updates are 10-20 us launches, less than the ~10 us of event record / wait packets that hand each
    // of them to the second stream and back
    const bool step = step_ok(rows);
    const bool single = !step && sw_.nbo_override == 0 && rows <= SINGLE_BELOW;
    if (step || single) s.next_end = n_;
    const bool last = s.next_end == n_;
    s.step_mode = step;
    // Last step: everything left of kend is final and the second stream has nothing more to do - it inverts the wide
    // diagonal blocks the backward substitution of the fit will need (all but the last ones), off the chain.
    if (invertible() && bs_done_ == 0 && last && kend_ / bw > 0) bs_done_ = s.inv_last_step = kend_ / bw;
    // End phase: the bulk updates move to the CU-masked stream (chol.hip: factor_lower says why)
    s.masked = sw_.have_masked_stream && rows <= MASK_BELOW;
    s.mixed_tall = is_mixed(sw_.products) && rows >= U1_F32_ABOVE;
    // Bulk-bound phase, fp64: U1(j) and U2(j) as ONE launch on the bulk stream, gated by a counter (factor_lower)
    const bool merged = !is_mixed(sw_.products) && sw_.nbo_override == 0 && !step && !last && sw_.headcnt_ready && sw_.merge_above > 0 &&
                        rows > sw_.merge_above && s.index < MERGED_STEPS_MAX && (s.next_end - kend_) % PLAN_NB == 0;
    if (merged) {
      s.bits = STEP_BIT_MERGED | (s.masked ? STEP_BIT_MASKED : 0u);
    } else {
      // Chain-bound phase: the host hands U2(j) to the bulk stream only once P(j) HAS finished (factor_lower)
      const bool throttle = !last && rows <= THROTTLE_BELOW;
      s.handover_whole_trailing = step && rows > HANDOVER_BULK_ABOVE;
      s.bits = (step ? STEP_BIT_STEP : 0u) | (throttle ? STEP_BIT_THROTTLED : 0u) | (single ? STEP_BIT_SINGLE : 0u) |
               (!last && s.masked ? STEP_BIT_MASKED : 0u);
      // The step tail of a large fit, like the all-step fit: the wide diagonal blocks that become final INSIDE the tail
      // (all but the last one) are inverted on the idle second stream under the tail's last four panels - the back
      // substitution of the fit used to invert them behind the factorisation (~0.15 ms of a 29 ms fit at N = 16384).
      if (step && bs_done_ > 0 && last_wide > bs_done_ && bs_done_ == kend_ / bw && last_wide * bw - PLAN_NB >= kend_)
        under_panels(s, bs_done_, last_wide - bs_done_, INV_BIT_TAIL);
    }
    k0_ = kend_;
    kend_ = s.next_end;
    return true;
  }

  // The one thing the plan cannot know: whether the host's wait for the mark of an inversion under the panels
  // succeeded (otherwise those blocks are not inverted, and the substitution inverts them behind the factorisation).
  // Both such waits fall on the last step today, so no later decision reads the answer; bs_done() stays true all the same.
  void inversion_under_panels(const OuterStep &s, bool ran) { if (ran) bs_done_ = s.inv_first + s.inv_count; }
  long long bs_done() const { return bs_done_; }

 private:
  bool invertible() const { return sw_.inv_requested && sw_.bs_BW > 0; }
  // the chain-bound tail as one launch per panel on the chain stream once few enough rows are left
  bool step_ok(long long rows) const {
    return sw_.nbo_override == 0 && step_fits(sw_.step_below, sw_.step_slots, rows) && sw_.step_buffers_ready;
  }
  long long clip(long long end) const { return end > n_ ? n_ : end; }
  void under_panels(OuterStep &s, long long first, long long count, unsigned bit) const {
    s.inv_first = first; s.inv_count = count; s.inv_bit = bit;
    s.mark_after = (first + count) * sw_.bs_BW - PLAN_NB;
  }
  const long long n_;
  const FactorSwitches sw_;
  long long k0_ = 0, kend_ = 0, index_ = 0, bs_done_;
  bool started_ = false;
};

// How the panels of the outer block [k0, kend) are launched.
struct PanelPlan {
  bool step_mode;   // ONE launch per panel (panel_fused_kernel<true> from the second panel on), nothing else
  bool inner_left;  // left-looking inside the block: one product of depth k - k0 before panel k
  bool fused;       // POTRF + TRSM in one launch
};

inline PanelPlan plan_panels(long long n, long long k0, long long kend, bool step_mode, const FactorSwitches &sw) {
  PanelPlan p;
  p.step_mode = step_mode && kend == n;  // (a step launch updates ALL columns right of its panel)
  // While more than INNER_LEFT_ABOVE rows remain: left-looking inside the outer block - panel k is brought up to date
  // with the panels [k0, k) of this outer block in ONE product of depth k - k0 just before it is factored, instead of
  // every panel updating all later columns of the outer block with depth 128 (same flop, a third of the C traffic:
  // 35.2 -> 35.0 ms at N = 16384; where the chain is the critical path the deeper product costs 1-3 %).
  p.inner_left = !p.step_mode && (n - k0) > INNER_LEFT_ABOVE;
  // The consumers of the fused kernel hold their slots for the whole POTRF (~30 us): while the bulk update fills the
  // chip that costs it more than the saved launch (measured: 43.3 -> 41.8 TFLOP/s), so the fused kernel takes over
  // where the panel chain is the critical path
  p.fused = sw.panel_fused && sw.fused_buffers_ready && ((n - k0) <= FUSED_BELOW || p.step_mode);
  return p;
}

// Grid of one step launch (panel_fused_kernel<true>) with `below` rows under its panel, the panels_done-th panel of its
// outer block (from 1).  Workgroups [0, trail_first) are critical: the factoring one, the nine that update its block, one
// per 64 rows below; then trail_workers trailing workgroups that share trail_tiles tiles; then hold_count placeholders.
struct StepLaunchShape {
  unsigned grid = 0, trail_first = 0xffffffffu, hold_index = 0xffffffffu, hold_count = 0;  // (defaults: those of PotrfArgs)
  long long trail_tiles = 0, trail_workers = 1;
  unsigned long long rowcnt_expect = 0;
};

inline StepLaunchShape step_launch_shape(long long below, long long panels_done, long long step_slots, long long cus) {
  StepLaunchShape sh;
  sh.grid = (unsigned)(STEP_FIXED_CRITICAL + (below + 63) / 64);
  if (below <= 0) return sh;
  const long long nt = (below + 63) / 64;  // 64-row blocks below = tile rows of the trailing triangle
  sh.trail_first = sh.grid;
  sh.rowcnt_expect = 2ull * (unsigned long long)panels_done;
  const long long tiles = nt * (nt + 1) / 2 + 2 * nt;
  // Workgroups go round-robin over the XCDs and, inside one, to its CUs in turn: the first `cus` of a launch get a
  // CU each, number cus + i lands next to number i (scripts/microbench/hwid_probe.hip).  The critical workgroups -
  // the factoring one, the nine that update its block, the row workgroups - keep their CUs to themselves:
  // workgroups cus .. cus + (their number) are PLACEHOLDERS that idle until the image is complete (next to a
  // trailing workgroup the POTRF takes 40-47 us instead of 27-30 and the diagonal block arrives after 10-13 us
  // instead of 6).  The trailing workgroups take the tiles worker, worker + workers, ...: as many as fit on the
  // CUs left, not one per tile (2600 starts and exits per launch at 4000 remaining rows cost ~10 %).  If the
  // dispatch order ever differs this costs idle slots and nothing else.
  const long long slots = step_slots, first_round = cus, ncrit = sh.grid;
  long long workers = tiles, nhold = 0;
  if (ncrit + workers > first_round && ncrit < first_round) {
    // all critical workgroups while the trailing update is short; from ~2900 remaining rows on it is what the
    // launch takes and needs the slots: only the factoring workgroup and the nine that feed it
    nhold = tiles <= 1200 ? ncrit : STEP_FIXED_CRITICAL;
    const long long cap = slots - ncrit - nhold;
    if (workers > cap) workers = cap;
    if (ncrit + workers <= first_round) nhold = 0;
  } else if (workers > slots - ncrit) {
    workers = slots - ncrit;
  }
  // (the row tiles come first in the tile order and every one needs a workgroup of its own up front: the row
  // workgroups wait for them)
  if (workers < 2 * nt) workers = 2 * nt < tiles ? 2 * nt : tiles;
  sh.trail_tiles = tiles;
  sh.trail_workers = workers;
  sh.grid += (unsigned)workers;
  if (nhold > 0) {
    sh.hold_index = (unsigned)first_round;
    sh.hold_count = (unsigned)nhold;
    sh.grid += (unsigned)nhold;
  }
  return sh;
}

}  // namespace agp
