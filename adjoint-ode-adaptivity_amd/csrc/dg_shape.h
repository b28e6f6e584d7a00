// dg_shape.h — which kernel runs, at what shape, once: the plan's tuning fields, the table of
// their keys (DG_TUNE_*, the environment overrides, the allowed values, the error texts) and
// the rules that turn them into the effective launch shapes (DESIGN.md §5 "Tunables and
// shapes").  Plain C++17, no HIP, so a host compiler builds it alone (tests/test_shape_host.py
// pins the table and the rules on the CPU).  Nothing here is stated a second time elsewhere.
#pragma once
#include <cstdint>
#include <cstdlib>

#include "dg_advec.h"

namespace dgk {

constexpr int kTileLanes = 256;      // lanes of a width-1 workgroup tile (kBlock, dg_common.h)
constexpr int kSweepMaxSteps = 40;   // steps per dataflow launch (block constants are kernargs)
constexpr int kPSMaxSteps = 32;  // k_psweep: 8 blocks of 4, the blocks' constants fit the kernarg segment
// overlapped waves (dg_ovl_tiles.h)
constexpr int kOvG = 6;               // ghost elements per window end: >= 5 (a step's cone), even
constexpr int kOvS = 128 - 2 * kOvG;  // elements a wave owns

inline unsigned grid_for(int64_t n, int64_t per) { return unsigned((n + per - 1) / per); }

// ---------------------------------------------------------------------------
// The shape inputs: the plan facts the rules read, and the tuning fields (dg_plan_tune)
// ---------------------------------------------------------------------------
struct Shape {
  int NP = 0, nstages = 5;
  bool uniform = true;
  int64_t ktot = 0;
  // tile width of the step kernels (tile = 256*tile_width elements)
  int tile_width = 1;  // dg_plan_create: 2 for N <= 2 (measured per-N)
  int msteps = 4;  // time steps fused per launch (1, 2 or 4)
  // the jump-record sweeps' shape (dg_lserk4_fwd_rec / _adj_rec: no snapshot per step, so
  // long launches on wide tiles pay): tile width 1, 2 or 4, steps per launch 1..8
  // defaults measured at N = 4, K = 2^20: 1024-element pair tiles, 10 steps per
  // launch (a 20-step sweep is 10 + 10 launches)
  int rec_tile_width = 2;
  int rec_tile_width_fwd = 0;  // the forward record sweep's own tile width (0: as rec_tile_width)
  int rec_msteps = 10;
  // the forward's own record steps per launch: -1 by size (20 on 1024-element pair tiles up to
  // 3*2^20 elements, else as rec_msteps), 0 as rec_msteps, > 0 explicit
  int rec_msteps_fwd = -1;
  int rec_lane_elems = 2;  // 2: the pair tiles of dg_rec.hip, 1: dg_advec.hip k_step/k_adj
  // the p-enriched estimate's shape (dg_lserk4_adj_p, dg_dwr.hip): tile width 1 or 2 (256 or
  // 512 elements), steps per launch 1, 2, 4 or 8 (8 on 512-element tiles)
  int p_tile_width = 2;
  int p_msteps = 4;
  // 1: the estimate runs as ONE dataflow launch (k_adjp_flow) when its steps split into >= 2
  // blocks of p_msteps; 0: one launch per block
  int p_flow = 1;
  // 1: dg_lserk4_sweep_p runs forward and estimate as ONE dataflow launch (k_psweep) where the
  // shape allows; 0: the chains
  int p_sweep = 1;
  // watchdog: polls before a waiting work item gives up (0: the default, ~2^20; tests set 1)
  int sweep_spin_limit = 0;
  // the dataflow sweep (dg_lserk4_sweep_rec, dg_sweep.hip): 1 one dataflow launch where the
  // shape allows it, 0 the launch-per-block pair
  int rec_sweep = 1;
  // the dataflow sweep's workgroup waves (tiles of 128 * waves elements): 0 = as the record
  // sweeps' tile width (4 * rec_tile_width), else 4, 8, 12 or 16 (12 / 16: dataflow only, both
  // directions on that tile, whatever the launch chains' widths; 16 at Np <= 5)
  int sweep_waves = 0;
  // consecutive elements per lane of the dataflow sweep's tiles: 2 (pair tiles), or 4 at
  // Np <= 3 on 4- or 8-wave workgroups (tiles of 64 * 4 * waves elements)
  int sweep_lane_elems = 2;
  // how the dataflow sweep's tiles exchange faces: 0 through LDS with a workgroup barrier per
  // Horner level (dg_rec_tiles.h), 1 overlapped waves: DPP within a wave, one LDS exchange and
  // barrier per step (dg_ovl_tiles.h)
  int sweep_exchange = 0;
  // how the config-3 kernels (nonlinear flux / per-stage limiter, dg_burgers*.hip) exchange
  // neighbour values: 0 workgroup tiles through LDS, a barrier per exchange (dg_burgers.hip);
  // 1 overlapped waves, DPP shifts, no barrier inside a step (dg_burgers_ov.hip)
  int nl_exchange = 0;
  // dg_lserk4_fwd with snapshots: 0 the stage-loop kernels (k_step / wave tiles; bit-identical
  // to the record sweeps' stage-loop kernels), 1 Horner-form pair tiles (k_step_rps, dg_rec.hip;
  // tiles of 512 * tile_width elements, msteps steps per launch)
  int snap_pairs = 0;
  int xcd_order = 1;  // XCD-aware tile order
  int lane_elems = 0;  // 0: workgroup tiles (one element per lane); 2 or 4: wave tiles
};

// ---------------------------------------------------------------------------
// The tuning keys
// ---------------------------------------------------------------------------
// Record steps per launch: pair tiles take 1, 2, 4, 5, 8, 10, 16 or 20 (a sweep is chunked by
// halving: 20 -> 10 -> 5 -> 2 -> 1); the one-element-per-lane kernels 1, 2, 4 or 8.
inline bool rec_msteps_ok(int k) {
  return k == 1 || k == 2 || k == 4 || k == 5 || k == 8 || k == 10 || k == 16 || k == 20;
}

namespace tune {
// allowed values of a key (value, the plan's Np)
inline bool any(int64_t, int) { return true; }
inline bool is_0(int64_t v, int) { return v == 0; }
inline bool is_01(int64_t v, int) { return v == 0 || v == 1; }
inline bool is_12(int64_t v, int) { return v == 1 || v == 2; }
inline bool is_012(int64_t v, int) { return v == 0 || v == 1 || v == 2; }
inline bool is_1248(int64_t v, int) { return v == 1 || v == 2 || v == 4 || v == 8; }
inline bool is_0248(int64_t v, int) { return v == 0 || v == 2 || v == 4 || v == 8; }
inline bool rec_steps(int64_t v, int) { return rec_msteps_ok(int(v)); }
inline bool waves(int64_t v, int np) {
  return v == 0 || v == 4 || v == 8 || v == 12 || (v == 16 && np <= 5);
}
inline bool lane24(int64_t v, int np) { return v == 2 || (v == 4 && np <= 3); }
inline bool spin(int64_t v, int) { return v >= 0 && v <= (1 << 30); }

struct Row {
  int key;
  const char* env;      // the override read at plan creation, or null
  int Shape::*field;    // the member the key sets (null: nothing is stored)
  bool (*ok)(int64_t, int);
  const char* text;     // dg_plan_tune's error for a value outside the set
  int Shape::*zeroed;   // side effect: a member set to 0 (null: none)
};

// In the order the environment is read: a "both directions" row before the forward's own, so
// DG_REC_FWD_* wins when both are set.
inline const Row kRows[] = {
    {DG_TUNE_TILE_WIDTH, "DG_TILE_WIDTH", &Shape::tile_width, is_12, "tile width must be 1 or 2",
     nullptr},
    {DG_TUNE_LANE_ELEMENTS, "DG_LANE_ELEMENTS", &Shape::lane_elems, is_0248,
     "lane elements must be 0, 2, 4 or 8", nullptr},
    {DG_TUNE_STEPS_PER_LAUNCH, "DG_STEPS_PER_LAUNCH", &Shape::msteps, is_1248,
     "steps per launch must be 1, 2, 4 or 8", nullptr},
    {DG_TUNE_REC_TILE_WIDTH, "DG_REC_TILE_WIDTH", &Shape::rec_tile_width, is_12,
     "record tile width must be 1 or 2", &Shape::rec_tile_width_fwd},  // both directions
    {DG_TUNE_REC_FWD_TILE_WIDTH, "DG_REC_FWD_TILE_WIDTH", &Shape::rec_tile_width_fwd, is_012,
     "forward record tile width must be 0 (as the adjoint's), 1 or 2", nullptr},
    {DG_TUNE_REC_STEPS_PER_LAUNCH, "DG_REC_STEPS_PER_LAUNCH", &Shape::rec_msteps, rec_steps,
     "record steps per launch must be 1, 2, 4, 5, 8, 10, 16 or 20",
     &Shape::rec_msteps_fwd},  // both directions: the forward "as rec_msteps" (0, not -1)
    {DG_TUNE_REC_FWD_STEPS_PER_LAUNCH, "DG_REC_FWD_STEPS_PER_LAUNCH", &Shape::rec_msteps_fwd,
     rec_steps, "record steps per launch must be 1, 2, 4, 5, 8, 10, 16 or 20", nullptr},
    {DG_TUNE_REC_LANE_ELEMENTS, "DG_REC_LANE_ELEMENTS", &Shape::rec_lane_elems, is_12,
     "record lane elements must be 1 or 2", nullptr},
    {DG_TUNE_P_TILE_WIDTH, "DG_P_TILE_WIDTH", &Shape::p_tile_width, is_12,
     "p-estimate tile width must be 1 or 2", nullptr},
    {DG_TUNE_P_STEPS_PER_LAUNCH, "DG_P_STEPS_PER_LAUNCH", &Shape::p_msteps, is_1248,
     "p-estimate steps per launch must be 1, 2, 4 or 8", nullptr},
    {DG_TUNE_P_FLOW, "DG_P_FLOW", &Shape::p_flow, is_01,
     "p-estimate flow: 0 (one launch per block) or 1 (one dataflow launch)", nullptr},
    {DG_TUNE_P_SWEEP, "DG_P_SWEEP", &Shape::p_sweep, is_01,
     "p sweep: 0 (the chains) or 1 (one dataflow launch)", nullptr},
    {DG_TUNE_REC_SWEEP, "DG_REC_SWEEP", &Shape::rec_sweep, is_01,
     "record sweep mode must be 0 or 1", nullptr},
    {DG_TUNE_SWEEP_LANE_ELEMENTS, "DG_SWEEP_LANE_ELEMENTS", &Shape::sweep_lane_elems, lane24,
     "sweep lane elements: 2, or 4 at Np <= 3", nullptr},
    {DG_TUNE_SNAP_PAIRS, "DG_SNAP_PAIRS", &Shape::snap_pairs, is_01,
     "snapshot pairs: 0 (stage-loop kernels) or 1 (Horner pair tiles)", nullptr},
    {DG_TUNE_SWEEP_EXCHANGE, "DG_SWEEP_EXCHANGE", &Shape::sweep_exchange, is_01,
     "sweep exchange: 0 (LDS + barrier per level) or 1 (overlapped waves)", nullptr},
    {DG_TUNE_NL_EXCHANGE, "DG_NL_EXCHANGE", &Shape::nl_exchange, is_01,
     "config-3 exchange: 0 (workgroup tiles, LDS) or 1 (overlapped waves)", nullptr},
    {DG_TUNE_SWEEP_WAVES, "DG_SWEEP_WAVES", &Shape::sweep_waves, waves,
     "sweep waves: 0 (as the record tile width), 4, 8, 12 or 16 (16 at Np <= 5)", nullptr},
    // removed in round 5 (item = workgroup id relied on in-order dispatch per XCD): only the
    // take counter (0) remains
    {DG_TUNE_SWEEP_TAKE, nullptr, nullptr, is_0,
     "sweep take: only 0 (the take counter) is supported", nullptr},
    {DG_TUNE_SWEEP_SPIN_LIMIT, nullptr, &Shape::sweep_spin_limit, spin,
     "spin limit: 0 (default) .. 2^30", nullptr},
    {DG_TUNE_XCD_ORDER, nullptr, &Shape::xcd_order, any, "", nullptr},  // stored as value != 0
};

inline void store(Shape* s, const Row& r, int64_t v) {
  if (r.field) s->*r.field = (r.key == DG_TUNE_XCD_ORDER) ? int(v != 0) : int(v);
  if (r.zeroed) s->*r.zeroed = 0;
}

// dg_plan_tune: DG_OK, or DG_ERR_ARG with *text = the message.
inline int set(Shape* s, int key, int64_t value, const char** text) {
  for (const Row& r : kRows) {
    if (r.key != key) continue;
    if (!r.ok(value, s->NP)) {
      *text = r.text;
      return DG_ERR_ARG;
    }
    store(s, r, value);
    return DG_OK;
  }
  *text = "unknown tuning key";
  return DG_ERR_ARG;
}

// The environment overrides of dg_plan_create (after the per-N defaults): lookup(name) -> the
// value's text or null.  Read through atoi; a value outside the key's set is ignored.
template <class Lookup> void from_env(Shape* s, Lookup lookup) {
  for (const Row& r : kRows) {
    const char* v = r.env ? lookup(r.env) : nullptr;
    if (!v) continue;
    const int k = std::atoi(v);
    if (r.ok(k, s->NP)) store(s, r, k);
  }
}
}  // namespace tune

// ---------------------------------------------------------------------------
// The rules
// ---------------------------------------------------------------------------
// Tile width of the forward record sweep (the adjoint's is rec_tile_width).
inline int rec_fwd_width(const Shape* p) {
  return p->rec_tile_width_fwd ? p->rec_tile_width_fwd : p->rec_tile_width;
}

// Record sweeps run on pair tiles (dg_rec.hip), Np <= 9, unless DG_TUNE_REC_LANE_ELEMENTS = 1
// selects the one-element-per-lane record kernels of dg_advec.hip: W = 1 with 1..4 steps, W = 2
// with 1..8; Np = 9: at most 2 steps there (1024-element one-element-per-lane tiles -- 16-wave
// workgroups, 74 KB of LDS -- measured 20 % slower).
inline bool rec_pairs(const Shape* p) { return p->rec_lane_elems == 2; }

// The record steps per launch the plan's shape allows for a requested value m on tiles of
// width w.
inline int rec_msteps_cap(const Shape* p, int m, int w) {
  if (!rec_pairs(p)) {
    int q = 1;
    while (q * 2 <= m && q < 8) q *= 2;
    m = q;
  }
  if (m == 8 && w == 1 && !rec_pairs(p)) m = 4;
  if (rec_pairs(p) && w == 1 && m > 10) m = (m == 16) ? 8 : 10;
  if (!rec_pairs(p) && p->NP > 8 && m > 2) m = 2;
  return m;
}

// Adjoint (and, unless overridden, forward) record steps per launch.
inline int rec_msteps(const Shape* p) { return rec_msteps_cap(p, p->rec_msteps, p->rec_tile_width); }

// Forward record steps per launch.  By size (the default): one 20-step launch on 1024-element
// pair tiles while a 10-step launch would be only ~1.5-4 rounds of workgroups (up to 3*2^20
// elements: at K = 2^20 / 2^21 the forward is 5 / 2 % faster than 10 + 10), beyond that the
// adjoint's setting (at 2^22 equal, at config 4's 67 M elements 10 + 10 is 3 % faster: the
// wider halo outweighs the launch saved).  The adjoint prefers 10 + 10 at every size.
inline int rec_msteps_fwd(const Shape* p) {
  int m = p->rec_msteps_fwd;
  if (m < 0)
    m = (rec_pairs(p) && rec_fwd_width(p) == 2 && p->ktot <= (int64_t(3) << 20)) ? 20
                                                                             : p->rec_msteps;
  return rec_msteps_cap(p, m ? m : p->rec_msteps, rec_fwd_width(p));
}

// The launch shape of the linear forward sweep: steps per launch (before the caps of the tile
// shape), elements per lane of the wave tiles (0: stage-loop workgroup tiles), pair-tile
// snapshots.  The plan's own (msteps, lane_elems, snap_pairs) for dg_lserk4_fwd;
// dg_lserk4_sweep_p marches at {4, 0, 0}.
struct FwdShape {
  int msteps, lane_elems, snap_pairs;
};
inline FwdShape plan_shape(const Shape* p) { return {p->msteps, p->lane_elems, p->snap_pairs}; }

// Steps per launch the plan's shape allows: 8 only with 512-element tiles (the cone is
// 8*NS elements per side) and Np <= 8; at Np = 9 at most 2 (hipcc/ROCm 7.2 fails
// instruction selection for the 4-step shape there).
inline int effective_msteps(const Shape* p, FwdShape s) {
  int m = s.msteps;
  if (m == 8 && !(p->tile_width == 2 || s.lane_elems == 8)) m = 4;
  if (m == 8 && s.lane_elems == 2) m = 4;  // 128-element wave tiles: cone too wide
  if (p->NP > 8 && m > 2) m = 2;
  return m;
}

// Steps per limited-forward launch (config 3): 1 or 2 (the cone is 10 elements per step).  The
// workgroup-tile kernels are barrier-bound, so the 2-step cone's extra halo (20 instead of
// 10 elements per 256-element tile) costs more than the HBM round trip it saves whenever the
// snapshots are written anyway: the default (msteps 4) runs 1 step per launch with snapshots
// and 2 without (A/B at K = 2^22: 82 against 88 µs per step with snapshots, 84 against 80.5
// without).  An explicit msteps of 1 or 2 is kept.  The overlapped waves run 1 step per
// launch (a 2-step window would own 24 of its 64 elements).
inline int nl_msteps(const Shape* p, bool snapshots) {
  return (p->msteps == 2 || (p->msteps > 2 && !snapshots && !p->nl_exchange)) ? 2 : 1;
}

// Elements per tile of the dataflow sweep on workgroups of `waves` waves: 64 * lane elements
// * waves, or waves * 116 + 12 on overlapped waves.
inline int sweep_tile_elems(const Shape* p, int waves) {
  return p->sweep_exchange == 1 ? waves * kOvS + 2 * kOvG : 64 * p->sweep_lane_elems * waves;
}

// Work items / last-block adjoint tiles of a dataflow sweep over the plan's ktot elements, or
// over `elems` (>= 0: the scratch sizing for the reserved capacity).
inline int64_t sweep_tiles_adj(const Shape* p, int waves, int msa, int64_t elems = -1) {
  const int64_t n = elems >= 0 ? elems : p->ktot;
  return grid_for(n, sweep_tile_elems(p, waves) - 2 * ((msa * 5 + 1) & ~1));
}
inline int64_t sweep_items(const Shape* p, int waves, int msf, int msa, int nsteps,
                           int64_t elems = -1) {
  const int64_t n = elems >= 0 ? elems : p->ktot;
  const int64_t nTF = grid_for(n, sweep_tile_elems(p, waves) - 2 * ((msf * 5 + 2) & ~1));
  return int64_t(nsteps / msf) * nTF + int64_t(nsteps / msa) * sweep_tiles_adj(p, waves, msa, n);
}

// The dataflow sweep's blocks for `nsteps` steps (dg_sweep.hip): `on` with the forward /
// adjoint steps per block when the plan runs it -- pair tiles of one width in both
// directions (1024 or 512 elements), the record shape's 5-, 10- or 20-step (1024 only)
// forward and 5- or 10-step adjoint launches as its blocks, nsteps a multiple of both and at
// most kSweepMaxSteps -- else off (the launch-per-block pair runs, same results).
// With the plan's sweep_waves set (DG_TUNE_SWEEP_WAVES) the dataflow launch runs both
// directions on tiles of 128 * sweep_waves elements, whatever the launch chains' widths: 12
// and 16 waves take the 10- or 20-step forward and 10-step adjoint blocks (16 at Np <= 5).
// Unset (0), the shape follows the record sweeps' tile width, with the measured exceptions
// below (12-wave tiles at Np <= 5, 8-wave tiles at Np = 9 on uniform meshes).
struct SweepShape {
  bool on;
  int waves, msf, msa;
};
inline SweepShape sweep_shape(const Shape* p, int nsteps) {
  const int f = rec_msteps_fwd(p), a = rec_msteps(p), w = p->rec_tile_width;
  const int sw = p->sweep_waves;
  int nw = sw;
  bool tiles;
  if (sw) {
    tiles = (sw == 4 || sw == 8) || ((sw == 12 || (sw == 16 && p->NP <= 5)) && f >= 10 && a == 10);
  } else if (p->NP == 9 && p->uniform) {
    // the launch chains run 1024-element forward and 512-element adjoint tiles here; the one
    // launch takes 8-wave (1024-element) tiles in both directions: 7.06-7.23e11 DOF-updates/s
    // at K = 2^20 against 6.65e11 for the chains (profiles/r04/opreload/)
    nw = 8;
    tiles = true;
  } else {
    // as the record sweeps' tile width; on the 6-wave-per-SIMD uniform bodies (Np <= 5) 12-wave
    // tiles where their shape allows (1536 elements, 2 workgroups per CU; forward halo 1.15
    // instead of 1.25, a third fewer items): +3-4 % at N = 4, +1-3 % at N = 2
    // (profiles/r04/take/, perN/, shape_ab/)
    nw = 4 * w;
    tiles = rec_fwd_width(p) == w && (w == 1 || w == 2);
    // (Np = 2 keeps 8 waves: at 8 waves per SIMD, four 8-wave groups per CU, see SweepOcc)
    if (tiles && w == 2 && p->uniform && p->NP >= 3 && p->NP <= 5 && p->sweep_lane_elems == 2 &&
        f >= 10 && a == 10)
      nw = 12;
  }
  tiles = tiles && (p->sweep_lane_elems == 2 || (p->NP <= 3 && (nw == 4 || nw == 8)));
  if (p->sweep_exchange == 1)  // overlapped waves: pairs on 8, 12 or 16 (Np <= 5) waves, 20- or
                               // 10-step forward and 10-step adjoint blocks
    tiles = tiles && p->sweep_lane_elems == 2 &&
            (nw == 8 || nw == 12 || (nw == 16 && p->NP <= 5)) && f >= 10 && a == 10;
  const int T = sweep_tile_elems(p, nw);  // elements per tile
  const bool on = p->rec_sweep && rec_pairs(p) && tiles &&
                  (f == 5 || f == 10 || (f == 20 && T >= 900)) && (a == 5 || a == 10) &&
                  nsteps > 0 && nsteps % f == 0 && nsteps % a == 0 && nsteps <= kSweepMaxSteps;
  return {on, nw, f, a};
}

// The p-enriched estimate's steps per launch: the plan's setting (8 needs 512-element tiles),
// halved until it fits the steps left.
inline int p_msteps(const Shape* p) {
  int m = p->p_msteps;
  if (m == 8 && p->p_tile_width != 2) m = 4;
  return m;
}

// The estimate's dataflow form applies: the plan asks for it, the Horner kernels are selected
// (`horner`: DG_P_HORNER, dg_dwr.hip), and the steps split into 2 .. 40/MS blocks of the plan's
// steps per launch (4 on 256-element tiles; 4 or 8 on 512-element tiles).
inline bool p_flow_shape(const Shape* lo, int nsteps, int horner) {
  const int m = p_msteps(lo);
  return lo->p_flow && (horner == 1 || horner == 3) &&
         (m == 4 || (m == 8 && lo->p_tile_width == 2)) && nsteps > 0 && nsteps % m == 0 &&
         nsteps / m >= 2 && nsteps <= kSweepMaxSteps;
}

// The whole sweep as one dataflow launch applies: the estimate's dataflow shape at 4-step
// blocks, the forward's stage-loop workgroup tiles (not the wave tiles of N <= 2), and
// 2..8 blocks.
inline bool p_sweep_shape(const Shape* lo, int nsteps, int horner) {
  return lo->p_sweep && p_flow_shape(lo, nsteps, horner) && p_msteps(lo) == 4 &&
         lo->lane_elems == 0 && lo->nstages == 5 && nsteps <= kPSMaxSteps;
}

// Tiles of one m-step block of the p launches over `elems` elements (extent 256 W - 10 m), and
// the work items of each launch: k_adjp_flow blocks x tiles; k_psweep twice that at m = 4
// (forward and estimate blocks).
inline int64_t p_tiles(const Shape* lo, int m, int64_t elems) {
  const int64_t TE = int64_t(kTileLanes) * lo->p_tile_width - 10 * m;
  return (elems + TE - 1) / TE;
}
inline int64_t p_flow_items(const Shape* lo, int nsteps, int64_t elems) {
  const int m = p_msteps(lo);
  return int64_t(nsteps / m) * p_tiles(lo, m, elems);
}
inline int64_t p_sweep_items(const Shape* lo, int nsteps, int64_t elems) {
  return 2 * int64_t(nsteps / 4) * p_tiles(lo, 4, elems);
}

}  // namespace dgk
