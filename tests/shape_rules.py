"""The plan's tuning keys and launch-shape rules, restated in Python.

Written from include/dg_advec.h's documentation of the keys and from the library's behaviour
before the rules moved into csrc/dg_shape.h; tests/test_shape_host.py compares it line for line
with a host program built on that header, tests/test_gpu_shape_queries.py with the library's
queries.  Nothing here reads the C++."""
import re

# key numbers (include/dg_advec.h; tests/test_abi.py holds _lib.py's copies to the header)
TILE_WIDTH, STEPS, XCD_ORDER, LANE_ELEMENTS, REC_TILE_WIDTH, REC_STEPS, REC_LANE_ELEMENTS, \
    REC_FWD_STEPS, P_TILE_WIDTH, P_STEPS, REC_FWD_TILE_WIDTH, REC_SWEEP, SPIN_LIMIT, SWEEP_WAVES, \
    SWEEP_LANE_ELEMENTS, SWEEP_TAKE, SWEEP_EXCHANGE, SNAP_PAIRS, P_FLOW, P_SWEEP, NL_EXCHANGE = \
    range(1, 22)

REC_STEP_VALUES = (1, 2, 4, 5, 8, 10, 16, 20)
REC_TEXT = "record steps per launch must be 1, 2, 4, 5, 8, 10, 16 or 20"

# the knobs, in the order the host program prints them, with the defaults of a new plan
# before the per-N defaults
KNOBS = (("tile_width", 1), ("msteps", 4), ("xcd_order", 1), ("lane_elems", 0),
         ("rec_tile_width", 2), ("rec_tile_width_fwd", 0), ("rec_msteps", 10),
         ("rec_msteps_fwd", -1), ("rec_lane_elems", 2), ("p_tile_width", 2), ("p_msteps", 4),
         ("p_flow", 1), ("p_sweep", 1), ("rec_sweep", 1), ("sweep_spin_limit", 0),
         ("sweep_waves", 0), ("sweep_lane_elems", 2), ("sweep_exchange", 0), ("snap_pairs", 0),
         ("nl_exchange", 0))


def allowed(key, NP):
  """The values dg_plan_tune accepts for a key at this Np (None: any value)."""
  return {
      TILE_WIDTH: (1, 2), STEPS: (1, 2, 4, 8), XCD_ORDER: None, LANE_ELEMENTS: (0, 2, 4, 8),
      REC_TILE_WIDTH: (1, 2), REC_STEPS: REC_STEP_VALUES, REC_LANE_ELEMENTS: (1, 2),
      REC_FWD_STEPS: REC_STEP_VALUES, P_TILE_WIDTH: (1, 2), P_STEPS: (1, 2, 4, 8),
      REC_FWD_TILE_WIDTH: (0, 1, 2), REC_SWEEP: (0, 1), SPIN_LIMIT: range(0, 2**30 + 1),
      SWEEP_WAVES: (0, 4, 8, 12) + ((16,) if NP <= 5 else ()),
      SWEEP_LANE_ELEMENTS: (2,) + ((4,) if NP <= 3 else ()), SWEEP_TAKE: (0,),
      SWEEP_EXCHANGE: (0, 1), SNAP_PAIRS: (0, 1), P_FLOW: (0, 1), P_SWEEP: (0, 1),
      NL_EXCHANGE: (0, 1)}[key]


# key -> (environment name or None, the knob it sets or None, dg_last_error's text)
KEYS = {
    TILE_WIDTH: ("DG_TILE_WIDTH", "tile_width", "tile width must be 1 or 2"),
    STEPS: ("DG_STEPS_PER_LAUNCH", "msteps", "steps per launch must be 1, 2, 4 or 8"),
    XCD_ORDER: (None, "xcd_order", ""),
    LANE_ELEMENTS: ("DG_LANE_ELEMENTS", "lane_elems", "lane elements must be 0, 2, 4 or 8"),
    REC_TILE_WIDTH: ("DG_REC_TILE_WIDTH", "rec_tile_width", "record tile width must be 1 or 2"),
    REC_STEPS: ("DG_REC_STEPS_PER_LAUNCH", "rec_msteps", REC_TEXT),
    REC_LANE_ELEMENTS: ("DG_REC_LANE_ELEMENTS", "rec_lane_elems",
                        "record lane elements must be 1 or 2"),
    REC_FWD_STEPS: ("DG_REC_FWD_STEPS_PER_LAUNCH", "rec_msteps_fwd", REC_TEXT),
    P_TILE_WIDTH: ("DG_P_TILE_WIDTH", "p_tile_width", "p-estimate tile width must be 1 or 2"),
    P_STEPS: ("DG_P_STEPS_PER_LAUNCH", "p_msteps",
              "p-estimate steps per launch must be 1, 2, 4 or 8"),
    REC_FWD_TILE_WIDTH: ("DG_REC_FWD_TILE_WIDTH", "rec_tile_width_fwd",
                         "forward record tile width must be 0 (as the adjoint's), 1 or 2"),
    REC_SWEEP: ("DG_REC_SWEEP", "rec_sweep", "record sweep mode must be 0 or 1"),
    SPIN_LIMIT: (None, "sweep_spin_limit", "spin limit: 0 (default) .. 2^30"),
    SWEEP_WAVES: ("DG_SWEEP_WAVES", "sweep_waves",
                  "sweep waves: 0 (as the record tile width), 4, 8, 12 or 16 (16 at Np <= 5)"),
    SWEEP_LANE_ELEMENTS: ("DG_SWEEP_LANE_ELEMENTS", "sweep_lane_elems",
                          "sweep lane elements: 2, or 4 at Np <= 3"),
    SWEEP_TAKE: (None, None, "sweep take: only 0 (the take counter) is supported"),
    SWEEP_EXCHANGE: ("DG_SWEEP_EXCHANGE", "sweep_exchange",
                     "sweep exchange: 0 (LDS + barrier per level) or 1 (overlapped waves)"),
    SNAP_PAIRS: ("DG_SNAP_PAIRS", "snap_pairs",
                 "snapshot pairs: 0 (stage-loop kernels) or 1 (Horner pair tiles)"),
    P_FLOW: ("DG_P_FLOW", "p_flow",
             "p-estimate flow: 0 (one launch per block) or 1 (one dataflow launch)"),
    P_SWEEP: ("DG_P_SWEEP", "p_sweep", "p sweep: 0 (the chains) or 1 (one dataflow launch)"),
    NL_EXCHANGE: ("DG_NL_EXCHANGE", "nl_exchange",
                  "config-3 exchange: 0 (workgroup tiles, LDS) or 1 (overlapped waves)"),
}
# the order dg_plan_create reads the environment in: a later name wins where two set one knob
ENV_ORDER = (TILE_WIDTH, LANE_ELEMENTS, STEPS, REC_TILE_WIDTH, REC_FWD_TILE_WIDTH, REC_STEPS,
             REC_FWD_STEPS, REC_LANE_ELEMENTS, P_TILE_WIDTH, P_STEPS, P_FLOW, P_SWEEP, REC_SWEEP,
             SWEEP_LANE_ELEMENTS, SNAP_PAIRS, SWEEP_EXCHANGE, NL_EXCHANGE, SWEEP_WAVES)
ENV_NAMES = tuple(KEYS[k][0] for k in ENV_ORDER)


class Shape:
  """The shape inputs of one plan."""

  def __init__(self, NP, uniform=True, nstages=5, ktot=1000, per_n=False, **knobs):
    self.NP, self.uniform, self.nstages, self.ktot = NP, uniform, nstages, ktot
    for name, default in KNOBS:
      setattr(self, name, default)
    if per_n:  # dg_plan_create's per-N defaults
      if NP <= 3:
        self.tile_width, self.lane_elems = 2, 4
      if NP == 9:
        self.rec_tile_width, self.rec_tile_width_fwd = 1, 2
    for name, v in knobs.items():
      assert hasattr(self, name), name
      setattr(self, name, v)

  def knobs(self):
    return " ".join(str(getattr(self, name)) for name, _ in KNOBS)

  def _store(self, key, value):
    knob = KEYS[key][1]
    if knob:
      setattr(self, knob, int(value != 0) if key == XCD_ORDER else value)
    if key == REC_TILE_WIDTH:
      self.rec_tile_width_fwd = 0  # both directions
    if key == REC_STEPS:
      self.rec_msteps_fwd = 0  # the forward "as the adjoint", not "by size"

  def tune(self, key, value):
    """dg_plan_tune: (return code, message)."""
    if key not in KEYS:
      return -1, "unknown tuning key"
    ok = allowed(key, self.NP)
    if key in (REC_STEPS, REC_FWD_STEPS):
      value32 = (value + 2**31) % 2**32 - 2**31  # these two keys are read as 32-bit ints
      if value32 not in ok:
        return -1, KEYS[key][2]
      value = value32
    elif ok is not None and value not in ok:
      return -1, KEYS[key][2]
    self._store(key, value)
    return 0, ""

  def environment(self, env):
    """The overrides dg_plan_create reads: C atoi of the text, a value outside the key's set
    is ignored."""
    for key in ENV_ORDER:
      text = env.get(KEYS[key][0])
      if text is None:
        continue
      m = re.match(r"\s*([+-]?\d+)", text)
      v = int(m.group(1)) if m else 0
      if v in allowed(key, self.NP):
        self._store(key, v)
    return self


# --- the rules --------------------------------------------------------------------------------
SWEEP_MAX_STEPS, PSWEEP_MAX_STEPS = 40, 32


def rec_fwd_width(s):
  return s.rec_tile_width_fwd or s.rec_tile_width


def rec_cap(s, m, w):
  """Record steps per launch the tiles of width w can run for a request m."""
  if s.rec_lane_elems == 2:  # pair tiles: 16 and 20 need 1024-element tiles
    if w == 1 and m > 10:
      return 8 if m == 16 else 10
    return m
  m = max(q for q in (1, 2, 4, 8) if q <= m)  # one element per lane: 1, 2, 4, 8
  if m == 8 and w == 1:
    m = 4
  return min(m, 2) if s.NP > 8 else m


def rec_steps(s):
  return rec_cap(s, s.rec_msteps, s.rec_tile_width)


def rec_steps_fwd(s):
  m = s.rec_msteps_fwd
  if m < 0:  # by size
    m = 20 if (s.rec_lane_elems == 2 and rec_fwd_width(s) == 2 and s.ktot <= 3 * 2**20) \
        else s.rec_msteps
  return rec_cap(s, m or s.rec_msteps, rec_fwd_width(s))


def fwd_steps(s, msteps=None, lane_elems=None):
  """Steps per launch of the snapshot forward (dg_plan_query out[7])."""
  m = s.msteps if msteps is None else msteps
  e = s.lane_elems if lane_elems is None else lane_elems
  if m == 8 and (e == 2 or not (s.tile_width == 2 or e == 8)):
    m = 4
  return min(m, 2) if s.NP > 8 else m


def nl_steps(s, snapshots):
  return 2 if (s.msteps == 2 or (s.msteps > 2 and not snapshots and not s.nl_exchange)) else 1


def sweep_tile(s, waves):
  return waves * 116 + 12 if s.sweep_exchange == 1 else 64 * s.sweep_lane_elems * waves


def sweep_blocks(s):
  """(tiles and blocks fit, waves, forward steps per block, adjoint steps per block)."""
  f, a, w, NP = rec_steps_fwd(s), rec_steps(s), s.rec_tile_width, s.NP
  big = f >= 10 and a == 10
  nw = s.sweep_waves
  if nw:
    ok = nw in (4, 8) or ((nw == 12 or (nw == 16 and NP <= 5)) and big)
  elif NP == 9 and s.uniform:
    nw, ok = 8, True
  else:
    nw, ok = 4 * w, rec_fwd_width(s) == w and w in (1, 2)
    if ok and w == 2 and s.uniform and 3 <= NP <= 5 and s.sweep_lane_elems == 2 and big:
      nw = 12
  ok = ok and (s.sweep_lane_elems == 2 or (NP <= 3 and nw in (4, 8)))
  if s.sweep_exchange == 1:
    ok = ok and s.sweep_lane_elems == 2 and (nw in (8, 12) or (nw == 16 and NP <= 5)) and big
  ok = ok and bool(s.rec_sweep) and s.rec_lane_elems == 2 and \
      (f in (5, 10) or (f == 20 and sweep_tile(s, nw) >= 900)) and a in (5, 10)
  return ok, nw, f, a


def ceil_div(n, d):
  return -(-n // d)


def sweep_query(s, nsteps, blocks=None):
  """(on, msf, msa, items, waves, tile elements, adjoint tiles of one block)."""
  ok, nw, f, a = blocks or sweep_blocks(s)
  on = ok and nsteps > 0 and nsteps % f == 0 and nsteps % a == 0 and nsteps <= SWEEP_MAX_STEPS
  T = sweep_tile(s, nw)
  tf, ta = T - 2 * ((5 * f + 2) & ~1), T - 2 * ((5 * a + 1) & ~1)
  items = 0
  if on:
    items = (nsteps // f) * ceil_div(s.ktot, tf) + (nsteps // a) * ceil_div(s.ktot, ta)
  return int(on), f, a, items, nw, T, tf, ta


def p_steps(s):
  return 4 if (s.p_msteps == 8 and s.p_tile_width != 2) else s.p_msteps


def p_flow(s, nsteps, horner=3):
  m = p_steps(s)
  return bool(s.p_flow) and horner in (1, 3) and (m == 4 or (m == 8 and s.p_tile_width == 2)) \
      and nsteps > 0 and nsteps % m == 0 and nsteps // m >= 2 and nsteps <= SWEEP_MAX_STEPS


def p_sweep(s, nsteps, horner=3):
  return bool(s.p_sweep) and p_flow(s, nsteps, horner) and p_steps(s) == 4 and \
      s.lane_elems == 0 and s.nstages == 5 and nsteps <= PSWEEP_MAX_STEPS


def p_extent(s, m):
  return 256 * s.p_tile_width - 10 * m


def p_trace(s, nsteps, horner=3):
  """(work items of the estimate's dataflow launch, of the one-launch sweep)."""
  m = p_steps(s)
  return ((nsteps // m) * ceil_div(s.ktot, p_extent(s, m)) if p_flow(s, nsteps, horner) else 0,
          2 * (nsteps // 4) * ceil_div(s.ktot, p_extent(s, 4)) if p_sweep(s, nsteps, horner)
          else 0)


def sweep_occupancy(s, waves):
  """dg_plan_query_sweep_kernel out[7]: the dataflow kernel's occupancy target in waves per
  SIMD (0: none) -- 8 at Np = 2 on 4- or 8-wave (overlapped: also 16-wave) workgroups of a
  uniform mesh, 6 on the other uniform meshes at Np <= 5, pair tiles only."""
  if s.sweep_lane_elems != 2 or not s.uniform or s.NP > 5 or waves not in (4, 8, 12, 16):
    return 0
  if waves == 4 and s.sweep_exchange:
    return 0
  if s.NP == 2 and (waves in (4, 8) or (s.sweep_exchange == 1 and waves == 16)):
    return 8
  return 6
