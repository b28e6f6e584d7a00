"""Helpers of tests/test_gpu_tile_edges.py: the owned extents of every tile family computed
from what the plan reports, the element counts that sit on their boundaries, sentinel-guarded
output buffers, and the numpy oracle of a whole batch (cached per input set).

Every stepper in csrc/ works on tiles of T elements with a halo of H per side and writes back
TE = T - 2*H owned elements; its grid is grid_for(batch*K, TE).  The helpers below restate
that formula per family from the plan's queries (never from literals of the test), so that a
count named "TE+1" really is one element past a tile: where the library reports work items
the restated formula is checked against them (``check_items``), and a mismatch fails with
"tile geometry changed" instead of silently running off-boundary counts.
"""
import ctypes
import math
import os
import re

import numpy as np

from oracle import adjoint as oadj
from oracle import advec as oadv
from oracle import setup1d

RTOL = 1e-10          # the project's parity bar (tests/test_gpu_parity.py)
SENTINEL = 1.25e300   # finite, so that `==` sees every overwritten guard word
GUARD = 2048          # doubles on either side of every output: more than one tile's row


class GeometryChanged(AssertionError):
  pass


def geometry_fail(what):
  raise GeometryChanged(f"tile geometry changed: {what}")


def grid_for(n, per):
  return (n + per - 1) // per  # grid_for, csrc/dg_shape.h


# --- owned extents (TE, H) per family, from the plan ----------------------------------
def _q(op, name, n, *args):
  out = (ctypes.c_int64 * n)()
  rc = getattr(op._lib, name)(op._plan, *args, out)
  assert rc == 0, name
  return [int(v) for v in out]


def stage_loop_extents(op, rec=False):
  """k_step / k_adj on workgroup tiles of 256*W lanes, one element per lane: H = 5*MS (+1 with
  the jump record), the same in both directions (csrc/dg_advec.hip:761 forward, :790 adjoint)."""
  q = _q(op, "dg_plan_query", 8)
  W, MS = q[6], q[7]
  H = 5 * MS + (1 if rec else 0)
  return [(256 * W - 2 * H, H)] * 2


def wave_extents(op, lane_elements):
  """k_wstep on one-wave tiles of 64*E elements: H = 5*MS (csrc/dg_wave.hip:36-38, :230).  The
  plan does not report E (DG_TUNE_LANE_ELEMENTS), the caller passes what it tuned."""
  MS = _q(op, "dg_plan_query", 8)[7]
  return [(64 * lane_elements - 10 * MS, 5 * MS)]


def halo_f(ms):
  return (5 * ms + 2) & ~1  # RpHalo<MS>::F, csrc/dg_rec_tiles.h:49


def halo_a(ms):
  return (5 * ms + 1) & ~1  # RpHalo<MS>::A, csrc/dg_rec_tiles.h:50


def snap_pair_extents(op):
  """k_step_rps on pair tiles of 512*W elements: H = RpHalo<MS>::F (csrc/dg_rec.hip:118)."""
  q = _q(op, "dg_plan_query", 8)
  W, MS = q[6], q[7]
  return [(512 * W - 2 * halo_f(MS), halo_f(MS))]


def record_extents(op):
  """forward_rec / adjoint_rec.  Pair tiles (2 elements per lane): T = 512 * width, forward
  H = RpHalo<MSF>::F on the forward's width, adjoint H = RpHalo<MSA>::A (csrc/dg_rec.hip:138,
  :157).  One element per lane: the stage-loop record kernels; only the forward takes the
  record's extra element, H = 5*MS + 1 (csrc/dg_advec.hip:761, csrc/dg_step_tile.h:67), the
  adjoint keeps H = 5*MS with the record too (csrc/dg_advec.hip:790, adj_tile :92-93)."""
  w, msa, lanes, msf = _q(op, "dg_plan_query_rec", 4)
  wf, msf2 = _q(op, "dg_plan_query_rec_fwd", 2)
  if msf2 != msf:
    geometry_fail(f"forward record steps {msf} / {msf2}")
  if lanes == 2:
    return [(512 * wf - 2 * halo_f(msf), halo_f(msf)), (512 * w - 2 * halo_a(msa), halo_a(msa))]
  return [(256 * wf - 2 * (5 * msf + 1), 5 * msf + 1), (256 * w - 10 * msa, 5 * msa)]


def sweep_query(op, nsteps):
  """(dataflow, msf, msa, items, waves, elements per tile) of dg_plan_query_sweep_ex."""
  return _q(op, "dg_plan_query_sweep_ex", 6, int(nsteps))


def sweep_extents(op, nsteps):
  """The dataflow launch: both directions on tiles of T elements (128 * waves, 256 * waves
  with 4 elements per lane, 116 * waves + 12 on overlapped waves, csrc/dg_ovl_tiles.h:40), TEF
  = T - 2*RpHalo<MSF>::F, TEA = T - 2*RpHalo<MSA>::A (csrc/dg_sweep_kernel.h:107-108, :309)."""
  on, msf, msa, _, _, T = sweep_query(op, nsteps)
  assert on, "this shape does not run as the dataflow launch"
  return [(T - 2 * halo_f(msf), halo_f(msf)), (T - 2 * halo_a(msa), halo_a(msa))]


def check_sweep_items(op, nsteps, ext):
  """dg_plan_query_sweep out[3] = nbF*nTF + nbA*nTA with the restated extents."""
  on, msf, msa, items, _, _ = sweep_query(op, nsteps)
  want = (nsteps // msf) * grid_for(op.ktot, ext[0][0]) + (nsteps // msa) * grid_for(op.ktot, ext[1][0])
  if not on or items != want:
    geometry_fail(f"dataflow sweep reports {items} work items at batch*K = {op.ktot}, the "
                  f"restated extents {ext} give {want}")
  return nsteps // msf, nsteps // msa


def p_extents(op):
  """adjp / adjp_flow / psweep on tiles of 256*W lanes, one element per lane: H = 5*MS
  (csrc/dg_dwr.hip:394, :484; the host side p_tiles, csrc/dg_shape.h; the psweep's blocks are 4
  steps)."""
  W, MS = _q(op, "dg_plan_query_p", 2)
  return [(256 * W - 10 * MS, 5 * MS)]


def p_items(op, nsteps):
  return _q(op, "dg_plan_query_p_trace", 3, int(nsteps))[:2]


def check_p_items(op, nsteps, ext, flow, sweep):
  """dg_plan_query_p_trace out[0] = nb * nT (the dataflow estimate), out[1] = 2 * (nsteps/4) *
  nT at 4-step blocks (the whole sweep)."""
  MS = _q(op, "dg_plan_query_p", 2)[1]
  got = p_items(op, nsteps)
  nT = grid_for(op.ktot, ext[0][0])
  if flow and got[0] != (nsteps // MS) * nT:
    geometry_fail(f"p flow reports {got[0]} items at batch*K = {op.ktot}, extents {ext} give "
                  f"{(nsteps // MS) * nT}")
  if sweep and got[1] != 2 * (nsteps // 4) * nT:
    geometry_fail(f"p sweep reports {got[1]} items at batch*K = {op.ktot}, extents {ext} give "
                  f"{2 * (nsteps // 4) * nT}")


CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    "adjoint-ode-adaptivity_amd", "csrc")
_CONSTANTS = {}


def source_constant(name, file, pattern=None):
  """An integer constant of the kernels' source that no query reports (the config-3 and limiter
  tile shapes), read from csrc/ so that a change there moves the counts with it -- or fails
  here when the definition is no longer found."""
  if name not in _CONSTANTS:
    with open(os.path.join(CSRC, file)) as f:
      m = re.search(pattern or rf"\b{name}\s*=\s*(\d+)\s*[,;]", f.read())
    if not m:
      geometry_fail(f"{name} not found in csrc/{file}")
    _CONSTANTS[name] = int(m.group(1))
  return _CONSTANTS[name]


def limiter_extents():
  """k_limit (slope_limit, slope_limit_1): tiles of kBlock lanes with H = 1, TE = kBlock - 2
  (csrc/dg_advec.hip:407-408; launches grid_for(ktot, kBlock - 2), :1634, :1648)."""
  H = source_constant("k_limit H", "dg_advec.hip",
                      r"constexpr int H = (\d+);\s*constexpr int TE = kBlock - 2 \* H;")
  return [(source_constant("kBlock", "dg_common.h") - 2 * H, H)]


def nl_extents(op, snapshots, known):
  """Config 3.  Forward: workgroup tiles of 256*kNLStepW = 512 elements, H = MS*5*cone (cone =
  cone_per_stage<LIM> = 2 with a limiter, csrc/dg_burgers.hip:391), or with nl_exchange = 1 (one
  step per launch) 4 windows of S = 64 - 2*G owned elements, G = 5*cone, TE = kOwWaves * S
  (csrc/dg_burgers_ov.hip:47-51, :345).  Adjoint: 256*kNLAdjW = 256-element tiles with H = 10
  with the decision record and 10*cone without (csrc/dg_burgers.hip:411; k_adj_nl works on
  half tiles TH = TE/2, :290), or on overlapped waves (record or no limiter) G = kOwAdjG = 10:
  TE = 4 * 44 (csrc/dg_burgers_ov.hip:214, :363).  The constants are read from csrc/
  (``source_constant``): no query reports them.  With ``snapshots`` a third entry gives the
  forward without snapshots where its steps per launch differ (nl_msteps, csrc/dg_shape.h)."""
  ex, ms_snap, ms_plain = _q(op, "dg_plan_query_nl", 3)
  kBlock = source_constant("kBlock", "dg_common.h")
  step_w = source_constant("kNLStepW", "dg_burgers.hip")
  adj_w = source_constant("kNLAdjW", "dg_burgers.hip")
  windows = source_constant("kOwTileWindows", "dg_nl.h")  # = kOwWaves, csrc/dg_burgers_ov.hip:40
  adj_g = source_constant("kOwAdjG", "dg_burgers_ov.hip")
  lim_cone = source_constant("cone_per_stage", "dg_nl.h",
                             r"cone_per_stage\(\)\s*\{\s*return LIM \? (\d+) : 1;")
  cone = lim_cone if op.limiter else 1

  def forward(MS):
    if ex and MS == 1:
      G = 5 * cone
      return (windows * (64 - 2 * G), G)
    return (kBlock * step_w - 2 * MS * 5 * cone, MS * 5 * cone)

  if ex and (known or not op.limiter):
    adj = (windows * (64 - 2 * adj_g), adj_g)
  else:
    H = 10 if (known and op.limiter) else 10 * cone
    adj = (kBlock * adj_w - 2 * H, H)
  ext = [forward(ms_snap if snapshots else ms_plain), adj]
  if snapshots and ms_plain != ms_snap:
    ext.append(forward(ms_plain))  # the forward without snapshots (2 steps per launch)
  return ext


# --- the element counts -----------------------------------------------------------------
BOUNDARY = ("TE-1", "TE", "TE+1", "TE+2", "2TE-1", "2TE", "2TE+1")
TINY = ("2", "3", "H-1", "H", "H+1", "2H+1")
EDGES = ("TEx3", "TE-1x3", "TE+1x2", "TE/2x5", "3xmany")
HALF = ("TH-1", "TH", "TH+1")  # k_adj_nl's half tile
LABELS = BOUNDARY + TINY + EDGES


def count_of(label, TE, H):
  """(K, batch) of a count label for one direction's extents; None below 2 elements."""
  table = {
      "TE-1": (TE - 1, 1), "TE": (TE, 1), "TE+1": (TE + 1, 1), "TE+2": (TE + 2, 1),
      "2TE-1": (2 * TE - 1, 1), "2TE": (2 * TE, 1), "2TE+1": (2 * TE + 1, 1),
      "2": (2, 1), "3": (3, 1), "H-1": (H - 1, 1), "H": (H, 1), "H+1": (H + 1, 1),
      "2H+1": (2 * H + 1, 1),
      "TEx3": (TE, 3), "TE-1x3": (TE - 1, 3), "TE+1x2": (TE + 1, 2), "TE/2x5": (TE // 2, 5),
      "3xmany": (3, math.ceil((TE + H) / 3) + 1),
      "TH-1": (TE // 2 - 1, 1), "TH": (TE // 2, 1), "TH+1": (TE // 2 + 1, 1),
  }
  K, batch = table[label]
  return (K, batch) if K >= 2 else None


def counts_of(label, extents):
  """The distinct (K, batch) of a label over a family's directions (forward, adjoint)."""
  out = []
  for TE, H in extents:
    c = count_of(label, TE, H)
    if c is not None and c not in out:
      out.append(c)
  return out


def uniform_for(label):
  """Half of the counts on a uniform mesh, half on a random non-uniform one."""
  labels = LABELS + HALF
  return labels.index(label) % 2 == 0


def make_vx(K, uniform, seed, x0=0.0, x1=1.0):
  if uniform:
    return setup1d.mesh_gen1d(x0, x1, K)[1]
  rng = np.random.default_rng(seed)
  v = np.concatenate(([0.0], np.cumsum(rng.uniform(0.5, 1.5, K))))
  v = x0 + (x1 - x0) * v / v[-1]
  v[0], v[-1] = x0, x1
  return v


# --- guarded buffers ----------------------------------------------------------------------
class Arena:
  """Outputs as 16-byte-aligned slices from the middle of larger sentinel-filled tensors."""

  def __init__(self, device):
    self.device = device
    self.bufs = []

  def new(self, *shape, dtype=None):
    import torch
    dtype = torch.float64 if dtype is None else dtype
    n = int(np.prod(shape))
    big = torch.empty(n + 2 * GUARD, dtype=dtype, device=self.device)
    fill = SENTINEL if dtype == torch.float64 else 0x5a5a
    big.fill_(fill)
    t = big[GUARD:GUARD + n]
    assert t.data_ptr() % 16 == 0
    self.bufs.append((big, n, fill))
    return t.view(*shape)

  def check(self):
    """Both guard regions of every buffer still hold the sentinel."""
    import torch
    torch.cuda.synchronize()
    for i, (big, n, fill) in enumerate(self.bufs):
      lo, hi = big[:GUARD], big[GUARD + n:]
      assert bool((lo == fill).all()), f"buffer {i}: written before its start"
      assert bool((hi == fill).all()), f"buffer {i}: written past its end"


def host(t):
  return t.detach().cpu().numpy()


def rel_err(x, ref):
  x, ref = np.asarray(x), np.asarray(ref)
  return float(np.max(np.abs(x - ref)) / max(np.max(np.abs(ref)), 1e-300))


def close(x, ref, what, rtol=RTOL):
  err = rel_err(x, ref)
  print(f"  {what}: {err:.3e}")
  assert err <= rtol, (what, err)


# --- the numpy oracle of a whole batch ---------------------------------------------------
def batched_setup(N, v_x, batch):
  """oracle.setup1d.startup1d of ``batch`` copies of the mesh side by side: the oracle's own
  operators (they go through vmapM / vmapP / mapI / mapO) then step every trajectory at once,
  each with its own inflow and outflow face."""
  S1 = setup1d.startup1d(N, v_x, metric="element")
  if batch == 1:
    return S1
  K, Np = S1["K"], S1["Np"]
  S = dict(S1)
  S["K"] = K * batch
  for key in ("x", "rx", "J", "nx", "Fscale", "Fx"):
    S[key] = np.tile(S1[key], (1, batch))
  offs = np.repeat(np.arange(batch) * K * Np, 2 * K)
  S["vmapM"] = np.tile(S1["vmapM"], batch) + offs
  S["vmapP"] = np.tile(S1["vmapP"], batch) + offs
  S["mapI"] = np.arange(batch) * 2 * K
  S["mapO"] = np.arange(batch) * 2 * K + 2 * K - 1
  S["vmapI"] = np.arange(batch) * K * Np
  S["vmapO"] = np.arange(batch) * K * Np + K * Np - 1
  for key in ("matlab", "EToE", "EToF", "EToV", "VX", "vmapB", "mapB"):
    S.pop(key, None)
  return S


def times_of(t0, dt, nsteps):
  t = [t0]
  for _ in range(nsteps):
    t.append(t[-1] + dt)  # time = time + dt, One_code.mlx:139
  return t


def raw_jumps(u, K, batch, uin):
  """The recorded left-face jump u_0 - (left neighbour's u_N, or the inflow value) per element
  of an (Np, batch*K) field."""
  left = np.concatenate(([0.0], u[-1, :-1]))
  left[np.arange(batch) * K] = uin
  return u[0] - left


_ORACLE = {}


def linear_oracle(key, N, v_x, batch, a, inflow, t0, dt, nsteps, u0_em, adjoint=True):
  """Forward states, the record, and (terminal weight u^N, J = |u^N|^2/2) w^0 and eta of the
  linear LSERK4 sweep, on the oracle's own forward states; cached per input set ``key`` and
  read-only."""
  key = (key, bool(adjoint))
  if key in _ORACLE:
    return _ORACLE[key]
  S = batched_setup(N, v_x, batch)
  K = len(v_x) - 1
  u0 = setup1d.from_elem_major(np.asarray(u0_em), N + 1)
  snaps, times = oadv.forward_sweep(u0, t0, dt, nsteps, a, S, inflow)
  rec = np.stack([raw_jumps(snaps[n], K, batch, oadv.inflow_value(a, times[n], inflow))
                  for n in range(1, nsteps + 1)]) if nsteps else np.zeros((0, K * batch))
  out = dict(S=S, times=times, snaps=[setup1d.to_elem_major(s) for s in snaps], rec=rec)
  if adjoint:
    w0, eta, _ = oadj.adjoint_sweep(snaps[-1], snaps, times, dt, a, S, inflow)
    out["w0"], out["eta"] = setup1d.to_elem_major(w0), eta
  for v in out.values():
    if isinstance(v, np.ndarray):
      v.setflags(write=False)
  for s in out["snaps"]:
    s.setflags(write=False)
  _ORACLE[key] = out
  return out


def rough_state(op, seed):
  """tests/test_gpu_rec.noisy_sine: sines plus per-node noise of 0.1 (O(0.1) jumps)."""
  import test_gpu_rec
  return test_gpu_rec.noisy_sine(op, seed, op.batch)


def bench_dt(N, v_x, a):
  S = setup1d.startup1d(N, v_x, metric="element")
  return oadv.bench_dt(S) * 2 * np.pi / a
