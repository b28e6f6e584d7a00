"""Every DG tile family at the element counts where its tiling changes.

Each stepper works on tiles of T elements with a halo of H per side, writes back TE = T - 2*H
owned elements and launches grid_for(batch*K, TE) tiles.  tests/tile_edges.py restates TE and H
per family from the plan's queries; every family below then runs at

  * the boundaries K = TE-1, TE, TE+1, TE+2, 2TE-1, 2TE, 2TE+1 (batch 1), for a family whose
    directions have different extents (TEF / TEA) at both directions' counts;
  * tiny meshes K = 2, 3, H-1, H, H+1, 2H+1 (shorter than a halo);
  * trajectory edges on tile edges: (K, batch) = (TE, 3), (TE-1, 3), (TE+1, 2), (TE/2, 5) and
    many three-element trajectories across a tile edge;
  * a refine walk across a boundary (test_refine_walk_*), and one boundary count off the
    suite's single parameter point (a = 1.3, mesh on [-0.7, 2.1], t0 = 3.7, inflow "a2");

alternating uniform and random non-uniform meshes (UNI = false is its own instantiation).

Every case is compared with the numpy oracle (oracle/advec.py, adjoint.py, burgers.py,
effectivity.p_estimate) at the project's 1e-10 of max|ref| on rough states (jumps of O(0.1), so
the indicator is well conditioned and the linear oracle runs on its own forward states); with
the sibling path where the header promises equality (dataflow = launch chains bit for bit,
record pair tiles = one element per lane at equal steps to test_gpu_rec.HORNER_RTOL); and every
output lives in the middle of a sentinel-filled tensor whose guards, and the record's pad entry
of an odd batch*K, must still hold the sentinel afterwards.  Where the library reports work
items the restated extents are checked against them in every case ("tile geometry changed").
"""
import numpy as np
import pytest

import tile_edges as te
from oracle import advec as oadv
from oracle import burgers as ob
from oracle import effectivity as oef
from oracle import limiter as olim
from oracle import setup1d
from test_gpu_rec import HORNER_RTOL

pytestmark = pytest.mark.gpu

TWO_PI = 2 * np.pi
HOME = dict(a=TWO_PI, x0=0.0, x1=1.0, t0=0.02, inflow="a")
AWAY = dict(a=1.3, x0=-0.7, x1=2.1, t0=3.7, inflow="a2")  # off the suite's one parameter point


def ids(shapes):
  return ["-".join(str(v) for v in s) for s in shapes]


def make_op(pkg, N, K, batch, uniform, point, **kw):
  v_x = te.make_vx(K, uniform, 1000 * N + K, point["x0"], point["x1"])
  mesh = pkg.BaseGalerkin1D(n=N, v_x=v_x)
  op = pkg.operators.DGAdvection1D(mesh, a=point["a"], batch=batch,
                                   inflow=kw.pop("inflow", point["inflow"]), **kw)
  assert op.uniform == (uniform or K == 1)
  return op, v_x


def fill(arena, src):
  t = arena.new(*src.shape)
  t.copy_(src)
  return t


def pad_intact(rec, ktot):
  """The header's promise: the record's pad entry of an odd batch*K "is not written"."""
  if rec.shape[1] != ktot:
    assert bool((rec[:, ktot:] == te.SENTINEL).all()), "the record's pad entry was written"


def check_record(rec, ktot, ref, umax):
  """The record against the oracle's jumps, and the pad entry of an odd batch*K untouched."""
  R = te.host(rec)
  err = float(np.max(np.abs(R[:, :ktot] - ref))) / umax if ref.size else 0.0
  print(f"  record: {err:.3e}")
  assert err <= te.RTOL, ("record", err)
  if R.shape[1] != ktot:
    assert np.all(R[:, ktot:] == te.SENTINEL), "the record's pad entry was written"


def check_linear(got, ora, op):
  umax = float(np.abs(ora["snaps"][0]).max())
  if "uN" in got:
    te.close(te.host(got["uN"]), ora["snaps"][-1], "u^N")
  if "snaps" in got:
    S = te.host(got["snaps"])
    for n, ref in enumerate(ora["snaps"]):
      assert te.rel_err(S[n], ref) <= te.RTOL, ("snapshot", n, te.rel_err(S[n], ref))
  if "rec" in got:
    check_record(got["rec"], op.ktot, ora["rec"], umax)
  if "w" in got:
    te.close(te.host(got["w"]), ora["w0"], "w^0")
  if "eta" in got:
    te.close(te.host(got["eta"]), ora["eta"], "eta")


# ---------------------------------------------------------------------------
# The linear families: (tune, extents, nsteps, run)
# ---------------------------------------------------------------------------
class StageLoop:
  """forward / adjoint on the stage-loop workgroup tiles.  shape = (N, W, MS)."""
  adjoint = True

  @staticmethod
  def tune(op, shape):
    _, W, MS = shape
    op.tune(tile_width=W, steps_per_launch=MS, lane_elements=0, snap_pairs=0)
    assert op.tile_width == W and op.steps_per_launch == (min(MS, 2) if op.N == 8 else MS)

  @staticmethod
  def extents(op, shape):
    return te.stage_loop_extents(op)

  @staticmethod
  def nsteps(op, shape):
    return 2 * op.steps_per_launch

  @staticmethod
  def run(op, shape, arena, u0, t0, dt, nsteps):
    u = fill(arena, u0)
    snaps = arena.new(nsteps + 1, op.field_numel)
    op.forward(u, t0, dt, nsteps, snaps)
    plain = fill(arena, u0)  # the ping-pong forward (no snapshots)
    op.forward(plain, t0, dt, nsteps)
    w = fill(arena, snaps[nsteps])
    eta = arena.new(op.ktot)
    keep = snaps.clone()
    op.adjoint(w, snaps, t0, dt, nsteps, eta=eta, eta_assign=True)
    assert bool((snaps == keep).all()), "adjoint wrote the snapshots"
    assert te.rel_err(te.host(plain), te.host(u)) <= 1e-12
    return dict(uN=u, snaps=snaps, w=w, eta=eta)


class Wave:
  """forward on one-wave tiles.  shape = (N, E, MS)."""
  adjoint = False

  @staticmethod
  def tune(op, shape):
    _, E, MS = shape
    op.tune(tile_width=1, steps_per_launch=MS, lane_elements=E, snap_pairs=0)
    assert op.steps_per_launch == MS  # a step count the plan accepts for this tile

  @staticmethod
  def extents(op, shape):
    return te.wave_extents(op, shape[1])

  @staticmethod
  def nsteps(op, shape):
    return 2 * op.steps_per_launch

  @staticmethod
  def run(op, shape, arena, u0, t0, dt, nsteps):
    u = fill(arena, u0)
    snaps = arena.new(nsteps + 1, op.field_numel)
    op.forward(u, t0, dt, nsteps, snaps)
    plain = fill(arena, u0)
    op.forward(plain, t0, dt, nsteps)
    assert te.rel_err(te.host(plain), te.host(u)) <= 1e-12
    return dict(uN=u, snaps=snaps)


class SnapPairs:
  """forward with snapshots on Horner-form pair tiles.  shape = (N, tw, ms)."""
  adjoint = False

  @staticmethod
  def tune(op, shape):
    _, tw, ms = shape
    op.tune(tile_width=tw, steps_per_launch=ms, lane_elements=0, snap_pairs=1)
    assert (op.tile_width, op.steps_per_launch) == (tw, ms)

  @staticmethod
  def extents(op, shape):
    return te.snap_pair_extents(op)

  @staticmethod
  def nsteps(op, shape):
    return 2 * op.steps_per_launch

  @staticmethod
  def run(op, shape, arena, u0, t0, dt, nsteps):
    u = fill(arena, u0)
    snaps = arena.new(nsteps + 1, op.field_numel)
    op.forward(u, t0, dt, nsteps, snaps)
    return dict(uN=u, snaps=snaps)


def record_pair(op, arena, u0, t0, dt, nsteps):
  u0g = fill(arena, u0)
  rec = arena.new(nsteps, op.jump_ld)
  uN = arena.new(op.field_numel)
  op.forward_rec(u0g, t0, dt, nsteps, rec, out=uN)
  w = fill(arena, uN)
  eta = arena.new(op.ktot)
  op.adjoint_rec(w, rec, t0, dt, nsteps, eta=eta, eta_assign=True)
  arena.check()
  pad_intact(rec, op.ktot)
  assert bool((u0g == u0).all()), "forward_rec wrote its input"
  return dict(uN=uN, rec=rec, w=w, eta=eta)


class Record:
  """forward_rec / adjoint_rec.  shape = (N, lanes, rtw, spl)."""
  adjoint = True

  @staticmethod
  def tune(op, shape):
    _, lanes, rtw, spl = shape
    op.tune(rec_tile_width=rtw, rec_steps_per_launch=spl, rec_lane_elements=lanes, rec_sweep=0)
    assert (op.rec_tile_width, op.rec_fwd_tile_width, op.rec_lane_elements) == (rtw, rtw, lanes)
    if lanes == 2:
      assert op.rec_steps_per_launch == op.rec_fwd_steps_per_launch == spl

  @staticmethod
  def extents(op, shape):
    return te.record_extents(op)

  @staticmethod
  def nsteps(op, shape):
    return 2 * op.rec_steps_per_launch

  @staticmethod
  def run(op, shape, arena, u0, t0, dt, nsteps):
    got = record_pair(op, arena, u0, t0, dt, nsteps)
    if shape[1] == 1:
      # the header's promise: two elements per lane equal one at equal steps per launch
      # (the bar of test_gpu_rec.test_pair_tiles_equal_one_element_per_lane)
      op.tune(rec_lane_elements=2, rec_steps_per_launch=op.rec_steps_per_launch)
      pair = record_pair(op, arena, u0, t0, dt, nsteps)
      umax = float(np.abs(te.host(u0)).max())
      err = float(np.max(np.abs(te.host(pair["rec"])[:, :op.ktot] -
                                te.host(got["rec"])[:, :op.ktot]))) / umax
      assert err <= HORNER_RTOL, ("record, pair tiles vs one element per lane", err)
      for k in ("uN", "w", "eta"):
        te.close(te.host(pair[k]), te.host(got[k]), f"{k}: pair tiles vs one element per lane",
                 HORNER_RTOL)
    return got


def sweep_once(op, arena, u0, t0, dt, nsteps):
  u0g = fill(arena, u0)
  rec = arena.new(nsteps, op.jump_ld)
  uN = arena.new(op.field_numel)
  w = arena.new(op.field_numel)
  eta = arena.new(op.ktot)
  op.sweep_rec(u0g, rec, w, t0, dt, nsteps, uN=uN, eta=eta, eta_assign=True)
  arena.check()
  pad_intact(rec, op.ktot)
  assert bool((u0g == u0).all()), "sweep_rec wrote its input"
  return dict(uN=uN, rec=rec, w=w, eta=eta)


class Dataflow:
  """sweep_rec / sweep_refine as one dataflow launch.
  shape = (N, waves, msf, msa, lane elements, exchange, nsteps)."""
  adjoint = True

  @staticmethod
  def tune(op, shape):
    _, waves, msf, msa, E, X, _ = shape
    op.tune(rec_tile_width=2, rec_steps_per_launch=msa, rec_fwd_steps_per_launch=msf,
            rec_lane_elements=2, rec_sweep=1, sweep_waves=waves, sweep_lane_elements=E,
            sweep_exchange=X)
    q = te.sweep_query(op, shape[6])
    assert q[0] == 1 and (q[1], q[2], q[4]) == (msf, msa, waves), q

  @staticmethod
  def extents(op, shape):
    return te.sweep_extents(op, shape[6])

  _stepped = set()

  @staticmethod
  def geometry(pkg, shape, ext, point):
    """Once per shape: from batch*K = m*TE to m*TE + 1 the launch's work items grow by exactly
    that direction's number of blocks (plus the other direction's where its boundary is the
    same count)."""
    if shape in Dataflow._stepped:
      return
    nsteps = shape[6]
    blocks = (nsteps // shape[2], nsteps // shape[3])
    for d in (0, 1):
      for m in (1, 2):
        n = m * ext[d][0]
        items = []
        for K in (n, n + 1):
          op, _ = make_op(pkg, shape[0], K, 1, True, point)
          Dataflow.tune(op, shape)
          items.append(te.sweep_query(op, nsteps)[3])
          op.close()
        want = blocks[d] + (blocks[1 - d] if n % ext[1 - d][0] == 0 else 0)
        if items[1] - items[0] != want:
          te.geometry_fail(f"dataflow items {items} at batch*K = {n}, {n + 1}: a step of {want} "
                           f"expected for extents {ext}")
    Dataflow._stepped.add(shape)

  @staticmethod
  def nsteps(op, shape):
    return shape[6]

  @staticmethod
  def run(op, shape, arena, u0, t0, dt, nsteps):
    import torch
    ext = te.sweep_extents(op, nsteps)
    te.check_sweep_items(op, nsteps, ext)
    got = sweep_once(op, arena, u0, t0, dt, nsteps)
    assert op.sweep_status() == 0, "a work item gave up waiting for a producer"
    # the fused refine decision (|eta| assigned), same launch shape
    w2, eta2 = arena.new(op.field_numel), arena.new(op.ktot)
    rec2 = arena.new(nsteps, op.jump_ld)
    res = arena.new(4, dtype=torch.int64)
    res.zero_()
    u0g = fill(arena, u0)
    op.sweep_refine(u0g, rec2, w2, t0, dt, nsteps, eta2, res[0:1], res[1:2].view(torch.float64),
                    res[2:3])
    arena.check()
    pad_intact(rec2, op.ktot)
    assert bool((u0g == u0).all()), "sweep_refine wrote its input"
    assert op.sweep_status() == 0
    np.testing.assert_array_equal(te.host(w2), te.host(got["w"]))
    np.testing.assert_array_equal(te.host(eta2), np.abs(te.host(got["eta"])))
    got["idx"] = int(te.host(res)[0])
    assert int(te.host(res)[2]) == 0
    # the header's promise: bit-identical to the two launch chains
    op.tune(rec_sweep=0)
    assert te.sweep_query(op, nsteps)[0] == 0
    chain = sweep_once(op, arena, u0, t0, dt, nsteps)
    op.tune(rec_sweep=1)
    for k in ("uN", "w", "eta"):
      np.testing.assert_array_equal(te.host(got[k]), te.host(chain[k]), err_msg=f"{k}: dataflow vs chains")
    np.testing.assert_array_equal(te.host(got["rec"])[:, :op.ktot],
                                  te.host(chain["rec"])[:, :op.ktot], err_msg="record")
    return got


def check_refine_index(idx, eta_ref):
  """sweep_refine's index is the oracle's argmax |eta| whenever the oracle's top two differ by
  more than 2e-10 relative -- which must hold for the chosen seeds."""
  mag = np.abs(eta_ref)
  top = np.sort(mag)[::-1]
  if top.size > 1:
    assert top[0] - top[1] > 2e-10 * top[0], "seed gives a tie: choose another"
  assert idx == int(np.argmax(mag)), (idx, int(np.argmax(mag)))


def drive(pkg, gpu, fam, shape, label, point=HOME):
  """One count label of a family's shape: every distinct (K, batch) of its directions."""
  N = shape[0]
  probe, _ = make_op(pkg, N, 8, 1, True, point)
  fam.tune(probe, shape)
  ext = fam.extents(probe, shape)
  probe.close()
  if hasattr(fam, "geometry"):
    fam.geometry(pkg, shape, ext, point)
  counts = te.counts_of(label, ext)
  assert counts or label in te.TINY
  for K, batch in counts:
    uniform = te.uniform_for(label)
    print(f"{fam.__name__} {shape} {label}: K={K} batch={batch} uniform={uniform} extents={ext}")
    op, v_x = make_op(pkg, N, K, batch, uniform, point)
    fam.tune(op, shape)
    if fam.extents(op, shape) != ext:
      te.geometry_fail(f"{fam.extents(op, shape)} at K = {K}, {ext} at K = 8")
    nsteps = fam.nsteps(op, shape)
    dt = te.bench_dt(N, v_x, point["a"])
    seed = 7 * N + 13 * K + batch
    u0 = te.rough_state(op, seed)
    arena = te.Arena(gpu)
    got = fam.run(op, shape, arena, u0, point["t0"], dt, nsteps)
    arena.check()
    key = (N, K, batch, uniform, seed, tuple(sorted(point.items())), nsteps)
    ora = te.linear_oracle(key, N, v_x, batch, point["a"], point["inflow"], point["t0"], dt,
                           nsteps, te.host(u0), adjoint=fam.adjoint)
    check_linear(got, ora, op)
    if "idx" in got:
      check_refine_index(got["idx"], ora["eta"])
    op.close()


STAGE_SHAPES = [(N, W, MS) for W, MS in ((1, 1), (1, 4), (2, 8)) for N in (1, 4, 8)]


@pytest.mark.parametrize("label", te.LABELS)
@pytest.mark.parametrize("shape", STAGE_SHAPES, ids=ids(STAGE_SHAPES))
def test_stage_loop_pair(pkg, gpu, shape, label):
  """(N, W, MS): TE = 256*W - 10*MS both ways (N = 8 caps MS at 2)."""
  drive(pkg, gpu, StageLoop, shape, label)


WAVE_SHAPES = [(1, 2, 1), (2, 2, 2), (4, 2, 4), (1, 4, 4), (2, 4, 1), (4, 4, 2), (4, 2, 1),
               (1, 2, 2), (2, 2, 4), (2, 4, 4), (4, 4, 1), (1, 4, 2)]


@pytest.mark.parametrize("label", te.LABELS)
@pytest.mark.parametrize("shape", WAVE_SHAPES, ids=ids(WAVE_SHAPES))
def test_wave_tile_forward(pkg, gpu, shape, label):
  """(N, lane elements, MS): TE = 64*E - 10*MS."""
  drive(pkg, gpu, Wave, shape, label)


SNAP_SHAPES = [(2, 1, 4), (4, 2, 8), (4, 1, 4), (2, 2, 8)]


@pytest.mark.parametrize("label", te.LABELS)
@pytest.mark.parametrize("shape", SNAP_SHAPES, ids=ids(SNAP_SHAPES))
def test_snapshot_forward_on_pair_tiles(pkg, gpu, shape, label):
  """(N, tw, ms): TE = 512*tw - 2*((5*ms + 2) & ~1)."""
  drive(pkg, gpu, SnapPairs, shape, label)


REC_SHAPES = [(4, 2, 1, 5), (1, 2, 1, 10), (8, 2, 2, 10), (4, 2, 2, 20),
              (4, 1, 1, 5), (8, 1, 1, 10), (1, 1, 2, 10), (4, 1, 2, 20)]


@pytest.mark.parametrize("label", te.LABELS)
@pytest.mark.parametrize("shape", REC_SHAPES, ids=ids(REC_SHAPES))
def test_record_pair(pkg, gpu, shape, label):
  """(N, lanes, rtw, spl): pair tiles TE = 512*rtw - 2*halo, forward halo (5*spl + 2) & ~1,
  adjoint (5*spl + 1) & ~1; one element per lane runs the stage-loop record kernels at the
  largest power of two <= spl the width allows, forward TE = 256*rtw - 2*(5*MS + 1) (the
  record's extra element), adjoint TE = 256*rtw - 10*MS."""
  drive(pkg, gpu, Record, shape, label)


# (N, waves, msf, msa, lane elements, exchange, nsteps); 4-wave pair tiles (512 elements) take
# no 20-step blocks, 16 waves need Np <= 5, 4 elements per lane Np <= 3
FLOW_SHAPES = [(4, 4, 10, 10, 2, 0, 20), (4, 8, 20, 10, 2, 0, 40), (6, 8, 10, 10, 2, 0, 20),
               (8, 12, 20, 10, 2, 0, 20), (4, 12, 10, 10, 2, 0, 40), (4, 16, 20, 10, 2, 0, 20),
               (1, 16, 10, 10, 2, 0, 20), (1, 4, 20, 10, 4, 0, 20), (2, 8, 10, 10, 4, 0, 40),
               (4, 8, 20, 10, 2, 1, 20), (6, 12, 10, 10, 2, 1, 20), (8, 4, 10, 10, 2, 0, 20)]


@pytest.mark.parametrize("label", te.LABELS)
@pytest.mark.parametrize("shape", FLOW_SHAPES, ids=ids(FLOW_SHAPES))
def test_dataflow_sweep(pkg, gpu, shape, label):
  """sweep_rec and sweep_refine as one launch at the counts of TEF and of TEA (nTF != nTA is
  where the first adjoint block's producer range, csrc/dg_sweep_kernel.h:149-155, changes)."""
  drive(pkg, gpu, Dataflow, shape, label)


@pytest.mark.parametrize("fam,shape", [(StageLoop, (4, 1, 4)), (Wave, (2, 2, 2)),
                                       (SnapPairs, (4, 1, 4)), (Record, (4, 2, 1, 5)),
                                       (Record, (4, 1, 1, 5)),
                                       (Dataflow, (4, 8, 20, 10, 2, 0, 20)),
                                       (Dataflow, (4, 8, 20, 10, 2, 1, 20))],
                         ids=lambda v: v.__name__ if isinstance(v, type) else "-".join(map(str, v)))
@pytest.mark.parametrize("label", ["TE", "TE+1"])
def test_linear_families_off_the_parameter_point(pkg, gpu, fam, shape, label):
  """a = 1.3 on [-0.7, 2.1] from t0 = 3.7 with inflow -sin(a^2 t): the plan parameter and the
  host-computed inflow tables at another value."""
  drive(pkg, gpu, fam, shape, label, point=AWAY)


# ---------------------------------------------------------------------------
# A refine walk across a boundary (the production path, non-uniform kernels)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("fam,shape", [(StageLoop, (4, 1, 4)), (Wave, (2, 2, 2)),
                                       (Wave, (1, 4, 4)), (SnapPairs, (4, 1, 4)),
                                       (SnapPairs, (2, 2, 8)), (Record, (4, 2, 1, 5)),
                                       (Record, (4, 1, 1, 5)), (Record, (1, 1, 2, 10)),
                                       (Dataflow, (4, 4, 10, 10, 2, 0, 20)),
                                       (Dataflow, (4, 8, 20, 10, 2, 1, 20))],
                         ids=lambda v: v.__name__ if isinstance(v, type) else "-".join(map(str, v)))
@pytest.mark.parametrize("which", [0, 1], ids=["fwd", "adj"])
def test_refine_walk_across_a_boundary(pkg, gpu, fam, shape, which):
  """K = TE-2 with reserve(TE+3), five device refines (elements 0, K-1 and three others), a
  sweep after each: K walks TE-1 .. TE+3 over the tile-count boundary."""
  import torch
  N = shape[0]
  probe, _ = make_op(pkg, N, 8, 1, True, HOME)
  fam.tune(probe, shape)
  ext = fam.extents(probe, shape)
  probe.close()
  if which == 1 and (len(ext) < 2 or ext[1] == ext[0]):
    which = 0  # one extent for both directions
  TE = ext[which][0]
  op, _ = make_op(pkg, N, TE - 2, 1, True, HOME)
  fam.tune(op, shape)
  op.reserve(TE + 3)
  idx = torch.zeros(1, dtype=torch.int64, device=gpu)
  for step, pick in enumerate((0, -1, TE // 2, 17, -1)):
    idx.fill_(pick if pick >= 0 else op.K - 1)
    assert op.refine(idx) == TE - 1 + step
    fam.tune(op, shape)
    assert fam.extents(op, shape) == ext and not op.uniform
    v_x = op.v_x()
    nsteps = fam.nsteps(op, shape)
    dt = te.bench_dt(N, v_x, HOME["a"])
    u0 = te.rough_state(op, 100 + step)
    arena = te.Arena(gpu)
    got = fam.run(op, shape, arena, u0, HOME["t0"], dt, nsteps)
    arena.check()
    ora = te.linear_oracle(("walk", fam.__name__, shape, which, step), N, v_x, 1, HOME["a"],
                           HOME["inflow"], HOME["t0"], dt, nsteps, te.host(u0),
                           adjoint=fam.adjoint)
    check_linear(got, ora, op)
    if "idx" in got:
      check_refine_index(got["idx"], ora["eta"])
  op.close()


# ---------------------------------------------------------------------------
# The p-estimate: the chain (flow = 0), the dataflow estimate (flow = 1), sweep_p
# ---------------------------------------------------------------------------
P_SHAPES = [(N, tw, spl) for tw, spl in ((1, 4), (2, 4), (2, 8)) for N in (1, 3, 7)]


def p_case(pkg, gpu, op, v_x, shape, path, point, ext, key):
  """One p-estimate on ``op`` (its forward tuned to the stage loop at 4 steps per launch)."""
  N, tw, spl = shape
  nsteps = 2 * spl
  K, batch = op.K, op.batch
  op.tune(tile_width=1, steps_per_launch=4, lane_elements=0, snap_pairs=0)
  est = pkg.operators.DWREstimate(op, tile_width=tw, steps_per_launch=spl)
  if te.p_extents(op) != ext:
    te.geometry_fail(f"{te.p_extents(op)} at K = {K}, {ext} at K = 8")
  est.tune(flow=1, sweep=1)  # the item counts of both launches, whichever path runs
  te.check_p_items(op, nsteps, ext, True, spl == 4)
  est.tune(flow=0 if path == "chain" else 1, sweep=1 if path == "sweep" else 0)
  if path == "flow":
    assert est.query_flow(nsteps)
  if path == "sweep":
    assert est.query_sweep(nsteps) == (spl == 4)  # 8-step blocks: sweep_p runs the chains
  dt = te.bench_dt(N, v_x, point["a"])
  seed = 7 * N + 13 * K + batch
  u0 = te.rough_state(op, seed)
  arena = te.Arena(gpu)
  snaps = arena.new(nsteps + 1, op.field_numel)
  w = arena.new(est.hi.field_numel)
  eta = arena.new(op.ktot)
  if path == "sweep":
    snaps[0].copy_(u0)
    est.sweep(snaps, w, point["t0"], dt, nsteps, eta=eta, eta_assign=True, eta_abs=False)
  else:
    u = fill(arena, u0)
    op.forward(u, point["t0"], dt, nsteps, snaps)
    keep = snaps.clone()
    est.estimate(w, snaps, point["t0"], dt, nsteps, eta=eta, eta_assign=True,
                 terminal_prolong=True)
    assert bool((snaps == keep).all()), "the estimate wrote the snapshots"
  arena.check()
  assert op.sweep_status() == 0
  ora = te.linear_oracle(key + (seed, nsteps), N, v_x, batch, point["a"], point["inflow"],
                         point["t0"], dt, nsteps, te.host(u0), adjoint=False)
  if "p" not in ora:
    S_hi = te.batched_setup(N + 1, v_x, batch)
    lo = [setup1d.from_elem_major(s, N + 1) for s in ora["snaps"]]
    P = oef.prolong_matrix(ora["S"], S_hi)
    eta_ref, w0_ref = oef.p_estimate(lo, ora["times"], dt, point["a"], ora["S"], S_hi,
                                     P @ lo[-1], point["inflow"])
    ora["p"] = (eta_ref, setup1d.to_elem_major(w0_ref))
  S = te.host(snaps)
  for n, ref in enumerate(ora["snaps"]):
    assert te.rel_err(S[n], ref) <= te.RTOL, ("snapshot", n)
  te.close(te.host(w), ora["p"][1], "w^0 (order N+1)")
  te.close(te.host(eta), ora["p"][0], "eta")
  est.close()


def p_probe(pkg, shape, K, point):
  N, tw, spl = shape
  op, _ = make_op(pkg, N, K, 1, True, point)
  op.tune(tile_width=1, steps_per_launch=4, lane_elements=0, snap_pairs=0)
  est = pkg.operators.DWREstimate(op, tile_width=tw, steps_per_launch=spl)
  assert (est.tile_width, est.steps_per_launch) == (tw, spl)
  est.tune(flow=1, sweep=1)
  est.close()
  return op


_P_STEP = set()


def p_geometry(pkg, shape, point):
  """The extents, and once per shape: the p launches' items step by the blocks (the sweep's by
  forward and estimate blocks) from K = m*TE to m*TE + 1."""
  probe = p_probe(pkg, shape, 8, point)
  ext = te.p_extents(probe)
  probe.close()
  if shape not in _P_STEP:
    TE, nsteps, spl = ext[0][0], 2 * shape[2], shape[2]
    for m in (1, 2):
      a, b = p_probe(pkg, shape, m * TE, point), p_probe(pkg, shape, m * TE + 1, point)
      ia, ib = te.p_items(a, nsteps), te.p_items(b, nsteps)
      want = (nsteps // spl, 2 * (nsteps // 4) if spl == 4 else 0)
      if (ib[0] - ia[0], ib[1] - ia[1]) != want:
        te.geometry_fail(f"p items {ia} at K = {m * TE}, {ib} at {m * TE + 1}: steps of {want} expected")
      a.close()
      b.close()
    _P_STEP.add(shape)
  return ext


def drive_p(pkg, gpu, shape, path, label, point=HOME):
  ext = p_geometry(pkg, shape, point)
  for K, batch in te.counts_of(label, ext):
    uniform = te.uniform_for(label)
    print(f"p {path} {shape} {label}: K={K} batch={batch} uniform={uniform} extents={ext}")
    op, v_x = make_op(pkg, shape[0], K, batch, uniform, point)
    p_case(pkg, gpu, op, v_x, shape, path, point, ext,
           (shape[0], K, batch, uniform, tuple(sorted(point.items()))))
    op.close()


@pytest.mark.parametrize("label", te.LABELS)
@pytest.mark.parametrize("path", ["chain", "flow", "sweep"])
@pytest.mark.parametrize("shape", P_SHAPES, ids=ids(P_SHAPES))
def test_p_estimate(pkg, gpu, shape, path, label):
  """(N, tw, spl): TE = 256*tw - 10*spl, terminal weight P u^N, against
  oracle.effectivity.p_estimate (the estimate p_indicator evaluates)."""
  drive_p(pkg, gpu, shape, path, label)


@pytest.mark.parametrize("path", ["chain", "flow", "sweep"])
def test_p_estimate_off_the_parameter_point(pkg, gpu, path):
  drive_p(pkg, gpu, (3, 2, 4), path, "TE+1", point=AWAY)


WALK = (0, -1, None, 17, -1)  # elements to split: 0, K-1, the middle, 17, K-1


def refine_walk(op, gpu, TE):
  """K = TE-2 -> TE-1 .. TE+3 by five device refines; yields (step, v_x) after each."""
  import torch
  op.reserve(TE + 3)
  idx = torch.zeros(1, dtype=torch.int64, device=gpu)
  for step, pick in enumerate(WALK):
    idx.fill_(op.K // 2 if pick is None else (pick if pick >= 0 else op.K - 1))
    assert op.refine(idx) == TE - 1 + step
    assert not op.uniform
    yield step, op.v_x()


@pytest.mark.parametrize("path", ["chain", "flow", "sweep"])
def test_refine_walk_p_estimate(pkg, gpu, path):
  shape = (3, 1, 4)
  ext = p_geometry(pkg, shape, HOME)
  TE = ext[0][0]
  op, _ = make_op(pkg, shape[0], TE - 2, 1, True, HOME)
  for step, v_x in refine_walk(op, gpu, TE):
    p_case(pkg, gpu, op, v_x, shape, path, HOME, ext, ("walk", path, step))
  op.close()


# ---------------------------------------------------------------------------
# Config 3: Burgers flux and/or the per-stage limiter
# ---------------------------------------------------------------------------
NL_PHYSICS = [("burgers", True), ("burgers", "1"), ("linear", True)]
# (flux, limiter), (N, nl_exchange, decision record)
NL_CASES = [(("burgers", True), (2, 0, True)), (("burgers", True), (4, 0, False)),
            (("burgers", True), (4, 1, True)), (("burgers", True), (2, 1, False)),
            (("burgers", "1"), (2, 0, True)), (("burgers", "1"), (4, 1, True)),
            (("burgers", "1"), (2, 0, False)), (("burgers", "1"), (2, 1, False)),
            (("linear", True), (4, 0, True)), (("linear", True), (2, 0, False)),
            (("linear", True), (2, 1, True)), (("linear", True), (2, 1, False))]


def jump_plus_sine(x, rng, x0, x1):
  """The config-3 state of tests/test_gpu_nonlinear.py: a sine, a jump and node noise."""
  s = (x - x0) / (x1 - x0)
  return np.sin(2 * np.pi * s) + 0.8 * (s > 0.5) + 0.05 * rng.standard_normal(x.shape)


def nl_case(pkg, gpu, op, v_x, physics, shape, point, ext, seed):
  """Two config-3 steps forward (snapshots, the decision record if asked) and back on ``op``,
  and the same two steps without snapshots (2 steps per launch on the workgroup tiles)."""
  import torch
  flux, limit = physics
  N, exchange, record = shape
  nsteps, inflow = 2, op.inflow
  K, batch = op.K, op.batch
  op.tune(nl_exchange=exchange)
  if te.nl_extents(op, True, record) != ext:
    te.geometry_fail(f"{te.nl_extents(op, True, record)} at K = {K}, {ext} at K = 8")
  S = setup1d.startup1d(N, v_x, metric="element")
  dt = te.bench_dt(N, v_x, point["a"])
  rng = np.random.default_rng(seed)
  u0s = [jump_plus_sine(S["x"], rng, v_x[0], v_x[-1]) for _ in range(batch)]
  u0 = torch.tensor(np.concatenate([setup1d.to_elem_major(u) for u in u0s]),
                    dtype=torch.float64, device=gpu)
  arena = te.Arena(gpu)
  u = fill(arena, u0)
  snaps = arena.new(nsteps + 1, op.field_numel)
  dec = arena.new(nsteps * op.ktot, dtype=torch.int16) if record else None
  op.forward(u, point["t0"], dt, nsteps, snaps, decisions=dec)
  plain = fill(arena, u0)
  op.forward(plain, point["t0"], dt, nsteps)
  w = fill(arena, snaps[nsteps])
  eta = arena.new(op.ktot)
  keep = snaps.clone()
  op.adjoint(w, snaps, point["t0"], dt, nsteps, eta=eta, eta_assign=True, decisions=dec)
  arena.check()
  assert bool((snaps == keep).all()), "the adjoint wrote the snapshots"
  Sn, W, E = te.host(snaps), te.host(w), te.host(eta)
  # the two launch shapes may contract differently (tests/test_gpu_nonlinear.py's 1e-12)
  assert te.rel_err(te.host(plain), Sn[nsteps]) <= 1e-12
  times = te.times_of(point["t0"], dt, nsteps)
  fl = K * (N + 1)
  worst = 0.0
  refs = dict(w=[], eta=[])
  for b in range(batch):
    ref, _ = ob.forward_sweep(u0s[b], point["t0"], dt, nsteps, point["a"], S, flux, inflow,
                              limit=limit)
    gs = [setup1d.from_elem_major(Sn[n, b * fl:(b + 1) * fl], N + 1) for n in range(nsteps + 1)]
    for n in range(nsteps + 1):
      worst = max(worst, te.rel_err(gs[n], ref[n]))
    worst = max(worst, te.rel_err(setup1d.from_elem_major(te.host(plain)[b * fl:(b + 1) * fl],
                                                          N + 1), ref[nsteps]))
    # the adjoint oracle on the GPU's own snapshots (the limiter's decisions are thresholds)
    w_ref, eta_ref, _ = ob.adjoint_sweep(gs[-1], gs, times, dt, point["a"], S, flux, inflow,
                                         limit=limit)
    refs["w"].append(setup1d.to_elem_major(w_ref))
    refs["eta"].append(eta_ref)
  print(f"  snapshots: {worst:.3e}")
  assert worst <= te.RTOL
  te.close(W, np.concatenate(refs["w"]), "w^0")
  te.close(E, np.concatenate(refs["eta"]), "eta")


def nl_geometry(pkg, physics, shape, point):
  probe, _ = make_op(pkg, shape[0], 8, 1, True, point, flux=physics[0], limiter=physics[1],
                     inflow="a")
  probe.tune(nl_exchange=shape[1])
  ext = te.nl_extents(probe, True, shape[2])
  probe.close()
  return ext


def drive_nl(pkg, gpu, physics, shape, label, point=HOME):
  ext = nl_geometry(pkg, physics, shape, point)
  # the forward without snapshots (a third extent, where it differs) at its boundaries only
  for K, batch in te.counts_of(label, ext if label in te.BOUNDARY else ext[:2]):
    uniform = te.uniform_for(label)
    print(f"nl {physics} {shape} {label}: K={K} batch={batch} uniform={uniform} extents={ext}")
    op, v_x = make_op(pkg, shape[0], K, batch, uniform, point, flux=physics[0],
                      limiter=physics[1], inflow="a")
    nl_case(pkg, gpu, op, v_x, physics, shape, point, ext, 7 * shape[0] + 13 * K + batch)
    op.close()


NL_LABELS = te.BOUNDARY + te.HALF + te.TINY + te.EDGES


@pytest.mark.parametrize("label", NL_LABELS)
@pytest.mark.parametrize("physics,shape", NL_CASES, ids=[ids([p])[0] + "-" + ids([s])[0]
                                                          for p, s in NL_CASES])
def test_config3(pkg, gpu, physics, shape, label):
  """(flux, limiter) x (N, nl_exchange, decision record): the extents of the forward with
  snapshots (1 step per launch), of the adjoint (narrow cone with the record, wide without;
  k_adj_nl's half tile TH = TE/2 too) and of the forward without snapshots (2 steps)."""
  drive_nl(pkg, gpu, physics, shape, label)


@pytest.mark.parametrize("physics", NL_PHYSICS, ids=ids(NL_PHYSICS))
def test_config3_off_the_parameter_point(pkg, gpu, physics):
  drive_nl(pkg, gpu, physics, (4, 0, True), "TE+1", point=AWAY)


@pytest.mark.parametrize("physics,shape", [(("burgers", True), (2, 0, True)),
                                           (("burgers", True), (2, 1, True)),
                                           (("linear", True), (2, 0, False))],
                         ids=["burgers-tiles-record", "burgers-waves-record", "linear-tiles-wide"])
@pytest.mark.parametrize("which", [0, 1], ids=["fwd", "adj"])
def test_refine_walk_config3(pkg, gpu, physics, shape, which):
  ext = nl_geometry(pkg, physics, shape, HOME)
  TE = ext[which][0]
  op, _ = make_op(pkg, shape[0], TE - 2, 1, True, HOME, flux=physics[0], limiter=physics[1],
                  inflow="a")
  for step, v_x in refine_walk(op, gpu, TE):
    nl_case(pkg, gpu, op, v_x, physics, shape, HOME, ext, 50 + step)
  op.close()


# ---------------------------------------------------------------------------
# Element-wise kernels (no halo) and the slope limiter (H = 1) at their block edges
# ---------------------------------------------------------------------------
_LIM = te.limiter_extents()[0]
BLOCK_KTOT = sorted({255, 256, 257, 511, 512, 513} |
                    {te.count_of(lab, *_LIM)[0] for lab in te.BOUNDARY})


def block_edge_case(pkg, gpu, N, ktot, point):
  import torch
  uniform = ktot % 2 == 0
  op, v_x = make_op(pkg, N, ktot, 1, uniform, point)
  S = setup1d.startup1d(N, v_x, metric="element")
  rng = np.random.default_rng(ktot + N)
  t = point["t0"] + 0.35
  u = jump_plus_sine(S["x"], rng, point["x0"], point["x1"])
  u[:, ::7] = u[:, ::7].mean(axis=0)  # some exactly-constant cells: not every cell is troubled
  ud = torch.tensor(setup1d.to_elem_major(u), dtype=torch.float64, device=gpu)
  keep = ud.clone()
  arena = te.Arena(gpu)
  out = [arena.new(op.field_numel) for _ in range(4)]
  ids_ = arena.new(ktot, dtype=torch.int32)
  ids_.zero_()
  op.rhs(ud, t, out=out[0])
  op.slope_limit(ud, out=out[1], ids=ids_)
  op.slope_limit_1(ud, out=out[2])
  op.init_sine([0.7], [3.0], [0.1], out=out[3])
  est = pkg.operators.DWREstimate(op)
  hi = arena.new(est.hi.field_numel)
  est.prolong(ud, out=hi)
  arena.check()
  assert bool((ud == keep).all())
  em = lambda x, Np: setup1d.from_elem_major(te.host(x), Np)  # noqa: E731
  ref, _ = oadv.advec_rhs1d(u, t, point["a"], S, point["inflow"])
  te.close(em(out[0], N + 1), ref, "rhs")
  lim, ids_ref = olim.slope_limit_n(u, S, return_ids=True)
  np.testing.assert_array_equal(np.nonzero(te.host(ids_))[0], ids_ref)
  assert 0 < ids_ref.size < ktot
  np.testing.assert_allclose(em(out[1], N + 1), lim, rtol=0, atol=1e-13)
  np.testing.assert_allclose(em(out[2], N + 1), olim.slope_limit_1(u, S), rtol=0, atol=1e-13)
  np.testing.assert_allclose(em(out[3], N + 1), 0.7 * np.sin(2 * np.pi * 3.0 * S["x"] + 0.1),
                             rtol=0, atol=1e-13)
  S_hi = setup1d.startup1d(N + 1, v_x, metric="element")
  te.close(em(hi, N + 2), oef.prolong_matrix(S, S_hi) @ u, "prolong")
  est.close()
  op.close()


@pytest.mark.parametrize("ktot", BLOCK_KTOT)
@pytest.mark.parametrize("N", [1, 4])
def test_halo_free_kernels(pkg, gpu, N, ktot):
  """rhs, prolong and init_sine, one element per lane on grids of grid_for(ktot, 256)
  (csrc/dg_advec.hip:1261, :1754, csrc/dg_dwr.hip:1234), at 255 .. 257 and 511 .. 513; and
  slope_limit / slope_limit_1, whose k_limit tiles have H = 1 and own TE = 254 elements
  (csrc/dg_advec.hip:407-408, grids :1928, :1942), at their own TE-1 .. TE+2 and 2TE-1 .. 2TE+1
  as well (253 .. 256, 507 .. 509)."""
  block_edge_case(pkg, gpu, N, ktot, HOME)


@pytest.mark.parametrize("ktot", [_LIM[0] + 1, 257])
def test_halo_free_kernels_off_the_parameter_point(pkg, gpu, ktot):
  block_edge_case(pkg, gpu, 4, ktot, AWAY)
