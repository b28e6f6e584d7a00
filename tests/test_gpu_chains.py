"""A split sweep equals the whole sweep: every entry point that runs a launch chain
(csrc/dg_chain.h), one call against the same launches issued as separate calls of one chunk
each.

Both sides run the same kernels on the same bytes and differ only in which buffer holds the
intermediate states (the plan's scratch fields inside one call, the caller's buffer between
calls), so every output must agree bit for bit.  The split side accumulates the time levels in
Python by the same repeated addition, puts DG_ADJ_ETA_ASSIGN on its first call only and
DG_ADJ_ETA_ABS on its last only.  One composition is not bit-identical by construction, on any
build (it is no property of the chain code): the adjoint's source term with src_coef != 0.  A
split call adds the source of its own node 0 by the closing k_axpy_copy (one fma) where the
whole sweep adds it inside the next launch's last stage, and takes no source at its own
terminal node.  Those cases are held to the 1e-12 that tests/test_gpu_checkpoint.py uses for
the same composition (measured: w^0 and eta differ by 1e-16 .. 6e-16 of their scale).

Sizes: N = 2 on a uniform and N = 4 on a random non-uniform mesh, K one element past two tiles
of the family (extents from tests/tile_edges.py; all below 1,100 elements), nsteps and steps
per launch such that the chain has 0, 1, 2, 3 and 4 launches, the 3- and 4-launch ones with
tail chunks shorter than the setting (7 = 4 + 2 + 1 at 4 per launch, 5 = 2 + 2 + 1 at 2).
Every output is also held to the numpy oracle at the suite's 1e-10 of max|ref| and sits
between sentinel guards (tests/tile_edges.py Arena)."""
import numpy as np
import pytest

import tile_edges as te
from oracle import adjoint as oadj
from oracle import burgers as ob
from oracle import effectivity as oef
from oracle import setup1d
from test_gpu_tile_edges import HOME, fill, jump_plus_sine, make_op

pytestmark = pytest.mark.gpu

MESHES = [(2, True), (4, False)]  # (N, uniform)
MESH_IDS = ["N2-uniform", "N4-refined"]
STEPS4 = [0, 4, 6, 7, 11]  # at 4 steps per launch: 0, 1, 2 (4+2), 3 (4+2+1), 4 (4+4+2+1)
STEPS5 = [0, 5, 7, 8, 13]  # the record's halving 5 -> 2 -> 1: 0, 1, 2 (5+2), 3, 4 (5+5+2+1)
STEPS2 = [0, 2, 4, 5, 7]   # config 3 at min(2, left): 0, 1, 2, 3 (2+2+1), 4 (2+2+2+1)
SRC_RTOL = 1e-12           # tests/test_gpu_checkpoint.py RTOL


def halving(m0):
  def chunk(left):
    m = m0
    while m > left:
      m >>= 1
    return max(m, 1)
  return chunk


def capped(m0):
  return lambda left: min(m0, left)


def spans_fwd(nsteps, chunk):
  out, n = [], 0
  while n < nsteps:
    m = chunk(nsteps - n)
    out.append((n, m))
    n += m
  return out


def spans_rev(nsteps, chunk):
  out, n = [], nsteps
  while n > 0:
    m = chunk(n)
    out.append((n - m, m))
    n -= m
  return out


def same(a, b, what):
  np.testing.assert_array_equal(te.host(a), te.host(b), err_msg=f"{what}: one call vs split calls")


def setup(pkg, N, uniform, extents, tune, **kw):
  """An operator one element past two tiles of the family ``extents(op)`` reports."""
  probe, _ = make_op(pkg, N, 8, 1, True, HOME, **kw)
  tune(probe)
  TE = min(e[0] for e in extents(probe))
  probe.close()
  K = 2 * TE + 1
  assert K <= 1100
  op, v_x = make_op(pkg, N, K, 1, uniform, HOME, **kw)
  tune(op)
  return op, v_x, te.bench_dt(N, v_x, HOME["a"])


def stage(ms=4):
  return lambda op: op.tune(tile_width=1, steps_per_launch=ms, lane_elements=0, snap_pairs=0)


_SRC = {}


def linear_ref(op, v_x, u0, dt, nsteps, src=0.0):
  """The oracle's states, record, and w^0 / |eta| for the terminal weight u^N."""
  key = (op.N, op.K, op.uniform, nsteps)
  ora = te.linear_oracle(("chains",) + key, op.N, v_x, 1, HOME["a"], HOME["inflow"], HOME["t0"], dt,
                         nsteps, te.host(u0))
  if src == 0.0 or nsteps == 0:  # (the empty sweep leaves w: no node to take a source at)
    return ora, ora["w0"], np.abs(ora["eta"])
  if key + (src,) not in _SRC:
    sn = [setup1d.from_elem_major(s, op.N + 1) for s in ora["snaps"]]
    w0, eta, _ = oadj.adjoint_sweep(sn[-1], sn, ora["times"], dt, HOME["a"], ora["S"],
                                    HOME["inflow"], src_coef=src)
    _SRC[key + (src,)] = (setup1d.to_elem_major(w0), np.abs(eta))
  return (ora,) + _SRC[key + (src,)]


def state(op):
  return te.rough_state(op, 7 * op.N + 13 * op.K)


# ---------------------------------------------------------------------------
# forward, without and with snapshots
# ---------------------------------------------------------------------------
FORWARD = {
    "stage": (stage(4), te.stage_loop_extents, False),
    "stage2": (stage(2), te.stage_loop_extents, False),
    "wave": (lambda op: op.tune(tile_width=1, steps_per_launch=4, lane_elements=4, snap_pairs=0),
             lambda op: te.wave_extents(op, 4), False),
    "pairs": (lambda op: op.tune(tile_width=1, steps_per_launch=4, lane_elements=0, snap_pairs=1),
              te.snap_pair_extents, True),
}


def forward_cases():
  for fam in FORWARD:
    for nsteps in ([0, 5] if fam == "stage2" else STEPS4):
      yield fam, nsteps


@pytest.mark.parametrize("fam,nsteps", list(forward_cases()))
@pytest.mark.parametrize("N,uniform", MESHES, ids=MESH_IDS)
def test_forward(pkg, gpu, N, uniform, fam, nsteps):
  """forward without snapshots (the u <-> scratch ping-pong; the pair tiles run with snapshots
  only), with snapshots at u == snapshots[0] and at u distinct."""
  tune, extents, pairs_only = FORWARD[fam]
  op, v_x, dt = setup(pkg, N, uniform, extents, tune)
  chunk = halving(op.steps_per_launch)
  t = te.times_of(HOME["t0"], dt, nsteps)
  u0 = state(op)
  ora, _, _ = linear_ref(op, v_x, u0, dt, nsteps)
  arena = te.Arena(gpu)
  split = spans_fwd(nsteps, chunk)
  assert len(split) == {0: 0, 4: 1, 6: 2, 7: 3, 11: 4, 5: 3}[nsteps]

  if not pairs_only:
    one, two = fill(arena, u0), fill(arena, u0)
    op.forward(one, t[0], dt, nsteps)
    for n0, m in split:
      op.forward(two, t[n0], dt, m)
    same(one, two, "u^N (no snapshots)")
    te.close(te.host(one), ora["snaps"][-1], "u^N (no snapshots)")

  for alias in (True, False):
    s1, s2 = arena.new(nsteps + 1, op.field_numel), arena.new(nsteps + 1, op.field_numel)
    if alias:
      s1[0].copy_(u0)
      s2[0].copy_(u0)
      op.forward(s1[0], t[0], dt, nsteps, s1)
      for n0, m in split:
        op.forward(s2[n0], t[n0], dt, m, s2[n0:n0 + m + 1])
    else:
      u1, u2 = fill(arena, u0), fill(arena, u0)
      op.forward(u1, t[0], dt, nsteps, s1)
      if not split:
        op.forward(u2, t[0], dt, 0, s2)
      for n0, m in split:
        op.forward(u2, t[n0], dt, m, s2[n0:n0 + m + 1])
      same(u1, u2, "u^N")
      same(u1, s1[nsteps], "u^N vs the last snapshot")
    same(s1, s2, f"snapshots (alias={alias})")
    S = te.host(s1)
    for n, ref in enumerate(ora["snaps"]):
      assert te.rel_err(S[n], ref) <= te.RTOL, ("snapshot", n, te.rel_err(S[n], ref))
  arena.check()
  op.close()


# ---------------------------------------------------------------------------
# adjoint from snapshots
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("src", [0.0, 0.3])
@pytest.mark.parametrize("ms,nsteps", [(4, n) for n in STEPS4] + [(2, 5)])
@pytest.mark.parametrize("N,uniform", MESHES, ids=MESH_IDS)
def test_adjoint(pkg, gpu, N, uniform, ms, nsteps, src):
  """adjoint at w on the terminal snapshot and at w distinct, src_coef 0 and non-zero."""
  op, v_x, dt = setup(pkg, N, uniform, te.stage_loop_extents, stage(ms))
  split = spans_rev(nsteps, halving(op.steps_per_launch))
  t = te.times_of(HOME["t0"], dt, nsteps)
  u0 = state(op)
  ora, w_ref, eta_ref = linear_ref(op, v_x, u0, dt, nsteps, src)
  arena = te.Arena(gpu)
  snaps = arena.new(nsteps + 1, op.field_numel)
  op.forward(fill(arena, u0), t[0], dt, nsteps, snaps)
  for alias in (True, False):
    sa, sb = fill(arena, snaps), fill(arena, snaps)
    wa = sa[nsteps] if alias else fill(arena, snaps[nsteps])
    wb = sb[nsteps] if alias else fill(arena, snaps[nsteps])
    ea, eb = arena.new(op.ktot), arena.new(op.ktot)
    op.adjoint(wa, sa, t[0], dt, nsteps, src_coef=src, eta=ea, eta_assign=True, eta_abs=True)
    for i, (n0, m) in enumerate(split):
      op.adjoint(wb, sb[n0:n0 + m + 1], t[n0], dt, m, src_coef=src, eta=eb, eta_assign=i == 0,
                 eta_abs=i == len(split) - 1)
    if not split:
      eb.zero_()  # the empty sweep assigns eta = 0 and leaves w
    assert bool((sa[:nsteps] == snaps[:nsteps]).all()), "adjoint wrote the snapshots"
    if src == 0.0 or len(split) <= 1:
      same(wa, wb, f"w^0 (alias={alias})")
      same(ea, eb, f"eta (alias={alias})")
    else:  # the source of the split nodes enters by another instruction (module docstring)
      te.close(te.host(wb), te.host(wa), "w^0, split vs whole", SRC_RTOL)
      te.close(te.host(eb), te.host(ea), "eta, split vs whole", SRC_RTOL)
    te.close(te.host(wa), w_ref, "w^0")
    te.close(te.host(ea), eta_ref, "eta")
  arena.check()
  op.close()


# ---------------------------------------------------------------------------
# the record pair
# ---------------------------------------------------------------------------
RECORD = {
    "pairs": lambda op: op.tune(rec_tile_width=1, rec_steps_per_launch=5, rec_lane_elements=2,
                                rec_sweep=0),
    "lanes": lambda op: op.tune(rec_tile_width=1, rec_steps_per_launch=4, rec_lane_elements=1,
                                rec_sweep=0),
}


@pytest.mark.parametrize("fam,nsteps", [("pairs", n) for n in STEPS5] + [("lanes", 7)])
@pytest.mark.parametrize("N,uniform", MESHES, ids=MESH_IDS)
def test_record_pair(pkg, gpu, N, uniform, fam, nsteps):
  """forward_rec at u0 == uN and distinct, adjoint_rec; pair tiles and one element per lane."""
  op, v_x, dt = setup(pkg, N, uniform, te.record_extents, RECORD[fam])
  assert op.rec_steps_per_launch == op.rec_fwd_steps_per_launch
  chunk = halving(op.rec_steps_per_launch)
  fsplit, rsplit = spans_fwd(nsteps, chunk), spans_rev(nsteps, chunk)
  t = te.times_of(HOME["t0"], dt, nsteps)
  u0 = state(op)
  ora, w_ref, eta_ref = linear_ref(op, v_x, u0, dt, nsteps)
  umax = float(np.abs(te.host(u0)).max())
  arena = te.Arena(gpu)
  rec = None
  for alias in (True, False):
    r1, r2 = arena.new(nsteps, op.jump_ld), arena.new(nsteps, op.jump_ld)
    a1, a2 = fill(arena, u0), fill(arena, u0)
    o1 = a1 if alias else arena.new(op.field_numel)
    o2 = a2 if alias else arena.new(op.field_numel)
    op.forward_rec(a1, t[0], dt, nsteps, r1, out=o1)
    if not fsplit:
      op.forward_rec(a2, t[0], dt, 0, r2, out=o2)
    for i, (n0, m) in enumerate(fsplit):
      op.forward_rec(a2 if i == 0 else o2, t[n0], dt, m, r2[n0:n0 + m], out=o2)
    if not alias:
      assert bool((a1 == u0).all()) and bool((a2 == u0).all()), "forward_rec wrote its input"
    same(o1, o2, f"u^N (alias={alias})")
    R1, R2 = te.host(r1)[:, :op.ktot], te.host(r2)[:, :op.ktot]
    np.testing.assert_array_equal(R1, R2, err_msg="record: one call vs split calls")
    te.close(te.host(o1), ora["snaps"][-1], "u^N")
    err = float(np.max(np.abs(R1 - ora["rec"]))) / umax if nsteps else 0.0
    assert err <= te.RTOL, ("record", err)
    if op.jump_ld != op.ktot:
      assert bool((r1[:, op.ktot:] == te.SENTINEL).all()), "the record's pad entry was written"
    rec = r1
  wa, wb = fill(arena, ora_state(gpu, ora)), fill(arena, ora_state(gpu, ora))
  # (the weights: the oracle's u^N on both sides, so that w^0 and eta meet the oracle's)
  ea, eb = arena.new(op.ktot), arena.new(op.ktot)
  keep = rec.clone()
  op.adjoint_rec(wa, rec, t[0], dt, nsteps, eta=ea, eta_assign=True, eta_abs=True)
  for i, (n0, m) in enumerate(rsplit):
    op.adjoint_rec(wb, rec[n0:n0 + m], t[n0], dt, m, eta=eb, eta_assign=i == 0,
                   eta_abs=i == len(rsplit) - 1)
  if not rsplit:
    eb.zero_()
  assert bool((rec == keep).all()), "adjoint_rec wrote the record"
  same(wa, wb, "w^0")
  same(ea, eb, "eta")
  te.close(te.host(wa), w_ref, "w^0")
  te.close(te.host(ea), eta_ref, "eta")
  arena.check()
  op.close()


def ora_state(gpu, ora):
  import torch
  return torch.tensor(np.ascontiguousarray(ora["snaps"][-1]), dtype=torch.float64, device=gpu)


# ---------------------------------------------------------------------------
# config 3
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("record", [True, False], ids=["record", "norecord"])
@pytest.mark.parametrize("ms,nsteps", [(2, n) for n in STEPS2] + [(4, 3)])
@pytest.mark.parametrize("N,uniform", MESHES, ids=MESH_IDS)
def test_config3(pkg, gpu, N, uniform, ms, nsteps, record):
  """The limited Burgers forward (with and without snapshots) and adjoint, with and without the
  decision record.  ms = 2: two steps per forward launch; ms = 4 (the default): one with
  snapshots, two without.  The adjoint runs one step per launch."""
  import torch
  flux, limit = "burgers", True
  op, v_x, dt = setup(pkg, N, uniform, lambda o: te.nl_extents(o, True, record),
                      lambda o: o.tune(steps_per_launch=ms, nl_exchange=0), flux=flux,
                      limiter=limit, inflow="a")
  _, ms_snap, ms_plain = te._q(op, "dg_plan_query_nl", 3)
  assert (ms_snap, ms_plain) == ((2, 2) if ms == 2 else (1, 2))
  t = te.times_of(HOME["t0"], dt, nsteps)
  S = setup1d.startup1d(N, v_x, metric="element")
  u0n = jump_plus_sine(S["x"], np.random.default_rng(5 * N + nsteps), v_x[0], v_x[-1])
  u0 = torch.tensor(setup1d.to_elem_major(u0n), dtype=torch.float64, device=gpu)
  arena = te.Arena(gpu)
  new_dec = lambda: arena.new(max(nsteps, 1) * op.ktot, dtype=torch.int16) if record else None  # noqa: E731
  part = lambda d, n0, m: d[n0 * op.ktot:(n0 + m) * op.ktot] if (record and m) else None  # noqa: E731

  # forward without snapshots
  p1, p2, d1, d2 = fill(arena, u0), fill(arena, u0), new_dec(), new_dec()
  op.forward(p1, t[0], dt, nsteps, decisions=part(d1, 0, nsteps))
  for n0, m in spans_fwd(nsteps, capped(ms_plain)):
    op.forward(p2, t[n0], dt, m, decisions=part(d2, n0, m))
  same(p1, p2, "u^N (no snapshots)")
  if record:
    same(d1[:nsteps * op.ktot], d2[:nsteps * op.ktot], "decisions (no snapshots)")
  # forward with snapshots, u distinct and u == snapshots[0]
  for alias in (False, True):
    s1, s2 = arena.new(nsteps + 1, op.field_numel), arena.new(nsteps + 1, op.field_numel)
    e1, e2 = new_dec(), new_dec()
    if alias:
      s1[0].copy_(u0)
      s2[0].copy_(u0)
      u1, u2 = s1[0], None
    else:
      u1, u2 = fill(arena, u0), fill(arena, u0)
    op.forward(u1, t[0], dt, nsteps, s1, decisions=part(e1, 0, nsteps))
    if nsteps == 0 and not alias:
      op.forward(u2, t[0], dt, 0, s2)
    for n0, m in spans_fwd(nsteps, capped(ms_snap)):
      op.forward(s2[n0] if alias else u2, t[n0], dt, m, s2[n0:n0 + m + 1],
                 decisions=part(e2, n0, m))
    same(s1, s2, f"snapshots (alias={alias})")
    if not alias:
      same(u1, u2, "u^N")
    if record:
      same(e1[:nsteps * op.ktot], e2[:nsteps * op.ktot], "decisions")
  snaps, dec = s1, e1
  # adjoint, w on the terminal snapshot and distinct
  for alias in (True, False):
    sa, sb = fill(arena, snaps), fill(arena, snaps)
    wa = sa[nsteps] if alias else fill(arena, snaps[nsteps])
    wb = sb[nsteps] if alias else fill(arena, snaps[nsteps])
    ea, eb = arena.new(op.ktot), arena.new(op.ktot)
    op.adjoint(wa, sa, t[0], dt, nsteps, eta=ea, eta_assign=True, eta_abs=True,
               decisions=part(dec, 0, nsteps))
    split = spans_rev(nsteps, capped(1))
    for i, (n0, m) in enumerate(split):
      op.adjoint(wb, sb[n0:n0 + m + 1], t[n0], dt, m, eta=eb, eta_assign=i == 0,
                 eta_abs=i == len(split) - 1, decisions=part(dec, n0, m))
    if not split:
      eb.zero_()
    same(wa, wb, f"w^0 (alias={alias})")
    same(ea, eb, f"eta (alias={alias})")
  arena.check()
  # the oracle: forward on its own states, the adjoint on the GPU's snapshots (the limiter's
  # decisions are thresholds), as tests/test_gpu_tile_edges.py nl_case
  Sn = te.host(snaps)
  ref, _ = ob.forward_sweep(u0n, t[0], dt, nsteps, HOME["a"], S, flux, op.inflow, limit=limit)
  gs = [setup1d.from_elem_major(Sn[n], N + 1) for n in range(nsteps + 1)]
  for n in range(nsteps + 1):
    assert te.rel_err(gs[n], ref[n]) <= te.RTOL, ("snapshot", n)
  te.close(setup1d.from_elem_major(te.host(p1), N + 1), ref[nsteps], "u^N (no snapshots)")
  if nsteps:
    w_ref, eta_ref, _ = ob.adjoint_sweep(gs[-1], gs, t, dt, HOME["a"], S, flux, op.inflow,
                                         limit=limit)
    te.close(te.host(wa), setup1d.to_elem_major(w_ref), "w^0")
    te.close(te.host(ea), np.abs(eta_ref), "eta")
  op.close()


# ---------------------------------------------------------------------------
# the p-estimate's chain
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("ms,nsteps", [(4, n) for n in STEPS4] + [(2, 5)])
@pytest.mark.parametrize("N,uniform", MESHES, ids=MESH_IDS)
def test_p_estimate_chain(pkg, gpu, N, uniform, ms, nsteps):
  """estimate with the dataflow launches tuned off, the terminal weight formed by the first
  launch; and sweep (its chains: the forward at 4 steps per launch on the stage-loop tiles,
  whatever the plan's own forward shape) equal to forward + estimate, the plan's shape
  untouched."""
  def tune(op):
    stage(4)(op)
    est = pkg.operators.DWREstimate(op, tile_width=1, steps_per_launch=ms)
    est.tune(flow=0, sweep=0)
    est.close()

  op, v_x, dt = setup(pkg, N, uniform, te.p_extents, tune)
  est = pkg.operators.DWREstimate(op, tile_width=1, steps_per_launch=ms)
  est.tune(flow=0, sweep=0)
  assert not est.query_flow(nsteps) and not est.query_sweep(nsteps)
  split = spans_rev(nsteps, halving(est.steps_per_launch))
  t = te.times_of(HOME["t0"], dt, nsteps)
  u0 = state(op)
  arena = te.Arena(gpu)
  snaps = arena.new(nsteps + 1, op.field_numel)
  op.forward(fill(arena, u0), t[0], dt, nsteps, snaps)
  keep = snaps.clone()
  wa, wb = arena.new(est.hi.field_numel), arena.new(est.hi.field_numel)
  ea, eb = arena.new(op.ktot), arena.new(op.ktot)
  est.estimate(wa, snaps, t[0], dt, nsteps, eta=ea, eta_assign=True, eta_abs=True,
               terminal_prolong=True)
  for i, (n0, m) in enumerate(split):
    est.estimate(wb, snaps[n0:n0 + m + 1], t[n0], dt, m, eta=eb, eta_assign=i == 0,
                 eta_abs=i == len(split) - 1, terminal_prolong=i == 0)
  if not split:
    est.prolong(snaps[0], out=wb)
    eb.zero_()
  assert bool((snaps == keep).all()), "the estimate wrote the snapshots"
  same(wa, wb, "w^0 (order N+1)")
  same(ea, eb, "eta")
  # sweep's chains from a plan whose own forward runs another shape
  op.tune(tile_width=1, steps_per_launch=2, lane_elements=4 if N <= 2 else 0, snap_pairs=1)
  shape = te._q(op, "dg_plan_query", 8)
  s2 = arena.new(nsteps + 1, op.field_numel)
  s2[0].copy_(u0)
  wc, ec = arena.new(est.hi.field_numel), arena.new(op.ktot)
  est.sweep(s2, wc, t[0], dt, nsteps, eta=ec, eta_assign=True, eta_abs=True)
  assert te._q(op, "dg_plan_query", 8) == shape, "sweep changed the plan"
  same(s2, snaps, "sweep's snapshots vs forward at 4 steps per launch")
  same(wc, wa, "sweep's w^0 vs estimate")
  same(ec, ea, "sweep's eta vs estimate")
  arena.check()
  # the oracle (tests/test_gpu_tile_edges.py p_case)
  ora, _, _ = linear_ref(op, v_x, u0, dt, nsteps)
  S_hi = te.batched_setup(N + 1, v_x, 1)
  lo = [setup1d.from_elem_major(s, N + 1) for s in ora["snaps"]]
  P = oef.prolong_matrix(ora["S"], S_hi)
  eta_ref, w0_ref = oef.p_estimate(lo, ora["times"], dt, HOME["a"], ora["S"], S_hi, P @ lo[-1],
                                   HOME["inflow"])
  Sn = te.host(snaps)
  for n, ref in enumerate(ora["snaps"]):
    assert te.rel_err(Sn[n], ref) <= te.RTOL, ("snapshot", n)
  te.close(te.host(wa), setup1d.to_elem_major(w0_ref), "w^0 (order N+1)")
  te.close(te.host(ea), np.abs(eta_ref), "eta")
  est.close()
  op.close()
