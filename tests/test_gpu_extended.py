"""The extended-precision anchor: every family of DG kernels with an arithmetic of
its own against the oracle in long double (oracle/extended.py), at a few ulp.

For each compared quantity q (every snapshot level, u^N, the record, w^0, eta) with qX the
long-double result, e64(q) the fp64 numpy oracle's distance from it on the same inputs and eg(q)
the GPU's (both max|. - qX| / max|qX|):

    eg(q) <= MARGIN * max(e64(q), FLOOR),  FLOOR = 4 * 2^-52,  and  e64(q) <= CAP = 1e-14

(tests/extended_oracle.py; the constants' reasons are in DESIGN.md §3).  The inputs are N(0,1)
nodal noise at dt = bench_dt, the plan's own Dr / LIFT / P, fp64 time levels.  Each pipeline is
self-contained (forward, then adjoint and indicator on its own forward states -- GPU, fp64
numpy and long double alike); where snapshots exist eta and w^0 are also compared with both
oracles fed the GPU's snapshots.  K = 2*TE + 1 of the family: both edge tiles and an interior
one; the extents tests/extended_oracle.py computes by formula are checked against the plan's.
"""
import numpy as np
import pytest

import extended_oracle as xo
import tile_edges as te
from test_gpu_tile_edges import Dataflow, Record, fill, make_op, pad_intact

pytestmark = pytest.mark.gpu
HOME, AWAY = xo.HOME, xo.AWAY


def dev(x, gpu):
  import torch
  return torch.tensor(np.ascontiguousarray(np.asarray(x, dtype=np.float64)), dtype=torch.float64,
                      device=gpu)


def ids(shapes):
  return ["-".join(str(v) for v in s) for s in shapes]


def open_op(pkg, key, fwd, **kw):
  """The plan of a case key on the helper's own mesh."""
  N, K, uniform, batch, point, _ = key
  op, v_x = make_op(pkg, N, K, batch, uniform, point, **kw)
  np.testing.assert_array_equal(v_x, fwd["v_x"])
  np.testing.assert_array_equal(op.mesh.d_r, fwd["mesh"].d_r)
  np.testing.assert_array_equal(op.mesh.lift, fwd["mesh"].lift)
  return op


def check_k(op, extents, key):
  """K = 2*TE + 1 (batch 1) or TE - 1 (batched) of the family's smaller extent."""
  TE = min(e[0] for e in extents)
  want = 2 * TE + 1 if key[3] == 1 else TE - 1
  if op.K != want:
    te.geometry_fail(f"the case runs K = {op.K}, the plan's extents {extents} ask for {want}")


def add_states(rep, snaps_host, fwd):
  for n, (x, d) in enumerate(zip(fwd["X"]["snaps"], fwd["D"]["snaps"])):
    if n:
      rep.add(f"u^{n}", snaps_host[n], x, d)
    else:
      np.testing.assert_array_equal(snaps_host[0], d)


# ---------------------------------------------------------------------------
# 1, 2: rhs
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("K,uniform", xo.RHS_MESHES, ids=["K37-uniform", "K60-refined"])
@pytest.mark.parametrize("inflow", ["a", "a2"])
@pytest.mark.parametrize("N", range(1, 9))
def test_rhs_linear(pkg, gpu, N, inflow, K, uniform):
  r = xo.rhs_ref(pkg, N, K, uniform, inflow, "linear")
  op, _ = make_op(pkg, N, K, 1, uniform, HOME, inflow=inflow)
  arena = te.Arena(gpu)
  out = arena.new(op.field_numel)
  op.rhs(dev(r["u"], gpu), r["t"], out=out)
  arena.check()
  rep = xo.Report(f"rhs N={N} {inflow} K={K}")
  rep.add("rhs", te.host(out), r["X"], r["D"])
  rep.check()
  op.close()


@pytest.mark.parametrize("K,uniform", xo.RHS_MESHES, ids=["K37-uniform", "K60-refined"])
@pytest.mark.parametrize("N", [1, 2, 4, 8])
def test_rhs_burgers(pkg, gpu, N, K, uniform):
  r = xo.rhs_ref(pkg, N, K, uniform, "a", "burgers")
  op, _ = make_op(pkg, N, K, 1, uniform, HOME, inflow="a", flux="burgers", limiter=False)
  arena = te.Arena(gpu)
  out = arena.new(op.field_numel)
  op.rhs(dev(r["u"], gpu), r["t"], out=out)
  arena.check()
  rep = xo.Report(f"rhs burgers N={N} K={K}")
  rep.add("rhs", te.host(out), r["X"], r["D"])
  rep.check()
  op.close()


# ---------------------------------------------------------------------------
# 3: the stage-loop forward with snapshots, and the adjoint
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(xo.STAGE)), ids=ids(xo.STAGE))
def test_stage_loop_pair(pkg, gpu, i):
  N, W, MS, scheme, src, alias = xo.STAGE[i]
  key = xo.stage_key(i)
  nsteps = key[5]
  fwd = xo.forward_ref(pkg, *key, scheme=scheme)
  op = open_op(pkg, key, fwd, time_scheme=scheme)
  op.tune(tile_width=W, steps_per_launch=MS, lane_elements=0, snap_pairs=0)
  q = te._q(op, "dg_plan_query", 8)
  assert q[5] == (5 if scheme == "lserk4" else 1) and q[6] == W
  check_k(op, [(256 * q[6] - 2 * q[7] * q[5], q[7] * q[5])], key)
  assert op.K == key[1] and op.uniform == key[2]
  t0, dt = HOME["t0"], fwd["dt"]
  arena = te.Arena(gpu)
  snaps = arena.new(nsteps + 1, op.field_numel)
  u = fill(arena, dev(fwd["u0"], gpu))
  op.forward(u, t0, dt, nsteps, snaps)
  keep = snaps.clone()
  w = snaps[nsteps] if alias else fill(arena, snaps[nsteps])
  eta = arena.new(op.ktot)
  op.adjoint(w, snaps, t0, dt, nsteps, src_coef=src, eta=eta, eta_assign=True)
  arena.check()
  assert bool((snaps[:nsteps] == keep[:nsteps]).all()), "adjoint wrote the snapshots"
  S = te.host(keep)
  rep = xo.Report(f"stage {xo.STAGE[i]}")
  add_states(rep, S, fwd)
  rep.add("u^N (u)", te.host(u), fwd["X"]["snaps"][-1], fwd["D"]["snaps"][-1])
  adj = xo.adjoint_ref(pkg, key, HOME, src, scheme)
  rep.add("w^0", te.host(w), adj["X"]["w0"], adj["D"]["w0"])
  rep.add("eta", te.host(eta), adj["X"]["eta"], adj["D"]["eta"])
  on = xo.adjoint_on(fwd, list(S), HOME, src, scheme)  # both oracles fed the GPU's snapshots
  rep.add("w^0 on the GPU's snapshots", te.host(w), on["X"]["w0"], on["D"]["w0"])
  rep.add("eta on the GPU's snapshots", te.host(eta), on["X"]["eta"], on["D"]["eta"])
  rep.check()
  op.close()


# ---------------------------------------------------------------------------
# 4, 5: wave-tile forward, snapshot forward on pair tiles
# ---------------------------------------------------------------------------
def forward_only(pkg, gpu, key, tune, extents, what):
  nsteps = key[5]
  fwd = xo.forward_ref(pkg, *key)
  op = open_op(pkg, key, fwd)
  tune(op)
  check_k(op, extents(op), key)
  arena = te.Arena(gpu)
  snaps = arena.new(nsteps + 1, op.field_numel)
  u = fill(arena, dev(fwd["u0"], gpu))
  op.forward(u, HOME["t0"], fwd["dt"], nsteps, snaps)
  arena.check()
  rep = xo.Report(what)
  add_states(rep, te.host(snaps), fwd)
  rep.add("u^N (u)", te.host(u), fwd["X"]["snaps"][-1], fwd["D"]["snaps"][-1])
  rep.check()
  op.close()


@pytest.mark.parametrize("i", range(len(xo.WAVE)), ids=ids(xo.WAVE))
def test_wave_tile_forward(pkg, gpu, i):
  N, E, MS = xo.WAVE[i]

  def tune(op):
    op.tune(tile_width=1, steps_per_launch=MS, lane_elements=E, snap_pairs=0)
    assert op.steps_per_launch == MS

  forward_only(pkg, gpu, xo.wave_key(i), tune, lambda op: te.wave_extents(op, E), f"wave {xo.WAVE[i]}")


@pytest.mark.parametrize("i", range(len(xo.SNAP)), ids=ids(xo.SNAP))
def test_snapshot_forward_on_pair_tiles(pkg, gpu, i):
  N, tw, ms = xo.SNAP[i]

  def tune(op):
    op.tune(tile_width=tw, steps_per_launch=ms, lane_elements=0, snap_pairs=1)
    assert (op.tile_width, op.steps_per_launch) == (tw, ms)

  forward_only(pkg, gpu, xo.snap_key(i), tune, te.snap_pair_extents, f"snap pairs {xo.SNAP[i]}")


# ---------------------------------------------------------------------------
# 6, 11: the record pair
# ---------------------------------------------------------------------------
def add_record_pair(rep, got, op, fwd, adj):
  rep.add("u^N", te.host(got["uN"]), fwd["X"]["snaps"][-1], fwd["D"]["snaps"][-1])
  rep.add("record", te.host(got["rec"])[:, :op.ktot], fwd["X"]["rec"], fwd["D"]["rec"])
  rep.add("w^0", te.host(got["w"]), adj["X"]["w0"], adj["D"]["w0"])
  rep.add("eta", te.host(got["eta"]), adj["X"]["eta"], adj["D"]["eta"])


def record_case(pkg, gpu, shape, key, point):
  from test_gpu_tile_edges import record_pair
  N, lanes, rtw, spl, batch, nsteps = shape
  fwd = xo.forward_ref(pkg, *key)
  adj = xo.adjoint_ref(pkg, key, point)
  op = open_op(pkg, key, fwd)
  Record.tune(op, (N, lanes, rtw, spl))
  check_k(op, te.record_extents(op), key)
  arena = te.Arena(gpu)
  got = record_pair(op, arena, dev(fwd["u0"], gpu), point["t0"], fwd["dt"], nsteps)
  rep = xo.Report(f"record {shape}")
  add_record_pair(rep, got, op, fwd, adj)
  rep.check()
  op.close()


@pytest.mark.parametrize("i", range(len(xo.RECORD)), ids=ids(xo.RECORD))
def test_record_pair(pkg, gpu, i):
  """Two elements per lane (Horner form), one element per lane, and batch 3 at K = TE - 1."""
  record_case(pkg, gpu, xo.RECORD[i], xo.record_key(xo.RECORD[i], i), HOME)


def test_record_pair_off_the_parameter_point(pkg, gpu):
  """a = 1.3 on [-0.7, 2.1] from t0 = 3.7, inflow -sin(a^2 t): the large sine argument, where
  the rule for the time levels shows."""
  record_case(pkg, gpu, xo.AWAY_RECORD, xo.record_key(xo.AWAY_RECORD, 1, AWAY), AWAY)


# ---------------------------------------------------------------------------
# 7: the dataflow sweep
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(xo.FLOW)), ids=ids(xo.FLOW))
def test_dataflow_sweep(pkg, gpu, i):
  import torch
  from test_gpu_tile_edges import sweep_once
  shape = xo.FLOW[i]
  key = xo.flow_key(i)
  nsteps = shape[6]
  fwd = xo.forward_ref(pkg, *key)
  adj = xo.adjoint_ref(pkg, key, HOME)
  op = open_op(pkg, key, fwd)
  Dataflow.tune(op, shape)
  ext = te.sweep_extents(op, nsteps)
  check_k(op, ext, key)
  te.check_sweep_items(op, nsteps, ext)
  arena = te.Arena(gpu)
  u0 = dev(fwd["u0"], gpu)
  got = sweep_once(op, arena, u0, HOME["t0"], fwd["dt"], nsteps)
  assert op.sweep_status() == 0, "a work item gave up waiting for a producer"
  rep = xo.Report(f"sweep_rec {shape}")
  add_record_pair(rep, got, op, fwd, adj)
  # sweep_refine: |eta| assigned, and the index
  w2, eta2 = arena.new(op.field_numel), arena.new(op.ktot)
  rec2 = arena.new(nsteps, op.jump_ld)
  res = arena.new(4, dtype=torch.int64)
  res.zero_()
  op.sweep_refine(fill(arena, u0), rec2, w2, HOME["t0"], fwd["dt"], nsteps, eta2, res[0:1],
                  res[1:2].view(torch.float64), res[2:3])
  arena.check()
  pad_intact(rec2, op.ktot)
  assert op.sweep_status() == 0
  assert int(te.host(res)[2]) == 0
  mag_x, mag_d = np.abs(adj["X"]["eta"]), np.abs(adj["D"]["eta"])
  rep.add("sweep_refine w^0", te.host(w2), adj["X"]["w0"], adj["D"]["w0"])
  rep.add("sweep_refine |eta|", te.host(eta2), mag_x, mag_d)
  rep.add("sweep_refine record", te.host(rec2)[:, :op.ktot], fwd["X"]["rec"], fwd["D"]["rec"])
  rep.check()
  # the index is decidable: the long-double top-2 gap exceeds the case's bound on eta
  top = np.sort(mag_x)[::-1]
  assert float(top[0] - top[1]) > 2 * xo.bound(xo.err(mag_d, mag_x)) * float(top[0])
  assert int(te.host(res)[0]) == int(np.argmax(mag_x))
  assert float(te.host(res[1:2].view(torch.float64))[0]) == float(te.host(eta2).max())
  op.close()


# ---------------------------------------------------------------------------
# 8: the p-estimate
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["chain", "flow", "sweep", "sweep-chains"])
@pytest.mark.parametrize("i", range(len(xo.P_CASES)), ids=ids(xo.P_CASES))
def test_p_estimate(pkg, gpu, i, path):
  """eta_p, w^0 (order N + 1) and dg_prolong: as a launch chain, as the dataflow estimate,
  through dg_lserk4_sweep_p (one launch, and its chains), the terminal weight formed by
  DG_ADJ_P_TERMINAL_PROLONG (chain, flow) or handed over from dg_prolong (chain)."""
  N, tw, spl = xo.P_CASES[i]
  key = xo.p_key(i)
  nsteps = key[5]
  fwd = xo.forward_ref(pkg, *key)
  ref = xo.p_ref(pkg, key, HOME)
  op = open_op(pkg, key, fwd)
  op.tune(tile_width=1, steps_per_launch=4, lane_elements=0, snap_pairs=0)
  est = pkg.operators.DWREstimate(op, tile_width=tw, steps_per_launch=spl)
  np.testing.assert_array_equal(est.P, xo.p_setups(pkg, fwd)[2])
  check_k(op, te.p_extents(op), key)
  est.tune(flow=1 if path in ("flow", "sweep") else 0, sweep=1 if path == "sweep" else 0)
  assert est.query_flow(nsteps) == (path in ("flow", "sweep"))
  assert est.query_sweep(nsteps) == (path == "sweep")
  t0, dt = HOME["t0"], fwd["dt"]
  arena = te.Arena(gpu)
  snaps = arena.new(nsteps + 1, op.field_numel)
  w = arena.new(est.hi.field_numel)
  eta = arena.new(op.ktot)
  rep = xo.Report(f"p {path} {xo.P_CASES[i]}")
  if path.startswith("sweep"):
    snaps[0].copy_(dev(fwd["u0"], gpu))
    est.sweep(snaps, w, t0, dt, nsteps, eta=eta, eta_assign=True, eta_abs=False)
  else:
    op.forward(fill(arena, dev(fwd["u0"], gpu)), t0, dt, nsteps, snaps)
    est.estimate(w, snaps, t0, dt, nsteps, eta=eta, eta_assign=True, terminal_prolong=True)
  arena.check()
  assert op.sweep_status() == 0
  S = te.host(snaps)
  add_states(rep, S, fwd)
  rep.add("eta_p", te.host(eta), ref["X"]["eta"], ref["D"]["eta"])
  rep.add("w^0 (order N+1)", te.host(w), ref["X"]["w0"], ref["D"]["w0"])
  on = xo.p_on(pkg, fwd, list(S), HOME)  # both oracles fed the GPU's snapshots
  rep.add("eta_p on the GPU's snapshots", te.host(eta), on["X"]["eta"], on["D"]["eta"])
  rep.add("w^0 on the GPU's snapshots", te.host(w), on["X"]["w0"], on["D"]["w0"])
  hi = arena.new(est.hi.field_numel)
  est.prolong(snaps[nsteps], out=hi)
  rep.add("dg_prolong", te.host(hi), on["X"]["prolong"], on["D"]["prolong"])
  if path == "chain":  # the terminal weight handed over instead of formed by the first launch
    w2, eta2 = fill(arena, hi), arena.new(op.ktot)
    est.estimate(w2, snaps, t0, dt, nsteps, eta=eta2, eta_assign=True)
    np.testing.assert_array_equal(te.host(w2), te.host(w))
    np.testing.assert_array_equal(te.host(eta2), te.host(eta))
  arena.check()
  rep.check()
  est.close()
  op.close()


# ---------------------------------------------------------------------------
# 9: Burgers flux with the limiter off
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("exchange", [0, 1])
@pytest.mark.parametrize("N", [2, 4])
def test_burgers_without_limiter(pkg, gpu, N, exchange):
  """forward with and without snapshots against each oracle's own states; the adjoint and eta
  against both oracles fed the GPU's snapshots."""
  K, uniform = xo.NL_K[exchange], (N + exchange) % 2 == 0
  ref = xo.nl_forward_ref(pkg, N, K, uniform)
  nsteps = xo.NL_STEPS
  op, v_x = make_op(pkg, N, K, 1, uniform, HOME, flux="burgers", limiter=False, inflow="a")
  np.testing.assert_array_equal(v_x, ref["v_x"])
  op.tune(nl_exchange=exchange)
  check_k(op, te.nl_extents(op, True, False), (N, K, uniform, 1))
  t0, dt = HOME["t0"], ref["dt"]
  arena = te.Arena(gpu)
  u0 = dev(ref["u0"], gpu)
  snaps = arena.new(nsteps + 1, op.field_numel)
  op.forward(fill(arena, u0), t0, dt, nsteps, snaps)
  plain = fill(arena, u0)
  op.forward(plain, t0, dt, nsteps)
  keep = snaps.clone()
  w = fill(arena, snaps[nsteps])
  eta = arena.new(op.ktot)
  op.adjoint(w, snaps, t0, dt, nsteps, eta=eta, eta_assign=True)
  arena.check()
  assert bool((snaps == keep).all()), "the adjoint wrote the snapshots"
  S = te.host(snaps)
  rep = xo.Report(f"burgers N={N} exchange={exchange}")
  add_states(rep, S, ref)
  rep.add("u^N (no snapshots)", te.host(plain), ref["X"]["snaps"][-1], ref["D"]["snaps"][-1])
  on = xo.nl_adjoint_on(ref, list(S))
  rep.add("w^0 on the GPU's snapshots", te.host(w), on["X"]["w0"], on["D"]["w0"])
  rep.add("eta on the GPU's snapshots", te.host(eta), on["X"]["eta"], on["D"]["eta"])
  rep.check()
  op.close()


# ---------------------------------------------------------------------------
# 10: the field transfer across a refinement
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("N", range(1, 9))
def test_field_transfer(pkg, gpu, N):
  """dg_field_to_children / dg_field_from_children (PL, PL^T and RL) against
  tests/transfer_oracle.py's loops in long double with the same widened matrices."""
  import torch
  import transfer_oracle as tor
  k_old, batch = 300, 2
  rng = np.random.default_rng(40 + N)
  split = np.sort(rng.choice(k_old, 130, replace=False))
  split[0], split[-1] = 0, k_old - 1
  split = np.unique(split)
  v_old = te.make_vx(k_old, False, 77 + N)
  parent = np.repeat(np.arange(k_old), 1 + np.isin(np.arange(k_old), split))
  v_new = v_old
  for k in split[::-1]:
    v_new = pkg.split_interval(v_new, k)
  K = len(parent)
  assert len(v_new) == K + 1
  mesh = pkg.BaseGalerkin1D(n=N, v_x=v_new)
  op = pkg.operators.DGAdvection1D(mesh, batch=batch)
  pl, rl = pkg.galerkin.split_interpolation(mesh)
  par = torch.tensor(parent, dtype=torch.int32, device=gpu)
  u_old = rng.standard_normal(batch * k_old * (N + 1))
  u_new = rng.standard_normal(batch * K * (N + 1))
  arena = te.Arena(gpu)
  rep = xo.Report(f"transfer N={N}")
  out = arena.new(op.field_numel)
  op.transfer(dev(u_old, gpu), par, k_old, out=out)
  rep.add("to_children PL", te.host(out), xo.transfer_ld(u_old, parent, k_old, pl, True, batch),
          tor.to_children(u_old, parent, k_old, pl, batch))
  for name, fn, A in (("PL^T", op.transfer_t, pl.T), ("RL", op.restrict, rl)):
    out = arena.new(batch * k_old * (N + 1))
    fn(dev(u_new, gpu), par, k_old, out=out)
    rep.add(f"from_children {name}", te.host(out),
            xo.transfer_ld(u_new, parent, k_old, np.ascontiguousarray(A), False, batch),
            tor.from_children(u_new, parent, k_old, np.ascontiguousarray(A), batch))
  arena.check()
  rep.check()
  op.close()
