"""The extended-precision anchor on the limited paths ("The limiter paths"): the
config-3 stage kernels with SlopeLimitN / SlopeLimit1 after every LSERK4 stage on both tile
layouts, their frozen-decision adjoint with and without the decision record, and the
stand-alone k_limit, against the long-double oracle of oracle/extended.py.

The bar is tests/extended_oracle.py's: eg <= MARGIN * max(e64, FLOOR) with e64 from the fp64 run
of the same restatement (k_limit: from oracle/limiter.py, which shares its coordinate form).  The
decisions are not compared to a tolerance but exactly: the record equals the long-double codes,
all three bits of all five stages of every step.  tests/test_oracle_extended.py proves from the
oracles alone that this is decidable for every case here (equal codes in fp64 and long double,
every decision margin >= GAP = 1e-11 of max|u|, e64 <= CAP).

A case: a smooth sine + a jump + N(0, 0.05^2) nodal noise, dt = bench_dt, 4 steps, K = 2*TE + 1 of
the record-driven adjoint's extent (two cases: of the snapshot forward's), the terminal weight
N(0,1) nodal noise (a piecewise-linear weight such as u^N excites two functionals per cell of the
transposed limiter; noise excites every node).
"""
import numpy as np
import pytest

import extended_oracle as xo
import tile_edges as te
from oracle import extended as ox
from test_gpu_extended import dev
from test_gpu_tile_edges import fill

pytestmark = pytest.mark.gpu


def open_plan(pkg, ref, **kw):
  """A plan on the case's own mesh object (the operators the oracles were handed)."""
  mesh = pkg.BaseGalerkin1D(n=ref["mesh"].n, v_x=ref["v_x"])
  for name in ("d_r", "lift", "v", "inv_v", "r_gl"):
    np.testing.assert_array_equal(getattr(mesh, name), getattr(ref["mesh"], name))
  return pkg.operators.DGAdvection1D(mesh, **kw)


def check_lim_k(op, c):
  fwd, adj = te.nl_extents(op, True, True)[:2]
  want = {"adj": 2 * adj[0] + 1, "fwd": 2 * fwd[0] + 1, "quiet": 3 * adj[0] + 1}[c[7]]
  if op.K != want:
    te.geometry_fail(f"the case runs K = {op.K}, the plan's extents {fwd}, {adj} ask for {want}")
  assert adj[0] % xo.LIM_UNIT[c[1]] == 0


@pytest.mark.parametrize("c", xo.LIM_CASES, ids=[xo.lim_id(c) for c in xo.LIM_CASES])
def test_limited_sweep(pkg, gpu, c):
  import torch
  ph, ex, N, uniform, point, src, seed, shape, own = c
  ref = xo.lim_forward_ref(pkg, c)
  p, dt, nsteps = ref["point"], ref["dt"], xo.NL_STEPS
  op = open_plan(pkg, ref, a=p["a"], inflow=p["inflow"], flux=ref["flux"],
                 limiter=True if ref["limit"] == "N" else "1")
  op.tune(nl_exchange=ex)
  assert op.nl_exchange == ex and op.uniform == uniform
  check_lim_k(op, c)
  K, t0 = op.K, p["t0"]
  arena = te.Arena(gpu)
  u0 = dev(ref["u0"], gpu)
  snaps = arena.new(nsteps + 1, op.field_numel)
  rec = arena.new(nsteps * K, dtype=torch.int16)
  op.forward(fill(arena, u0), t0, dt, nsteps, snaps, decisions=rec)
  plain = fill(arena, u0)
  op.forward(plain, t0, dt, nsteps)  # no snapshots: two steps per launch on the workgroup tiles
  keep = snaps.clone()
  runs = []
  for d in (rec, None):
    w, eta = fill(arena, dev(ref["g"], gpu)), arena.new(K)
    op.adjoint(w, snaps, t0, dt, nsteps, src_coef=src, eta=eta, eta_assign=True, decisions=d)
    runs.append((te.host(w), te.host(eta)))
  arena.check()
  assert bool((snaps == keep).all()), "the adjoint wrote the snapshots"
  S = te.host(snaps)
  rep = xo.Report(xo.lim_id(c))
  # the record: every bit of every stage, against the long-double run's decisions
  words = (te.host(rec).astype(np.int64) & 0xFFFF).reshape(nsteps, K)
  np.testing.assert_array_equal(words, ox.pack_codes(ref["X"]["codes"]))
  np.testing.assert_array_equal(S[0], ref["D"]["snaps"][0])
  for n in range(1, nsteps + 1):
    rep.add(f"u^{n}", S[n], ref["X"]["snaps"][n], ref["D"]["snaps"][n])
  rep.add("u^N (no snapshots)", te.host(plain), ref["X"]["snaps"][-1], ref["D"]["snaps"][-1])
  on = xo.lim_adjoint_on(ref, list(S), src)  # both runs fed the GPU's snapshots
  np.testing.assert_array_equal(ox.pack_codes(on["X"]["codes"]), words)
  assert min(on["X"]["margin"], on["D"]["margin"]) >= xo.GAP
  for (w, eta), how in zip(runs, ("with the record", "re-testing")):
    rep.add(f"w^0 {how}", w, on["X"]["w0"], on["D"]["w0"])
    rep.add(f"eta {how}", eta, on["X"]["eta"], on["D"]["eta"])
  if own:  # the self-contained pipeline: forward, then adjoint, each on its own states
    o = xo.lim_adjoint_own(pkg, c)
    rep.add("w^0 (own states)", runs[0][0], o["X"]["w0"], o["D"]["w0"])
    rep.add("eta (own states)", runs[0][1], o["X"]["eta"], o["D"]["eta"])
  if shape == "quiet":  # narrow-cone and wide-cone units in the same record-driven launch
    units = xo.quiet_units(words, xo.LIM_UNIT[ex])
    assert units.any(axis=1).all() and (~units).any(axis=1).all()
  print("  worst: %.2f (%s; eg %.2e, e64 %.2e)" % rep.worst())
  rep.check()
  op.close()


@pytest.mark.parametrize("i", range(len(xo.KLIMIT)), ids=["-".join(map(str, s)) for s in xo.KLIMIT])
def test_stand_alone_limiter(pkg, gpu, i):
  """dg_slope_limit_n / dg_slope_limit_1 (k_limit, with the TVB minmod in one case) at
  ktot = 2*254 + 1: the values to the bar with e64 from oracle/limiter.py, ``ids`` equal to the
  long-double troubled set."""
  import torch
  N, uniform, kind, M = xo.KLIMIT[i]
  r = xo.klimit_ref(pkg, i)
  op = open_plan(pkg, r)
  assert op.uniform == uniform
  (TE, H), = te.limiter_extents()
  if op.K != 2 * TE + 1:
    te.geometry_fail(f"k_limit runs K = {op.K}, its extent {TE} asks for {2 * TE + 1}")
  if r["M"]:
    op.set_tvb(r["M"])
  arena = te.Arena(gpu)
  out = arena.new(op.field_numel)
  rep = xo.Report(f"k_limit {xo.KLIMIT[i]}")
  if kind == "N":
    ids = arena.new(op.ktot, dtype=torch.int32)
    op.slope_limit(dev(r["u"], gpu), out=out, ids=ids)
    np.testing.assert_array_equal(np.nonzero(te.host(ids))[0], np.nonzero(r["X"]["codes"])[0])
    assert set(np.unique(te.host(ids))) <= {0, 1}
  else:
    op.slope_limit_1(dev(r["u"], gpu), out=out)
  arena.check()
  rep.add(f"SlopeLimit{kind}", te.host(out), r["X"]["y"], r["C"]["y"], cap=r["cond"])
  print("  worst: %.2f (%s; eg %.2e, e64 %.2e)" % rep.worst())
  rep.check()
  op.close()
