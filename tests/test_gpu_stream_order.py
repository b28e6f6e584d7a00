"""Every entry point with a ``stream`` parameter, and the Python layers that promise "enqueued
on torch's current stream", held to that stream on a delayed side stream (tests/stream_order.py
has the protocol).  Each case must come back bit-identical to its own default-stream run, and
``pending`` -- the delay still running when the call returned -- must be true for every entry
point without a waiting "Sync:" line in include/dg_advec.h and false for those with one
(tests/test_abi.SYNC_LINES): an undocumented wait fails here, and so does a documented one that
no longer waits.  Three stand-in entry points first show that the harness sees what it is for.

Shapes are the smallest at which a launch structure still has its parts: N = 2, batch 2,
K = 2 TE + 1 of the family (TE from tests/tile_edges.py), two full launches plus a remainder
launch for the chains; the dataflow launches at their smallest tile; support kernels at 257 or
513 elements.  The chain cases of a family run before its dataflow case.
"""
import ctypes
from collections import namedtuple

import numpy as np
import pytest

import stream_order as so
import tile_edges as te
from test_abi import SYNC_LINES, entry_point_comments
from test_gpu_rec import noisy_sine
from test_gpu_tile_edges import (HOME, Dataflow, Record, SnapPairs, StageLoop, Wave, make_op,
                                 nl_geometry, p_probe)

pytestmark = pytest.mark.gpu

T0 = HOME["t0"]
NEAR = 1.0 - 2.0 ** -30   # config 3: A = NEAR * B keeps every limiter decision (asserted)
WAITS = ("stream", "device")

# Python layers that wait for the stream although they only enqueue kernels: none is left (the
# findings of DESIGN.md §3 "Stream order" were fixed); a layer that ends in .cpu() / .item() is
# a values-only case instead.
Case = namedtuple("Case", "id entry build fresh values_only", defaults=(False, False))


@pytest.fixture(scope="module")
def delay(pkg, gpu):
  d = so.Delay(gpu)
  print(f"\n[stream order] one copy pair of {so.DELAY_WORDS * 8 >> 20} MiB: {d.pair_ms:.3f} ms")
  yield d
  if so.LOG:
    worst = max(so.LOG, key=lambda r: r["wall"])
    print(f"\n[stream order] stream form {so.STREAM_FORM}; {len(so.LOG)} runs, "
          f"{sum(r['wall'] for r in so.LOG):.1f} s; slowest {worst['name']} {worst['wall']:.2f} s")
    fam = {}
    for r in so.LOG:
      k = r["name"].split("-")[0]
      if k not in fam or r["t_host"] > fam[k]["t_host"]:
        fam[k] = r
    for k, r in fam.items():
      print(f"[stream order]   {k}: largest t_host {r['t_host'] * 1e3:.3f} ms ({r['name']}), "
            f"delay {r['pairs']} pairs = {r['delay_ms']:.1f} ms")


# ---------------------------------------------------------------------------
# The harness's own proof
# ---------------------------------------------------------------------------
def standin(pkg, gpu, how):
  """dst = src (513 doubles) by dg_stream_copy: on the current stream, with stream = NULL while
  the side stream is current, or on the current stream after a device synchronisation."""
  import torch
  lib = pkg._lib.load()
  n = 513
  src, dst = torch.empty(n + 1, dtype=torch.float64, device=gpu)[:n], \
      torch.empty(n + 1, dtype=torch.float64, device=gpu)[:n]
  gen = torch.Generator(device=gpu).manual_seed(5)
  A = {"src": torch.randn(n, dtype=torch.float64, device=gpu, generator=gen)}
  B = {"src": torch.randn(n, dtype=torch.float64, device=gpu, generator=gen)}

  def run():
    if how == "sync":
      torch.cuda.synchronize()
    st = None if how == "null" else ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)
    rc = lib.dg_stream_copy(ctypes.c_void_p(src.data_ptr()), ctypes.c_void_p(dst.data_ptr()), n, st)
    assert rc == 0
  return so.Ctx(run, {"src": src, "dst": dst}, A, B, ["dst"])


@pytest.fixture(scope="module")
def stream_form(pkg, gpu, delay):
  """Selects the side stream's form: torch.cuda.Stream() if null-stream work overtakes it
  while it is delayed, else a hipStreamNonBlocking stream wrapped in ExternalStream."""
  for form in ("torch", "external"):
    so.STREAM_FORM = form
    r = so.run_case(f"selftest-null-{form}", lambda: standin(pkg, gpu, "null"), delay)
    if r.differing() and r.pending:
      return form
  pytest.fail("null-stream work does not overtake a delayed side stream of either form")


def test_null_stream_stand_in_is_caught(pkg, gpu, delay, stream_form):
  r = so.run_case("selftest-null", lambda: standin(pkg, gpu, "null"), delay)
  assert r.differing() == ["dst"] and r.pending
  print(f"stream form: {stream_form}")


def test_correct_stand_in_passes(pkg, gpu, delay, stream_form):
  r = so.run_case("selftest-correct", lambda: standin(pkg, gpu, "stream"), delay)
  assert not r.differing() and r.pending


def test_synchronising_stand_in_is_not_pending(pkg, gpu, delay, stream_form):
  r = so.run_case("selftest-sync", lambda: standin(pkg, gpu, "sync"), delay)
  assert not r.differing() and not r.pending


# ---------------------------------------------------------------------------
# Builders
# ---------------------------------------------------------------------------
def family_op(pkg, fam, shape, which=0, batch=2, tune=None, **kw):
  """A plan of the family's shape at K = 2 TE + 1 (TE of direction ``which``)."""
  probe, _ = make_op(pkg, shape[0], 8, 1, True, HOME)
  fam.tune(probe, shape)
  TE = fam.extents(probe, shape)[which][0]
  probe.close()
  op, v_x = make_op(pkg, shape[0], 2 * TE + 1, batch, True, HOME, **kw)
  (tune or fam.tune)(op, shape)
  return op, te.bench_dt(shape[0], v_x, HOME["a"])


def chain_steps(ms):
  """Two full launches plus a remainder launch (the chains halve: 4 + 4 + 2, 8 + 8 + 4)."""
  return 2 * ms + max(1, ms // 2)


def two_states(op):
  return noisy_sine(op, 11, op.batch), noisy_sine(op, 12, op.batch)


def snapshots_of(op, u0, dt, nsteps, decisions=None):
  snaps = op.new_field(nsteps + 1)
  op.forward(u0.clone(), T0, dt, nsteps, snaps, decisions=decisions)
  return snaps


def forward_case(op, dt, nsteps, snaps, raw=False, decisions=False):
  import torch
  u = op.new_field()
  a, b = two_states(op)
  if op.flux != "linear" or op.limiter:
    a = NEAR * b
  bufs, outs, same = {"u": u}, ["u"], []
  S = dec = None
  if snaps:
    S = bufs["snapshots"] = op.new_field(nsteps + 1)
    outs.append("snapshots")
  if decisions:
    dec = bufs["decisions"] = torch.empty(nsteps * op.ktot, dtype=torch.int16, device=op.device)
    outs.append("decisions")
    same.append("decisions")
    da, db = torch.empty_like(dec), torch.empty_like(dec)
    snapshots_of(op, a, dt, nsteps, da)
    snapshots_of(op, b, dt, nsteps, db)
    assert torch.equal(da, db), "A and B take different limiter decisions"

  def run():
    if raw:  # dg_lserk4_fwd has no wrapper of its own
      rc = op._lib.dg_lserk4_fwd(op._plan, ctypes.c_void_p(u.data_ptr()), T0, dt, nsteps,
                                 None if S is None else ctypes.c_void_p(S.data_ptr()),
                                 ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
      assert rc == 0
    else:
      op.forward(u, T0, dt, nsteps, S, decisions=dec)
  return so.Ctx(run, bufs, {"u": a}, {"u": b}, outs, same)


def adjoint_case(op, dt, nsteps, mode, src=0.0, raw=False, record=None):
  """mode: "assign", "accumulate" or "abs" (the hipMemsetAsync of an empty sweep aside, the
  three ways the launches treat eta); record: None, False (limited plan, decisions recomputed)
  or True (the decision record is read)."""
  import torch
  b = two_states(op)[1]
  a = NEAR * b if record is not None else two_states(op)[0]
  limited = record is not None and op.limiter
  dec = {k: (torch.empty(nsteps * op.ktot, dtype=torch.int16, device=op.device)
             if limited else None) for k in "ab"}
  SA, SB = (snapshots_of(op, a, dt, nsteps, dec["a"]),
            snapshots_of(op, b, dt, nsteps, dec["b"]))
  if limited:  # also where the adjoint re-tests every cell itself (record = False)
    assert torch.equal(dec["a"], dec["b"]), "A and B take different limiter decisions"
  w, S, eta = op.new_field(), op.new_field(nsteps + 1), op.new_field()[:op.ktot].clone()
  bufs = {"w": w, "snapshots": S, "eta": eta}
  A, B = {"w": SA[nsteps].clone(), "snapshots": SA}, {"w": SB[nsteps].clone(), "snapshots": SB}
  if record:
    bufs["decisions"] = torch.empty_like(dec["a"])
    A["decisions"], B["decisions"] = dec["a"], dec["b"]
  if mode == "accumulate":
    A["eta"], B["eta"] = torch.full_like(eta, 0.25), torch.full_like(eta, -1.5)

  def run():
    if raw:
      rc = op._lib.dg_lserk4_adj(op._plan, ctypes.c_void_p(w.data_ptr()),
                                 ctypes.c_void_p(S.data_ptr()), T0, dt, nsteps, src,
                                 ctypes.c_void_p(eta.data_ptr()),
                                 ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
      assert rc == 0
    else:
      op.adjoint(w, S, T0, dt, nsteps, src_coef=src, eta=eta, eta_assign=mode != "accumulate",
                 eta_abs=mode == "abs", decisions=bufs.get("decisions"))
  # an empty sweep's only work is the zero fill of an assigned eta: zero for A and for B
  return so.Ctx(run, bufs, A, B, ["w", "eta"], ["eta"] if nsteps == 0 else [])


def stage(pkg, scheme="lserk4"):
  def tune(op, shape):
    op.tune(tile_width=shape[1], steps_per_launch=shape[2], lane_elements=0, snap_pairs=0)
  return family_op(pkg, StageLoop, (2, 1, 4), tune=tune, time_scheme=scheme)


def b_stage_fwd(snaps, scheme="lserk4", raw=False):
  def build(pkg, gpu):
    op, dt = stage(pkg, scheme)
    return forward_case(op, dt, chain_steps(op.steps_per_launch), snaps, raw)
  return build


def b_stage_adj(mode, src=0.0, scheme="lserk4", raw=False, empty=False):
  def build(pkg, gpu):
    op, dt = stage(pkg, scheme)
    nsteps = 0 if empty else chain_steps(op.steps_per_launch)
    return adjoint_case(op, dt, nsteps, mode, src, raw)
  return build


def b_wave(pkg, gpu):
  op, dt = family_op(pkg, Wave, (2, 2, 2))
  return forward_case(op, dt, chain_steps(2), True)


def b_snap_pairs(pkg, gpu):
  op, dt = family_op(pkg, SnapPairs, (2, 1, 4))
  return forward_case(op, dt, chain_steps(4), True)


def record_case(op, dt, nsteps, direction):
  a, b = two_states(op)
  if direction == "fwd":
    u0, uN, rec = op.new_field(), op.new_field(), op.new_jumps(nsteps)
    return so.Ctx(lambda: op.forward_rec(u0, T0, dt, nsteps, rec, out=uN),
                  {"u0": u0, "uN": uN, "jumps": rec}, {"u0": a}, {"u0": b}, ["uN", "jumps"])
  recs, ws = [], []
  for u in (a, b):
    rec, w = op.new_jumps(nsteps), op.new_field()
    op.forward_rec(u, T0, dt, nsteps, rec, out=w)
    recs.append(rec)
    ws.append(w)
  w, rec, eta = op.new_field(), op.new_jumps(nsteps), op.new_field()[:op.ktot].clone()
  return so.Ctx(lambda: op.adjoint_rec(w, rec, T0, dt, nsteps, eta=eta, eta_assign=True),
                {"w": w, "jumps": rec, "eta": eta}, {"w": ws[0], "jumps": recs[0]},
                {"w": ws[1], "jumps": recs[1]}, ["w", "eta"])


def b_record(lanes, direction):
  def build(pkg, gpu):
    op, dt = family_op(pkg, Record, (2, lanes, 1, 5), which=0 if direction == "fwd" else 1)
    ms = op.rec_fwd_steps_per_launch if direction == "fwd" else op.rec_steps_per_launch
    return record_case(op, dt, chain_steps(ms), direction)
  return build


FLOW = (4, 4, 10, 10, 2, 0, 20)


def b_sweep(nsteps, refine=False, alias=False, status=False):
  """sweep_rec / sweep_refine on the (N, waves, blocks) = (4, 4, 10 / 10) plan: the dataflow
  launch at 20 steps, the chain fallback at 15."""
  def build(pkg, gpu):
    import torch
    op, dt = family_op(pkg, Dataflow, FLOW)  # batch 2: an even batch*K, the record has no pad
    assert op.ktot % 2 == 0
    assert op.query_sweep(nsteps)[0] == (nsteps == 20)
    a, b = two_states(op)
    u0, uN, w = op.new_field(), op.new_field(), op.new_field()
    rec, eta = op.new_jumps(nsteps), op.new_field()[:op.ktot].clone()
    bufs = {"u0": u0, "uN": uN, "w": w, "jumps": rec, "eta": eta}
    A, B, outs, same = {"u0": a}, {"u0": b}, ["uN", "w", "jumps", "eta"], []
    if refine:
      if alias:
        host = torch.zeros(2, dtype=torch.int64).pin_memory()
        bufs["host"] = host
        idx = pkg.operators.host_alias(host[0:1])
        val = pkg.operators.host_alias(host[1:2])
        assert idx and val
        outs.append("host")
      else:
        idx = bufs["idx"] = torch.zeros(1, dtype=torch.int64, device=gpu)
        val = bufs["value"] = torch.zeros(1, dtype=torch.float64, device=gpu)
        outs += ["idx", "value"]
        same.append("idx")
      bufs["nonfinite"] = torch.zeros(1, dtype=torch.int64, device=gpu)
      A["nonfinite"] = B["nonfinite"] = torch.full((1,), 3, dtype=torch.int64, device=gpu)
      outs.append("nonfinite")
      same.append("nonfinite")

    def run():
      if refine:
        op.sweep_refine(u0, rec, w, T0, dt, nsteps, eta, idx, val, bufs["nonfinite"], uN=uN)
      else:
        op.sweep_rec(u0, rec, w, T0, dt, nsteps, uN=uN, eta=eta, eta_assign=True)
      if status:
        assert op.sweep_status() == 0
    return so.Ctx(run, bufs, A, B, outs, same)
  return build


def p_pair(pkg, flow, sweep):
  probe = p_probe(pkg, (3, 1, 4), 8, HOME)
  TE = te.p_extents(probe)[0][0]
  probe.close()
  op, v_x = make_op(pkg, 3, 2 * TE + 1, 2, True, HOME)
  op.tune(tile_width=1, steps_per_launch=4, lane_elements=0, snap_pairs=0)
  est = pkg.operators.DWREstimate(op, tile_width=1, steps_per_launch=4)
  est.tune(flow=flow, sweep=sweep)
  return op, est, te.bench_dt(3, v_x, HOME["a"])


def b_p(what, flow):
  """adj_p, adj_p_refine and sweep_p at (tw, spl) = (1, 4), N = 3: the chains (10 steps: 4 + 4
  + 2) and the one-launch forms (8 steps: two blocks)."""
  def build(pkg, gpu):
    import torch
    op, est, dt = p_pair(pkg, flow, flow)
    nsteps = 8 if flow else 10
    if what == "sweep":
      assert est.query_sweep(nsteps) == bool(flow)
    else:
      assert est.query_flow(nsteps) == bool(flow)
    a, b = two_states(op)
    w, S, eta = est.new_field(), op.new_field(nsteps + 1), op.new_field()[:op.ktot].clone()
    bufs = {"w": w, "snapshots": S, "eta": eta}
    outs, same = ["w", "eta"], []
    if what == "sweep":
      # the forward runs inside the call: snapshot 0 is the input, the rest are outputs
      u0 = bufs["u0"] = S[0]
      rest = bufs["rest"] = S[1:]
      del bufs["snapshots"]
      A, B = {"u0": a}, {"u0": b}
      outs.append("rest")
    else:
      A, B = {"snapshots": snapshots_of(op, a, dt, nsteps)}, \
          {"snapshots": snapshots_of(op, b, dt, nsteps)}
    idx = val = nf = None
    if what != "adj":
      idx = bufs["idx"] = torch.zeros(1, dtype=torch.int64, device=gpu)
      val = bufs["value"] = torch.zeros(1, dtype=torch.float64, device=gpu)
      nf = bufs["nonfinite"] = torch.zeros(1, dtype=torch.int64, device=gpu)
      A["nonfinite"] = B["nonfinite"] = torch.full((1,), 3, dtype=torch.int64, device=gpu)
      outs += ["idx", "value", "nonfinite"]
      same += ["idx", "nonfinite"]

    def run():
      if what == "adj":
        est.estimate(w, S, T0, dt, nsteps, eta=eta, eta_assign=True, terminal_prolong=True)
      elif what == "refine":
        est.estimate_refine(w, S, T0, dt, nsteps, eta, idx, val, nf, terminal_prolong=True)
      else:
        est.sweep(S, w, T0, dt, nsteps, eta=eta, idx=idx, value=val, nonfinite=nf)
    return so.Ctx(run, bufs, A, B, outs, same)
  return build


def b_prolong(pkg, gpu):
  op, est, _ = p_pair(pkg, 0, 0)
  a, b = two_states(op)
  u, hi = op.new_field(), est.new_field()
  return so.Ctx(lambda: est.prolong(u, out=hi), {"u": u, "hi": hi}, {"u": a}, {"u": b}, ["hi"])


def nl_op(pkg, physics, exchange, record):
  ext = nl_geometry(pkg, physics, (2, exchange, record), HOME)
  op, v_x = make_op(pkg, 2, 2 * ext[0][0] + 1, 2, True, HOME, flux=physics[0],
                    limiter=physics[1], inflow="a")
  op.tune(nl_exchange=exchange)
  return op, te.bench_dt(2, v_x, HOME["a"])


def b_nl_fwd(physics, exchange):
  def build(pkg, gpu):
    op, dt = nl_op(pkg, physics, exchange, True)
    return forward_case(op, dt, 4, True, decisions=True)
  return build


def b_nl_adj(physics, exchange, record):
  def build(pkg, gpu):
    op, dt = nl_op(pkg, physics, exchange, record)
    return adjoint_case(op, dt, 4, "assign", record=record)
  return build


def small_op(pkg, K=257, **kw):
  op, v_x = make_op(pkg, 2, K, 1, False, HOME, **kw)
  return op


def b_rhs(flux):
  def build(pkg, gpu):
    op = small_op(pkg, flux=flux, inflow="a")
    a, b = two_states(op)
    u, out = op.new_field(), op.new_field()
    return so.Ctx(lambda: op.rhs(u, 0.35, out=out), {"u": u, "rhs": out}, {"u": a}, {"u": b},
                  ["rhs"])
  return build


def b_limit(which):
  def build(pkg, gpu):
    import torch
    op = small_op(pkg)
    b = two_states(op)[1]
    u, out = op.new_field(), op.new_field()
    bufs, outs, same = {"u": u, "ulim": out}, ["ulim"], []
    if which == "n":
      ids_ = bufs["ids"] = torch.zeros(op.ktot, dtype=torch.int32, device=gpu)
      outs.append("ids")
      same.append("ids")
      run = lambda: op.slope_limit(u, out=out, ids=ids_)  # noqa: E731
    else:
      run = lambda: op.slope_limit_1(u, out=out)  # noqa: E731
    return so.Ctx(run, bufs, {"u": NEAR * b}, {"u": b}, outs, same)
  return build


def b_argmax(ex):
  def build(pkg, gpu):
    import torch
    op = small_op(pkg, K=513)
    gen = torch.Generator(device=gpu).manual_seed(9)
    a = torch.randn(513, dtype=torch.float64, device=gpu, generator=gen)
    b = torch.randn(513, dtype=torch.float64, device=gpu, generator=gen)
    x, idx = torch.empty_like(a), torch.zeros(1, dtype=torch.int64, device=gpu)
    if not ex:
      return so.Ctx(lambda: op.argmax_async(x, use_abs=True, out=idx), {"x": x, "idx": idx},
                    {"x": a}, {"x": b}, ["idx"])
    a[100], b[200] = float("inf"), float("-inf")  # the winner is not finite: the count grows
    val = torch.zeros(1, dtype=torch.float64, device=gpu)
    nf = torch.zeros(1, dtype=torch.int64, device=gpu)
    three = torch.full((1,), 3, dtype=torch.int64, device=gpu)
    return so.Ctx(lambda: op.argmax_ex(x, idx, val, nf, use_abs=True),
                  {"x": x, "idx": idx, "value": val, "nonfinite": nf},
                  {"x": a, "nonfinite": three}, {"x": b, "nonfinite": three},
                  ["idx", "value", "nonfinite"], ["value", "nonfinite"])
  return build


def b_sum_rows(pkg, gpu):
  import torch
  gen = torch.Generator(device=gpu).manual_seed(2)
  a = torch.randn(5, 257, dtype=torch.float64, device=gpu, generator=gen)
  b = torch.randn(5, 257, dtype=torch.float64, device=gpu, generator=gen)
  x, out = torch.empty_like(a), torch.empty(257, dtype=torch.float64, device=gpu)
  return so.Ctx(lambda: pkg.operators.sum_rows(x, 5, out=out), {"x": x, "out": out}, {"x": a},
                {"x": b}, ["out"])


def b_slice_candidate(pkg, gpu):
  import torch
  op = small_op(pkg)
  gen = torch.Generator(device=gpu).manual_seed(3)
  a = torch.randn(3, 260, dtype=torch.float64, device=gpu, generator=gen)
  b = torch.randn(3, 260, dtype=torch.float64, device=gpu, generator=gen)
  x, cand = torch.empty_like(a), torch.zeros(2, dtype=torch.int64, device=gpu)
  return so.Ctx(lambda: op.slice_candidate(x, 257, 3.0, 1000, cand), {"x": x, "cand": cand},
                {"x": a}, {"x": b}, ["cand"])


def b_candidates(pkg, gpu):
  import torch
  gen = torch.Generator(device=gpu).manual_seed(4)
  def cands():  # (value bits, index): the indices are the same valid ones in A and B
    v = torch.rand(5, dtype=torch.float64, device=gpu, generator=gen)
    return torch.stack((v.view(torch.int64), torch.arange(5, device=gpu) * 100 + 7), 1).contiguous()
  c = torch.zeros(5, 2, dtype=torch.int64, device=gpu)
  idx = torch.zeros(1, dtype=torch.int64, device=gpu)
  val = torch.zeros(1, dtype=torch.float64, device=gpu)
  nf = torch.zeros(1, dtype=torch.int64, device=gpu)
  three = torch.full((1,), 3, dtype=torch.int64, device=gpu)
  return so.Ctx(lambda: pkg.operators.candidates_argmax(c, idx, val, nf),
                {"cands": c, "idx": idx, "value": val, "nonfinite": nf},
                {"cands": cands(), "nonfinite": three}, {"cands": cands(), "nonfinite": three},
                ["idx", "value", "nonfinite"], ["idx", "nonfinite"])


def b_init_sine(pkg, gpu):
  import torch
  op, _ = make_op(pkg, 2, 257, 3, False, HOME)
  gen = torch.Generator(device=gpu).manual_seed(6)
  par = lambda: torch.rand(9, dtype=torch.float64, device=gpu, generator=gen) + 0.5  # noqa: E731
  p, u = torch.empty(9, dtype=torch.float64, device=gpu), op.new_field()
  return so.Ctx(lambda: op.init_sine(p[0:3], p[3:6], p[6:9], out=u), {"par": p, "u": u},
                {"par": par()}, {"par": par()}, ["u"])


def b_stream_copy(n):
  def build(pkg, gpu):
    return standin_wrapper(pkg, gpu, n)
  return build


def standin_wrapper(pkg, gpu, n):
  import torch
  gen = torch.Generator(device=gpu).manual_seed(n)
  a = torch.randn(n, dtype=torch.float64, device=gpu, generator=gen)
  b = torch.randn(n, dtype=torch.float64, device=gpu, generator=gen)
  src = torch.empty(n + 1, dtype=torch.float64, device=gpu)[:n]
  dst = torch.empty(n + 1, dtype=torch.float64, device=gpu)[:n]
  return so.Ctx(lambda: pkg.operators.stream_copy(src, dst), {"src": src, "dst": dst},
                {"src": a}, {"src": b}, ["dst"])


def refined_op(pkg, gpu):
  """A 257-element plan split at three elements (host-synchronised), its parent map."""
  import torch
  op = small_op(pkg, K=254)
  op.reserve(257)
  marks = torch.zeros(254, dtype=torch.uint8, device=gpu)
  marks[[0, 100, 253]] = 1
  parent = torch.zeros(257, dtype=torch.int32, device=gpu)
  assert op.refine_marked(marks, parent=parent) == (257, 3)
  return op, parent


def b_children(to):
  def build(pkg, gpu):
    import torch
    op, parent = refined_op(pkg, gpu)
    n_old, n_new = 254 * op.Np, 257 * op.Np
    n_in, n_out = (n_old, n_new) if to else (n_new, n_old)
    gen = torch.Generator(device=gpu).manual_seed(8)
    a = torch.randn(n_in, dtype=torch.float64, device=gpu, generator=gen)
    b = torch.randn(n_in, dtype=torch.float64, device=gpu, generator=gen)
    x = torch.empty(n_in, dtype=torch.float64, device=gpu)
    out = torch.empty(n_out, dtype=torch.float64, device=gpu)
    fn = op.transfer if to else op.transfer_t
    return so.Ctx(lambda: fn(x, parent, 254, out=out), {"x": x, "out": out}, {"x": a}, {"x": b},
                  ["out"])
  return build


def b_mark(strategy, param):
  def build(pkg, gpu):
    import torch
    probe = small_op(pkg, K=8)
    S, B_, _ = probe.query_mark()
    probe.close()
    op = small_op(pkg, K=S * B_ + 1)
    gen = torch.Generator(device=gpu).manual_seed(10)
    a = torch.randn(op.K, dtype=torch.float64, device=gpu, generator=gen)
    b = torch.randn(op.K, dtype=torch.float64, device=gpu, generator=gen)
    eta = torch.empty_like(a)
    marks = torch.zeros(op.K, dtype=torch.uint8, device=gpu)
    info = torch.zeros(4, dtype=torch.int64, device=gpu)
    return so.Ctx(lambda: op.mark(eta, strategy, param, marks=marks, info=info),
                  {"eta": eta, "marks": marks, "info": info}, {"eta": a}, {"eta": b},
                  ["marks", "info"])
  return build


def b_refine(marked):
  """A plan that changes: dg_plan_refine / dg_plan_refine_marked on a fresh plan per run, seen
  through the split's outputs, a following dg_advec_rhs on the stream and dg_plan_get_mesh."""
  def build(pkg, gpu):
    import torch
    op = small_op(pkg, K=254)
    op.reserve(257)
    n = (257 if marked else 255) * op.Np
    gen = torch.Generator(device=gpu).manual_seed(12)
    a = torch.randn(n, dtype=torch.float64, device=gpu, generator=gen)
    b = torch.randn(n, dtype=torch.float64, device=gpu, generator=gen)
    u, rhs = torch.empty_like(a), torch.empty_like(a)
    bufs, outs = {"u": u, "rhs": rhs}, ["rhs"]
    if marked:
      marks = bufs["marks"] = torch.zeros(254, dtype=torch.uint8, device=gpu)
      m = torch.zeros(254, dtype=torch.uint8, device=gpu)
      m[[0, 100, 253]] = 1
      parent = bufs["parent"] = torch.zeros(257, dtype=torch.int32, device=gpu)
      outs.append("parent")
      same = ["parent", "mesh"]
      A, B = {"u": a, "marks": m}, {"u": b, "marks": m}

      def run():
        op.refine_marked(marks, parent=parent)
        op.rhs(u, 0.35, out=rhs)
    else:
      idx = bufs["idx"] = torch.zeros(1, dtype=torch.int64, device=gpu)
      i = torch.full((1,), 100, dtype=torch.int64, device=gpu)
      h = bufs["h_split"] = torch.zeros(1, dtype=torch.float64, device=gpu)
      outs.append("h_split")
      same = ["h_split", "mesh"]
      A, B = {"u": a, "idx": i}, {"u": b, "idx": i}

      def run():
        op.refine(idx, h)
        op.rhs(u, 0.35, out=rhs)
    return so.Ctx(run, bufs, A, B, outs, same,
                  after=lambda: {"mesh": torch.tensor(op.v_x(), device=gpu)})
  return build


# --- ensembles -----------------------------------------------------------------------------
def time_ensemble(pkg, gpu):
  import torch
  y0 = np.random.default_rng(1).uniform(0.2, 2.5, 129)
  ens = pkg.dgtime.DGTimeEnsemble(2, np.linspace(0.0, 1.0, 6), y0)
  td = torch.as_tensor(ens.times, device=gpu)
  a = torch.as_tensor(y0, device=gpu)
  b = torch.as_tensor(np.random.default_rng(2).uniform(0.2, 2.5, 129), device=gpu)
  return ens, td, a, b


def b_time(what):
  def build(pkg, gpu):
    ens, td, a, b = time_ensemble(pkg, gpu)
    if what == "march":
      def run():
        Y, its, _ = ens.march(td)
        return {"Y": Y, "iters": its}
      return so.Ctx(run, {"y0": ens.y0}, {"y0": a}, {"y0": b}, [], ["iters"])
    Ys = []
    for y in (a, b):
      ens.y0.copy_(y)
      Ys.append(ens.march(td)[0])
    Y = Ys[0].clone()
    if what == "adjoint":
      def run():
        V, err = ens.adjoint(Y, td)
        return {"V": V, "err": err}
      return so.Ctx(run, {"y0": ens.y0, "Y": Y}, {"y0": a, "Y": Ys[0]}, {"y0": b, "Y": Ys[1]}, [])

    def run():  # the Python layer: march, adjoint, indicator
      Yn, _, _ = ens.march(td)
      _, err = ens.adjoint(Yn, td)
      return {"indicator": ens.indicator(err)}
    return so.Ctx(run, {"y0": ens.y0}, {"y0": a}, {"y0": b}, [])
  return build


def b_fd(pkg, gpu):
  import torch
  from test_gpu_fd_ensemble import MESH
  u0 = np.random.default_rng(3).uniform(-2.0, 2.0, 257)
  ens = pkg.fd_ensemble.FDEnsemble(MESH, u0, ref_factor=5)
  b = torch.as_tensor(np.random.default_rng(4).uniform(-2.0, 2.0, 257), device=gpu)

  def run():
    U, V, err = ens.sweep(with_v=True)
    return {"U": U, "V": V, "err": err}
  return so.Ctx(run, {"u0": ens.u0}, {"u0": ens.u0.clone()}, {"u0": b}, [])


_ADAM_WARM = []


def b_resnet(what):
  def build(pkg, gpu):
    import torch
    import resnet_oracle as ro
    ens = pkg.resnet_ensemble.ResNetEnsemble(*ro.case("edge257"), ref_factor=4)
    a = ens.u0.clone()
    gen = torch.Generator(device=gpu).manual_seed(13)
    b = a + 0.01 * torch.randn(a.shape, dtype=a.dtype, device=gpu, generator=gen)
    if what == "train":
      # train changes theta and the optimiser state, so every run gets its own ensemble and
      # loses the warm-up of the harness's first run: the first-use work of a new ensemble
      # (the upload of its time mesh, which waits for the stream, and the gradient scratch)
      # is done here instead, by a call that leaves theta and the optimiser alone
      ens.loss_and_grad()
      if not _ADAM_WARM:  # torch's one-time set-up of Adam in a process takes seconds: not t_host
        pkg.resnet_ensemble.ResNetEnsemble(*ro.case("edge257"), ref_factor=4).train(1)
        _ADAM_WARM.append(True)
      torch.cuda.synchronize()

    def run():
      if what == "sweep":
        U, V, err = ens.sweep(with_v=True)
        return {"U": U, "V": V, "err": err}
      if what == "grad":
        loss, grads, loss_ic = ens.loss_and_grad(per_member=True)
        return {"loss": loss, "loss_ic": loss_ic, "grad": ens.grad.clone()}
      if what == "indicator":
        mean, total = ens.indicator()
        return {"mean": mean, "total": total}
      return {"losses": ens.train(2), "theta": ens.theta}
    return so.Ctx(run, {"u0": ens.u0}, {"u0": a}, {"u0": b}, [])
  return build


def b_ensemble(record, indicator, batch=2):
  def build(pkg, gpu):
    v_x = te.make_vx(1501, True, 0)
    mesh = pkg.BaseGalerkin1D(n=2, v_x=v_x)
    sw = pkg.ensemble.EnsembleSweep(mesh, range(batch), 10, te.bench_dt(2, v_x, HOME["a"]),
                                    record=record, indicator=indicator)
    a = sw.u0.clone()
    b = noisy_sine(sw.op, 14, batch)

    def run():
      return {"partial": sw.run().clone(), "eta": sw.eta.clone(), "w": sw.w.clone()}
    return so.Ctx(run, {"u0": sw.u0}, {"u0": a}, {"u0": b}, [])
  return build


def b_adaptive(pkg, gpu):
  """One iteration of the adapt driver on carried nodal data (it ends in .item(): values only)."""
  import torch
  mesh = pkg.BaseGalerkin1D(n=2, v_x=te.make_vx(257, True, 0))
  gen = torch.Generator(device=gpu).manual_seed(15)
  n = 257 * 3
  a = torch.randn(n, dtype=torch.float64, device=gpu, generator=gen)
  b = torch.randn(n, dtype=torch.float64, device=gpu, generator=gen)
  ad = pkg.adaptive.AdaptiveSweep(mesh, 4, 2, flux="linear", limiter=False, ic=a)
  u0 = ad._carry[0][:n]

  def run():
    ad.iterate()
    return {"eta": ad._eta.clone(), "idx": ad.idx.clone(), "h_split": ad.h_split.clone(),
            "carried": ad.u0().clone()}
  return so.Ctx(run, {"u0": u0}, {"u0": a}, {"u0": b}, [], ["h_split"],
                after=lambda: {"mesh": torch.tensor(ad.op.v_x(), device=gpu)})


BURGERS, LINLIM = ("burgers", True), ("linear", True)

CASES = [
    # stage-loop forward / adjoint, LSERK4 and Euler
    Case("stage-fwd-snapshots", "dg_lserk4_fwd_ex", b_stage_fwd(True)),
    Case("stage-fwd-pingpong", "dg_lserk4_fwd_ex", b_stage_fwd(False)),
    Case("stage-fwd-raw", "dg_lserk4_fwd", b_stage_fwd(True, raw=True)),
    Case("stage-adj-assign", "dg_lserk4_adj_ex", b_stage_adj("assign")),
    Case("stage-adj-accumulate-src", "dg_lserk4_adj_ex", b_stage_adj("accumulate", 0.3)),
    Case("stage-adj-abs", "dg_lserk4_adj_ex", b_stage_adj("abs")),
    Case("stage-adj-empty-assign", "dg_lserk4_adj_ex", b_stage_adj("assign", empty=True)),
    Case("stage-adj-raw", "dg_lserk4_adj", b_stage_adj("accumulate", 0.3, raw=True)),
    Case("euler-fwd-snapshots", "dg_lserk4_fwd_ex", b_stage_fwd(True, "euler")),
    Case("euler-fwd-pingpong", "dg_lserk4_fwd_ex", b_stage_fwd(False, "euler")),
    Case("euler-adj-assign", "dg_lserk4_adj_ex", b_stage_adj("assign", 0.0, "euler")),
    Case("wave-fwd", "dg_lserk4_fwd_ex", b_wave),
    Case("snappairs-fwd", "dg_lserk4_fwd_ex", b_snap_pairs),
    # the jump record: pairs on both lane layouts, then the sweep (chains before dataflow)
    Case("record-fwd-lanes2", "dg_lserk4_fwd_rec", b_record(2, "fwd")),
    Case("record-adj-lanes2", "dg_lserk4_adj_rec", b_record(2, "adj")),
    Case("record-fwd-lanes1", "dg_lserk4_fwd_rec", b_record(1, "fwd")),
    Case("record-adj-lanes1", "dg_lserk4_adj_rec", b_record(1, "adj")),
    Case("sweep-rec-chains", "dg_lserk4_sweep_rec", b_sweep(15)),
    Case("sweep-refine-chains", "dg_lserk4_sweep_refine", b_sweep(15, refine=True)),
    Case("sweep-rec-dataflow", "dg_lserk4_sweep_rec", b_sweep(20)),
    Case("sweep-refine-dataflow", "dg_lserk4_sweep_refine", b_sweep(20, refine=True)),
    Case("sweep-refine-hostalias", "dg_lserk4_sweep_refine", b_sweep(20, refine=True, alias=True)),
    Case("sweep-status", "dg_sweep_status", b_sweep(20, status=True)),
    # the p-estimate
    Case("p-prolong", "dg_prolong", b_prolong),
    Case("p-adj-chain", "dg_lserk4_adj_p", b_p("adj", 0)),
    Case("p-refine-chain", "dg_lserk4_adj_p_refine", b_p("refine", 0)),
    Case("p-sweep-chain", "dg_lserk4_sweep_p", b_p("sweep", 0)),
    Case("p-adj-flow", "dg_lserk4_adj_p", b_p("adj", 1)),
    Case("p-refine-flow", "dg_lserk4_adj_p_refine", b_p("refine", 1)),
    Case("p-sweep-flow", "dg_lserk4_sweep_p", b_p("sweep", 1)),
] + [
    Case(f"nl-{phys[0]}-x{x}-{what}", entry, build)
    for phys in (BURGERS, LINLIM) for x in (0, 1)
    for what, entry, build in (
        ("fwd-record", "dg_lserk4_fwd_ex", b_nl_fwd(phys, x)),
        ("adj-record", "dg_lserk4_adj_ex", b_nl_adj(phys, x, True)),
        ("adj-norecord", "dg_lserk4_adj_ex", b_nl_adj(phys, x, False)))
] + [
    Case("support-rhs-linear", "dg_advec_rhs", b_rhs("linear")),
    Case("support-rhs-burgers", "dg_advec_rhs", b_rhs("burgers")),
    Case("support-limit-n", "dg_slope_limit_n", b_limit("n")),
    Case("support-limit-1", "dg_slope_limit_1", b_limit("1")),
    Case("support-argmax", "dg_argmax", b_argmax(False)),
    Case("support-argmax-ex", "dg_argmax_ex", b_argmax(True)),
    Case("support-sum-rows", "dg_sum_rows", b_sum_rows),
    Case("support-slice-candidate", "dg_slice_candidate", b_slice_candidate),
    Case("support-candidates-argmax", "dg_candidates_argmax", b_candidates),
    Case("support-init-sine", "dg_init_sine", b_init_sine),
    Case("support-stream-copy-odd", "dg_stream_copy", b_stream_copy(513)),
    Case("support-stream-copy-aligned", "dg_stream_copy", b_stream_copy(512)),
    Case("support-to-children", "dg_field_to_children", b_children(True)),
    Case("support-from-children", "dg_field_from_children", b_children(False)),
    Case("support-mark-top", "dg_plan_mark", b_mark("top", 37)),
    Case("support-mark-max", "dg_plan_mark", b_mark("max", 0.5)),
    Case("support-refine", "dg_plan_refine", b_refine(False), True),
    Case("support-refine-marked", "dg_plan_refine_marked", b_refine(True), True),
    Case("ensemble-time-march", "dg_time_march", b_time("march")),
    Case("ensemble-time-adjoint", "dg_time_adjoint", b_time("adjoint")),
    Case("ensemble-fd-sweep", "dg_fd_adapt_sweep", b_fd),
    Case("ensemble-resnet-sweep", "dg_resnet_adapt_sweep", b_resnet("sweep")),
    Case("ensemble-resnet-grad", "dg_resnet_loss_grad", b_resnet("grad")),
    # the Python layers
    Case("layer-time-indicator", None, b_time("layer")),
    Case("layer-resnet-indicator", None, b_resnet("indicator")),
    Case("layer-resnet-train", None, b_resnet("train"), True),
    Case("layer-ensemble-jumps", None, b_ensemble("jumps", "jump")),
    Case("layer-ensemble-snapshots", None, b_ensemble("snapshots", "jump")),
    Case("layer-ensemble-p", None, b_ensemble("snapshots", "p")),
    Case("layer-adaptive-iteration", None, b_adaptive, True, True),
]


def test_every_stream_entry_point_has_a_case():
  """One case at least per function of the header with a ``void* stream`` parameter."""
  import re
  with_stream = {name for name, (params, _) in entry_point_comments().items()
                 if re.search(r"void\s*\*\s*stream", params)}
  assert with_stream == {c.entry for c in CASES if c.entry}, \
      sorted(with_stream ^ {c.entry for c in CASES if c.entry})


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_entry_point_keeps_to_its_stream(pkg, gpu, delay, stream_form, case):
  r = so.run_case(case.id, lambda: case.build(pkg, gpu), delay, fresh=case.fresh)
  print(f"{case.id}: t_host {r.t_host * 1e3:.3f} ms, delay {r.pairs} pairs "
        f"({r.pairs * delay.pair_ms:.1f} ms), pending {r.pending}, differing {r.differing()}")
  assert not r.differing(), f"outputs {r.differing()} differ from the default-stream run"
  if case.values_only:
    return
  waits = SYNC_LINES.get(case.entry) in WAITS
  assert r.pending == (not waits), (
      "the call returned only after the delay had drained: an undocumented wait" if not waits
      else "the header says this entry point waits for the stream, and it did not")
