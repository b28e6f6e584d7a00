"""The ABI's buffer contract (include/dg_advec.h "Aliasing and alignment"): which
array arguments of one call may share memory, that buffers which only touch are accepted,
that 8-byte alignment suffices, and that the Python wrappers refuse a bad output before a
pointer reaches the library.

  (a) ``TABLE`` names every unordered pair of tensor parameters of every public wrapper as
      "refused" or "allowed" (the one documented exact alias; any other overlap of that pair is
      refused too); a wrapper or pair the table does not know fails the test.
  (b) every pair, placed overlapping in three ways inside one backing tensor: DGLibraryError
      with DG_ERR_ARG, and the backing tensor bit-identical afterwards (nothing was enqueued).
  (c) the same pairs placed touching, in both orders: the bits of the run on separately
      allocated tensors, and nothing written outside the buffers.
  (d) the allowed aliases against separate buffers, bit for bit, on every launch chain.
  (e) every field-sized argument at a pointer that is 8- but not 16-byte aligned: the bits of
      the aligned run; the two arguments that need 16 bytes (the jump record, stream_copy) refuse.
  (f) the wrappers' own checks, against a recording stub in place of the library: the stated
      exception type, and no call recorded.

Every comparison is bit for bit or an exception: the module has no tolerance.
"""
import inspect
import itertools

import numpy as np
import pytest

from oracle import advec as oadv
from oracle import setup1d
from test_gpu_rec import noisy_sine

pytestmark = pytest.mark.gpu

R, A = "refused", "allowed"


def _all(*names):
  return {p: R for p in itertools.combinations(names, 2)}


# wrapper -> {(a, b) in signature order: "refused" | "allowed"}
TABLE = {
    "refine": _all("idx", "h_split"),
    "mark": _all("eta", "marks", "info"),
    "refine_marked": _all("marks", "parent"),
    "transfer": _all("u", "parent", "out"),
    "transfer_t": _all("w", "parent", "out"),
    "restrict": _all("u", "parent", "out"),
    "rhs": _all("u", "out"),
    "forward": {**_all("u", "snapshots", "decisions"), ("u", "snapshots"): A},
    "adjoint": {**_all("w", "snapshots", "eta", "decisions"), ("w", "snapshots"): A},
    "forward_rec": {**_all("u0", "jumps", "out"), ("u0", "out"): A},
    "adjoint_rec": _all("w", "jumps", "eta"),
    "sweep_rec": _all("u0", "jumps", "w", "uN", "eta"),
    "sweep_refine": _all("u0", "jumps", "w", "eta", "idx", "value", "nonfinite", "uN"),
    "slope_limit": _all("u", "out", "ids"),
    "slope_limit_1": _all("u", "out"),
    "argmax_async": _all("x", "out"),
    "argmax_ex": _all("x", "idx", "value", "nonfinite"),
    "slice_candidate": _all("x", "cand"),
    "prolong": _all("u", "out"),
    "estimate": _all("w", "snapshots", "eta"),
    "estimate_refine": _all("w", "snapshots", "eta", "idx", "value", "nonfinite"),
    "sweep": _all("snapshots", "w", "eta", "idx", "value", "nonfinite"),
    "stream_copy": _all("src", "dst"),
    "sum_rows": _all("x", "out"),
    "candidates_argmax": _all("cands", "idx", "value", "nonfinite"),
}

TENSORS = {"idx", "h_split", "eta", "marks", "info", "parent", "u", "out", "w", "snapshots",
           "decisions", "u0", "jumps", "uN", "value", "nonfinite", "trace", "ids", "x", "cand",
           "src", "dst", "cands"}
# amp / freq / phase are host values: init_sine copies them to tensors of its own
SCALARS = {"M", "amp", "count", "divisor", "dt", "eta_abs", "eta_assign", "flow", "freq",
           "k_capacity", "k_old", "lane_elements", "max_marked", "n", "nl_exchange", "nsteps",
           "offset", "param", "phase", "rec_fwd_steps_per_launch", "rec_fwd_tile_width",
           "rec_lane_elements", "rec_steps_per_launch", "rec_sweep", "rec_tile_width", "rows",
           "snap_pairs", "src_coef", "steps_per_launch", "strategy", "sweep", "sweep_exchange",
           "sweep_lane_elements", "sweep_take", "sweep_waves", "t", "t0", "terminal_prolong",
           "terminal_state", "tile", "tile_width", "use_abs", "xcd_order"}


def public_wrappers(ops):
  out = {}
  for cls in (ops.DGAdvection1D, ops.DWREstimate):
    for name, fn in inspect.getmembers(cls, inspect.isfunction):
      if not name.startswith("_"):
        out.setdefault(name, []).append(fn)
  for name in ("stream_copy", "sum_rows", "candidates_argmax"):
    out[name] = [getattr(ops, name)]
  return out


def test_table_covers_every_wrapper(pkg):
  """(a): every parameter of every public wrapper is a known tensor or a known scalar, and every
  pair of tensor parameters of one wrapper has a row in TABLE (and TABLE has no stale row)."""
  seen = set()
  for name, fns in public_wrappers(pkg.operators).items():
    for fn in fns:
      params = [p for p in inspect.signature(fn).parameters if p != "self"]
      unknown = [p for p in params if p not in TENSORS and p not in SCALARS]
      assert not unknown, f"{name}: parameters {unknown} are neither in TENSORS nor in SCALARS"
      tensors = [p for p in params if p in TENSORS]
      if len(tensors) < 2:
        continue
      assert name in TABLE, f"{name} takes the tensors {tensors} and has no row in TABLE"
      seen.add(name)
      want = set(itertools.combinations(tensors, 2))
      have = {tuple(sorted(k, key=tensors.index)) for k in TABLE[name]
              if set(k) <= set(tensors)}
      assert want <= have, f"{name}: pairs {sorted(want - have)} are missing from TABLE"
  assert seen == set(TABLE), f"TABLE rows without a wrapper: {sorted(set(TABLE) - seen)}"
  assert all(v in (R, A) for row in TABLE.values() for v in row.values())


# --------------------------------------------------------------------------------------------
# The calls: per wrapper one or more variants, each with its tensor arguments' (dtype, numel),
# reference inputs and the invocation.
# --------------------------------------------------------------------------------------------
PATTERN = 0x7FF8DEADBEEFCAFE  # a NaN with a payload: untouched memory is recognisable

_cache = {}


def ctx(pkg, N, K, batch, **kw):
  """A plan on a seeded random non-uniform mesh (cached), with the oracle's dt."""
  key = (N, K, batch, tuple(sorted(kw.items())))
  if key not in _cache:
    rng = np.random.default_rng(1000 * N + K)
    v_x = np.concatenate(([0.0], np.cumsum(rng.uniform(0.5, 1.5, K))))
    v_x /= v_x[-1]
    mesh = pkg.BaseGalerkin1D(n=N, v_x=v_x)
    S = setup1d.startup1d(N, v_x, metric="element")
    op = pkg.operators.DGAdvection1D(mesh, batch=batch, **kw)
    _cache[key] = (op, mesh, oadv.bench_dt(S))
  return _cache[key]


class Call:
  """One wrapper call: ``specs`` name -> (dtype, numel), ``inputs`` name -> reference content
  (absent: the untouched-memory pattern), ``invoke(bufs)``; ``unit`` the bytes of "one
  element" (Np doubles) by which field-sized buffers are shifted; ``align`` name -> bytes."""

  def __init__(self, tag, specs, inputs, invoke, unit, align=None, fields=()):
    self.tag, self.specs, self.inputs, self.invoke = tag, specs, inputs, invoke
    self.unit, self.align, self.fields = unit, align or {}, fields
    self._ref = None

  def nbytes(self, n):
    dtype, numel = self.specs[n]
    return numel * dtype.itemsize

  def alignment(self, n):
    return self.align.get(n, self.specs[n][0].itemsize)

  def fresh(self, device):
    import torch
    bufs = {}
    for n, (dtype, numel) in self.specs.items():
      raw = torch.full(((numel * dtype.itemsize + 7) // 8,), PATTERN, dtype=torch.int64,
                       device=device).view(torch.uint8)[:numel * dtype.itemsize].view(dtype)
      if n in self.inputs:
        raw.copy_(self.inputs[n].reshape(-1))
      bufs[n] = raw
    return bufs

  def reference(self, device):
    """The buffers' bytes after the call on separately allocated tensors (computed once)."""
    import torch
    if self._ref is None:
      bufs = self.fresh(device)
      self.invoke(bufs)
      torch.cuda.synchronize()
      self._ref = {n: t.view(torch.uint8).clone() for n, t in bufs.items()}
    return self._ref


def arena(call, device, place):
  """One backing tensor holding every buffer of ``call`` at the byte offsets ``place`` (inputs
  copied in, the rest the pattern): (backing bytes, a copy of them, the views)."""
  import torch
  total = max(off + call.nbytes(n) for n, off in place.items()) + 512
  back = torch.full((total // 8 + 1,), PATTERN, dtype=torch.int64, device=device).view(torch.uint8)
  assert back.data_ptr() % 256 == 0
  bufs = {}
  for n, off in place.items():
    dtype, _ = call.specs[n]
    assert off >= 0 and off % call.alignment(n) == 0, (n, off)
    bufs[n] = back[off:off + call.nbytes(n)].view(dtype)
  for n in place:
    if n in call.inputs:
      bufs[n].copy_(call.inputs[n].reshape(-1))
  torch.cuda.synchronize()
  return back, back.clone(), bufs


def spread(call, skip=(), start=0):
  """Well-separated 256-byte-aligned offsets for every buffer but ``skip``; (offsets, end)."""
  place, cur = {}, start
  for n in call.specs:
    if n in skip:
      continue
    place[n] = cur
    cur = (cur + call.nbytes(n) + 511) // 256 * 256
  return place, cur


def solve(call, big, small, rel):
  """Offsets (big, small) with small = big + rel(b0), both aligned; b0 searched in [0, 256)."""
  for b0 in range(0, 256, call.alignment(big)):
    s = b0 + rel(b0)
    if s % call.alignment(small) == 0:
      return b0, s
  raise AssertionError(f"no aligned placement of {small} against {big}")


def placements(call, a, b, kind):
  """Relative byte offsets {a: .., b: ..} of the pair, labelled.  ``kind`` "overlap": identical
  start, shifted by one element, the smaller buffer's last double on the larger one's first and
  its first double on the larger one's last (so an extent computed too short at either end lets
  a placement through); "adjacent": the end of one is the start of the other, both orders (an
  extent computed too long refuses one)."""
  big, small = (a, b) if call.nbytes(a) >= call.nbytes(b) else (b, a)
  nb, ns = call.nbytes(big), call.nbytes(small)
  out = []
  if kind == "adjacent":
    out.append(("small after big",) + solve(call, big, small, lambda b0: nb))
    out.append(("small before big",) + solve(call, big, small, lambda b0: -ns))
  else:
    al = call.alignment(small)
    out.append(("identical start",) + solve(call, big, small, lambda b0: 0))
    shift = call.unit if min(nb, ns) >= 2 * call.unit else 8
    shift = -(-shift // al) * al
    if shift < nb:
      out.append(("shifted by one element",) + solve(call, big, small, lambda b0: shift))
    if ns > 8:  # small's last double on big's first (its last 16 bytes if both need 16)
      last = 16 if call.alignment(big) == call.alignment(small) == 16 else 8
      out.append(("last double inside",) + solve(call, big, small, lambda b0: last - ns))
      if nb > ns:  # and its first double on big's last: pins the far end of big's extent
        out.append(("first double on the last",) + solve(call, big, small,
                                                         lambda b0: (nb - last) // al * al))
    elif nb > 8:  # a one-element buffer on big's last double
      out.append(("on the last double",) + solve(call, big, small,
                                                  lambda b0: (nb - ns) // al * al))
  return [(label, {big: ob, small: os_}) for label, ob, os_ in out]


def place_pair(call, rel):
  """Absolute offsets: the other buffers spread out first, then the pair around a base."""
  others, end = spread(call, skip=tuple(rel))
  room = max(call.nbytes(n) for n in rel) + 512
  base = (end + room + 255) // 256 * 256
  return {**others, **{n: base + off for n, off in rel.items()}}


def field_calls(pkg, gpu, shape, nsteps=8):
  """The linear plan's wrappers at ``shape`` = (N, K, batch)."""
  import torch
  N, K, batch = shape
  op, mesh, dt = ctx(pkg, N, K, batch)
  Np, ktot, field = op.Np, op.ktot, op.field_numel
  f64, i64 = torch.float64, torch.int64
  u0 = noisy_sine(op, 7 + K, batch)
  unit = 8 * Np
  tag = f"N{N}K{K}b{batch}"
  op.tune(steps_per_launch=4, snap_pairs=0)
  snaps = op.new_field(nsteps + 1)
  op.forward(u0.clone(), 0.0, dt, nsteps, snaps)
  eta0 = torch.zeros(ktot, dtype=f64, device=gpu)
  calls = {}

  def fwd(pairs):
    def run(b):
      op.tune(steps_per_launch=4, snap_pairs=pairs)
      op.forward(b["u"], 0.0, dt, nsteps, b["snapshots"])
    return run

  def adj(b):
    op.tune(steps_per_launch=4, snap_pairs=0)
    op.adjoint(b["w"], b["snapshots"], 0.0, dt, nsteps, src_coef=0.25, eta=b["eta"])

  calls["rhs"] = [Call(tag, {"u": (f64, field), "out": (f64, field)}, {"u": u0},
                       lambda b: op.rhs(b["u"], 0.3, out=b["out"]), unit, fields=("u", "out"))]
  calls["forward"] = [
      Call(f"{tag}-{'pairs' if pairs else 'stages'}",
           {"u": (f64, field), "snapshots": (f64, (nsteps + 1) * field)}, {"u": u0}, fwd(pairs),
           unit, fields=("u", "snapshots")) for pairs in (0, 1)]
  calls["adjoint"] = [Call(tag, {"w": (f64, field), "snapshots": (f64, (nsteps + 1) * field),
                                 "eta": (f64, ktot)},
                           {"w": snaps[nsteps], "snapshots": snaps, "eta": eta0}, adj, unit,
                           fields=("w", "snapshots"))]
  return calls


def rec_calls(pkg, gpu, shape):
  """The jump-record wrappers at ``shape``: the launch chains at 8 steps, the sweep pair at 20
  steps as the dataflow launch and as the chains."""
  import torch
  N, K, batch = shape
  op, mesh, dt = ctx(pkg, N, K, batch)
  Np, ktot, field = op.Np, op.ktot, op.field_numel
  f64, i64 = torch.float64, torch.int64
  u0 = noisy_sine(op, 3 + K, batch)
  g = noisy_sine(op, 5 + K, batch)
  unit = 8 * Np
  tag = f"N{N}K{K}b{batch}"
  ld = op.jump_ld
  eta0 = torch.zeros(ktot, dtype=f64, device=gpu)
  zero1 = torch.zeros(1, dtype=i64, device=gpu)
  al = {"jumps": 16}

  def shape_chain():
    op.tune(rec_tile_width=2, rec_steps_per_launch=4, rec_lane_elements=2)

  def shape_sweep(dataflow):
    op.tune(rec_tile_width=2, rec_steps_per_launch=10, rec_fwd_steps_per_launch=20,
            rec_lane_elements=2, rec_sweep=dataflow)
    assert op.query_sweep(20)[0] == bool(dataflow)

  shape_chain()
  jumps8 = op.new_jumps(8)
  op.forward_rec(u0, 0.0, dt, 8, jumps8, out=op.new_field())

  def frec(b):
    shape_chain()
    op.forward_rec(b["u0"], 0.0, dt, 8, b["jumps"], out=b["out"])

  def arec(b):
    shape_chain()
    op.adjoint_rec(b["w"], b["jumps"], 0.0, dt, 8, eta=b["eta"])

  def srec(dataflow):
    def run(b):
      shape_sweep(dataflow)
      op.sweep_rec(b["u0"], b["jumps"], b["w"], 0.0, dt, 20, uN=b["uN"], eta=b["eta"],
                   terminal_state=False)
      if dataflow:
        assert op.sweep_status() == 0
    return run

  def sref(dataflow):
    def run(b):
      shape_sweep(dataflow)
      op.sweep_refine(b["u0"], b["jumps"], b["w"], 0.0, dt, 20, b["eta"], b["idx"], b["value"],
                      b["nonfinite"], uN=b["uN"])
      if dataflow:
        assert op.sweep_status() == 0
    return run

  calls = {}
  calls["forward_rec"] = [Call(tag, {"u0": (f64, field), "jumps": (f64, 8 * ld),
                                     "out": (f64, field)}, {"u0": u0}, frec, unit, al,
                               fields=("u0", "out"))]
  calls["adjoint_rec"] = [Call(tag, {"w": (f64, field), "jumps": (f64, 8 * ld),
                                     "eta": (f64, ktot)},
                               {"w": g, "jumps": jumps8, "eta": eta0}, arec, unit, al,
                               fields=("w",))]
  five = {"u0": (f64, field), "jumps": (f64, 20 * ld), "w": (f64, field), "uN": (f64, field),
          "eta": (f64, ktot)}
  calls["sweep_rec"] = [Call(f"{tag}-{'dataflow' if d else 'chains'}", five,
                             {"u0": u0, "w": g, "eta": eta0}, srec(d), unit, al,
                             fields=("u0", "w", "uN")) for d in (1, 0)]
  eight = {**five, "idx": (i64, 1), "value": (f64, 1), "nonfinite": (i64, 1)}
  calls["sweep_refine"] = [Call(f"{tag}-{'dataflow' if d else 'chains'}", eight,
                                {"u0": u0, "nonfinite": zero1}, sref(d), unit, al,
                                fields=("u0", "w", "uN")) for d in (1, 0)]
  return calls


def config3_calls(pkg, gpu):
  """Config 3 (Burgers flux + SlopeLimitN per stage) at ktot = 509 with the decision record,
  and the two stand-alone limiters on the linear plan of that size."""
  import torch
  N, K, nsteps = 4, 509, 3
  op, mesh, dt = ctx(pkg, N, K, 1, flux="burgers", limiter=True)
  lin, _, _ = ctx(pkg, N, K, 1)
  field, ktot = op.field_numel, op.ktot
  f64, i16, i32 = torch.float64, torch.int16, torch.int32
  x = torch.tensor(mesh.to_device_layout(mesh.x), device=gpu)
  u0 = torch.sin(2 * np.pi * x) + 0.8 * (torch.floor(x * 6) % 2)  # jumps the limiter acts on
  unit = 8 * op.Np
  snaps = op.new_field(nsteps + 1)
  dec = torch.zeros(nsteps * ktot, dtype=i16, device=gpu)
  op.forward(u0.clone(), 0.0, dt, nsteps, snaps, decisions=dec)
  assert int(torch.count_nonzero(dec)) > 0, "the limiter never acted: the record is untested"
  eta0 = torch.zeros(ktot, dtype=f64, device=gpu)
  calls = {}
  calls["forward"] = [Call("config3", {"u": (f64, field), "snapshots": (f64, (nsteps + 1) * field),
                                       "decisions": (i16, nsteps * ktot)}, {"u": u0},
                           lambda b: op.forward(b["u"], 0.0, dt, nsteps, b["snapshots"],
                                                decisions=b["decisions"]),
                           unit, fields=("u", "snapshots"))]
  calls["adjoint"] = [Call("config3", {"w": (f64, field), "snapshots": (f64, (nsteps + 1) * field),
                                       "eta": (f64, ktot), "decisions": (i16, nsteps * ktot)},
                           {"w": snaps[nsteps], "snapshots": snaps, "eta": eta0, "decisions": dec},
                           lambda b: op.adjoint(b["w"], b["snapshots"], 0.0, dt, nsteps,
                                                eta=b["eta"], decisions=b["decisions"]),
                           unit, fields=("w", "snapshots"))]
  calls["slope_limit"] = [Call("K509", {"u": (f64, field), "out": (f64, field), "ids": (i32, ktot)},
                               {"u": u0},
                               lambda b: lin.slope_limit(b["u"], out=b["out"], ids=b["ids"]),
                               unit, fields=("u", "out"))]
  calls["slope_limit_1"] = [Call("K509", {"u": (f64, field), "out": (f64, field)}, {"u": u0},
                                 lambda b: lin.slope_limit_1(b["u"], out=b["out"]), unit,
                                 fields=("u", "out"))]
  return calls


def p_calls(pkg, gpu, N=3, K=300):
  """The p-enriched estimate at (N, K, 1), 8 steps (two blocks of 4): ``estimate`` as the
  dataflow launch and as the launch chain, the fused calls as the dataflow launch."""
  import torch
  nsteps = 8
  op, mesh, dt = ctx(pkg, N, K, 1)
  if ("est", N, K) not in _cache:
    _cache["est", N, K] = pkg.operators.DWREstimate(op)
  est = _cache["est", N, K]
  f64, i64 = torch.float64, torch.int64
  lo, hi, ktot = op.field_numel, est.hi.field_numel, op.ktot
  u0 = noisy_sine(op, 19, 1)
  op.tune(steps_per_launch=4, snap_pairs=0)
  snaps = op.new_field(nsteps + 1)
  op.forward(u0.clone(), 0.0, dt, nsteps, snaps)
  w = est.prolong(snaps[nsteps])
  eta0 = torch.zeros(ktot, dtype=f64, device=gpu)
  zero1 = torch.zeros(1, dtype=i64, device=gpu)
  start = torch.cat([u0, torch.zeros(nsteps * lo, dtype=f64, device=gpu)])
  unit = 8 * op.Np
  three = {"w": (f64, hi), "snapshots": (f64, (nsteps + 1) * lo), "eta": (f64, ktot)}
  six = {**three, "idx": (i64, 1), "value": (f64, 1), "nonfinite": (i64, 1)}
  tag = f"pN{N}K{K}"

  def estimate(flow):
    def run(b):
      est.tune(flow=flow)
      assert est.query_flow(nsteps) == bool(flow)
      est.estimate(b["w"], b["snapshots"], 0.0, dt, nsteps, eta=b["eta"])
      est.tune(flow=1)
    return run

  def estimate_refine(b):
    est.tune(flow=1)
    est.estimate_refine(b["w"], b["snapshots"], 0.0, dt, nsteps, b["eta"], b["idx"], b["value"],
                        b["nonfinite"])

  calls = {}
  calls["prolong"] = [Call(tag, {"u": (f64, lo), "out": (f64, hi)}, {"u": u0},
                           lambda b: est.prolong(b["u"], out=b["out"]), unit,
                           fields=("u", "out"))]
  calls["estimate"] = [Call(f"{tag}-{'dataflow' if flow else 'chain'}", three,
                            {"w": w, "snapshots": snaps, "eta": eta0}, estimate(flow), unit,
                            fields=("w", "snapshots")) for flow in (1, 0)]
  calls["estimate_refine"] = [Call(tag, six, {"w": w, "snapshots": snaps, "nonfinite": zero1},
                                   estimate_refine, unit, fields=("w", "snapshots"))]

  def psweep(b):
    op.tune(steps_per_launch=4, snap_pairs=0)
    est.tune(flow=1)
    est.sweep(b["snapshots"], b["w"], 0.0, dt, nsteps, eta=b["eta"], idx=b["idx"],
              value=b["value"], nonfinite=b["nonfinite"])
    assert op.sweep_status() == 0

  calls["sweep"] = [Call(tag, six, {"snapshots": start, "nonfinite": zero1}, psweep, unit,
                         fields=("w", "snapshots"))]
  return calls


def small_calls(pkg, gpu):
  """Marking, refinement, the field transfers, the reductions and the module functions."""
  import torch
  ops = pkg.operators
  N, K = 4, 600
  op, mesh, dt = ctx(pkg, N, K, 1)
  f64, i64, i32, u8 = torch.float64, torch.int64, torch.int32, torch.uint8
  gen = torch.Generator(device=gpu).manual_seed(5)
  eta = torch.randn(K, dtype=f64, device=gpu, generator=gen)
  marks = torch.zeros(K, dtype=u8, device=gpu)
  marks[[0, 17, 18, 300, 511, 512, 599]] = 1
  n_marked = 7
  zero1 = torch.zeros(1, dtype=i64, device=gpu)
  unit = 8 * op.Np

  def fresh_plan():
    p = ops.DGAdvection1D(mesh)
    p.reserve(2 * K)
    return p

  def refine(b):
    with fresh_plan() as p:
      p.refine(b["idx"], b["h_split"])
      torch.cuda.synchronize()

  def refine_marked(b):
    with fresh_plan() as p:
      assert p.refine_marked(b["marks"], b["parent"]) == (K + n_marked, n_marked)

  if "refined" not in _cache:
    p = fresh_plan()
    parent = torch.zeros(K + n_marked, dtype=i32, device=gpu)
    p.refine_marked(marks, parent)
    _cache["refined"] = (p, parent)
  fine, parent = _cache["refined"]
  coarse_u = noisy_sine(op, 23, 1)
  fine_u = torch.randn(fine.field_numel, dtype=f64, device=gpu, generator=gen)
  x3 = torch.randn(3 * K, dtype=f64, device=gpu, generator=gen)
  cands = torch.stack([torch.randn(4, dtype=f64, device=gpu, generator=gen).abs().view(i64),
                       torch.arange(4, dtype=i64, device=gpu) * 150], dim=1).reshape(-1)
  idx17 = torch.full((1,), 17, dtype=i64, device=gpu)
  src = torch.randn(1002, dtype=f64, device=gpu, generator=gen)  # 16-byte multiple: can touch
  am = {"x": (f64, K), "idx": (i64, 1), "value": (f64, 1), "nonfinite": (i64, 1)}
  across = lambda n_in, n_out, name: {name: (f64, n_in), "parent": (i32, K + n_marked),  # noqa: E731
                                      "out": (f64, n_out)}
  calls = {
      "refine": [Call("K600", {"idx": (i64, 1), "h_split": (f64, 1)}, {"idx": idx17}, refine,
                      unit)],
      "mark": [Call("K600", {"eta": (f64, K), "marks": (u8, K), "info": (i64, 4)}, {"eta": eta},
                    lambda b: op.mark(b["eta"], "top", 5, marks=b["marks"], info=b["info"]),
                    unit)],
      "refine_marked": [Call("K600", {"marks": (u8, K), "parent": (i32, K + n_marked)},
                             {"marks": marks}, refine_marked, unit)],
      "transfer": [Call("K600", across(op.field_numel, fine.field_numel, "u"),
                        {"u": coarse_u, "parent": parent},
                        lambda b: fine.transfer(b["u"], b["parent"], K, out=b["out"]), unit,
                        fields=("u", "out"))],
      "transfer_t": [Call("K600", across(fine.field_numel, op.field_numel, "w"),
                          {"w": fine_u, "parent": parent},
                          lambda b: fine.transfer_t(b["w"], b["parent"], K, out=b["out"]), unit,
                          fields=("w", "out"))],
      "restrict": [Call("K600", across(fine.field_numel, op.field_numel, "u"),
                        {"u": fine_u, "parent": parent},
                        lambda b: fine.restrict(b["u"], b["parent"], K, out=b["out"]), unit,
                        fields=("u", "out"))],
      "argmax_async": [Call("K600", {"x": (f64, K), "out": (i64, 1)}, {"x": eta},
                            lambda b: op.argmax_async(b["x"], out=b["out"]), unit)],
      "argmax_ex": [Call("K600", am, {"x": eta, "nonfinite": zero1},
                         lambda b: op.argmax_ex(b["x"], b["idx"], b["value"], b["nonfinite"]),
                         unit)],
      "slice_candidate": [Call("K600", {"x": (f64, 3 * K), "cand": (i64, 2)}, {"x": x3},
                               lambda b: op.slice_candidate(b["x"].view(3, K), K, 3.0, 100,
                                                            b["cand"]), unit)],
      "stream_copy": [Call("n1002", {"src": (f64, 1002), "dst": (f64, 1002)}, {"src": src},
                           lambda b: ops.stream_copy(b["src"], b["dst"]), unit,
                           {"src": 16, "dst": 16})],
      "sum_rows": [Call("3xK600", {"x": (f64, 3 * K), "out": (f64, K)}, {"x": x3},
                        lambda b: ops.sum_rows(b["x"], 3, out=b["out"]), unit)],
      "candidates_argmax": [Call("W4", {"cands": (i64, 8), "idx": (i64, 1), "value": (f64, 1),
                                        "nonfinite": (i64, 1)},
                                 {"cands": cands, "nonfinite": zero1},
                                 lambda b: ops.candidates_argmax(b["cands"], b["idx"], b["value"],
                                                                 b["nonfinite"]), unit)],
  }
  return calls


def all_calls(pkg, gpu):
  """wrapper -> its variants; the linear sweeps at (4, 600, 1) and (2, 257, 3)."""
  if "calls" not in _cache:
    calls = {}
    for part in (field_calls(pkg, gpu, (4, 600, 1)), field_calls(pkg, gpu, (2, 257, 3)),
                 rec_calls(pkg, gpu, (2, 257, 3)), rec_calls(pkg, gpu, (4, 600, 1)),
                 config3_calls(pkg, gpu), p_calls(pkg, gpu), small_calls(pkg, gpu)):
      for name, variants in part.items():
        calls.setdefault(name, []).extend(variants)
    assert set(calls) == set(TABLE)
    _cache["calls"] = calls
  return _cache["calls"]


PAIRS = [(w, a, b) for w, row in TABLE.items() for (a, b) in row]
PAIR_IDS = [f"{w}-{a}-{b}" for w, a, b in PAIRS]


def variants(pkg, gpu, wrapper, a, b):
  out = [c for c in all_calls(pkg, gpu)[wrapper] if a in c.specs and b in c.specs]
  assert out, f"no call of {wrapper} takes both {a} and {b}"
  return out


def overlaps(call, wrapper, a, b):
  """The refused placements of a pair.  A pair with an allowed identity loses that placement and
  gains the identities next to it."""
  rel = placements(call, a, b, "overlap")
  if TABLE[wrapper][(a, b)] == R:
    return rel
  fb = call.nbytes(a)  # a is the field: u, w or u0
  if wrapper == "forward":  # allowed: u == snapshots + 0
    return rel[1:] + [("u on snapshot 1", {a: fb, b: 0})]
  if wrapper == "adjoint":  # allowed: w == snapshots + nsteps * field
    n = call.nbytes(b) // fb - 1
    return rel + [("w on snapshot nsteps - 1", {a: (n - 1) * fb, b: 0}),
                  ("w one element before the terminal snapshot", {a: n * fb - call.unit, b: 0}),
                  ("w one element past the terminal snapshot", {a: n * fb + call.unit, b: 0})]
  assert wrapper == "forward_rec"  # allowed: out == u0
  return rel[1:]


@pytest.mark.parametrize("wrapper,a,b", PAIRS, ids=PAIR_IDS)
def test_overlap_is_refused_before_anything_is_enqueued(pkg, gpu, wrapper, a, b):
  """(b): DG_ERR_ARG for every overlapping placement, and not one byte of the backing tensor
  changed (the inputs were copied in before the snapshot was taken)."""
  import torch
  for call in variants(pkg, gpu, wrapper, a, b):
    cases = overlaps(call, wrapper, a, b)
    assert len(cases) >= (1 if max(call.nbytes(a), call.nbytes(b)) <= 8 else 2)
    for label, rel in cases:
      back, before, bufs = arena(call, gpu, place_pair(call, rel))
      with pytest.raises(pkg._lib.DGLibraryError, match=r"code -1: .*overlap"):
        call.invoke(bufs)
      torch.cuda.synchronize()
      assert torch.equal(back, before), f"{wrapper} [{call.tag}] {a}/{b} {label}: memory changed"


@pytest.mark.parametrize("wrapper,a,b", PAIRS, ids=PAIR_IDS)
def test_adjacent_buffers_are_accepted(pkg, gpu, wrapper, a, b):
  """(c): the two buffers touching, in both orders: every buffer holds the bits of the run on
  separately allocated tensors and nothing else in the backing tensor changed."""
  import torch
  for call in variants(pkg, gpu, wrapper, a, b):
    ref = call.reference(gpu)
    for label, rel in placements(call, a, b, "adjacent"):
      place = place_pair(call, rel)
      ends = sorted((place[n], place[n] + call.nbytes(n)) for n in (a, b))
      assert ends[0][1] == ends[1][0], "the buffers must touch"
      back, before, bufs = arena(call, gpu, place)
      call.invoke(bufs)
      torch.cuda.synchronize()
      for n, off in place.items():
        before[off:off + call.nbytes(n)] = ref[n]
      assert torch.equal(back, before), f"{wrapper} [{call.tag}] {a}/{b} {label}"


def test_slice_candidate_reads_its_last_row_to_column_n_only(pkg, gpu):
  """x's extent is (rows - 1) * ld + n doubles, not rows * ld: cand on the unread tail of the
  last row is accepted (the bits of a separate cand), cand on the last double read is refused."""
  import torch
  op, _, _ = ctx(pkg, 4, 600, 1)
  rows, ld, n = 3, 600, 597
  back = torch.randn(rows * ld, dtype=torch.float64, device=gpu,
                     generator=torch.Generator(device=gpu).manual_seed(9))
  x = back.view(rows, ld)
  want = op.slice_candidate(x, n, 3.0, 100, torch.zeros(2, dtype=torch.int64, device=gpu))
  torch.cuda.synchronize()
  before = back.clone()
  end = (rows - 1) * ld + n
  with pytest.raises(pkg._lib.DGLibraryError, match=r"code -1: .*overlap"):
    op.slice_candidate(x, n, 3.0, 100, back[end - 1:end + 1].view(torch.int64))
  torch.cuda.synchronize()
  assert torch.equal(back.view(torch.int64), before.view(torch.int64))
  tail = back[end:end + 2].view(torch.int64)
  op.slice_candidate(x, n, 3.0, 100, tail)
  torch.cuda.synchronize()
  assert torch.equal(tail, want)
  assert torch.equal(back[:end].view(torch.int64), before[:end].view(torch.int64))


def test_init_sine_output_may_not_touch_its_inputs(pkg, gpu):
  """dg_init_sine's check (the wrapper makes its own input tensors, so through the ABI): u over
  amp, freq or phase is DG_ERR_ARG; the three inputs, only read, may be one array."""
  import ctypes
  import torch
  op, _, _ = ctx(pkg, 2, 257, 3)
  lib = pkg._lib.load()
  back = torch.full((op.field_numel + 64,), 0.5, dtype=torch.float64, device=gpu)
  before = back.clone()
  ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
  par = back[op.field_numel + 8:op.field_numel + 8 + op.batch]
  for which in range(3):
    for inside in (back[0:], back[op.field_numel - 1:], back[5:]):
      args = [ptr(par)] * 3
      args[which] = ptr(inside)
      assert lib.dg_init_sine(op._plan, *args, ptr(back), None) == pkg._lib.DG_ERR_ARG
      assert b"overlap" in lib.dg_last_error()
  torch.cuda.synchronize()
  assert torch.equal(back, before)
  u = back[:op.field_numel]  # adjacent to nothing it reads; amp == freq == phase
  assert lib.dg_init_sine(op._plan, ptr(par), ptr(par), ptr(par), ptr(u), None) == 0
  want = op.init_sine([0.5] * 3, [0.5] * 3, [0.5] * 3)
  torch.cuda.synchronize()
  assert torch.equal(u, want)


# --------------------------------------------------------------------------------------------
# (d) the allowed aliases
# --------------------------------------------------------------------------------------------
def launches(nsteps, per_launch):
  """Launches of a chain that takes the largest of per_launch, per_launch/2, .. that fits."""
  n, count = nsteps, 0
  while n > 0:
    m = per_launch
    while m > n:
      m >>= 1
    n -= max(m, 1)
    count += 1
  return count


def step_counts(per_launch):
  """3, 8 and 13 steps, plus the fewest steps that take one, two and three launches: both
  ping-pong parities and the single launch that goes through scratch."""
  first = [next(n for n in range(1, 64) if launches(n, per_launch) == c) for c in (1, 2, 3)]
  out = sorted(set(first) | {3, 8, 13})
  assert {launches(n, per_launch) % 2 for n in out} == {0, 1}
  return out


LINEAR_SHAPES = [(4, 600, 1), (2, 257, 3)]


@pytest.mark.parametrize("shape", LINEAR_SHAPES, ids=str)
@pytest.mark.parametrize("pairs", [0, 1], ids=["stages", "pairs"])
def test_forward_in_place_on_snapshot_0(pkg, gpu, shape, pairs):
  """u == snapshots + 0 on the stage-loop kernels and on the Horner pair tiles: snapshot 0 keeps
  u^0, every snapshot equals the separate-buffer run's."""
  import torch
  op, _, dt = ctx(pkg, *shape)
  op.tune(steps_per_launch=4, snap_pairs=pairs)
  u0 = noisy_sine(op, 31, shape[2])
  for nsteps in step_counts(op.steps_per_launch):
    sep, u = op.new_field(nsteps + 1), u0.clone()
    op.forward(u, 0.02, dt, nsteps, sep)
    al = op.new_field(nsteps + 1)
    al[0].copy_(u0)
    op.forward(al[0], 0.02, dt, nsteps, al)
    torch.cuda.synchronize()
    assert torch.equal(al[0], u0) and torch.equal(sep[nsteps], u)
    assert torch.equal(al.view(torch.int64), sep.view(torch.int64)), f"nsteps = {nsteps}"
  op.tune(snap_pairs=0)


@pytest.mark.parametrize("record", [False, True], ids=["retest", "record"])
def test_config3_aliases(pkg, gpu, record):
  """Config 3 (Burgers + SlopeLimitN per stage), with and without the decision record: u on
  snapshot 0 forward, w on the terminal snapshot in the adjoint."""
  import torch
  calls = config3_calls(pkg, gpu)
  op, mesh, dt = ctx(pkg, 4, 509, 1, flux="burgers", limiter=True)
  u0 = calls["forward"][0].inputs["u"]
  counts = step_counts(op.nl_steps_per_launch[0])
  # the limited adjoint has no steps-per-launch setting to query: it recomputes step n from
  # snapshots[n], one launch per step (include/dg_advec.h, dg_plan_set_physics), so its launch
  # count is nsteps itself
  assert {n % 2 for n in counts} == {0, 1}
  for nsteps in counts:
    dec = lambda: (torch.zeros(nsteps * op.ktot, dtype=torch.int16, device=gpu)  # noqa: E731
                   if record else None)
    sep, u, d_sep = op.new_field(nsteps + 1), u0.clone(), dec()
    op.forward(u, 0.0, dt, nsteps, sep, decisions=d_sep)
    al, d_al = op.new_field(nsteps + 1), dec()
    al[0].copy_(u0)
    op.forward(al[0], 0.0, dt, nsteps, al, decisions=d_al)
    torch.cuda.synchronize()
    assert torch.equal(al.view(torch.int64), sep.view(torch.int64)), f"forward, {nsteps} steps"
    if record:
      assert torch.equal(d_al, d_sep)
    w, eta_sep = sep[nsteps].clone(), torch.zeros(op.ktot, dtype=torch.float64, device=gpu)
    op.adjoint(w, sep, 0.0, dt, nsteps, eta=eta_sep, decisions=d_sep)
    eta_al = torch.zeros_like(eta_sep)
    op.adjoint(al[nsteps], al, 0.0, dt, nsteps, eta=eta_al, decisions=d_al)
    torch.cuda.synchronize()
    assert torch.equal(al[nsteps].view(torch.int64), w.view(torch.int64)), f"w, {nsteps} steps"
    assert torch.equal(eta_al.view(torch.int64), eta_sep.view(torch.int64))
    assert torch.equal(al[:nsteps], sep[:nsteps]), "the adjoint wrote a non-terminal snapshot"


@pytest.mark.parametrize("shape", LINEAR_SHAPES, ids=str)
@pytest.mark.parametrize("lane_elements", [2, 1], ids=["pair-tiles", "one-per-lane"])
def test_forward_rec_in_place(pkg, gpu, shape, lane_elements):
  """uN == u0 on the record path's pair tiles and on one element per lane: the state and the
  record of the run into a separate buffer."""
  import torch
  op, _, dt = ctx(pkg, *shape)
  op.tune(rec_tile_width=2, rec_steps_per_launch=4, rec_lane_elements=lane_elements)
  assert op.rec_lane_elements == lane_elements
  u0 = noisy_sine(op, 37, shape[2])
  for nsteps in step_counts(op.rec_fwd_steps_per_launch):
    rec_sep, rec_al = op.new_jumps(nsteps).fill_(0.0), op.new_jumps(nsteps).fill_(0.0)
    sep = op.forward_rec(u0, 0.02, dt, nsteps, rec_sep, out=op.new_field())
    u = u0.clone()
    assert op.forward_rec(u, 0.02, dt, nsteps, rec_al) is u
    torch.cuda.synchronize()
    assert torch.equal(u.view(torch.int64), sep.view(torch.int64)), f"nsteps = {nsteps}"
    assert torch.equal(rec_al.view(torch.int64), rec_sep.view(torch.int64))
  op.tune(rec_lane_elements=2)


# --------------------------------------------------------------------------------------------
# (e) alignment
# --------------------------------------------------------------------------------------------
def aligned_cases(pkg, gpu):
  """Every call with a field-sized argument; the linear sweeps at K * Np odd (N = 4, K = 601),
  so consecutive snapshots alternate between the two alignments as well; the p-estimate also at
  (2, 1601, 1): K * Np odd and four 512-element tiles, two of them interior, the tiles whose
  snapshot rows go straight into LDS (tile_issue_lds)."""
  if "aligned" not in _cache:
    calls = {}
    for part in (field_calls(pkg, gpu, (4, 601, 1)), rec_calls(pkg, gpu, (4, 601, 1)),
                 config3_calls(pkg, gpu), p_calls(pkg, gpu), p_calls(pkg, gpu, 2, 1601),
                 small_calls(pkg, gpu)):
      for name, vs in part.items():
        calls.setdefault(name, []).extend(v for v in vs if v.fields)
    _cache["aligned"] = {k: v for k, v in calls.items() if v}
  return _cache["aligned"]


FIELD_WRAPPERS = ["rhs", "forward", "adjoint", "forward_rec", "adjoint_rec", "sweep_rec",
                  "sweep_refine", "slope_limit", "slope_limit_1", "prolong", "estimate",
                  "estimate_refine", "sweep", "transfer", "transfer_t", "restrict"]


@pytest.mark.parametrize("wrapper", FIELD_WRAPPERS)
def test_eight_byte_alignment_suffices(pkg, gpu, wrapper):
  """(e): each field-sized argument in turn at an odd double offset (8- but not 16-byte aligned),
  the others 256-byte aligned: the bits of the separately allocated (aligned) run."""
  import torch
  cases = aligned_cases(pkg, gpu)
  assert set(cases) == set(FIELD_WRAPPERS)
  for call in cases[wrapper]:
    ref = call.reference(gpu)
    for odd in call.fields:
      place, _ = spread(call)
      place = {n: off + (8 if n == odd else 0) for n, off in place.items()}
      back, before, bufs = arena(call, gpu, place)
      assert bufs[odd].data_ptr() % 16 == 8
      assert all(t.data_ptr() % 16 == 0 for n, t in bufs.items() if n != odd)
      call.invoke(bufs)
      torch.cuda.synchronize()
      for n, off in place.items():
        before[off:off + call.nbytes(n)] = ref[n]
      assert torch.equal(back, before), f"{wrapper} [{call.tag}]: {odd} at 8 mod 16"


def test_sixteen_byte_arguments_refuse(pkg, gpu):
  """The jump record and stream_copy's buffers are read and written 16 bytes per lane with no
  scalar edge path: an 8-byte-aligned pointer is DG_ERR_ARG with nothing enqueued."""
  import torch
  op, _, dt = ctx(pkg, 4, 601, 1)
  u, w = noisy_sine(op, 1, 1), op.new_field().fill_(1.0)
  raw = torch.zeros(8 * op.jump_ld + 2, dtype=torch.float64, device=gpu)
  odd = raw[1:1 + 8 * op.jump_ld]
  assert odd.data_ptr() % 16 == 8
  keep = (u.clone(), w.clone())
  Err = pkg._lib.DGLibraryError
  with pytest.raises(Err, match="code -1: .*16-byte aligned"):
    op.forward_rec(u, 0.0, dt, 8, odd)
  with pytest.raises(Err, match="code -1: .*16-byte aligned"):
    op.adjoint_rec(w, odd, 0.0, dt, 8)
  with pytest.raises(Err, match="code -1: .*16-byte aligned"):
    op.sweep_rec(u, odd, w, 0.0, dt, 8)
  src = torch.ones(12, dtype=torch.float64, device=gpu)
  dst = torch.zeros(13, dtype=torch.float64, device=gpu)
  with pytest.raises(Err, match="code -1: .*16-byte aligned"):
    pkg.operators.stream_copy(src, dst[1:])
  with pytest.raises(Err, match="code -1: .*16-byte aligned"):
    pkg.operators.stream_copy(src[1:11], dst[2:12])
  torch.cuda.synchronize()
  assert torch.equal(u, keep[0]) and torch.equal(w, keep[1])
  assert not raw.any() and not dst.any()


# --------------------------------------------------------------------------------------------
# (f) the wrappers' own checks, with no launch possible
# --------------------------------------------------------------------------------------------
class Stub:
  """Stands in for the ctypes library: records the name of every call and returns DG_OK."""

  def __init__(self):
    self.calls = []

  def __getattr__(self, name):
    def fn(*args):
      self.calls.append(name)
      return 0
    return fn


def refused(stub, exc, what, fn, *args, **kw):
  """``fn`` raises ``exc`` and the library saw nothing: a missing check shows up as a recorded
  call, not as a kernel writing through a bad pointer."""
  try:
    fn(*args, **kw)
    raised = None
  except exc as e:
    raised = e
  assert stub.calls == [], f"{what}: the call reached the library: {stub.calls}"
  assert raised is not None, f"{what}: no {exc.__name__}"


def bad_outputs(torch, gpu, dtype, numel):
  """(what, tensor, exception) for an output of ``numel`` elements of ``dtype``."""
  other = torch.float32 if dtype != torch.float32 else torch.float64
  return [("wrong dtype", torch.zeros(numel, dtype=other, device=gpu), TypeError),
          ("a CPU tensor", torch.zeros(numel, dtype=dtype), TypeError),
          ("not a tensor", [0] * numel, TypeError),
          ("non-contiguous", torch.zeros(2 * numel + 2, dtype=dtype, device=gpu)[::2], TypeError),
          ("one element too few", torch.zeros(numel - 1, dtype=dtype, device=gpu), ValueError)]


def test_module_functions_validate_before_the_library_sees_a_pointer(pkg, gpu, monkeypatch):
  import torch
  ops = pkg.operators
  stub = Stub()
  monkeypatch.setattr(pkg._lib, "load", lambda: stub)
  f64, i64 = torch.float64, torch.int64
  x = torch.ones(12, dtype=f64, device=gpu)
  for what, out, exc in bad_outputs(torch, gpu, f64, 4):
    refused(stub, exc, f"sum_rows, out {what}", ops.sum_rows, x, 3, out=out)
  for rows in (5, 0, -3, 24):
    refused(stub, ValueError, f"sum_rows, rows = {rows}", ops.sum_rows, x, rows)
  cands = torch.zeros(8, dtype=i64, device=gpu)
  ok = {"idx": torch.zeros(1, dtype=i64, device=gpu), "value": torch.zeros(1, dtype=f64, device=gpu),
        "nonfinite": torch.zeros(1, dtype=i64, device=gpu)}
  for name, dtype in (("idx", i64), ("value", f64), ("nonfinite", i64)):
    for what, bad, exc in bad_outputs(torch, gpu, dtype, 1):
      refused(stub, exc, f"candidates_argmax, {name} {what}", ops.candidates_argmax, cands,
              **{**ok, name: bad})
  refused(stub, TypeError, "candidates_argmax, idx None", ops.candidates_argmax, cands, None)
  for n in (7, 1, 0):
    refused(stub, ValueError, "ops.candidates_argmax", ops.candidates_argmax, cands[:n], **ok)
  refused(stub, TypeError, "ops.candidates_argmax", ops.candidates_argmax, cands.cpu(), **ok)
  # the stub is what the functions call: valid arguments reach it
  ops.sum_rows(x, 3, out=torch.zeros(4, dtype=f64, device=gpu))
  ops.candidates_argmax(cands, **ok)
  ops.candidates_argmax(cands, ok["idx"])
  assert stub.calls == ["dg_sum_rows", "dg_candidates_argmax", "dg_candidates_argmax"]


def test_methods_validate_before_the_library_sees_a_pointer(pkg, gpu):
  import torch
  f64, i64 = torch.float64, torch.int64
  mesh = pkg.BaseGalerkin1D(n=2, k=40)
  op = pkg.operators.DGAdvection1D(mesh)
  real, stub = op._lib, Stub()
  op._lib = stub
  try:
    x = torch.ones(40, dtype=f64, device=gpu)
    for what, out, exc in bad_outputs(torch, gpu, i64, 1):
      refused(stub, exc, f"argmax_async, out {what}", op.argmax_async, x, out=out)
    for name, dtype in (("idx", i64), ("value", f64), ("nonfinite", i64)):
      ok = {"idx": torch.zeros(1, dtype=i64, device=gpu)}
      for what, bad, exc in bad_outputs(torch, gpu, dtype, 1):
        refused(stub, exc, f"argmax_ex, {name} {what}", op.argmax_ex, x, **{**ok, name: bad})
    rows = torch.ones(3, 40, dtype=f64, device=gpu)
    cand = torch.zeros(2, dtype=i64, device=gpu)
    for what, bad, exc in bad_outputs(torch, gpu, i64, 2):
      refused(stub, exc, f"slice_candidate, cand {what}", op.slice_candidate, rows, 40, 3.0, 0,
              bad)
    for n in (41, 0, -1):
      refused(stub, ValueError, "op.slice_candidate", op.slice_candidate, rows, n, 3.0, 0, cand)
    for bad_x in (rows[:, ::2], rows.cpu(), rows.float(), rows.reshape(-1)):
      refused(stub, TypeError, "op.slice_candidate", op.slice_candidate, bad_x, 20, 3.0, 0, cand)
    # fields: a CPU tensor, a wrong dtype, a strided view, one element too few or too many
    u = op.new_field()
    for bad, exc in ((u.cpu(), TypeError), (u.float(), TypeError), (u[:-1], ValueError),
                     (torch.zeros(2 * u.numel(), dtype=f64, device=gpu)[::2], ValueError),
                     (torch.zeros(u.numel() + 1, dtype=f64, device=gpu), ValueError)):
      refused(stub, exc, "op.rhs", op.rhs, u, 0.0, out=bad)
      refused(stub, exc, "op.rhs", op.rhs, bad, 0.0, out=u)
    op.argmax_async(x, out=torch.zeros(1, dtype=i64, device=gpu))
    op.argmax_ex(x, torch.zeros(1, dtype=i64, device=gpu))
    op.slice_candidate(rows, 40, 3.0, 0, cand)
    op.rhs(u, 0.0, out=op.new_field())
    assert stub.calls == ["dg_argmax", "dg_argmax_ex", "dg_slice_candidate", "dg_advec_rhs"]
  finally:
    op._lib = real
    op.close()
