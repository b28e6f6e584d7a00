"""Helper of tests/test_gpu_stream_order.py: one entry point run on a DELAYED side stream.

include/dg_advec.h promises that compute calls are asynchronous on ``stream`` and every Python
wrapper passes torch's current stream.  On the default stream (where the rest of the suite
runs) a launch, fill or copy written with stream 0 instead of ``st``, a wrapper that hands the
library ``None``, or a torch op issued outside the current stream all give the same bits.  Here
they do not.  ``run_case`` runs a case three times:

1. Reference, on the default stream: inputs A, outputs filled with sentinel S1, run,
   synchronise, keep the outputs.  This run absorbs lazy allocations, and the callable's
   host-side return-to-return time ``t_host`` is taken from it.
2. Stale state, on the default stream: inputs B, run, synchronise.  The plan's scratch, record
   and lists now hold B-derived values of the same shapes.  B stays in the inputs, S1 goes into
   the outputs.  Every floating-point output of B must differ from A's (a condition on the
   case; integer outputs that record decisions pinned equal in A and B are named in
   ``same_ok``).
3. Delayed, on a fresh side stream ``s`` with no host synchronisation until the end: a delay of
   ordinary bounded work (repeated ``Tensor.copy_`` of one 256 MiB buffer, at least
   10 x ``t_host`` of device time -- 10 x the host time of step 1's loads is added, since step
   3 enqueues its loads behind the delay too -- and never less than ``MIN_DELAY_MS`` or one
   copy pair), event E,
   the copies that
   load A into the inputs and sentinel S2 into the outputs, the entry point under
   ``torch.cuda.stream(s)``, ``pending = not E.query()`` read at once, a copy of every output
   into a buffer allocated beforehand, ``s.synchronize()``.

Work that lands on the null stream, or on any stream other than ``s``, runs during the delay:
it reads B and B-derived scratch and writes over S1; afterwards S2 and the on-stream work
overwrite or miss it, and the copies differ from the reference.  A call that waits for the
stream or the device returns after the delay has drained: ``pending`` is false.

Safety of the stale state: a misordered launch must still read in-range data, so every
index-like input (idx, parent, marks, interp codes, offsets, decisions, candidate indices, time
meshes) holds the same valid values in A and B; only fp64 payloads differ, on the same plan,
shapes and tunables.  Entry points that change the plan are built afresh for each of the three
runs (``fresh=True``): their stale state is the B in their buffers only.
"""
import ctypes
import math
import time

S1 = {"float": -3.5e200, "int": 0x5a}
S2 = {"float": 7.75e250, "int": 0x33}
DELAY_WORDS = 1 << 25   # doubles: one 256 MiB buffer, copied back and forth
FACTOR = 10             # the delay's device time in units of the case's t_host
MIN_DELAY_MS = 5.0      # and its floor: work misplaced on another stream is seen only if it
                        # lands before step 3's S2 fill, i.e. within the delay; 5 ms is some
                        # hundred times the ~10 us it takes a launch, fill or copy to start

LOG = []                # one dict per run_case: name, t_host, pairs, delay_ms, pending, wall


class Ctx:
  """What a case hands the harness.

  run      enqueues the entry point on torch's current stream; may return a dict of tensors it
           allocated itself (outputs of the Python layers), compared like the named outputs
  bufs     name -> tensor the entry point reads or writes (CUDA, or pinned host memory the
           kernels write through ``host_alias``)
  A, B     name -> tensor: two valid input sets for the input and in-out names of ``bufs``
  outputs  names of ``bufs`` that are outputs or in-outs
  same_ok  outputs (and returned names) that may be equal for A and B
  after    optional: called once the run has been synchronised, returns a dict of further
           tensors to compare (what only a waiting call can read, e.g. the plan's mesh)
  """

  def __init__(self, run, bufs, A, B, outputs, same_ok=(), after=None):
    assert set(A) == set(B) and set(A) <= set(bufs) and set(outputs) <= set(bufs)
    self.run, self.bufs, self.A, self.B = run, bufs, A, B
    self.outputs, self.same_ok, self.after = list(outputs), set(same_ok), after


def _kind(t):
  return "float" if t.is_floating_point() else "int"


def _load(ctx, vals, sentinel):
  """Inputs := vals, pure outputs := sentinel, on torch's current stream (pinned host outputs
  at once on the host)."""
  for name, t in ctx.bufs.items():
    if name in vals:
      t.copy_(vals[name])
    elif name in ctx.outputs:
      t.fill_(sentinel[_kind(t)])


def _extra(ctx, extra):
  out = dict(extra) if isinstance(extra, dict) else {}  # a wrapper's own return value: not ours
  if ctx.after is not None:
    out.update(ctx.after())
  return out


def _keep(ctx, extra):
  out = {n: ctx.bufs[n].clone() for n in ctx.outputs}
  for n, t in _extra(ctx, extra).items():
    out[n] = t.clone()
  return out


def _same(a, b):
  """Bit-identical (NaNs included): the tensors' bytes."""
  import torch
  return a.shape == b.shape and a.dtype == b.dtype and torch.equal(
      a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8))


class Delay:
  """The delay: pairs of ``Tensor.copy_`` between two 256 MiB buffers (torch's own copy, not a
  wrapper under test).  ``pair_ms`` is the device time of one pair, measured once with events
  around 8 of them after a warm-up."""

  def __init__(self, device):
    import torch
    self.a = torch.zeros(DELAY_WORDS, dtype=torch.float64, device=device)
    self.b = torch.empty_like(self.a)
    self.enqueue(2)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    self.enqueue(8)
    e1.record()
    torch.cuda.synchronize()
    self.pair_ms = e0.elapsed_time(e1) / 8

  def enqueue(self, pairs):
    for _ in range(pairs):
      self.b.copy_(self.a)
      self.a.copy_(self.b)

  def pairs_for(self, t_host):
    return max(1, math.ceil(max(FACTOR * t_host * 1e3, MIN_DELAY_MS) / self.pair_ms))


# --- the side stream ---------------------------------------------------------------------
# "torch": torch.cuda.Stream().  "external": hipStreamCreateWithFlags(hipStreamNonBlocking)
# from the runtime torch has loaded, wrapped in torch.cuda.ExternalStream -- for a torch whose
# pool streams block on the null stream (the module's self-test selects the form).
STREAM_FORM = "torch"
_HIP_STREAM_NON_BLOCKING = 1
_external = []


def _create_stream(device):
  import torch
  if STREAM_FORM == "torch":
    return torch.cuda.Stream(device)
  hip = ctypes.CDLL("libamdhip64.so")
  h = ctypes.c_void_p()
  with torch.cuda.device(device):
    rc = hip.hipStreamCreateWithFlags(ctypes.byref(h), ctypes.c_uint(_HIP_STREAM_NON_BLOCKING))
  assert rc == 0 and h.value, "hipStreamCreateWithFlags failed"
  _external.append(h)
  return torch.cuda.ExternalStream(h.value, device=device)


PROBE_PAIRS = 12   # the delay of the independence probe below (about 2 ms)
_tried = []        # candidates stay referenced, so that the next one is another stream


def new_stream(device, delay):
  """A side stream that null-stream work overtakes while it is delayed.  The runtime maps its
  streams onto a few hardware queues, and work queued on the null stream behind a delayed stream
  of the SAME hardware queue runs after the delay, in order: such a stream would hide every
  misplaced launch.  So each candidate is probed (a short delay on it, then a fill on the null
  stream, which must finish while the delay is still running) and the first independent one is
  taken; the probe synchronises, before step 3 begins."""
  import torch
  null = torch.cuda.default_stream(device)
  word = torch.zeros(1, dtype=torch.int64, device=device)
  for _ in range(16):
    s = _create_stream(device)
    _tried.append(s)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
      delay.enqueue(PROBE_PAIRS)
      es = torch.cuda.Event()
      es.record(s)
    with torch.cuda.stream(null):
      word.fill_(1)
      en = torch.cuda.Event()
      en.record(null)
    en.synchronize()
    independent = not es.query()
    s.synchronize()
    if independent:
      return s
  raise AssertionError("no side stream that null-stream work overtakes (16 candidates)")


class Result:
  def __init__(self, ref, got, pending, t_host, pairs):
    self.ref, self.got, self.pending, self.t_host, self.pairs = ref, got, pending, t_host, pairs

  def differing(self):
    return sorted(n for n in self.ref if not _same(self.ref[n], self.got[n]))


def run_case(name, make, delay, fresh=False):
  """The three runs of the module docstring; returns a ``Result`` (reference outputs, the
  delayed run's, ``pending``, ``t_host`` in seconds, copy pairs of the delay)."""
  import torch
  wall = time.perf_counter()
  # 1. reference
  ctx = make()
  dev = next(t.device for t in ctx.bufs.values() if t.is_cuda)
  t0 = time.perf_counter()
  _load(ctx, ctx.A, S1)
  t_load = time.perf_counter() - t0
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  extra = ctx.run()
  t_host = time.perf_counter() - t0
  torch.cuda.synchronize()
  ref = _keep(ctx, extra)
  # 2. stale state
  if fresh:
    ctx = make()
  _load(ctx, ctx.B, S1)
  torch.cuda.synchronize()
  extra = ctx.run()
  torch.cuda.synchronize()
  stale = _keep(ctx, extra)
  alike = [n for n in ref if n not in ctx.same_ok and ref[n].is_floating_point()
           and _same(ref[n], stale[n])]
  assert not alike, f"{name}: outputs {alike} are the same for A and B (a condition on the case)"
  assert any(not _same(ref[n], stale[n]) for n in ref), f"{name}: A and B give the same outputs"
  if fresh:
    ctx = make()
  _load(ctx, ctx.B, S1)
  got = {n: torch.empty_like(ctx.bufs[n]) for n in ctx.outputs}
  pairs = delay.pairs_for(t_host + t_load)  # the loads of step 3 are enqueued inside it too
  s = new_stream(dev, delay)
  with torch.cuda.stream(s):  # blocks of these sizes in s's allocator pool, for the wrappers
    warm = [torch.empty_like(t) for t in ref.values() if t.is_cuda]  # that allocate outputs
  del warm
  torch.cuda.synchronize()
  # 3. the delayed run: nothing below waits for the device before s.synchronize()
  host_out = [n for n in ctx.outputs if not ctx.bufs[n].is_cuda]
  for n in host_out:  # pinned host outputs: the host fills them itself, before the delay
    if n not in ctx.A:
      ctx.bufs[n].fill_(S2[_kind(ctx.bufs[n])])
  with torch.cuda.stream(s):
    delay.enqueue(pairs)
    E = torch.cuda.Event()
    E.record(s)
    for n, t in ctx.bufs.items():
      if t.is_cuda:
        if n in ctx.A:
          t.copy_(ctx.A[n])
        elif n in ctx.outputs:
          t.fill_(S2[_kind(t)])
    extra = ctx.run()
    pending = not E.query()
    for n in ctx.outputs:
      if ctx.bufs[n].is_cuda:
        got[n].copy_(ctx.bufs[n])
  s.synchronize()
  for n in host_out:
    got[n].copy_(ctx.bufs[n])
  for n, t in _extra(ctx, extra).items():
    got[n] = t
  torch.cuda.synchronize()
  LOG.append(dict(name=name, t_host=t_host, pairs=pairs, delay_ms=pairs * delay.pair_ms,
                  pending=pending, wall=time.perf_counter() - wall))
  return Result(ref, got, pending, t_host, pairs)
