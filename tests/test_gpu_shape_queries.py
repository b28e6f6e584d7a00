"""Every shape query of the library against tests/shape_rules.py.

Plans at N = 1, 2, 4, 7, 8 with K = 1000, uniform and not, batch 1 and 3, and one at N = 1 with
K = 3*2^20 + 1 (the other side of the forward record sweep's size rule).  Each key's values are
applied one at a time (every allowed value, and refused ones with their message), then a
fixed-seed sample of 200 combinations within a family; after each, dg_plan_query, _rec,
_rec_fwd, _nl, _p, _sweep / _sweep_ex / _sweep_kernel at nsteps 5, 7, 10, 20, 40 and _p_flow /
_p_sweep / _p_trace at 4, 8, 20, 32, 40 must equal the restatement.  Plans are created, tuned
and queried only: nothing is launched.  (The restatement was held to the library before the
rules moved into csrc/dg_shape.h, by this test run unchanged on that library.)"""
import ctypes
import os
import random
import re

import numpy as np
import pytest

import shape_rules as R

pytestmark = pytest.mark.gpu

SWEEP_STEPS = (5, 7, 10, 20, 40)
P_STEPS = (4, 8, 20, 32, 40)
FAMILIES = {
    "record": (R.REC_TILE_WIDTH, R.REC_FWD_TILE_WIDTH, R.REC_STEPS, R.REC_FWD_STEPS,
               R.REC_LANE_ELEMENTS),
    "sweep": (R.REC_SWEEP, R.SWEEP_WAVES, R.SWEEP_LANE_ELEMENTS, R.SWEEP_EXCHANGE,
              R.REC_TILE_WIDTH, R.REC_STEPS, R.REC_FWD_STEPS),
    "forward": (R.TILE_WIDTH, R.STEPS, R.LANE_ELEMENTS, R.SNAP_PAIRS),
    "p": (R.P_TILE_WIDTH, R.P_STEPS, R.P_FLOW, R.P_SWEEP, R.LANE_ELEMENTS),
    "config3": (R.STEPS, R.NL_EXCHANGE),
}


def horner():
  """The process's DG_P_HORNER mode, as the library reads it."""
  text = os.environ.get("DG_P_HORNER")
  if text is None:
    return 3
  m = re.match(r"\s*([+-]?\d+)", text)  # C atoi
  k = int(m.group(1)) if m else 0
  return k if k in (0, 1, 2) else 3


def values(key, NP):
  """Candidates for a key: every allowed value and some refused ones."""
  if key == R.SPIN_LIMIT:
    return (0, 1, 2**30, 2**30 + 1, -1, 0)
  if key == R.XCD_ORDER:
    return (0, 5, 1)
  return tuple(R.allowed(key, NP)) + (3, 7, -1, 16, 32)


class Plan:
  def __init__(self, pkg, N, K, uniform, batch):
    vx = np.arange(K + 1) / 1024.0  # exact: uniform to the last bit at any K
    if not uniform:
      vx[1:-1] += 0.3 / 1024.0 * np.sin(7.0 * np.arange(1, K))
    self.op = pkg.operators.DGAdvection1D(pkg.BaseGalerkin1D(n=N, v_x=vx), batch=batch)
    self.lib, self.plan = self.op._lib, self.op._plan
    self.N, self.K, self.batch = N, K, batch
    self.s = R.Shape(N + 1, uniform, 5, K * batch, per_n=True).environment(os.environ)

  def q(self, name, n, *args):
    out = (ctypes.c_int64 * n)()
    assert getattr(self.lib, name)(self.plan, *args, out) == 0, name
    return [int(x) for x in out]

  def flag(self, name, nsteps):
    out = ctypes.c_int32(-1)
    assert getattr(self.lib, name)(self.plan, nsteps, ctypes.byref(out)) == 0, name
    return out.value

  def tune(self, key, value):
    rc = self.lib.dg_plan_tune(self.plan, key, value)
    want_rc, want_text = self.s.tune(key, value)
    assert rc == want_rc, (key, value, rc)
    if rc:
      assert self.lib.dg_last_error().decode() == want_text, (key, value)

  def check(self, why):
    s, h = self.s, horner()
    assert self.q("dg_plan_query", 8) == [self.N, s.NP, self.K, self.batch, int(s.uniform),
                                          s.nstages, s.tile_width, R.fwd_steps(s)], why
    assert self.q("dg_plan_query_rec", 4) == [s.rec_tile_width, R.rec_steps(s),
                                              s.rec_lane_elems, R.rec_steps_fwd(s)], why
    assert self.q("dg_plan_query_rec_fwd", 2) == [R.rec_fwd_width(s), R.rec_steps_fwd(s)], why
    assert self.q("dg_plan_query_nl", 3) == [s.nl_exchange, R.nl_steps(s, True),
                                             R.nl_steps(s, False)], why
    assert self.q("dg_plan_query_p", 2) == [s.p_tile_width, R.p_steps(s)], why
    blocks = R.sweep_blocks(s)
    for n in SWEEP_STEPS:
      on, f, a, items, nw, T, _, _ = R.sweep_query(s, n, blocks)
      assert self.q("dg_plan_query_sweep", 4, n) == [on, f, a, items], (why, n)
      assert self.q("dg_plan_query_sweep_ex", 6, n) == [on, f, a, items, nw, T], (why, n)
      kern = [s.NP, int(s.uniform), nw, f, a, s.sweep_lane_elems, s.sweep_exchange,
              R.sweep_occupancy(s, nw)] if on else [0] * 8
      assert self.q("dg_plan_query_sweep_kernel", 8, n) == kern, (why, n)
    for n in P_STEPS:
      assert self.flag("dg_plan_query_p_flow", n) == int(R.p_flow(s, n, h)), (why, n)
      assert self.flag("dg_plan_query_p_sweep", n) == int(R.p_sweep(s, n, h)), (why, n)
      assert self.q("dg_plan_query_p_trace", 3, n) == [*R.p_trace(s, n, h), 8], (why, n)


def exercise(p, seed):
  p.check("defaults")
  for key in sorted(R.KEYS) + [0, 22]:
    for v in (values(key, p.s.NP) if key in R.KEYS else (0, 1)):
      p.tune(key, v)
      p.check((key, v))
  rng = random.Random(seed)
  for i in range(200):
    fam = rng.choice(sorted(FAMILIES))
    for key in FAMILIES[fam]:
      p.tune(key, rng.choice(tuple(R.allowed(key, p.s.NP))))
    p.check((fam, i))


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("uniform", [True, False])
@pytest.mark.parametrize("N", [1, 2, 4, 7, 8])
def test_queries_match_the_rules(pkg, gpu, N, uniform, batch):
  exercise(Plan(pkg, N, 1000, uniform, batch), 1000 * N + 10 * batch + int(uniform))


def test_queries_beyond_the_forward_size_rule(pkg, gpu):
  """K = 3*2^20 + 1: the forward record sweep takes the adjoint's steps per launch."""
  p = Plan(pkg, 1, 3 * 2**20 + 1, True, 1)
  assert p.q("dg_plan_query_rec", 4)[3] == 10
  exercise(p, 7)
