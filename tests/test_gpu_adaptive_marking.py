"""adaptive.AdaptiveSweep with a marking strategy: the config-3 adapt loop (Burgers flux,
SlopeLimitN per stage) refining a set of elements per iteration."""
import numpy as np
import pytest

import mark_oracle as mo

pytestmark = pytest.mark.gpu

N, K0, NSTEPS = 4, 200, 8


def sweep(pkg, max_refinements, marking, v_x=None):
  mesh = pkg.BaseGalerkin1D(n=N, k=K0) if v_x is None else pkg.BaseGalerkin1D(n=N, v_x=v_x)
  return pkg.adaptive.AdaptiveSweep(mesh, NSTEPS, max_refinements, flux="burgers", limiter=True,
                                    marking=marking)


def test_top_one_is_the_unmarked_loop(pkg, gpu):
  a, b = sweep(pkg, 6, None), sweep(pkg, 6, ("top", 1))
  split = []
  for _ in range(5):
    before = b.op.v_x()
    a.iterate()
    dofs, n = b.iterate()
    assert n == 1 and dofs == 2 * (N + 1) * (b.K - 1) * NSTEPS
    after = b.op.v_x()
    new = np.flatnonzero(~np.isin(after, before))
    assert len(new) == 1
    split.append(int(new[0]) - 1)
    assert a.dt == b.dt
  assert split == a.history and b.history == [1] * 5
  np.testing.assert_array_equal(a.op.v_x(), b.op.v_x())


def test_max_fraction_loop_follows_the_oracle(pkg, gpu):
  import torch
  run = sweep(pkg, 3000, ("max", 0.5))
  for it in range(4):
    K, vx = run.K, run.op.v_x()
    ref_mesh = pkg.BaseGalerkin1D(n=N, v_x=vx)
    assert abs(run.dt - ref_mesh.cfl_dt()) <= 1e-12 * ref_mesh.cfl_dt()
    dt = run.dt
    run.forward(dt)
    run.adjoint(dt)
    eta = run.eta().cpu().numpy()
    run.refine()
    marks = run._marks[:K].cpu().numpy()
    np.testing.assert_array_equal(marks, mo.max_fraction(eta, 0.5, cap=3000 + K0 - K))
    n = run.sync()
    assert n == int(marks.sum()) >= 1 and run.K == K + n and run.history[-1] == n
    np.testing.assert_array_equal(run.op.v_x(), mo.split_marked(vx, marks)[0])
  # the refined plan computes what a plan created on its mesh computes
  fresh = sweep(pkg, 0, None, v_x=run.op.v_x())
  dt = run.dt
  assert abs(dt - fresh.dt) <= 1e-12 * dt
  for s in (run, fresh):
    s.forward(dt)
    s.adjoint(dt)
  assert torch.equal(run.eta(), fresh.eta())
  assert torch.equal(run.snapshots(), fresh.snapshots())


def test_a_small_reserve_truncates_in_rank_order(pkg, gpu):
  run = sweep(pkg, 3, ("max", 2.0 ** -60))
  dt = run.dt
  run.forward(dt)
  run.adjoint(dt)
  eta = run.eta().cpu().numpy()
  assert int(mo.max_fraction(eta, 2.0 ** -60).sum()) > 3  # more candidates than room
  run.refine()
  marks = run._marks[:K0].cpu().numpy()
  np.testing.assert_array_equal(marks, mo.top_count(eta, 3))
  assert run.sync() == 3 and run.K == K0 + 3
  with pytest.raises(RuntimeError, match="capacity"):
    run.iterate()
  assert run.K == K0 + 3


def test_a_nan_indicator_raises_before_any_split(pkg, gpu):
  run = sweep(pkg, 50, ("top", 4))
  dt = run.dt
  run.forward(dt)
  run.adjoint(dt)
  run._eta[17] = float("nan")
  vx = run.op.v_x()
  run.refine()
  with pytest.raises(FloatingPointError):
    run.sync()
  assert run.K == K0 and run.op.K == K0 and run.history == []
  np.testing.assert_array_equal(run.op.v_x(), vx)


def test_marking_arguments(pkg, gpu):
  with pytest.raises(ValueError):
    sweep(pkg, 3, ("bulk", 0.5))
  run = sweep(pkg, 0, ("top", 2))
  with pytest.raises(RuntimeError, match="capacity"):
    run.iterate()
