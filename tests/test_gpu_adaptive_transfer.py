"""adaptive.AdaptiveSweep with nodal initial data (``ic`` a tensor): the config-3 adapt loop
(Burgers flux, SlopeLimitN per stage) carrying the data across every refinement on the device,
against tests/transfer_oracle.py."""
import numpy as np
import pytest

import mark_oracle as mo
import transfer_oracle as to

pytestmark = pytest.mark.gpu

N, K0, NSTEPS = 4, 200, 8
NP = N + 1
IC = (1.0, 1.0, 0.0)


def sweep(pkg, max_refinements, marking, ic=IC, v_x=None):
  mesh = pkg.BaseGalerkin1D(n=N, k=K0) if v_x is None else pkg.BaseGalerkin1D(n=N, v_x=v_x)
  return pkg.adaptive.AdaptiveSweep(mesh, NSTEPS, max_refinements, flux="burgers", limiter=True,
                                    marking=marking, ic=ic)


def sine_on_initial_mesh(pkg):
  """The tensor op.init_sine writes on the initial mesh."""
  with pkg.operators.DGAdvection1D(pkg.BaseGalerkin1D(n=N, k=K0)) as op:
    return op.init_sine([IC[0]], [IC[1]], [IC[2]])


def bits(x):
  return np.ascontiguousarray(x).view(np.int64)


@pytest.mark.parametrize("marking", (None, ("max", 0.5)), ids=("argmax", "max"))
def test_first_iteration_matches_the_analytic_ic(pkg, gpu, marking):
  import torch
  a, b = sweep(pkg, 300, marking), sweep(pkg, 300, marking, ic=sine_on_initial_mesh(pkg))
  assert a.dt == b.dt
  for s in (a, b):
    s.forward()
    s.adjoint()
  assert torch.equal(a.snapshots(), b.snapshots()) and torch.equal(a.eta(), b.eta())
  for s in (a, b):
    s.refine()
  assert a.sync() == b.sync() and a.history == b.history and a.K == b.K > K0
  np.testing.assert_array_equal(a.op.v_x(), b.op.v_x())
  with pytest.raises(RuntimeError):
    a.u0()


@pytest.mark.parametrize("marking", (None, ("max", 0.5)), ids=("argmax", "max"))
def test_carried_data_follows_the_oracle(pkg, gpu, marking):
  import torch
  run = sweep(pkg, 3000, marking, ic=sine_on_initial_mesh(pkg))
  run.op._split_matrix("PL")
  PL = run.op._split["PL"][0]
  for it in range(4):
    K, vx = run.K, run.op.v_x()
    before = run.u0().cpu().numpy()
    assert before.size == K * NP
    dt = run.dt
    run.forward(dt)
    assert torch.equal(run.snapshots()[0], run.u0())
    run.adjoint(dt)
    run.refine()
    n = run.sync()
    if marking is None:
      marks = np.zeros(K, dtype=np.uint8)
      marks[n] = 1
    else:
      marks = run._marks[:K].cpu().numpy()
      assert n == int(marks.sum()) >= 1
    vx_new, parent = mo.split_marked(vx, marks)
    np.testing.assert_array_equal(run.op.v_x(), vx_new)
    assert run.K == len(parent)
    after = run.u0().cpu().numpy()
    want = to.to_children(before, parent, K, PL)
    err = float(np.max(np.abs(after - want)))
    print(f"iteration {it}: K {K} -> {run.K}, carried u0 vs the oracle {err:.3e}")
    assert err <= 1e-13 * np.max(np.abs(before))
    same = to.roles(parent) == 0
    np.testing.assert_array_equal(bits(after).reshape(-1, NP)[same],
                                  bits(before).reshape(-1, NP)[parent[same]])
  # a sweep created on the final mesh with the carried data computes the same
  fresh = sweep(pkg, 0, None, ic=run.u0().clone(), v_x=run.op.v_x())
  dt = run.dt
  assert abs(dt - fresh.dt) <= 1e-12 * dt
  for s in (run, fresh):
    s.forward(dt)
    s.adjoint(dt)
  assert torch.equal(run.snapshots(), fresh.snapshots())
  assert torch.equal(run.eta(), fresh.eta())


def test_a_nan_indicator_leaves_the_carried_data(pkg, gpu):
  import torch
  run = sweep(pkg, 50, ("top", 4), ic=sine_on_initial_mesh(pkg))
  dt = run.dt
  run.forward(dt)
  run.adjoint(dt)
  run._eta[17] = float("nan")
  vx, u0 = run.op.v_x(), run.u0().clone()
  run.refine()
  with pytest.raises(FloatingPointError):
    run.sync()
  assert run.K == K0 and run.op.K == K0 and run.history == []
  np.testing.assert_array_equal(run.op.v_x(), vx)
  assert run.u0().numel() == K0 * NP and torch.equal(run.u0(), u0)


def test_initial_data_arguments(pkg, gpu):
  import torch
  good = sine_on_initial_mesh(pkg)
  with pytest.raises(ValueError):
    sweep(pkg, 4, None, ic=good[:-1])
  with pytest.raises(TypeError):
    sweep(pkg, 4, None, ic=good.cpu())
  with pytest.raises(TypeError):
    sweep(pkg, 4, None, ic=good.float())
  run = sweep(pkg, 4, None, ic=good.view(K0, NP))  # any shape with that many elements
  assert torch.equal(run.u0(), good)
  good.zero_()  # the sweep holds its own copy
  assert float(run.u0().abs().max()) > 0.5
