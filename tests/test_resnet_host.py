"""The ResNet-as-ODE ensemble on the host (no GPU): the numpy oracle (tests/resnet_oracle.py)
against independent statements of the same mathematics, the host helpers of
resnet_ensemble, and the conditioning of every input set tests/test_gpu_resnet_ensemble.py
uses (checked here, not assumed there)."""
import numpy as np
import pytest

import resnet_oracle as ro


def perturbed(params, l, k, f, h):
  out = [tuple(x.copy() for x in p) for p in params]
  out[l][k][f] += h
  return out


def fd_case(name):
  return ro.make_case(2, (5, 7, 4), 513) if name == "net3" else ro.case(name)


@pytest.mark.parametrize("name", ["net3", "rf", "one_member"])
def test_oracle_gradients_match_central_differences(name):
  """Analytic parameter gradients of the mean loss against central differences with step
  1e-6; the bar is absolute, 1e-8 of the layer's largest gradient entry (a relative bar trips
  on entries near zero).  The mean loss is piecewise smooth in the parameters, with a kink
  wherever a member's u_l meets a bias: a central difference is the derivative only if no
  member crosses a kink inside the step, so the inputs keep every |u_l - b| above 100 steps
  (asserted; the 4097-member set has a member 7.7e-7 from a bias and is not used here)."""
  times, params, u0, target = fd_case(name)
  h = 1e-6
  U = ro.forward(np.diff(times), params, u0)
  assert min(np.abs(U[l][:, None] - p[0][None, :]).min() for l, p in enumerate(params)) >= 100 * h
  _, grads, _ = ro.loss_grad(times, params, u0, target)
  for l, layer in enumerate(params):
    bar = 1e-8 * max(float(np.abs(g).max()) for g in grads[l])
    for k in range(3):
      for f in range(layer[k].size):
        fd = (ro.mean_loss(times, perturbed(params, l, k, f, h), u0, target)
              - ro.mean_loss(times, perturbed(params, l, k, f, -h), u0, target)) / (2 * h)
        assert abs(fd - grads[l][k][f]) <= bar, (l, k, f, fd, grads[l][k][f])


def test_backward_recursion_is_the_bidiagonal_solve():
  """adjointSolve's pattern (J_F^T - I) v = -K on a 3-layer case: J_F is the Jacobian of the
  fine-grid steps (row n, column n-1: d Phi / d u at u_fine[n-1]), K = dJ/dU is
  sign(u_fine[nf] - target) at the last node and 0 elsewhere.  The oracle's recursion equals
  the dense solve."""
  times, params, u0, target = ro.case("main")
  rf = 4
  s = ro.sweep(times, params, u0, target, rf)
  dt, t_coarse, dt_fine, t_fine = ro.grids(times, rf)
  Uf = ro.interp_members(t_fine, t_coarse, s["U"])
  nf = dt_fine.size
  assert nf == 12
  for ic in (0, 17, 4096):
    J = np.zeros((nf + 1, nf + 1))
    for n in range(1, nf + 1):
      J[n, n - 1] = ro.dphi_du(Uf[n - 1, ic:ic + 1], dt_fine[n - 1], params[(n - 1) // rf])[0]
    K = np.zeros(nf + 1)
    K[nf] = np.sign(Uf[nf, ic] - target[ic])
    v = np.linalg.solve(J.T - np.eye(nf + 1), -K)
    assert ro.rel(s["V"][:, ic], v) <= 1e-13


def test_oracle_interpolation_is_numpy_interp():
  times, params, u0, target = ro.case("main")
  for rf in (2, 3, 4, 16):
    dt, t_coarse, _, t_fine = ro.grids(times, rf)
    U = ro.forward(dt, params, u0[:64])
    Uf = ro.interp_members(t_fine, t_coarse, U)
    for ic in range(U.shape[1]):
      np.testing.assert_array_equal(Uf[:, ic], np.interp(t_fine, t_coarse, U[:, ic]))


def test_split_layer_and_refine_time_on_hand_worked_meshes(pkg):
  rn = pkg.resnet_ensemble
  layer = lambda c: (np.array([c, c + 1.0]), np.array([c + 2.0]), np.array([c + 3.0]))  # noqa: E731
  times, params = np.array([0.0, 0.5, 1.0]), [layer(10.0), layer(20.0)]
  # idx = 1: the first interval is halved, layer 0 is copied to position 1
  t1, p1 = rn.split_layer(times, params, 1)
  np.testing.assert_array_equal(t1, [0.0, 0.25, 0.5, 1.0])
  assert [p[0][0] for p in p1] == [10.0, 10.0, 20.0]
  # idx = L: the last interval is halved, the last layer is copied to the end
  t2, p2 = rn.split_layer(times, params, 2)
  np.testing.assert_array_equal(t2, [0.0, 0.5, 0.75, 1.0])
  assert [p[0][0] for p in p2] == [10.0, 20.0, 20.0]
  # a non-uniform 3-interval mesh, the middle interval
  t3, p3 = rn.split_layer(np.array([0.0, 0.125, 0.625, 1.0]), params + [layer(30.0)], 2)
  np.testing.assert_array_equal(t3, [0.0, 0.125, 0.375, 0.625, 1.0])
  assert [p[0][0] for p in p3] == [10.0, 20.0, 20.0, 30.0]
  # the copy is a copy: changing it leaves its source alone; the inputs are untouched
  p3[2][0][0] = -1.0
  assert p3[1][0][0] == 20.0 and len(params) == 2 and times.size == 3
  for a, b in zip(p2[2], params[1]):
    np.testing.assert_array_equal(a, b)
  for bad in (0, 3):
    with pytest.raises(ValueError):
      rn.split_layer(times, params, bad)
  # the oracle's own statement agrees
  for idx in (1, 2):
    to, po = ro.split_layer(times, params, idx)
    tn, pn = rn.split_layer(times, params, idx)
    np.testing.assert_array_equal(to, tn)
    for a, b in zip(po, pn):
      for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)
  dt_fine, t_fine = rn.refine_time(np.array([0.5, 0.25]), 2)
  np.testing.assert_array_equal(dt_fine, [0.25, 0.25, 0.125, 0.125])
  np.testing.assert_array_equal(t_fine, [0.0, 0.25, 0.5, 0.625, 0.75])
  dt_fine, t_fine = rn.refine_time(np.array([0.75]), 3)
  np.testing.assert_array_equal(dt_fine, [0.25, 0.25, 0.25])
  np.testing.assert_array_equal(t_fine, [0.0, 0.25, 0.5, 0.75])


def test_ensemble_refuses_cpu(pkg):
  import torch
  if torch.cuda.is_available():
    pytest.skip("GPU present")
  times, params, u0, target = ro.case("one_member")
  with pytest.raises(pkg._lib.DGLibraryError):
    pkg.resnet_ensemble.ResNetEnsemble(times, params, u0, target)


def check_conditioning(times, params, u0, target, rf, what):
  """min |z| and min |u_L - target| over ALL members >= 1e-9, and the oracle's own
  float64-vs-longdouble difference d <= 1e-13 (what keeps the GPU tests' 1e-12 meaningful)."""
  s = ro.sweep(times, params, u0, target, rf)
  hi = ro.sweep(times, params, u0, target, rf, np.longdouble)
  assert s["U"].shape[1] == np.asarray(u0).size  # no member is left out
  d = max(ro.rel(s[k], hi[k]) for k in ("U", "V", "err"))
  print(f"{what}: zmin {s['zmin']:.2e} smin {s['smin']:.2e} d {d:.2e}")
  assert s["zmin"] >= 1e-9, what
  assert s["smin"] >= 1e-9, what
  assert d <= 1e-13, what
  return d


@pytest.mark.parametrize("name", sorted(ro.CASES))
def test_gpu_inputs_are_well_conditioned(name):
  times, params, u0, target = ro.case(name)
  assert u0.size == ro.CASES[name][2]
  for rf in ro.CASES[name][3]:
    check_conditioning(times, params, u0, target, rf, f"{name} rf {rf}")


def test_gpu_adapt_inputs_are_well_conditioned():
  """Every iteration of the depth-adaptation test: conditioning as above, and the two largest
  mean indicators differ by more than 1e-9 relative, so the argmax is not a rounding matter."""
  times, params, u0, target = ro.case("main")
  its = ro.adapt_loop(times, params, u0, target, 4, ro.ADAPT_ITERATIONS)
  for i, it in enumerate(its[:-1]):
    check_conditioning(it["times"], it["params"], u0, target, 4, f"adapt iteration {i}")
    top = np.sort(it["mean"])[::-1]
    assert (top[0] - top[1]) / top[0] > 1e-9
  assert len(its[-1]["params"]) == 3 + ro.ADAPT_ITERATIONS


@pytest.mark.parametrize("name", ["main", "one_member", "wide129", "deep256"])
def test_gpu_gradient_inputs_are_well_conditioned(name):
  times, params, u0, target = ro.case(name)
  loss, grads, _ = ro.loss_grad(times, params, u0, target)
  loss_hi, grads_hi, _ = ro.loss_grad(times, params, u0, target, np.longdouble)
  d = max(ro.rel(g, h) for gl, hl in zip(grads, grads_hi) for g, h in zip(gl, hl))
  d = max(d, abs(float(loss - loss_hi)) / float(loss_hi))
  print(f"{name}: gradient d {d:.2e}")
  assert d <= 1e-13


def test_gpu_training_inputs_are_well_conditioned():
  """Adam's update is lr * m_hat / (sqrt(v_hat) + eps), +-lr at the first steps whatever the
  gradient's size, so a gradient error dg moves a parameter by up to lr * eps * dg / g^2.
  With dg <= 1e-12 * gmax (the GPU gradient's bar) that must stay below 1e-11, a tenth of the
  1e-10 bar on the trained parameters, for every entry that is not exactly zero (a neuron
  no member activates has exactly zero gradients on the device too: its sums add zeros)."""
  times, params, u0, target = ro.case("main")
  lr, eps = 1e-3, 1e-8
  _, _, all_grads = ro.adam_train(times, params, u0, target, ro.TRAIN_EPOCHS, lr=lr)
  for grads in all_grads:
    flat = np.concatenate([g for layer in grads for g in layer])
    gmax, gmin = np.abs(flat).max(), np.abs(flat[flat != 0.0]).min()
    assert lr * eps * 1e-12 * gmax / gmin ** 2 <= 1e-11, (gmax, gmin)
