"""The split matrices of galerkin.split_interpolation and the transfer operators they define
(tests/transfer_oracle.py), on the host: no GPU."""
import numpy as np
import pytest

import mark_oracle as mo
import transfer_oracle as to

ORDERS = range(1, 9)


def matrices(pkg, N):
  mesh = pkg.BaseGalerkin1D(n=N, k=2)
  PL, RL = pkg.galerkin.split_interpolation(mesh)
  return mesh, PL, RL


def random_refinement(N, K, seed):
  """(old vertices, marks, new vertices, parent) of a random non-uniform mesh."""
  rng = np.random.default_rng(seed)
  vx = np.concatenate(([0.0], np.cumsum(rng.uniform(0.2, 1.8, K))))
  vx /= vx[-1]
  marks = (rng.random(K) < 0.5).astype(np.uint8)
  marks[[0, K - 1]] = 1, 0
  new, parent = mo.split_marked(vx, marks)
  return vx, marks, new, parent


@pytest.mark.parametrize("N", ORDERS)
def test_left_child_rows_sum_to_one(pkg, N):
  _, PL, _ = matrices(pkg, N)
  assert PL.shape == (N + 1, N + 1)
  assert np.max(np.abs(PL.sum(axis=1) - 1.0)) <= 1e-13


@pytest.mark.parametrize("N", ORDERS)
def test_right_child_is_the_reversed_left_child(pkg, N):
  mesh, PL, _ = matrices(pkg, N)
  direct = mesh.vandermonde1D(N, 0.5 * (mesh.r_gl + 1.0)) @ mesh.inv_v
  assert np.max(np.abs(to.reversed_matrix(PL) - direct)) <= 1e-13


@pytest.mark.parametrize("N", ORDERS)
def test_projection_inverts_interpolation(pkg, N):
  _, PL, RL = matrices(pkg, N)
  PR, RR = to.reversed_matrix(PL), to.reversed_matrix(RL)
  assert np.max(np.abs(RL @ PL + RR @ PR - np.eye(N + 1))) <= 1e-13


@pytest.mark.parametrize("N", ORDERS)
def test_prolonging_a_polynomial_is_exact(pkg, N):
  """A degree-N polynomial with O(1) Legendre coefficients on the domain's reference
  interval, sampled on a random non-uniform mesh and prolonged, is its samples on the split
  mesh to 1e-12 max|p| (the bar tests/test_host.py holds the host operators to)."""
  K = 13
  vx, marks, new, parent = random_refinement(N, K, 40 + N)
  coef = np.random.default_rng(N).uniform(-1.0, 1.0, N + 1)
  p = lambda x: np.polynomial.legendre.legval(2.0 * x - 1.0, coef)  # noqa: E731
  old = pkg.BaseGalerkin1D(n=N, v_x=vx)
  fine = pkg.BaseGalerkin1D(n=N, v_x=new)
  PL, _ = pkg.galerkin.split_interpolation(old)
  got = to.to_children(old.to_device_layout(p(old.x)), parent, K, PL)
  want = fine.to_device_layout(p(fine.x))
  err = np.max(np.abs(got - want))
  print(f"N = {N}: max error {err:.3e}, max|p| {np.max(np.abs(want)):.3e}")
  assert err <= 1e-12 * np.max(np.abs(want))


@pytest.mark.parametrize("batch", (1, 3))
@pytest.mark.parametrize("N", ORDERS)
def test_dot_product_identity(pkg, N, batch):
  K = 11
  _, _, _, parent = random_refinement(N, K, 70 + N)
  _, PL, _ = matrices(pkg, N)
  rng = np.random.default_rng(5 * N + batch)
  u = rng.standard_normal(batch * K * (N + 1))
  w = rng.standard_normal(batch * len(parent) * (N + 1))
  lhs = np.dot(to.to_children(u, parent, K, PL, batch), w)
  rhs = np.dot(u, to.from_children(w, parent, K, PL.T.copy(), batch))
  scale = np.dot(np.abs(to.to_children(np.abs(u), parent, K, np.abs(PL), batch)), np.abs(w))
  assert abs(lhs - rhs) <= 1e-13 * scale


@pytest.mark.parametrize("N", ORDERS)
def test_restriction_conserves_mass_and_inverts_prolongation(pkg, N):
  K, batch = 12, 2
  vx, _, new, parent = random_refinement(N, K, 90 + N)
  mesh, PL, RL = matrices(pkg, N)
  rng = np.random.default_rng(11 * N)
  fine = rng.standard_normal(batch * len(parent) * (N + 1))
  coarse = to.from_children(fine, parent, K, RL, batch)
  m_fine, m_coarse = to.mass(mesh, new, fine, batch), to.mass(mesh, vx, coarse, batch)
  bound = 1e-13 * to.mass(mesh, new, np.abs(fine), batch) * np.max(np.abs(RL).sum(axis=1)) * 2
  assert np.all(np.abs(m_fine - m_coarse) <= bound), (m_fine, m_coarse)
  u = rng.standard_normal(batch * K * (N + 1))
  back = to.from_children(to.to_children(u, parent, K, PL, batch), parent, K, RL, batch)
  assert np.max(np.abs(back - u)) <= 1e-13 * np.max(np.abs(u))


def test_oracle_copies_unsplit_elements_bit_for_bit(pkg):
  _, PL, RL = matrices(pkg, 3)
  parent = np.array([0, 1, 1, 2, 3, 3], dtype=np.int32)
  u = np.arange(16, dtype=np.float64)
  u[0:4] = [np.nan, -0.0, np.inf, -np.inf]
  out = to.to_children(u, parent, 4, PL).view(np.int64).reshape(6, 4)
  src = u.view(np.int64).reshape(4, 4)
  np.testing.assert_array_equal(out[[0, 3]], src[[0, 2]])
  back = to.from_children(out.view(np.float64).ravel(), parent, 4, RL).view(np.int64)
  np.testing.assert_array_equal(back.reshape(4, 4)[[0, 2]], src[[0, 2]])
  np.testing.assert_array_equal(to.roles(parent), [0, 1, 2, 0, 1, 2])


def test_parent_of_split(pkg):
  import torch
  op = pkg.operators.DGAdvection1D
  for j, want in ((0, [0, 0, 1, 2, 3]), (2, [0, 1, 2, 2, 3]), (3, [0, 1, 2, 3, 3]),
                  (-5, [0, 0, 1, 2, 3]), (99, [0, 1, 2, 3, 3])):  # clamped as dg_plan_refine
    parent = op.parent_of_split(torch.tensor([j], dtype=torch.int64), 4)
    assert parent.dtype == torch.int32 and parent.tolist() == want
    op.check_parent(parent, 4)
    marks = np.zeros(4, dtype=np.uint8)
    marks[min(max(j, 0), 3)] = 1
    np.testing.assert_array_equal(parent.numpy(), mo.split_marked(np.arange(5.0), marks)[1])
  with pytest.raises(TypeError):
    op.parent_of_split(torch.tensor([1], dtype=torch.int32), 4)


def test_check_parent(pkg):
  import torch
  check = pkg.operators.DGAdvection1D.check_parent
  t = lambda v: torch.tensor(v, dtype=torch.int32)  # noqa: E731
  for good, k_old in (([0, 1, 2], 3), ([0, 0, 1, 1, 2, 2], 3), ([0, 1, 1, 2], 3), ([0], 1),
                      ([0, 0], 1)):
    check(t(good), k_old)
  for bad, k_old in (([1, 2, 3], 4),            # does not start at 0
                     ([0, 1, 2], 4),            # does not end at k_old - 1
                     ([0, 1, 3, 3], 4),         # steps by 2
                     ([0, 1, 1, 0, 1, 2], 3),   # steps back
                     ([0, 1, 1, 1, 2], 3),      # a value three times
                     ([0, 0, 0], 1),            # longer than 2 k_old
                     ([0, 1], 3)):              # shorter than k_old
    with pytest.raises(ValueError):
      check(t(bad), k_old)
  with pytest.raises(TypeError):
    check(torch.tensor([0.0, 1.0]), 2)
  with pytest.raises(TypeError):
    check([0, 1], 2)
