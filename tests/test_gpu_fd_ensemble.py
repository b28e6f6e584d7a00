"""The finite-difference DWR adapt loop for ODE ensembles on the GPU (csrc/dg_fd.hip via
fd_ensemble.FDEnsemble).  Needs an MI355X.

Pinned by the reference itself: with one member and u0 = 1 the device loop must reproduce
tests/golden/fd_adapt_golden.json — the outputs of python/Main_finite_difference.py's own
functions (tests/golden/make_fd_golden.py) — refine indices bit-exact, floats to 1e-12.
Ensembles are checked member by member against the oracle (oracle/fd.py).

Every instantiation (ref_factor 2..16) runs on a non-uniform mesh whose interior coarse
nodes take both branches of the on-the-fly np.interp (interpolated and exact node), with the
same 1e-12 bar on U, V and the window sums: a numpy transcription of the kernel's recursion
agrees with oracle/fd.py to <= 1.2e-15 there for every ref_factor, so the bar keeps three
orders of magnitude of headroom.  Block edges (256 lanes), the V == NULL path, a one-step
mesh and the argument checks follow."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from oracle import fd as ofd

pytestmark = pytest.mark.gpu


def rel(x, ref):
  return float(np.max(np.abs(np.asarray(x) - np.asarray(ref))) / max(np.max(np.abs(ref)), 1e-300))


def test_reproduces_the_reference_golden_run(pkg, gpu):
  with open(os.path.join(GOLDEN, "fd_adapt_golden.json")) as f:
    g = json.load(f)
  cfg = g["config"]
  times = np.linspace(0.0, 2.0, cfg["n_steps0"] + 1)
  ens = pkg.fd_ensemble.FDEnsemble(times, [cfg["u0"]], ref_factor=cfg["ref_factor"])
  for it in g["iterations"]:
    np.testing.assert_array_equal(ens.times, np.array(it["times"]))
    U, V, err = ens.sweep(with_v=True)
    assert rel(U[:, 0].cpu().numpy(), it["u"]) <= 1e-12
    assert rel(V[:, 0].cpu().numpy(), it["v"]) <= 1e-12
    assert rel(err[0].cpu().numpy(), it["err_steps"]) <= 1e-12
    assert ens.adapt() == it["ref_idx"]


def test_ensemble_members_match_the_oracle(pkg, gpu):
  rng = np.random.default_rng(3)
  u0 = rng.uniform(-2.5, 2.5, 4097)
  times = np.sort(np.concatenate(([0.0, 2.0], rng.uniform(0.05, 1.95, 9))))
  rf = 4
  ens = pkg.fd_ensemble.FDEnsemble(times, u0, ref_factor=rf)
  U, V, err = (t.cpu().numpy() for t in ens.sweep(with_v=True))
  dt_n = np.diff(times)
  for j in (0, 1, 1000, 4096):
    u = ofd.forward_solve(ofd.sin_update, dt_n, u0[j])
    v = ofd.adj_solve(ofd.u2_k, ofd.sin_jf, dt_n, u, rf)
    steps = ofd.window_errors(ofd.err_est(ofd.sin_update, u, v, dt_n, rf), rf)
    assert rel(U[:, j], u) <= 1e-12
    assert rel(V[:, j], v) <= 1e-12
    assert rel(err[j], steps) <= 1e-12
  # the ensemble indicator is the fixed-order member sum
  ens.adapt()
  acc = err[0].copy()
  for r in range(1, err.shape[0]):
    acc = acc + err[r]
  np.testing.assert_array_equal(ens.history[-1]["err_steps"], acc)


# a non-uniform 10-step mesh (sort([0, 2] + 9 uniform draws, seed 3)) and members with a
# fixed point (0.0), a negative and a large-argument start value
MESH = np.sort(np.concatenate(([0.0, 2.0], np.random.default_rng(3).uniform(0.05, 1.95, 9))))
UNIFORM = np.linspace(0.0, 2.0, 9)
MEMBERS = np.array([1.0, -2.5, 0.0, 0.3, 30.0])
RF_EDGE = 5  # refine factor of the block-edge launches
SENTINEL = -777.25
_oracle = {}


def oracle(times, rf, u0):
  """(U, V, window sums) of oracle/fd.py for one member, computed once per case."""
  key = (times.tobytes(), rf, float(u0))
  if key not in _oracle:
    dt_n = np.diff(times)
    u = ofd.forward_solve(ofd.sin_update, dt_n, u0)
    v = ofd.adj_solve(ofd.u2_k, ofd.sin_jf, dt_n, u, rf)
    _oracle[key] = (u, v, ofd.window_errors(ofd.err_est(ofd.sin_update, u, v, dt_n, rf), rf))
  return _oracle[key]


def interior_codes(pkg, times, rf):
  """interp_codes of the interior coarse nodes (fine indices rf, 2 rf, ...), built as
  FDEnsemble.sweep builds them."""
  fe = pkg.fd_ensemble
  dt_n = np.diff(times)
  dt_fine, nf = fe.refine_all(dt_n, rf)
  t_coarse = np.concatenate(([0], np.cumsum(dt_n)), axis=None)
  t_fine = np.concatenate(([0], np.cumsum(dt_fine)), axis=None)
  return fe.interp_codes(t_coarse, t_fine)[rf:nf:rf]


def check_members(times, rf, U, V, err, members, lanes=None):
  lanes = range(len(members)) if lanes is None else lanes
  for u0, l in zip(members, lanes):
    u, v, steps = oracle(times, rf, u0)
    assert rel(U[:, l], u) <= 1e-12, (rf, u0)
    assert rel(V[:, l], v) <= 1e-12, (rf, u0)
    assert rel(err[l], steps) <= 1e-12, (rf, u0)


def sweep_np(pkg, times, u0, rf, with_v=True):
  U, V, err = pkg.fd_ensemble.FDEnsemble(times, u0, ref_factor=rf).sweep(with_v=with_v)
  return U.cpu().numpy(), (V.cpu().numpy() if with_v else None), err.cpu().numpy()


@pytest.mark.parametrize("rf", range(2, 17))
def test_every_ref_factor_matches_the_oracle(pkg, gpu, rf):
  assert np.sum(interior_codes(pkg, MESH, rf) >= 0) >= 1  # the interpolation branch runs
  U, V, err = sweep_np(pkg, MESH, MEMBERS, rf)
  assert V.shape == ((MESH.size - 1) * rf + 1, MEMBERS.size)
  check_members(MESH, rf, U, V, err, MEMBERS)


def test_exact_node_branch_on_both_meshes(pkg, gpu):
  """Over the parametrised set the exact-node branch of np.interp occurs too (the cumsum of
  the fine steps lands bitwise on some coarse nodes); on a uniform mesh every interior
  node takes it."""
  assert any(np.any(interior_codes(pkg, MESH, rf) < 0) for rf in range(2, 17))
  for rf in (2, 4, 8, 16):
    assert np.all(interior_codes(pkg, UNIFORM, rf) < 0)
    U, V, err = sweep_np(pkg, UNIFORM, MEMBERS, rf)
    check_members(UNIFORM, rf, U, V, err, MEMBERS)


@pytest.mark.parametrize("rf", [2, 7, 16])
def test_sweep_without_v_is_bit_identical(pkg, gpu, rf):
  """adapt() passes V == NULL: U and the window sums do not depend on it."""
  U, V, err = sweep_np(pkg, MESH, MEMBERS, rf)
  U0, V0, err0 = sweep_np(pkg, MESH, MEMBERS, rf, with_v=False)
  assert V0 is None
  np.testing.assert_array_equal(U0, U)
  np.testing.assert_array_equal(err0, err)


@pytest.mark.parametrize("n_ics", [1, 255, 256, 257])
def test_block_edges_lane_independence(pkg, gpu, n_ics):
  base = sweep_np(pkg, MESH, MEMBERS, RF_EDGE)
  m = np.arange(n_ics) % MEMBERS.size
  U, V, err = sweep_np(pkg, MESH, MEMBERS[m], RF_EDGE)
  np.testing.assert_array_equal(U, base[0][:, m])
  np.testing.assert_array_equal(V, base[1][:, m])
  np.testing.assert_array_equal(err, base[2][m])
  lanes = sorted({l for l in (0, 255, 256, n_ics - 1) if l < n_ics})
  check_members(MESH, RF_EDGE, U, V, err, MEMBERS[m[lanes]], lanes)


@pytest.mark.parametrize("rf", [2, 3, 16])
def test_single_step_mesh(pkg, gpu, rf):
  """n_steps = 1: two nodes, one window, the fine grid's last node is the coarse one."""
  times = np.array([0.0, 0.7])
  U, V, err = sweep_np(pkg, times, MEMBERS, rf)
  assert U.shape == (2, MEMBERS.size) and V.shape == (rf + 1, MEMBERS.size)
  assert err.shape == (MEMBERS.size, 1)
  check_members(times, rf, U, V, err, MEMBERS)


def test_rejections(pkg, gpu):
  err_t = pkg._lib.DGLibraryError
  for rf in (1, 17):
    with pytest.raises(err_t):
      pkg.fd_ensemble.FDEnsemble(MESH, MEMBERS, ref_factor=rf).sweep(with_v=True)
  with pytest.raises(err_t):
    pkg.fd_ensemble.FDEnsemble(MESH[:1], MEMBERS, ref_factor=4).sweep()  # no step
  with pytest.raises(err_t):
    pkg.fd_ensemble.FDEnsemble(MESH[:0], MEMBERS, ref_factor=4).sweep()  # empty mesh


@pytest.mark.parametrize("n,rf", [(10, 1), (10, 17), (0, 4)])
def test_rejections_launch_nothing(pkg, gpu, n, rf):
  """dg_fd_adapt_sweep called directly on sentinel-filled outputs (buffers sized for
  10 steps at ref_factor 17)."""
  lib = pkg._lib.load()
  n_ics, nmax, rmax = 8, 10, 17
  z = lambda k, dt=torch.float64: torch.zeros(k, dtype=dt, device=gpu)  # noqa: E731
  dt_n, tc, tf, code = z(nmax), z(nmax + 1), z(nmax * rmax + 1), z(nmax * rmax + 1, torch.int32)
  u0 = z(n_ics)
  full = lambda k: torch.full((k,), SENTINEL, dtype=torch.float64, device=gpu)  # noqa: E731
  U, V, err = full((nmax + 1) * n_ics), full((nmax * rmax + 1) * n_ics), full(n_ics * nmax)
  p = lambda x: x.data_ptr()  # noqa: E731
  rc = lib.dg_fd_adapt_sweep(n, rf, p(dt_n), p(tc), p(tf), p(code), p(u0), n_ics, p(U), p(V),
                             p(err), torch.cuda.current_stream(gpu).cuda_stream)
  torch.cuda.synchronize()
  assert rc == pkg._lib.DG_ERR_ARG
  assert bool((U == SENTINEL).all()) and bool((V == SENTINEL).all())
  assert bool((err == SENTINEL).all())
