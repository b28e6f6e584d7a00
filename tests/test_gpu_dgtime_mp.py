"""Every instantiation of csrc/dg_time.hip (march Np = 2..9, adjoint forward Np = 2..8),
the 128-lane block edges, the Newton controls (maxit, tol, mixed trip counts in a wave) and
the argument checks, against the extended-precision fixture
tests/golden/dgtime_mp_golden.json (oracle/dgtime_mp.py at 50 digits, written by
tests/golden/make_dgtime_golden.py; the GPU host needs no mpmath).  Needs an MI355X.

Iteration counts equal the fixture's exactly (the generator asserts that no Newton error of
the mp run lies within 1e-3 relative of tol, so no count can legitimately flip).  Y, V and
err lie within bound(N, q) = max(8 x floor_a(N, q), 1e-13) of max|fixture| per member, where
floor_a is the distance of the numpy nodal-form restatement (oracle.dgtime.*_nodal, fed the
package's own host operators, end to end on its own Y) from the mp result: the kernel
differs from that restatement only in FMA contraction, summation order and sincos
rounding, each a source of the size floor_a already contains, hence the factor 8.
From the generator's output (fp64 on the CPU, never from a GPU run):

| N | bound Y | bound V | bound err | polyfit form (floor_b) Y | V | err |
|---|---------|---------|-----------|--------------------------|---|-----|
| 1 | 1.0e-13 | 3.0e-13 | 1.0e-12 | 1.7e-15 | 3.6e-14 | 1.5e-13 |
| 2 | 1.0e-13 | 3.8e-13 | 1.1e-12 | 1.5e-15 | 5.1e-14 | 2.2e-13 |
| 3 | 1.0e-13 | 3.7e-12 | 1.3e-11 | 2.0e-15 | 3.8e-13 | 1.3e-12 |
| 4 | 1.0e-13 | 2.6e-12 | 9.2e-12 | 3.9e-15 | 8.2e-13 | 2.5e-12 |
| 5 | 1.0e-13 | 1.2e-10 | 3.4e-10 | 3.9e-15 | 1.4e-11 | 3.9e-11 |
| 6 | 1.0e-13 | 6.0e-10 | 1.7e-09 | 3.9e-15 | 7.0e-11 | 2.1e-10 |
| 7 | 1.0e-13 | 6.2e-09 | 1.7e-08 | 7.6e-15 | 7.8e-10 | 2.1e-09 |
| 8 | 1.0e-13 | -       | -       | 3.5e-15 | -       | -       |

(The tests read the unrounded floors from the fixture; y0 = 40 sets most of them.)  The
growth with N is the conditioning of adj_march.m:79, which evaluates u_h before the slab
(max|Pext| = 2e4 at N = 7) and so amplifies the few-1e-15 error every fp64 march has in Y
(it comes from the fp64 stiffness S = (V V')\\Dr); floors (a) and (b) agree at every order,
so neither the polyfit nor the nodal form carries it.
At the two fixed points (y0 = 0, fl(pi)) err is a residual <= 1e-15 left by cancellation;
there it is compared on the scale of the cancelling terms max|V| max|Y| with the bound
from floor_a["err_fixed"], measured on that same scale.
"""
import json
import math
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

with open(os.path.join(GOLDEN, "dgtime_mp_golden.json")) as _f:
  G = json.load(_f)
TIMES = np.array(G["times"])
Y0 = np.array(G["y0"])
FIXED = [j for j, y in enumerate(Y0) if abs(math.sin(y)) < 1e-12]  # 0.0 and fl(pi)
N_EDGE = 4  # order of the block-edge launches
SENTINEL = -777.25


def rel(x, ref):
  return float(np.max(np.abs(np.asarray(x) - np.asarray(ref))) / max(np.max(np.abs(ref)), 1e-300))


def bound(floor_a):
  return max(8.0 * floor_a, 1e-13)


def check_forward(e, Y, its, members, lanes=None):
  """Lanes `lanes` of (Y, its) hold the fixture members `members` of entry e."""
  lanes = members if lanes is None else lanes
  Yr, ir = np.array(e["Y"]), np.array(e["its"])
  b = bound(e["floor_a"]["Y"])
  for j, l in zip(members, lanes):
    assert list(its[:, l]) == list(ir[:, j]), (j, l)
    r = rel(Y[:, :, l], Yr[:, :, j])
    assert r <= b, (j, l, r, b)


def check_adjoint(e, V, err, members, lanes=None):
  lanes = members if lanes is None else lanes
  Yr, Vr, er = np.array(e["Y"]), np.array(e["V"]), np.array(e["err"])
  fa = e["floor_a"]
  for j, l in zip(members, lanes):
    r = rel(V[:, :, l], Vr[:, :, j])
    assert r <= bound(fa["V"]), (j, l, r)
    if j in FIXED:
      scale = float(np.max(np.abs(Vr[:, :, j])) * np.max(np.abs(Yr[:, :, j])))
      d = float(np.max(np.abs(err[l] - er[j])))
      assert d <= bound(fa["err_fixed"]) * scale, (j, l, d, scale)
    else:
      r = rel(err[l], er[j])
      assert r <= bound(fa["err"]), (j, l, r)


_runs = {}


def run(pkg, N, y0=Y0, times=TIMES, adjoint=True, **kw):
  """march (+ adjoint) of one launch as numpy arrays; the fixture-member launch is cached."""
  key = (N, adjoint) if (y0 is Y0 and times is TIMES and not kw) else None
  if key in _runs:
    return _runs[key]
  ens = pkg.dgtime.DGTimeEnsemble(N, times, y0, tol=kw.get("tol", G["tol"]),
                                  maxit=kw.get("maxit", G["maxit"]))
  Y, its, td = ens.march()
  out = [Y.cpu().numpy(), its.cpu().numpy()]
  if adjoint:
    out += [t.cpu().numpy() for t in ens.adjoint(Y, td)]
  if key is not None:
    _runs[key] = out
  return out


@pytest.mark.parametrize("N", range(1, 9))
def test_march_every_order(pkg, gpu, N):
  Y, its = run(pkg, N, adjoint=N <= 7)[:2]
  check_forward(G["orders"][str(N)], Y, its, range(Y0.size))


@pytest.mark.parametrize("N", range(1, 8))
def test_adjoint_every_order(pkg, gpu, N):
  _, _, V, err = run(pkg, N)
  check_adjoint(G["orders"][str(N)], V, err, range(Y0.size))


@pytest.mark.parametrize("n_ics", [1, 127, 128, 129, 257])
def test_block_edges_lane_independence(pkg, gpu, n_ics):
  """Members cycle through the lanes; every lane is bit-identical to its member's lane in
  the one-block launch of the 8 members, and the edge lanes meet the fixture's bound."""
  base = run(pkg, N_EDGE)
  m = np.arange(n_ics) % Y0.size
  Y, its, V, err = run(pkg, N_EDGE, y0=Y0[m])
  np.testing.assert_array_equal(Y, base[0][:, :, m])
  np.testing.assert_array_equal(its, base[1][:, m])
  np.testing.assert_array_equal(V, base[2][:, :, m])
  np.testing.assert_array_equal(err, base[3][m])
  lanes = sorted({l for l in (0, 127, 128, n_ics - 1) if l < n_ics})
  e = G["orders"][str(N_EDGE)]
  check_forward(e, Y, its, [int(m[l]) for l in lanes], lanes)
  check_adjoint(e, V, err, [int(m[l]) for l in lanes], lanes)


@pytest.mark.parametrize("case", G["control"], ids=lambda c: f"{c['name']}-N{c['N']}")
def test_newton_control(pkg, gpu, case):
  """maxit and tol against the mp iterates cut at the same count (dg_march.m:44:
  `while it <= maxit && err > tol`, err = 1 on entry)."""
  y0, times = np.array(case["y0"]), np.array(case["times"])
  Y, its = run(pkg, case["N"], y0=y0, times=times, adjoint=False, tol=case["tol"],
               maxit=case["maxit"])
  check_forward(case, Y, its, range(y0.size))
  if case["name"] == "maxit0":  # it <= 0 admits exactly one iteration
    assert np.all(its == 1)
  if case["name"] == "wide_maxit2":  # the slab of width 3 needs more: every lane is cut at 3
    assert np.all(its == 3)
  if case["name"] == "wide_converged":
    assert np.all(its > 3)
  if case["name"] == "tol1":  # err = 1 on entry is not > 1: no iteration, Y = the start value
    assert np.all(its == 0)
    np.testing.assert_array_equal(Y, np.broadcast_to(y0, Y.shape))
  if case["name"] == "tol_half":  # stops after the first iteration whose step is <= 0.5
    conv = np.array(G["orders"][str(case["N"])]["its"])
    assert np.all(its >= 1) and np.all(its <= conv) and np.any(its < conv)


def test_mixed_trip_counts_in_one_wave(pkg, gpu):
  """The fixed-point members leave the Newton loop after one iteration while their
  neighbours in the wave iterate on: each lane equals its member launched alone."""
  N = 3
  Y, its, V, err = run(pkg, N)
  assert np.all(its[:, FIXED] == 1)
  others = [j for j in range(Y0.size) if j not in FIXED]
  assert np.all(its[:, others].max(axis=0) >= 3)
  for j in range(Y0.size):
    Yj, itj, Vj, ej = run(pkg, N, y0=Y0[j:j + 1])
    np.testing.assert_array_equal(Yj[:, :, 0], Y[:, :, j])
    np.testing.assert_array_equal(itj[:, 0], its[:, j])
    np.testing.assert_array_equal(Vj[:, :, 0], V[:, :, j])
    np.testing.assert_array_equal(ej[0], err[j])


def _raw_march(pkg, gpu, Np, n_slabs, maxit):
  """dg_time_march called directly on sentinel-filled outputs and operator buffers large
  enough for Np = 10.  Returns (rc, Y, its)."""
  lib = pkg._lib.load()
  z = lambda n: torch.zeros(n, dtype=torch.float64, device=gpu)  # noqa: E731
  nq, n_ics = 8, 8
  S, Phi, wq = z(100), z(nq * 10), z(nq)
  td = torch.linspace(0.0, 1.0, 6, dtype=torch.float64, device=gpu)
  y0 = torch.ones(n_ics, dtype=torch.float64, device=gpu)
  Y = torch.full((5 * 10 * n_ics,), SENTINEL, dtype=torch.float64, device=gpu)
  its = torch.full((5 * n_ics,), -7, dtype=torch.int32, device=gpu)
  p = lambda x: x.data_ptr()  # noqa: E731
  rc = lib.dg_time_march(Np, nq, p(S), p(Phi), p(wq), n_slabs, p(td), n_ics, p(y0), 1e-7, maxit,
                         p(Y), p(its), torch.cuda.current_stream(gpu).cuda_stream)
  torch.cuda.synchronize()
  return rc, Y.cpu().numpy(), its.cpu().numpy()


@pytest.mark.parametrize("Np,n_slabs,maxit", [(1, 5, 500), (10, 5, 500), (3, 0, 500), (3, 5, -1)],
                         ids=["Np1", "Np10", "no-slabs", "negative-maxit"])
def test_march_rejections_launch_nothing(pkg, gpu, Np, n_slabs, maxit):
  rc, Y, its = _raw_march(pkg, gpu, Np, n_slabs, maxit)
  assert rc == pkg._lib.DG_ERR_ARG
  with pytest.raises(pkg._lib.DGLibraryError):
    pkg._lib.check(rc, "dg_time_march")
  assert np.all(Y == SENTINEL) and np.all(its == -7)


def test_ensemble_rejections(pkg, gpu):
  err_t = pkg._lib.DGLibraryError
  with pytest.raises(err_t):
    pkg.dgtime.DGTimeEnsemble(9, TIMES, Y0).march()  # Np = 10
  with pytest.raises(err_t):
    pkg.dgtime.DGTimeEnsemble(2, TIMES[:1], Y0).march()  # n_slabs = 0
  with pytest.raises(err_t):
    pkg.dgtime.DGTimeEnsemble(2, TIMES, Y0, maxit=-1).march()
  # forward Np = 9 marches but has no adjoint instantiation (adjoint Np would be 10)
  ens = pkg.dgtime.DGTimeEnsemble(8, TIMES, Y0)
  Y, its, td = ens.march()
  with pytest.raises(err_t):
    ens.adjoint(Y, td)


def test_adjoint_rejection_launches_nothing(pkg, gpu):
  lib = pkg._lib.load()
  z = lambda n: torch.zeros(n, dtype=torch.float64, device=gpu)  # noqa: E731
  nq, n_ics, Ks = 8, 8, 5
  td = torch.linspace(0.0, 1.0, Ks + 1, dtype=torch.float64, device=gpu)
  p = lambda x: x.data_ptr()  # noqa: E731
  # operator and input buffers large enough for an adjoint Np of 10
  Sa, Ma, Phia, Pext, Ifa, wq = z(100), z(100), z(nq * 10), z(nq * 10), z(100), z(nq)
  y0, Y = z(n_ics), z(Ks * 10 * n_ics)
  for Npf, ks in ((1, Ks), (9, Ks), (3, 0)):
    V = torch.full((Ks * 10 * n_ics,), SENTINEL, dtype=torch.float64, device=gpu)
    err = torch.full((n_ics * Ks,), SENTINEL, dtype=torch.float64, device=gpu)
    rc = lib.dg_time_adjoint(Npf, nq, p(Sa), p(Ma), p(Phia), p(Pext), p(Ifa), p(wq), ks, p(td),
                             n_ics, p(y0), p(Y), p(V), p(err),
                             torch.cuda.current_stream(gpu).cuda_stream)
    torch.cuda.synchronize()
    assert rc == pkg._lib.DG_ERR_ARG, Npf
    assert bool((V == SENTINEL).all()) and bool((err == SENTINEL).all())
