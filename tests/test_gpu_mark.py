"""dg_plan_mark / dg_plan_refine_marked on the GPU against tests/mark_oracle.py, at the
element counts where the marking kernels' grids change (taken from dg_plan_query_mark)."""
import ctypes

import numpy as np
import pytest

import mark_oracle as mo

pytestmark = pytest.mark.gpu

# (a plan needs K >= 2, dg_plan_create: 2 and 3 are the smallest even and odd meshes)
SIZES = ("2", "3", "B-1", "B", "B+1", "2B+1", "SB+1")
INPUTS = ("ties", "distinct", "nonfinite", "zeros", "single")
PATTERNS = ("none", "all", "first", "last", "alternating", "boundary_runs", "random")
GUARD = 64
_cache = {}


def geometry(pkg):
  """(B, S): elements per workgroup, block sums per scan iteration."""
  if "geom" not in _cache:
    with pkg.operators.DGAdvection1D(pkg.BaseGalerkin1D(n=1, k=4)) as op:
      B, S, bits = op.query_mark()
    # the grid this file computes: ceil(K / B) workgroups, ceil(that / S) scan iterations; the
    # largest size below must stay a test of seconds
    if not (B >= 64 and B % 64 == 0 and S >= 2 and 64 % bits == 0 and S * B + 1 <= 1 << 22):
      raise AssertionError(f"mark geometry changed: B = {B}, S = {S}, digit bits = {bits}")
    _cache["geom"] = (B, S)
  return _cache["geom"]


def size_of(pkg, name):
  B, S = geometry(pkg)
  return {"2": 2, "3": 3, "B-1": B - 1, "B": B, "B+1": B + 1, "2B+1": 2 * B + 1,
          "SB+1": S * B + 1}[name]


def mesh_of(pkg, N, K):
  """A non-uniform mesh (every element its own metric), built once per (N, K)."""
  if ("mesh", N, K) not in _cache:
    rng = np.random.default_rng(1000 + K)
    vx = np.concatenate(([0.0], np.cumsum(rng.uniform(0.5, 1.5, K)))) / K
    _cache["mesh", N, K] = pkg.BaseGalerkin1D(n=N, v_x=vx)
  return _cache["mesh", N, K]


def new_plan(pkg, N, K, batch=1, reserve=None):
  op = pkg.operators.DGAdvection1D(mesh_of(pkg, N, K), batch=batch)
  op.reserve(2 * K if reserve is None else reserve)
  return op


def make_eta(pkg, kind, K):
  B, _ = geometry(pkg)
  rng = np.random.default_rng(7 * K + INPUTS.index(kind))
  if kind in ("ties", "nonfinite"):
    eta = rng.choice([0.25, 1.0, 3.0], K) * rng.choice([-1.0, 1.0], K)
    if kind == "nonfinite":
      where = sorted({k for k in (0, K - 1, B - 1, B, 2 * B - 1, 2 * B) if 0 <= k < K})
      for n, k in enumerate(where):
        eta[k] = (np.inf, -np.inf, np.nan)[n % 3]
    return eta
  if kind == "distinct":
    eta = 10.0 ** rng.uniform(-300, 300, K) * rng.choice([-1.0, 1.0], K)
    sub = np.arange(0, K, 97)
    eta[sub] = 5e-324 * (1 + np.arange(len(sub)))  # denormals
    return eta
  eta = np.zeros(K)
  if kind == "single":
    eta[K // 3] = -2.5
  return eta


def guarded(torch, gpu, n, dtype, fill):
  buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=gpu)
  return buf, buf[GUARD:GUARD + n]


def check_guards(buf, n, fill):
  assert bool((buf[:GUARD] == fill).all()) and bool((buf[GUARD + n:] == fill).all()), \
      "wrote outside the buffer"


def bits_of(x):
  return int(np.float64(x).view(np.int64))


@pytest.mark.parametrize("kind", INPUTS)
@pytest.mark.parametrize("size", SIZES)
def test_marks_and_info_equal_the_oracle(pkg, gpu, size, kind):
  import torch
  K = size_of(pkg, size)
  if ("plan", K) not in _cache:
    _cache["plan", K] = new_plan(pkg, 1, K)
  op = _cache["plan", K]
  vx = op.mesh.v_x
  eta_h = make_eta(pkg, kind, K)
  eta = torch.tensor(eta_h, dtype=torch.float64, device=gpu)
  order = mo.rank_order(eta_h)
  cases = [("top", m, None) for m in (0, 1, 2, K // 2, K - 1, K, K + 5)]
  cases += [("max", th, None) for th in (1.0, 0.5, 2.0 ** -60)]
  cases.append(("max", 0.5, int(mo.max_fraction(eta_h, 0.5, order=order).sum()) // 2))
  cases.append(("top", K, K // 3))
  for strategy, param, cap in cases:
    mbuf, marks = guarded(torch, gpu, K, torch.uint8, 0xAB)
    ibuf, info = guarded(torch, gpu, 4, torch.int64, -77)
    op.mark(eta, strategy, param, max_marked=cap, marks=marks, info=info)
    want = (mo.top_count(eta_h, param, cap, order) if strategy == "top"
            else mo.max_fraction(eta_h, param, cap, order))
    got = marks.cpu().numpy()
    what = f"K={K} {kind} {strategy} {param} cap={cap}"
    np.testing.assert_array_equal(got, want, err_msg=what)
    count, nonfinite, width = mo.info(eta_h, want, vx)
    assert info.tolist() == [count, nonfinite, bits_of(width), 0], what
    check_guards(mbuf, K, 0xAB)
    check_guards(ibuf, 4, -77)
    if strategy == "top" and param == 1 and cap is None:
      assert int(np.flatnonzero(got)[0]) == op.argmax(eta, use_abs=True) == order[0]


@pytest.mark.parametrize("size", SIZES)
def test_top_one_is_the_argmax_refine(pkg, gpu, size):
  """m = 1: the marked element is argmax's, and refine_marked leaves the mesh, the metric and
  the operator bit-identical to refine(idx) on a twin plan."""
  import torch
  K = size_of(pkg, size)
  eta = torch.tensor(make_eta(pkg, "ties", K), dtype=torch.float64, device=gpu)
  op, twin = new_plan(pkg, 1, K, reserve=K + 1), new_plan(pkg, 1, K, reserve=K + 1)
  marks, info = op.mark(eta, "top", 1)
  idx = twin.argmax_async(eta, use_abs=True)
  assert torch.nonzero(marks).flatten().tolist() == [int(idx.item())]
  assert op.refine_marked(marks) == (K + 1, 1)
  assert twin.refine(idx) == K + 1
  np.testing.assert_array_equal(op.v_x(), twin.v_x())
  u = torch.randn(op.field_numel, dtype=torch.float64, device=gpu,
                  generator=torch.Generator(device=gpu).manual_seed(K))
  assert torch.equal(op.rhs(u, 0.3), twin.rhs(u, 0.3))
  op.close(), twin.close()


def pattern(pkg, name, K):
  B, _ = geometry(pkg)
  k = np.arange(K)
  if name == "none":
    return np.zeros(K, dtype=bool)
  if name == "all":
    return np.ones(K, dtype=bool)
  if name == "first":
    return k == 0
  if name == "last":
    return k == K - 1
  if name == "alternating":
    return k % 2 == 1
  if name == "boundary_runs":  # adjacent marks across every workgroup boundary
    m = np.zeros(K, dtype=bool)
    for b in range(B, K, B):
      m[b - 3:b + 3] = True
    if K <= B:
      m[max(K // 2 - 1, 0):K // 2 + 2] = True
    return m
  return np.random.default_rng(K).random(K) < 0.3


def check_split(pkg, gpu, N, K, marks_h, batch=1):
  """refine_marked on a fresh plan: mesh, parent, K, and the operator against a plan created
  on the refined mesh."""
  import torch
  count = int(np.count_nonzero(marks_h))
  op = new_plan(pkg, N, K, batch=batch, reserve=K + max(count, 1))
  vx0 = op.v_x()
  marks = torch.tensor(marks_h.astype(np.uint8) * 3, device=gpu)  # any nonzero byte counts
  pbuf, parent = guarded(torch, gpu, K + count, torch.int32, -5)
  assert op.refine_marked(marks, parent=parent) == (K + count, count)
  want_vx, want_parent = mo.split_marked(vx0, marks_h)
  vx1 = op.v_x()
  np.testing.assert_array_equal(vx1, want_vx)
  np.testing.assert_array_equal(parent.cpu().numpy(), want_parent)
  check_guards(pbuf, K + count, -5)
  assert op.K == K + count and op.ktot == batch * op.K
  fresh = pkg.operators.DGAdvection1D(N, v_x=vx1, batch=batch)
  u = torch.randn(op.field_numel, dtype=torch.float64, device=gpu,
                  generator=torch.Generator(device=gpu).manual_seed(K + count))
  assert fresh.uniform == op.uniform
  assert torch.equal(op.rhs(u, 0.3), fresh.rhs(u, 0.3))
  op.close(), fresh.close()


@pytest.mark.parametrize("name", PATTERNS)
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("N", (1, 4))
def test_split_equals_the_oracle(pkg, gpu, N, size, name):
  K = size_of(pkg, size)
  check_split(pkg, gpu, N, K, pattern(pkg, name, K))


def test_split_of_a_batched_plan(pkg, gpu):
  B, _ = geometry(pkg)
  K = 2 * B + 1
  check_split(pkg, gpu, 4, K, pattern(pkg, "random", K), batch=3)


def test_no_marks_leave_a_uniform_plan_uniform(pkg, gpu):
  import torch
  B, _ = geometry(pkg)
  K = B + 1
  op = pkg.operators.DGAdvection1D(pkg.BaseGalerkin1D(n=1, k=K))
  assert op.uniform
  vx0 = op.v_x()
  parent = torch.full((K,), -1, dtype=torch.int32, device=gpu)
  marks = torch.zeros(K, dtype=torch.uint8, device=gpu)
  assert op.refine_marked(marks, parent=parent) == (K, 0)  # capacity == K: nothing to hold
  assert op.uniform
  np.testing.assert_array_equal(op.v_x(), vx0)
  assert parent.tolist() == list(range(K))
  op.close()


def test_capacity_is_respected(pkg, gpu):
  import torch
  B, _ = geometry(pkg)
  K = B + 1
  marks_h = np.zeros(K, dtype=np.uint8)
  marks_h[[0, B - 1, B, 7, 300]] = 1
  op = new_plan(pkg, 1, K, reserve=K + 5)
  assert op.refine_marked(torch.tensor(marks_h, device=gpu)) == (K + 5, 5)  # exactly full
  op.close()
  op = new_plan(pkg, 1, K, reserve=K + 5)
  vx0 = op.v_x()
  marks_h[11] = 1
  with pytest.raises(pkg._lib.DGLibraryError, match="capacity"):
    op.refine_marked(torch.tensor(marks_h, device=gpu))
  assert op.K == K
  np.testing.assert_array_equal(op.v_x(), vx0)
  q = (ctypes.c_int64 * 8)()
  assert op._lib.dg_plan_query(op._plan, q) == 0 and q[2] == K
  op.close()


def test_argument_errors(pkg, gpu):
  import torch
  lib, ERR = pkg._lib.load(), pkg._lib.DG_ERR_ARG
  K = 8
  op = new_plan(pkg, 1, K)
  eta = torch.ones(K, dtype=torch.float64, device=gpu)
  marks = torch.zeros(K, dtype=torch.uint8, device=gpu)
  info = torch.zeros(4, dtype=torch.int64, device=gpu)
  p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
  TOP, MAX = pkg._lib.DG_MARK_TOP_COUNT, pkg._lib.DG_MARK_MAX_FRACTION
  good = [op._plan, p(eta), TOP, 2.0, -1, p(marks), p(info), None]
  assert lib.dg_plan_mark(*good) == 0
  for pos in (0, 1, 5, 6):  # null plan, eta, marks, info
    args = list(good)
    args[pos] = None
    assert lib.dg_plan_mark(*args) == ERR, pos
  for strategy, param in ((2, 1.0), (-1, 1.0), (TOP, -1.0), (TOP, 1.5), (TOP, float("nan")),
                          (MAX, 0.0), (MAX, -0.5), (MAX, 1.0000001), (MAX, float("nan"))):
    args = list(good)
    args[2], args[3] = strategy, param
    assert lib.dg_plan_mark(*args) == ERR, (strategy, param)
  assert lib.dg_plan_refine_marked(None, p(marks), None, None, None) == ERR
  assert lib.dg_plan_refine_marked(op._plan, None, None, None, None) == ERR
  out = (ctypes.c_int64 * 4)()
  assert lib.dg_plan_query_mark(None, out) == ERR
  assert lib.dg_plan_query_mark(op._plan, None) == ERR
  torch.cuda.synchronize()
  assert marks.tolist() == [1, 1, 0, 0, 0, 0, 0, 0]  # the failed calls wrote nothing
  with pytest.raises(ValueError):
    op.mark(eta, "bulk", 0.5)
  with pytest.raises(TypeError):
    op.mark(eta.float(), "top", 1)
  with pytest.raises(ValueError):
    op.mark(eta[::2], "top", 1)
  op.close()


@pytest.mark.parametrize("size", ("B+1", "SB+1"))
def test_two_runs_give_the_same_bits(pkg, gpu, size):
  import torch
  K = size_of(pkg, size)
  eta = torch.tensor(make_eta(pkg, "ties", K), dtype=torch.float64, device=gpu)
  res = []
  for _ in range(2):
    op = new_plan(pkg, 1, K)
    out = []
    for strategy, param in (("top", K // 3), ("max", 0.5)):
      marks, info = op.mark(eta, strategy, param)
      out += [marks.clone(), info.clone()]
    op.refine_marked(out[0])
    out.append(torch.tensor(op.v_x()))
    res.append(out)
    op.close()
  for a, b in zip(*res):
    assert torch.equal(a, b)
