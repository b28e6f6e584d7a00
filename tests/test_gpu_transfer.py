"""dg_field_to_children / dg_field_from_children on the GPU (DGAdvection1D.transfer,
transfer_t, restrict) against tests/transfer_oracle.py fed the same host matrices.

The bound is 1e-13 * max|input|, derived: an Np- or 2Np-term dot product errs by at most
gamma_k * (absolute row sum) * max|input|, and the largest absolute row sums for N <= 8 are
2.03 (PL), 6.4 ([PL^T PR^T]) and 4.5 ([RL RR]), i.e. 2.0e-15, 1.3e-14 and 9e-15; two correct
evaluations differ by at most twice that, 2.6e-14, and 1e-13 leaves about four times that for
FMA contraction and summation order.  Unsplit elements are compared on the bits.

The sizes put batch * K_new one below, at and one above one and two workgroups of 256 lanes.
With batch = 3 the totals 256, 257, 511 and 512 do not exist (they are no multiples of 3): the
multiples of 3 that bracket the workgroup sizes (255, 258, 510, 513) stand in.  Marking every
element gives an even K_new: an odd target runs at K_new + 1.
"""
import ctypes

import numpy as np
import pytest

import mark_oracle as mo
import transfer_oracle as to

pytestmark = pytest.mark.gpu

ORDERS = range(1, 9)
TOTALS = {1: (255, 256, 257, 511, 512, 513), 3: (255, 258, 510, 513)}
PATTERNS = ("none", "all", "first", "last", "adjacent", "half")
SHAPES = [(b, t) for b in (1, 3) for t in TOTALS[b]]
GUARD = 64
FILL = -777.0
TOL = 1e-13
_cache = {}


def marks_for(pattern, k_new):
  """(k_old, marks) of a refinement with K_new = k_new (k_new + 1 for "all" at odd k_new)."""
  if pattern == "none":
    return k_new, np.zeros(k_new, dtype=np.uint8)
  if pattern == "all":
    k_old = (k_new + 1) // 2
    return k_old, np.ones(k_old, dtype=np.uint8)
  if pattern in ("first", "last"):
    marks = np.zeros(k_new - 1, dtype=np.uint8)
    marks[0 if pattern == "first" else -1] = 1
    return k_new - 1, marks
  if pattern == "adjacent":
    marks = np.zeros(k_new - 2, dtype=np.uint8)
    marks[(k_new - 2) // 3:(k_new - 2) // 3 + 2] = 1
    return k_new - 2, marks
  k_old = (2 * k_new + 2) // 3  # "half": k_old + (about k_old / 2 marked) = k_new
  marks = np.zeros(k_old, dtype=np.uint8)
  marks[np.random.default_rng(k_new).permutation(k_old)[:k_new - k_old]] = 1
  return k_old, marks


def mesh_of(pkg, N, K):
  """A non-uniform mesh, built once per (N, K)."""
  if (N, K) not in _cache:
    rng = np.random.default_rng(2000 + K)
    vx = np.concatenate(([0.0], np.cumsum(rng.uniform(0.5, 1.5, K)))) / K
    _cache[N, K] = pkg.BaseGalerkin1D(n=N, v_x=vx)
  return _cache[N, K]


def refined(pkg, torch, gpu, N, k_old, batch, marks, op=None):
  """A plan refined by dg_plan_refine_marked itself: (op, parent on the device, on the host)."""
  if op is None:
    op = pkg.operators.DGAdvection1D(mesh_of(pkg, N, k_old), batch=batch)
    op.reserve(4 * k_old)
  assert op.K == k_old
  parent = torch.full((k_old + int(marks.sum()) + 2 * GUARD,), -1, dtype=torch.int32, device=gpu)
  k_new, n = op.refine_marked(torch.tensor(marks, device=gpu), parent=parent[GUARD:])
  assert n == int(marks.sum()) and k_new == k_old + n
  inner = parent[GUARD:GUARD + k_new]
  host = inner.cpu().numpy()
  np.testing.assert_array_equal(host, mo.split_marked(np.arange(k_old + 1.0), marks)[1])
  return op, inner, host


def matrix(op, name):
  """The host matrix the plan hands to the kernels (the oracle gets the same bits)."""
  op._split_matrix(name)
  return op._split[name][0]


def guarded(torch, gpu, n):
  buf = torch.full((n + 2 * GUARD,), FILL, dtype=torch.float64, device=gpu)
  return buf, buf[GUARD:GUARD + n]


def check_guards(buf, n):
  assert bool((buf[:GUARD] == FILL).all()) and bool((buf[GUARD + n:] == FILL).all()), \
      "wrote outside the buffer"


def bits(x):
  return np.ascontiguousarray(x).view(np.int64)


def compare(got, want, scale, unsplit_rows, Np, what):
  """|got - want| <= TOL * scale everywhere, equal bits on the rows of unsplit elements."""
  err = float(np.max(np.abs(got - want)))
  print(f"{what}: max error {err:.3e}, bound {TOL * scale:.3e}")
  assert err <= TOL * scale, what
  np.testing.assert_array_equal(bits(got).reshape(-1, Np)[unsplit_rows],
                                bits(want).reshape(-1, Np)[unsplit_rows], err_msg=what)


def unsplit_rows(role, parent, batch, k_old):
  """Rows (elements, all trajectories) of unsplit elements in the new and in the old field."""
  k_new = len(parent)
  new = np.flatnonzero(role == 0)
  old = parent[new]
  off_n, off_o = np.arange(batch)[:, None] * k_new, np.arange(batch)[:, None] * k_old
  return (new[None, :] + off_n).ravel(), (old[None, :] + off_o).ravel()


@pytest.mark.parametrize("batch,total", SHAPES)
@pytest.mark.parametrize("N", ORDERS)
def test_three_operators_follow_the_oracle(pkg, gpu, N, batch, total):
  import torch
  Np = N + 1
  for pattern in PATTERNS:
    k_old, marks = marks_for(pattern, total // batch)
    op, parent, parent_h = refined(pkg, torch, gpu, N, k_old, batch, marks)
    with op:
      k_new = op.K
      role = to.roles(parent_h)
      rows_new, rows_old = unsplit_rows(role, parent_h, batch, k_old)
      rng = np.random.default_rng(N * 1000 + total)
      u = rng.standard_normal(batch * k_old * Np)
      w = rng.standard_normal(batch * k_new * Np)
      u_d, w_d = torch.tensor(u, device=gpu), torch.tensor(w, device=gpu)
      tag = f"N={N} batch={batch} K_new={k_new} {pattern}"

      buf, out = guarded(torch, gpu, batch * k_new * Np)
      assert op.transfer(u_d, parent, k_old, out=out) is out
      got = out.cpu().numpy()
      check_guards(buf, out.numel())
      compare(got, to.to_children(u, parent_h, k_old, matrix(op, "PL"), batch),
              np.max(np.abs(u)), rows_new, Np, "transfer " + tag)
      if pattern == "none":
        assert torch.equal(out, u_d)

      for fn, name in ((op.transfer_t, "PLT"), (op.restrict, "RL")):
        buf, out = guarded(torch, gpu, batch * k_old * Np)
        assert fn(w_d, parent, k_old, out=out) is out
        got = out.cpu().numpy()
        check_guards(buf, out.numel())
        compare(got, to.from_children(w, parent_h, k_old, matrix(op, name), batch),
                np.max(np.abs(w)), rows_old, Np, f"{name} {tag}")
        if pattern == "none":
          assert torch.equal(out, w_d)


@pytest.mark.parametrize("N", ORDERS)
def test_fields_at_odd_addresses(pkg, gpu, N):
  """Fields that are 8- but not 16-byte aligned (views at an odd offset) take the kernels'
  8-byte accesses: the same bits as the aligned call, nothing written outside."""
  import torch
  Np, batch = N + 1, 3
  k_old, marks = marks_for("half", 171)
  op, parent, _ = refined(pkg, torch, gpu, N, k_old, batch, marks)
  with op:
    n_old, n_new = batch * k_old * Np, op.field_numel
    gen = torch.Generator(device="cpu").manual_seed(100 + N)
    for fn, n_in, n_out in ((op.transfer, n_old, n_new), (op.transfer_t, n_new, n_old),
                            (op.restrict, n_new, n_old)):
      x = torch.randn(n_in + 1, dtype=torch.float64, generator=gen).to(gpu)
      aligned = fn(x[1:].clone(), parent, k_old)
      assert aligned.data_ptr() % 16 == 0 and x[1:].data_ptr() % 16 == 8
      for shift_in, shift_out in ((1, 0), (0, 1), (1, 1)):
        src = x[1:] if shift_in else x[1:].clone()
        buf = torch.full((n_out + 2 * GUARD + 1,), FILL, dtype=torch.float64, device=gpu)
        out = buf[GUARD + shift_out:GUARD + shift_out + n_out]
        assert out.data_ptr() % 16 == 8 * shift_out
        fn(src, parent, k_old, out=out)
        assert torch.equal(out, aligned)
        assert bool((buf[:GUARD + shift_out] == FILL).all())
        assert bool((buf[GUARD + shift_out + n_out:] == FILL).all())


@pytest.mark.parametrize("N", ORDERS)
def test_special_values(pkg, gpu, N):
  """NaN (with a payload), -0 and +-inf in unsplit elements survive all three operators bit for
  bit; an inf or a NaN in one split element reaches only that element's children / parent."""
  import torch
  Np, k_old, batch = N + 1, 90, 3
  marks = np.zeros(k_old, dtype=np.uint8)
  marks[[0, 7, 8, 40, 89]] = 1
  op, parent, parent_h = refined(pkg, torch, gpu, N, k_old, batch, marks)
  with op:
    k_new = op.K
    role = to.roles(parent_h)
    payload = np.array([0x7FF8000000ABCDEF], dtype=np.uint64).view(np.float64)[0]
    specials = [payload, -0.0, np.inf, -np.inf]
    rng = np.random.default_rng(N)
    # old field: specials in unsplit elements 3 (trajectory 0), 88 (1), 1 (2); one inf in the
    # split element 40 of trajectory 1 and one NaN in the split element 89 of trajectory 2
    u = rng.standard_normal((batch, k_old, Np))
    for b, k in ((0, 3), (1, 88), (2, 1)):
      u[b, k, :] = [specials[i % 4] for i in range(Np)]
    u[1, 40, 0] = np.inf
    u[2, 89, N] = np.nan
    got = op.transfer(torch.tensor(u.ravel(), device=gpu), parent, k_old).cpu().numpy()
    got = got.reshape(batch, k_new, Np)
    for b, k in ((0, 3), (1, 88), (2, 1)):
      n = int(np.flatnonzero(parent_h == k)[0])
      np.testing.assert_array_equal(bits(got[b, n]), bits(u[b, k]))
    touched = np.zeros((batch, k_new), dtype=bool)
    for b, k in ((0, 3), (1, 88), (2, 1), (1, 40), (2, 89)):
      touched[b, parent_h == k] = True
    assert np.all(np.isfinite(got[~touched]))
    assert np.all((~np.isfinite(got[1, parent_h == 40])).any(axis=1))  # both children
    assert np.all(np.isnan(got[2, parent_h == 89]).any(axis=1))
    with np.errstate(all="ignore"):
      want = to.to_children(u.ravel(), parent_h, k_old, matrix(op, "PL"), batch)
    ok = ~touched.ravel()
    assert (np.max(np.abs(got.reshape(-1, Np)[ok] - want.reshape(-1, Np)[ok]))
            <= TOL * np.max(np.abs(u[np.isfinite(u)])))

    # new field: the same for the two operators back to the old mesh
    left = lambda k: int(np.flatnonzero(parent_h == k)[0])  # noqa: E731
    w = rng.standard_normal((batch, k_new, Np))
    for b, k in ((0, 3), (1, 88), (2, 1)):
      w[b, left(k), :] = [specials[(i + 1) % 4] for i in range(Np)]
    w[1, left(40) + 1, 0] = -np.inf  # a right child
    w[2, left(7), N] = np.nan        # a left child whose neighbour 8 is split too
    w_d = torch.tensor(w.ravel(), device=gpu)
    for fn, name in ((op.transfer_t, "PLT"), (op.restrict, "RL")):
      got = fn(w_d, parent, k_old).cpu().numpy().reshape(batch, k_old, Np)
      for b, k in ((0, 3), (1, 88), (2, 1)):
        np.testing.assert_array_equal(bits(got[b, k]), bits(w[b, left(k)]))
      touched = np.zeros((batch, k_old), dtype=bool)
      for b, k in ((0, 3), (1, 88), (2, 1), (1, 40), (2, 7)):
        touched[b, k] = True
      assert np.all(np.isfinite(got[~touched])), name
      assert not np.all(np.isfinite(got[1, 40])) and np.isnan(got[2, 7]).any(), name
      assert np.all(np.isfinite(got[2, 8])), name
    assert role[left(40) + 1] == 2 and role[left(7)] == 1 and role[left(3)] == 0


@pytest.mark.parametrize("N", ORDERS)
def test_device_identities(pkg, gpu, N):
  """restrict(transfer(u)) == u to 1e-13 max|u|; <transfer u, w> == <u, transfer_t w> to 1e-12
  of sum |transfer u| |w|; equal calls give equal bits."""
  import torch
  Np, batch = N + 1, 3
  k_old, marks = marks_for("half", 300)
  op, parent, _ = refined(pkg, torch, gpu, N, k_old, batch, marks)
  with op:
    gen = torch.Generator(device="cpu").manual_seed(N)
    u = torch.randn(batch * k_old * Np, dtype=torch.float64, generator=gen).to(gpu)
    w = torch.randn(op.field_numel, dtype=torch.float64, generator=gen).to(gpu)
    pu = op.transfer(u, parent, k_old)
    back = op.restrict(pu, parent, k_old)
    err = float((back - u).abs().max())
    print(f"N = {N}: restrict(transfer(u)) - u = {err:.3e}")
    assert err <= 1e-13 * float(u.abs().max())
    ptw = op.transfer_t(w, parent, k_old)
    lhs, rhs = float(torch.dot(pu, w)), float(torch.dot(u, ptw))
    scale = float(torch.dot(pu.abs(), w.abs()))
    print(f"N = {N}: <Pu, w> - <u, P^T w> = {lhs - rhs:.3e} of {scale:.3e}")
    assert abs(lhs - rhs) <= 1e-12 * scale
    assert torch.equal(op.transfer(u, parent, k_old), pu)
    assert torch.equal(op.transfer_t(w, parent, k_old), ptw)
    assert torch.equal(op.restrict(pu, parent, k_old), back)


@pytest.mark.parametrize("N", (1, 4, 8))
def test_two_refinements_compose(pkg, gpu, N):
  """Transfer twice across two successive refinements: the oracle's composition, and for a
  degree-N polynomial its samples on the twice-split mesh."""
  import torch
  Np, batch, k0 = N + 1, 2, 150
  rng = np.random.default_rng(N)
  m1 = (rng.random(k0) < 0.4).astype(np.uint8)
  op, p1, p1_h = refined(pkg, torch, gpu, N, k0, batch, m1)
  with op:
    k1 = op.K
    coef = rng.uniform(-1.0, 1.0, Np)
    vx0 = mesh_of(pkg, N, k0).v_x
    poly = lambda x: np.polynomial.legendre.legval(2.0 * x / vx0[-1] - 1.0, coef)  # noqa: E731
    mesh0 = mesh_of(pkg, N, k0)
    u0 = np.concatenate([mesh0.to_device_layout(poly(mesh0.x)),
                         rng.standard_normal(k0 * Np)])
    u1 = op.transfer(torch.tensor(u0, device=gpu), p1, k0)
    m2 = (rng.random(k1) < 0.4).astype(np.uint8)
    m2[np.flatnonzero(to.roles(p1_h) == 1)[0]] = 1  # a child of the first round splits again
    _, p2, p2_h = refined(pkg, torch, gpu, N, k1, batch, m2, op=op)
    u2 = op.transfer(u1, p2, k1).cpu().numpy()
    PL = matrix(op, "PL")
    want = to.to_children(to.to_children(u0, p1_h, k0, PL, batch), p2_h, k1, PL, batch)
    err = float(np.max(np.abs(u2 - want)))
    print(f"N = {N}: two transfers vs the oracle's {err:.3e}")
    # the first transfer's error passes through the second (row sums of PL: at most 2.03)
    assert err <= TOL * (2.03 * np.max(np.abs(u0)) + float(u1.abs().max()))
    vx2 = mo.split_marked(mo.split_marked(vx0, m1)[0], m2)[0]
    np.testing.assert_array_equal(op.v_x(), vx2)
    mesh2 = pkg.BaseGalerkin1D(n=N, v_x=vx2)
    exact = mesh2.to_device_layout(poly(mesh2.x))
    e_poly = float(np.max(np.abs(u2[:op.K * Np] - exact)))
    print(f"N = {N}: polynomial on the twice-split mesh {e_poly:.3e}")
    assert e_poly <= 1e-12 * np.max(np.abs(exact))


def test_argument_errors(pkg, gpu):
  import torch
  N, k_old, batch = 3, 40, 2
  Np = N + 1
  marks = np.zeros(k_old, dtype=np.uint8)
  marks[5:9] = 1
  op, parent, _ = refined(pkg, torch, gpu, N, k_old, batch, marks)
  lib, DGError = pkg._lib, pkg._lib.DGLibraryError
  with op:
    n_old, n_new = batch * k_old * Np, op.field_numel
    buf = torch.zeros(n_old + n_new, dtype=torch.float64, device=gpu)
    u, w = buf[:n_old], buf[n_old:]
    op.transfer(u, parent, k_old, out=w)  # adjacent ranges do not overlap
    op.restrict(w, parent, k_old, out=u)
    with pytest.raises(DGError, match="overlap"):
      op.transfer(u, parent, k_old, out=buf[n_old - 1:n_old - 1 + n_new])
    with pytest.raises(DGError, match="overlap"):
      op.transfer(buf[n_new - 1:n_new - 1 + n_old], parent, k_old, out=buf[:n_new])
    with pytest.raises(DGError, match="overlap"):
      op.transfer_t(buf[:n_new], parent, k_old, out=buf[1:1 + n_old])
    with pytest.raises(DGError, match="overlap"):
      op.restrict(w, parent, k_old, out=buf[n_old + 8:n_old + 8 + n_old])
    fresh = torch.zeros(n_new, dtype=torch.float64, device=gpu)
    for bad in (0, -1, op.K + 1, (op.K - 1) // 2):
      with pytest.raises(ValueError):
        op.transfer(u, parent, bad, out=fresh)
    with pytest.raises(ValueError):  # a short output, a long input
      op.transfer(u, parent, k_old, out=fresh[:-1])
    with pytest.raises(ValueError):
      op.transfer(buf[:n_old + 1], parent, k_old)
    with pytest.raises(ValueError):
      op.restrict(w, parent, k_old, out=torch.zeros(n_old - 1, dtype=torch.float64, device=gpu))
    with pytest.raises(ValueError):
      op.transfer(u, parent[:-1], k_old)
    with pytest.raises(TypeError):
      op.transfer(u.float(), parent, k_old)
    with pytest.raises(TypeError):
      op.transfer(u.cpu(), parent, k_old)
    with pytest.raises(TypeError):
      op.transfer(u, parent.long(), k_old)
    with pytest.raises(TypeError):
      op.transfer(u, parent.cpu(), k_old)
    with pytest.raises(TypeError):
      op.transfer_t(w, parent, k_old, out=torch.zeros(n_old, dtype=torch.float32, device=gpu))
    # the C ABI's own checks
    raw = lib.load()
    A = matrix(op, "PL").ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    good = [op._plan, ptr(parent), k_old, A, ptr(u), ptr(fresh), None]
    for fn in (raw.dg_field_to_children, raw.dg_field_from_children):
      for slot in (0, 1, 3, 4, 5):
        args = list(good)
        args[slot] = None
        assert fn(*args) == lib.DG_ERR_ARG
        assert b"null" in raw.dg_last_error()
      for bad in (0, -3, op.K + 1, (op.K - 1) // 2):
        args = list(good)
        args[2] = bad
        assert fn(*args) == lib.DG_ERR_ARG
        assert b"k_old" in raw.dg_last_error()
    assert raw.dg_field_to_children(*good) == lib.DG_OK
    torch.cuda.synchronize()
