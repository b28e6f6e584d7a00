"""The oracle in x87 long double (64-bit significand): the anchor of the fp64 parity tests.

TEST INFRASTRUCTURE ONLY (see oracle/__init__.py).  Never on bench.py's path.

oracle/advec.py, adjoint.py and burgers.py (``limit=False``) are dtype-generic: handed a
widened setup dict and widened fields they compute in ``np.longdouble`` throughout.  This
module provides the widening and restates only what would drop back to fp64:

* ``inflow_value`` (``math.sin`` returns a double) and with it every caller that reaches it
  through its module (``advec_rhs1d``, ``lift_residual``, the stage loops, ``burgers.rhs``,
  ``burgers.step_jvp``);
* ``effectivity.p_estimate`` / ``jump_indicator`` (``eta -=`` / ``eta +=`` into float64).

Input convention ("Extended-precision anchor").  A case's inputs are fp64
numbers, widened exactly: fields, ``VX``, the per-element ``2/h_k`` (or the one ``2/mean(h)``
of a mesh the plan calls uniform: ``startup1d(metric="element")``), the ``Dr`` and ``LIFT`` the
plan was created with (``setup``'s arguments), ``a``, ``dt``.  The time levels
``t[n+1] = t[n] + dt`` and the stage times ``t[n] + c_s*dt`` are formed in fp64, as
include/dg_advec.h states them ("time = time + dt"), and then widened; the sine and its
argument ``a*t`` / ``a*a*t`` are evaluated in long double.  The LSERK4 coefficients are the
fp64 constants of oracle/setup1d.py (the kernels' constants), widened.
"""
import numpy as np

from . import adjoint as _adj
from . import advec as _adv
from . import burgers as _bur
from .advec import INFLOW_A, INFLOW_A2, INFLOW_ZERO
from .setup1d import RK4A, RK4B, RK4C, startup1d

LD = np.longdouble


def widen(S):
  """A copy of a setup dict (oracle.setup1d.startup1d, tests/tile_edges.batched_setup) with
  every float array and float scalar as long double; index maps and ints untouched."""
  out = {}
  for k, v in S.items():
    if isinstance(v, np.ndarray) and v.dtype.kind == "f":
      out[k] = v.astype(LD)
    elif isinstance(v, (float, np.floating)):
      out[k] = LD(v)
    else:
      out[k] = v
  return out


def with_operators(S, Dr=None, LIFT=None):
  """A copy of ``S`` with the caller's differentiation and lift matrices (the ones the plan was
  created with; setup1d's agree with the package's only to 1e-12, tests/test_host.py)."""
  S = dict(S)
  if Dr is not None:
    S["Dr"] = np.array(Dr, dtype=np.float64)
  if LIFT is not None:
    S["LIFT"] = np.array(LIFT, dtype=np.float64)
  return S


def setup(N, VX, Dr=None, LIFT=None):
  """(S64, SX): startup1d(metric="element") with the caller's operators, and its widening."""
  S = with_operators(startup1d(N, VX, metric="element"), Dr, LIFT)
  return S, widen(S)


def field(u):
  return np.asarray(u, dtype=np.float64).astype(LD)


def times_of(t0, dt, nsteps):
  """t[n+1] = t[n] + dt in fp64 (One_code.mlx:139)."""
  t = [float(t0)]
  for _ in range(nsteps):
    t.append(t[-1] + float(dt))
  return t


def stage_time(time, dt, s):
  """t + c_s*dt in fp64 (One_code.mlx:121)."""
  return float(time) + float(RK4C[s]) * float(dt)


def inflow_value(a, t, inflow):
  """oracle.advec.inflow_value with the argument and the sine in long double; ``a`` and ``t``
  are fp64 numbers."""
  if inflow == INFLOW_ZERO:
    return LD(0.0)
  a, t = LD(float(a)), LD(float(t))
  return -np.sin(a * a * t) if inflow == INFLOW_A2 else -np.sin(a * t)


# --- linear advection -------------------------------------------------------------------
def advec_rhs1d(u, t, a, S, inflow=INFLOW_A):
  return _adv.advec_rhs_uin(u, inflow_value(a, t, inflow), a, S)


def lift_residual(u, t, a, S, inflow=INFLOW_A):
  du = _adv.face_jumps(u, inflow_value(a, t, inflow), a, S)
  return S["LIFT"] @ (S["Fscale"] * du)


def lserk4_step(u, time, dt, a, S, inflow=INFLOW_A):
  resu = np.zeros_like(u)
  for s in range(5):
    rhsu, _ = advec_rhs1d(u, stage_time(time, dt, s), a, S, inflow)
    resu = LD(RK4A[s]) * resu + LD(dt) * rhsu
    u = u + LD(RK4B[s]) * resu
  return u


def euler_step(u, time, dt, a, S, inflow=INFLOW_A):
  rhsu, _ = advec_rhs1d(u, time, a, S, inflow)
  return u + LD(dt) * rhsu


def step(u, time, dt, a, S, inflow=INFLOW_A, scheme="lserk4"):
  return (lserk4_step if scheme == "lserk4" else euler_step)(u, time, dt, a, S, inflow)


def forward_sweep(u0, t0, dt, nsteps, a, S, inflow=INFLOW_A, scheme="lserk4"):
  """oracle.advec.forward_sweep: (snapshots, fp64 time levels)."""
  times = times_of(t0, dt, nsteps)
  snaps = [field(u0) if u0.dtype != LD else u0.copy()]
  for n in range(nsteps):
    snaps.append(step(snaps[-1], times[n], dt, a, S, inflow, scheme))
  return snaps, times


def adjoint_step(w_next, dt, a, S, scheme="lserk4"):
  """oracle.adjoint.adjoint_step (state-independent; long double with widened ``S``, ``w``)."""
  return _adj.adjoint_step(w_next, LD(dt), a, S, scheme)


def adjoint_sweep(wT, snaps, times, dt, a, S, inflow=INFLOW_A, src_coef=0.0, scheme="lserk4"):
  """oracle.adjoint.adjoint_sweep: (w^0, eta)."""
  nsteps = len(snaps) - 1
  eta = np.zeros(S["K"], dtype=LD)
  w = wT.copy()
  src = LD(float(src_coef))
  for n in range(nsteps - 1, -1, -1):
    if n != nsteps - 1:
      w = w + src * snaps[n + 1]
    R = lift_residual(snaps[n + 1], times[n + 1], a, S, inflow)
    eta = eta + LD(dt) * np.sum(w * R, axis=0)
    w = adjoint_step(w, dt, a, S, scheme)
  if nsteps:
    w = w + src * snaps[0]
  return w, eta


def jump_indicator(snaps, times, dt, a, S, g, inflow=INFLOW_ZERO):
  """oracle.effectivity.jump_indicator for the terminal weight ``g`` (no source)."""
  nsteps = len(snaps) - 1
  ws = [None] * (nsteps + 1)
  ws[nsteps] = g.copy()
  for n in range(nsteps - 1, -1, -1):
    ws[n] = adjoint_step(ws[n + 1], dt, a, S)
  eta = np.zeros(S["K"], dtype=LD)
  for n in range(nsteps):
    R = lift_residual(snaps[n + 1], times[n + 1], a, S, inflow)
    eta = eta + LD(dt) * np.sum(ws[n + 1] * R, axis=0)
  return eta


def raw_jumps(u, K, batch, uin):
  """tests/tile_edges.raw_jumps: the recorded left-face jump per element of an (Np, batch*K)
  field."""
  left = np.concatenate((np.zeros(1, dtype=u.dtype), u[-1, :-1]))
  left[np.arange(batch) * K] = uin
  return u[0] - left


def p_estimate(snaps, times, dt, a, S_hi, P, g_hi, inflow=INFLOW_ZERO):
  """oracle.effectivity.p_estimate with the caller's prolongation ``P`` (widened): (eta, w^0)."""
  nsteps = len(snaps) - 1
  ps = [P @ u for u in snaps]
  ws = [None] * (nsteps + 1)
  ws[nsteps] = g_hi.copy()
  for n in range(nsteps - 1, -1, -1):
    ws[n] = adjoint_step(ws[n + 1], dt, a, S_hi)
  eta = np.zeros(S_hi["K"], dtype=LD)
  for n in range(nsteps):
    R = ps[n + 1] - lserk4_step(ps[n], times[n], dt, a, S_hi, inflow)
    eta = eta - np.sum(ws[n + 1] * R, axis=0)
  return eta, ws[0]


# --- Burgers flux, no limiter -----------------------------------------------------------
def nl_rhs(u, t, a, S, kind=_bur.FLUX_BURGERS, inflow=INFLOW_A):
  f = _bur.flux(u, kind)
  du = _bur.flux_jumps(u, inflow_value(a, t, inflow), a, S, kind)
  return -a * S["rx"] * (S["Dr"] @ f) + S["LIFT"] @ (S["Fscale"] * du)


def nl_jump_residual(u, t, a, S, kind=_bur.FLUX_BURGERS, inflow=INFLOW_A):
  du = _bur.flux_jumps(u, inflow_value(a, t, inflow), a, S, kind)
  return S["LIFT"] @ (S["Fscale"] * du)


def nl_step(u, time, dt, a, S, kind=_bur.FLUX_BURGERS, inflow=INFLOW_A):
  resu = np.zeros_like(u)
  for s in range(5):
    resu = LD(RK4A[s]) * resu + LD(dt) * nl_rhs(u, stage_time(time, dt, s), a, S, kind, inflow)
    u = u + LD(RK4B[s]) * resu
  return u


def nl_forward_sweep(u0, t0, dt, nsteps, a, S, kind=_bur.FLUX_BURGERS, inflow=INFLOW_A):
  times = times_of(t0, dt, nsteps)
  snaps = [field(u0) if u0.dtype != LD else u0.copy()]
  for n in range(nsteps):
    snaps.append(nl_step(snaps[-1], times[n], dt, a, S, kind, inflow))
  return snaps, times


def nl_step_jvp(u, du, time, dt, a, S, kind, inflow):
  resu, dres = np.zeros_like(u), np.zeros_like(u)
  for s in range(5):
    rhsu = nl_rhs(u, stage_time(time, dt, s), a, S, kind, inflow)
    drhs = _bur.rhs_tangent(u, du, a, S, kind)
    resu = LD(RK4A[s]) * resu + LD(dt) * rhsu
    dres = LD(RK4A[s]) * dres + LD(dt) * drhs
    u = u + LD(RK4B[s]) * resu
    du = du + LD(RK4B[s]) * dres
  return u, du


def nl_step_vjp(u, w, time, dt, a, S, kind=_bur.FLUX_BURGERS, inflow=INFLOW_A):
  """oracle.burgers.step_vjp without a limiter (a step couples k-5 .. k+5)."""
  Np, K = u.shape
  reach = 5
  P = min(2 * reach + 1, K)
  out = np.zeros_like(u)
  for c in range(P):
    cols = np.arange(c, K, P)
    for p in range(Np):
      seed = np.zeros_like(u)
      seed[p, cols] = 1.0
      _, d = nl_step_jvp(u, seed, time, dt, a, S, kind, inflow)
      prod = np.sum(d * w, axis=0)  # per element
      for off in range(-reach, reach + 1):
        ok = (cols + off >= 0) & (cols + off < K)
        out[p, cols[ok]] = out[p, cols[ok]] + prod[cols[ok] + off]
  return out


def nl_adjoint_sweep(wT, snaps, times, dt, a, S, kind=_bur.FLUX_BURGERS, inflow=INFLOW_A):
  """oracle.burgers.adjoint_sweep (limit=False, no source): (w^0, eta)."""
  nsteps = len(snaps) - 1
  eta = np.zeros(S["K"], dtype=LD)
  w = wT.copy()
  for n in range(nsteps - 1, -1, -1):
    R = nl_jump_residual(snaps[n + 1], times[n + 1], a, S, kind, inflow)
    eta = eta + LD(dt) * np.sum(w * R, axis=0)
    w = nl_step_vjp(snaps[n], w, times[n], dt, a, S, kind, inflow)
  return w, eta
