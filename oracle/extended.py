"""The oracle in x87 long double (64-bit significand): the anchor of the fp64 parity tests.

TEST INFRASTRUCTURE ONLY (see oracle/__init__.py).  Never on bench.py's path.

oracle/advec.py, adjoint.py and burgers.py (``limit=False``) are dtype-generic: handed a
widened setup dict and widened fields they compute in ``np.longdouble`` throughout.  This
module provides the widening and restates only what would drop back to fp64:

* ``inflow_value`` (``math.sin`` returns a double) and with it every caller that reaches it
  through its module (``advec_rhs1d``, ``lift_residual``, the stage loops, ``burgers.rhs``,
  ``burgers.step_jvp``);
* ``effectivity.p_estimate`` / ``jump_indicator`` (``eta -=`` / ``eta +=`` into float64);
* every path with a limiter (``oracle.limiter.minmod`` casts to ``float``): the stage limiters in
  the mesh-free form of csrc/dg_nl.h with their decision codes and decision margins, the limited
  LSERK4 sweep, its frozen-decision tangent and coloured adjoint, the jump indicator (the
  section "limited paths" below, which runs in long double or in fp64 as its inputs are).

Input convention ("Extended-precision anchor").  A case's inputs are fp64
numbers, widened exactly: fields, ``VX``, the per-element ``2/h_k`` (or the one ``2/mean(h)``
of a mesh the plan calls uniform: ``startup1d(metric="element")``), the ``Dr`` and ``LIFT`` the
plan was created with (``setup``'s arguments; for the limiters also its ``V``, ``invV`` and
``r``, ``with_operators``), ``a``, ``dt``.  The time levels
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


def with_operators(S, Dr=None, LIFT=None, V=None, invV=None, r=None):
  """A copy of ``S`` with the caller's differentiation and lift matrices (the ones the plan was
  created with; setup1d's agree with the package's only to 1e-12, tests/test_host.py), and for
  the limiters its Vandermonde matrix, that matrix's inverse and its nodes.  With ``r`` the
  fp64 node coordinates ``x`` are formed again from ``VX`` and the caller's nodes
  (StartUp1D.m:20, as k_limit forms them)."""
  S = dict(S)
  if Dr is not None:
    S["Dr"] = np.array(Dr, dtype=np.float64)
  if LIFT is not None:
    S["LIFT"] = np.array(LIFT, dtype=np.float64)
  if V is not None:
    S["V"] = np.array(V, dtype=np.float64)
  if invV is not None:
    S["invV"] = np.array(invV, dtype=np.float64)
  if r is not None:
    S["r"] = np.array(r, dtype=np.float64)
    VX = S["VX"]
    S["x"] = np.ones((len(S["r"]), 1)) * VX[None, :-1] + \
        (0.5 * (S["r"] + 1))[:, None] * (VX[1:] - VX[:-1])[None, :]
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


# --- limited paths (config 3): the stage limiter in the mesh-free form ---------------------------
# Everything below is dtype-generic: handed a widened setup and long-double fields it computes in
# long double (the reference); handed the fp64 setup and fp64 fields it computes in fp64 with the
# host's fp64 sine (the ``e64`` of the bar).  One trajectory per call (batch 1).
#
# The limiter is stated as the stage kernels state it (csrc/dg_nl.h:15-19): on a limited cell
#   y_i = v + (r_i / 2) hm,   hm = minmod(2 (Dr ul)(1), v+ - v, v - v-),
# which is SlopeLimitLin.m:10-18 with h m = hm and x_i - x0 = h r_i / 2: no mesh coordinate enters,
# so there is no eps |x| / h cancellation (``slope_limit_coord`` is the coordinate form, for the
# proof that both state the same function).  Each call also returns the per-element decision code
# of the record (4 | br for a limited cell, br = 0 signs differ / 1..3 the active argument, first
# minimum on ties; 0 for an untroubled cell) and the decision margin: the smallest perturbation (in
# the maximum norm over the compared quantities, divided by max|input|) that flips a decision.
EPS0 = 1.0e-8  # SlopeLimitN.m:12


def uin_of(a, t, inflow, like):
  """The inflow value in the precision of ``like``: the long-double sine, or the fp64 one."""
  if like.dtype == LD:
    return inflow_value(a, t, inflow)
  return _adv.inflow_value(float(a), float(t), inflow)


def minmod_br(a, b, c):
  """minmod.m:6-12 of three arrays and which argument it returned (csrc/dg_nl.h minmod_br): 0
  when the signs differ (value 0), else 1..3, the first minimum of |.|."""
  pos = (a > 0) & (b > 0) & (c > 0)
  neg = (a < 0) & (b < 0) & (c < 0)
  mag = np.stack((np.abs(a), np.abs(b), np.abs(c)))
  k = np.argmin(mag, axis=0)  # the first minimum
  m = np.take_along_axis(mag, k[None], axis=0)[0]
  val = np.where(pos, m, np.where(neg, -m, np.zeros_like(m)))
  return val, np.where(pos | neg, k + 1, 0)


def _minmod_margin(a, b, c):
  """Per element, the smallest max-norm change of (a, b, c) that changes minmod_br's ``br``:
  active (one sign): the least magnitude reaching zero, or the two least magnitudes meeting;
  inactive: the arguments on the minority side (zeros included) all crossing to the other."""
  args = np.stack((a, b, c))
  mag = np.sort(np.abs(args), axis=0)
  active = np.all(args > 0, axis=0) | np.all(args < 0, axis=0)
  zero = np.zeros_like(args)
  to_pos = np.max(np.where(args <= 0, np.abs(args), zero), axis=0)
  to_neg = np.max(np.where(args >= 0, np.abs(args), zero), axis=0)
  return np.where(active, np.minimum(mag[0], mag[1] - mag[0]), np.minimum(to_pos, to_neg))


def _neighbours(v):
  """The neighbour averages, replicated at the trajectory's ends (SlopeLimitN.m:18)."""
  return np.concatenate((v[:1], v[:-1])), np.concatenate((v[1:], v[-1:]))


def _lim_parts(v, S):
  avg = S["V"][0, 0] * (S["invV"][0] @ v)  # SlopeLimitN.m:9
  uh0, uh1 = S["invV"][0] @ v, S["invV"][1] @ v
  ul = S["V"][:, 0:1] * uh0[None, :] + S["V"][:, 1:2] * uh1[None, :]  # :28
  return avg, ul


def _slope_arg(v, S):
  """h ux(1) = 2 (Dr ul)(1) (SlopeLimitLin.m:16) as csrc/dg_nl.h:18 writes it,
  2 (Dr V)(1,1:2) uh(1:2): the same number in exact arithmetic, without the cancellation of
  |Dr(1,:)| |ul| (40 eps at N = 7) that the product with the nodal ul carries in fp64."""
  d0, d1 = S["Dr"][0] @ S["V"][:, 0], S["Dr"][0] @ S["V"][:, 1]
  return 2 * (d0 * (S["invV"][0] @ v) + d1 * (S["invV"][1] @ v))


def stage_limiter(v, S, kind="N", M=None, h=None):
  """SlopeLimitN (``kind`` "N", troubled cells only) or SlopeLimit1 ("1", every cell) of the
  (Np, K) field ``v``, mesh-free.  ``M`` > 0 with the element widths ``h``: the TVB minmod
  (minmodB.m:6-11, |ux| > M h^2 with ux = a1 / h).  Returns (y, code (K,), margin)."""
  K = v.shape[1]
  inf = np.full(K, np.inf, dtype=v.dtype)
  avg, ul = _lim_parts(v, S)
  vm, vp = _neighbours(avg)
  b, c = avg - vm, vp - avg
  if kind == "1":
    troubled, margin = np.ones(K, dtype=bool), inf.copy()
  else:
    u0, uN = v[0], v[-1]
    q1 = np.abs((avg - minmod_br(avg - u0, b, c)[0]) - u0)  # :21
    q2 = np.abs((avg + minmod_br(uN - avg, b, c)[0]) - uN)  # :22
    troubled = (q1 > EPS0) | (q2 > EPS0)  # :23
    # (minmod is continuous in its arguments, so only the two compares against eps0 decide)
    over = np.maximum(np.where(q1 > EPS0, q1 - EPS0, 0), np.where(q2 > EPS0, q2 - EPS0, 0))
    margin = np.where(troubled, over, np.minimum(EPS0 - q1, EPS0 - q2))
  a1 = _slope_arg(v, S)
  hm, br = minmod_br(a1, c, b)  # :18, arguments (ux, (v+ - v)/h, (v - v-)/h) scaled by h
  mm = _minmod_margin(a1, c, b)
  # the replicated neighbour makes one argument an exact zero in every precision: minmod is 0 there
  # whatever the others are, no decision to flip
  mm[0] = mm[K - 1] = np.inf
  if M:
    lim = M * h * h * h
    keep = ~(np.abs(a1) > lim)  # minmodB.m:8-9: the element's own slope is kept
    hm, br = np.where(keep, a1, hm), np.where(keep, 1, br)
    mm = np.minimum(np.where(keep, inf, mm), np.abs(np.abs(a1) - lim))
  margin = np.where(troubled, np.minimum(margin, mm), margin)
  y = np.where(troubled[None, :], avg[None, :] + (S["r"] / 2)[:, None] * hm[None, :], v)
  code = np.where(troubled, 4 | br, 0)
  return y, code, float(np.min(margin) / np.max(np.abs(v)))


def node_coordinates(S):
  """x_i = xa + (r_i + 1)/2 (xb - xa) from the setup's own ``VX`` and ``r`` (k_limit's statement;
  long double when ``S`` is widened -- never a widened fp64 ``x``)."""
  VX = S["VX"]
  return VX[None, :-1] + ((S["r"] + 1) / 2)[:, None] * (VX[1:] - VX[:-1])[None, :]


def slope_limit(v, S, kind="N", M=None):
  """The stand-alone limiter (dg_slope_limit_n / _1, TVB with ``M``) in the mesh-free form with
  h = x_N - x_0 of ``node_coordinates``: (y, code, margin)."""
  x = node_coordinates(S)
  return stage_limiter(v, S, kind, M, x[-1] - x[0])


def slope_limit_coord(v, S, kind="N", M=None):
  """The same function in SlopeLimitLin.m:10-18's coordinate form (as oracle/limiter.py and
  k_limit state it): y = v + (x - x0) m.  Returns (y, code)."""
  x = node_coordinates(S)
  _, code, _ = slope_limit(v, S, kind, M)
  avg, ul = _lim_parts(v, S)
  vm, vp = _neighbours(avg)
  h = x[-1] - x[0]  # :10
  x0 = x[0] + h / 2  # :11
  ux = (2 / h) * (S["Dr"][0] @ ul)  # :16
  m, br = minmod_br(ux, (vp - avg) / h, (avg - vm) / h)  # :18
  if M:
    keep = ~(np.abs(ux) > M * h * h)
    m, br = np.where(keep, ux, m), np.where(keep, 1, br)
  troubled = code != 0
  y = np.where(troubled[None, :], avg[None, :] + (x - x0[None, :]) * m[None, :], v)
  return y, np.where(troubled, 4 | br, 0)


def stage_limiter_jvp(dv, S, code):
  """The limiter's derivative applied to ``dv`` ((Np, K) or (Np, K, C)) with the decisions
  ``code`` frozen: an untroubled cell passes dv; a limited one gives davg + (r/2) dhm, dhm the
  tangent of the recorded minmod argument (0 for br = 0)."""
  ex = (slice(None),) + (None,) * (dv.ndim - 2)
  davg = S["V"][0, 0] * np.tensordot(S["invV"][0], dv, 1)
  col = (slice(None),) + (None,) * (dv.ndim - 1)
  d0, d1 = S["Dr"][0] @ S["V"][:, 0], S["Dr"][0] @ S["V"][:, 1]  # _slope_arg, which is linear
  da1 = 2 * (d0 * np.tensordot(S["invV"][0], dv, 1) + d1 * np.tensordot(S["invV"][1], dv, 1))
  dvm, dvp = _neighbours(davg)
  br = (code & 3)[ex]
  zero = np.zeros_like(davg)
  dhm = np.where(br == 1, da1, np.where(br == 2, dvp - davg, np.where(br == 3, davg - dvm, zero)))
  dy = davg[None] + (S["r"] / 2)[col] * dhm[None]
  return np.where(((code & 4) != 0)[ex][None], dy, dv)


def lim_rhs(u, t, a, S, kind, inflow):
  f = _bur.flux(u, kind)
  du = _bur.flux_jumps(u, uin_of(a, t, inflow, u), a, S, kind)
  return -a * S["rx"] * (S["Dr"] @ f) + S["LIFT"] @ (S["Fscale"] * du)


def lim_jump_residual(u, t, a, S, kind, inflow):
  du = _bur.flux_jumps(u, uin_of(a, t, inflow, u), a, S, kind)
  return S["LIFT"] @ (S["Fscale"] * du)


def lim_step(u, time, dt, a, S, kind=_bur.FLUX_BURGERS, inflow=INFLOW_A, limit="N"):
  """One LSERK4 step with the limiter after every stage's update (One_code.mlx:120-137).
  Returns (u^{n+1}, codes (5, K), the step's smallest margin, [(stage input, code)] for the
  tangent)."""
  T = u.dtype.type
  resu = np.zeros_like(u)
  codes, margin, stages = [], np.inf, []
  for s in range(5):
    resu = T(RK4A[s]) * resu + T(dt) * lim_rhs(u, stage_time(time, dt, s), a, S, kind, inflow)
    y, code, mg = stage_limiter(u + T(RK4B[s]) * resu, S, limit)
    stages.append((u, code))
    codes.append(code)
    margin = min(margin, mg)
    u = y
  return u, np.stack(codes), margin, stages


def lim_forward_sweep(u0, t0, dt, nsteps, a, S, kind=_bur.FLUX_BURGERS, inflow=INFLOW_A,
                      limit="N"):
  """(snapshots, fp64 time levels, codes (nsteps, 5, K), the sweep's smallest margin)."""
  times = times_of(t0, dt, nsteps)
  snaps, codes, margin = [u0.copy()], [], np.inf
  for n in range(nsteps):
    u, c, mg, _ = lim_step(snaps[-1], times[n], dt, a, S, kind, inflow, limit)
    snaps.append(u)
    codes.append(c)
    margin = min(margin, mg)
  return snaps, times, np.stack(codes), margin


def pack_codes(codes):
  """(nsteps, 5, K) stage codes as the record's 16-bit words (nsteps, K): 3 bits per stage."""
  return sum(codes[:, s].astype(np.int64) << (3 * s) for s in range(5))


def lim_step_tangent(du, stages, dt, a, S, kind):
  """d step [du] with the limiter's decisions frozen (``stages`` of ``lim_step``); ``du`` is
  (Np, K) or (Np, K, C), one trajectory."""
  T = du.dtype.type
  col = (slice(None),) + (None,) * (du.ndim - 1)
  ex = (slice(None),) + (None,) * (du.ndim - 2)
  sc = S["rx"][0][ex]  # the element's 2/h (rx = Fscale, constant per element)
  half_a = T(a) / 2
  dres = np.zeros_like(du)
  for s, (us, code) in enumerate(stages):
    df = us[(Ellipsis,) + (None,) * (du.ndim - 2)] * du if kind == _bur.FLUX_BURGERS else du
    zero = np.zeros_like(df[0, :1])
    dl = (df[0] - np.concatenate((zero, df[-1, :-1]))) * (-half_a)  # AdvecRHS1D.m:11, nx = -1
    dr = (df[-1] - np.concatenate((df[0, 1:], df[-1, -1:]))) * half_a  # nx = +1; outflow: 0 (:16)
    drhs = -T(a) * sc[None] * np.tensordot(S["Dr"], df, 1) \
        + S["LIFT"][:, 0][col] * (sc * dl)[None] + S["LIFT"][:, 1][col] * (sc * dr)[None]
    dres = T(RK4A[s]) * dres + T(dt) * drhs
    du = stage_limiter_jvp(du + T(RK4B[s]) * dres, S, code)
  return du


def lim_step_vjp(u, w, time, dt, a, S, kind=_bur.FLUX_BURGERS, inflow=INFLOW_A, limit="N"):
  """J^T w of one limited step by coloured tangents, as oracle.burgers.step_vjp (a limited step
  couples k-10 .. k+10); also the recomputed step's codes and margin."""
  Np, K = u.shape
  _, codes, margin, stages = lim_step(u, time, dt, a, S, kind, inflow, limit)
  reach = 10
  P = min(2 * reach + 1, K)
  out = np.zeros_like(u)
  for c in range(P):
    cols = np.arange(c, K, P)
    seed = np.zeros((Np, K, Np), dtype=u.dtype)
    for p in range(Np):
      seed[p, cols, p] = 1
    d = lim_step_tangent(seed, stages, dt, a, S, kind)
    prod = np.sum(d * w[:, :, None], axis=0)  # (K, Np): per element, per seeded node
    for off in range(-reach, reach + 1):
      ok = (cols + off >= 0) & (cols + off < K)
      out[:, cols[ok]] = out[:, cols[ok]] + prod[cols[ok] + off].T
  return out, codes, margin


def lim_adjoint_sweep(wT, snaps, times, dt, a, S, kind=_bur.FLUX_BURGERS, inflow=INFLOW_A,
                      limit="N", src_coef=0.0):
  """oracle.burgers.adjoint_sweep with the limiter: (w^0, eta, the recomputed codes
  (nsteps, 5, K), their smallest margin).  eta is the jump indicator
  eta_k = dt sum_n sum_i w^{n+1}_{k,i} R_i(u^{n+1}, t_{n+1})."""
  T = wT.dtype.type
  nsteps = len(snaps) - 1
  eta = np.zeros(S["K"], dtype=wT.dtype)
  w = wT.copy()
  src = T(float(src_coef))
  codes, margin = [None] * nsteps, np.inf
  for n in range(nsteps - 1, -1, -1):
    if n != nsteps - 1:
      w = w + src * snaps[n + 1]
    R = lim_jump_residual(snaps[n + 1], times[n + 1], a, S, kind, inflow)
    eta = eta + T(dt) * np.sum(w * R, axis=0)
    w, codes[n], mg = lim_step_vjp(snaps[n], w, times[n], dt, a, S, kind, inflow, limit)
    margin = min(margin, mg)
  if nsteps:
    w = w + src * snaps[0]
  return w, eta, np.stack(codes), margin


def lim_jump_indicator(snaps, times, dt, a, S, g, kind=_bur.FLUX_BURGERS, inflow=INFLOW_A,
                       limit="N"):
  """The jump indicator of a limited sweep for the terminal weight ``g`` (no source)."""
  return lim_adjoint_sweep(g, snaps, times, dt, a, S, kind, inflow, limit)[1]
