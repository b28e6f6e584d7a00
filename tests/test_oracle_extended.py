"""oracle/extended.py: the long-double oracle really computes in long double, and every case of
tests/test_gpu_extended.py meets the reference-alone condition e64 <= CAP.

The proof that no stage rounds to fp64 is a 40-digit mpmath restatement (explicit loops over
elements, nodes and faces; a dense transpose for the adjoint) of the RHS, one LSERK4 step, one
adjoint step and the jump indicator on a tiny case: the long-double oracle meets it to 1e-18 of
max|ref| (its eps is 1.1e-19), the fp64 oracle only to about 1e-16.
"""
import numpy as np
import pytest

import extended_oracle as xo
from conftest import load_pkg
from oracle import adjoint as oadj
from oracle import advec as oadv
from oracle import effectivity as oef
from oracle import extended as ox
from oracle import setup1d

LD = np.longdouble


def test_long_double_is_extended():
  assert np.finfo(np.longdouble).nmant >= 63


# --- the mpmath restatement ---------------------------------------------------------------------
def mp_case():
  """N = 2, K = 4, non-uniform, 3 steps, inflow a2, the package's own Dr / LIFT."""
  pkg = load_pkg()
  v_x = np.array([0.0, 0.21, 0.5, 0.62, 1.0])
  mesh = pkg.BaseGalerkin1D(n=2, v_x=v_x)
  S, SX = ox.setup(2, v_x, mesh.d_r, mesh.lift)
  assert np.ptp(S["rx"]) > 0  # per-element 2/h_k
  rng = np.random.default_rng(3)
  u0 = rng.standard_normal((3, 4))
  g = rng.standard_normal((3, 4))
  dt = oadv.bench_dt(S)
  return S, SX, u0, g, 2 * np.pi, 0.02, dt


class MP:
  """The scheme on lists of mpf, u[k][i] (element k, node i); every input an fp64 number."""

  def __init__(self, S, a, dt, inflow):
    import mpmath
    self.mp = mpmath
    f = mpmath.mpf
    self.K, self.Np = S["K"], S["Np"]
    self.Dr = [[f(float(v)) for v in row] for row in S["Dr"]]
    self.LIFT = [[f(float(v)) for v in row] for row in S["LIFT"]]
    self.sc = [f(float(S["rx"][0, k])) for k in range(self.K)]
    assert np.array_equal(S["rx"][0], S["Fscale"][0])
    self.a, self.dt, self.inflow = f(float(a)), f(float(dt)), inflow
    self.A = [f(float(v)) for v in setup1d.RK4A]
    self.B = [f(float(v)) for v in setup1d.RK4B]
    self.zero = f(0)

  def field(self, u):
    return [[self.mp.mpf(float(u[i, k])) for i in range(self.Np)] for k in range(self.K)]

  def array(self, u):
    return np.array([[u[k][i] for k in range(self.K)] for i in range(self.Np)], dtype=object)

  def uin(self, t):
    """t an fp64 number (the time level formed in fp64)."""
    if self.inflow == "zero":
      return self.zero
    t = self.mp.mpf(float(t))
    return -self.mp.sin(self.a * self.a * t if self.inflow == "a2" else self.a * t)

  def jumps(self, u, uin):
    """(du at the left face, du at the right face) per element: (u- - u+) * (a nx) / 2."""
    K, L = self.K, self.Np - 1
    out = []
    for k in range(K):
      left = u[k - 1][L] if k > 0 else uin
      dl = (u[k][0] - left) * (-self.a) / 2
      dr = (u[k][L] - u[k + 1][0]) * self.a / 2 if k + 1 < K else self.zero
      out.append((dl, dr))
    return out

  def lift(self, u, uin):
    du = self.jumps(u, uin)
    return [[self.LIFT[i][0] * (self.sc[k] * du[k][0]) + self.LIFT[i][1] * (self.sc[k] * du[k][1])
             for i in range(self.Np)] for k in range(self.K)]

  def rhs(self, u, uin):
    R = self.lift(u, uin)
    return [[-self.a * self.sc[k] * sum(self.Dr[i][j] * u[k][j] for j in range(self.Np)) + R[k][i]
             for i in range(self.Np)] for k in range(self.K)]

  def step(self, u, t):
    res = [[self.zero] * self.Np for _ in range(self.K)]
    for s in range(5):
      r = self.rhs(u, self.uin(ox.stage_time(t, float(self.dt), s)))
      res = [[self.A[s] * res[k][i] + self.dt * r[k][i] for i in range(self.Np)] for k in range(self.K)]
      u = [[u[k][i] + self.B[s] * res[k][i] for i in range(self.Np)] for k in range(self.K)]
    return u

  def flat(self, u):
    return [u[k][i] for k in range(self.K) for i in range(self.Np)]

  def unflat(self, v):
    return [[v[k * self.Np + i] for i in range(self.Np)] for k in range(self.K)]

  def adjoint_step(self, w):
    """(dense homogeneous step matrix)^T w."""
    n = self.K * self.Np
    keep, self.inflow = self.inflow, "zero"
    cols = []
    for j in range(n):
      e = [self.zero] * n
      e[j] = self.mp.mpf(1)
      cols.append(self.flat(self.step(self.unflat(e), 0.0)))
    self.inflow = keep
    wf = self.flat(w)
    return self.unflat([sum(cols[j][i] * wf[i] for i in range(n)) for j in range(n)])


def rel(x, ref):
  """max|x - ref| / max|ref| with ref an object array of mpf."""
  x = np.asarray(x)
  d = max(abs(_mpf(x[idx]) - ref[idx]) for idx in np.ndindex(ref.shape))
  return float(d / max(abs(v) for v in ref.ravel()))


def _mpf(v):
  """A long double (or double) as an mpf, exactly: high part + remainder."""
  import mpmath
  v = LD(v)
  hi = float(v)
  return mpmath.mpf(hi) + mpmath.mpf(float(v - LD(hi)))


def test_long_double_oracle_meets_the_mpmath_restatement():
  mpmath = pytest.importorskip("mpmath")
  mpmath.mp.dps = 40
  S, SX, u0, g, a, t0, dt = mp_case()
  inflow, nsteps = "a2", 3
  m = MP(S, a, dt, inflow)
  times = ox.times_of(t0, dt, nsteps)
  um = m.field(u0)
  figures = {}

  def both(what, x, d, ref):
    ex, ed = rel(x, ref), rel(d, ref)
    figures[what] = (ex, ed)
    print(f"  {what}: long double {ex:.2e}, fp64 {ed:.2e}")

  # RHS at a stage time
  t = ox.stage_time(t0, dt, 3)
  both("rhs", ox.advec_rhs1d(ox.field(u0), t, a, SX, inflow)[0],
       oadv.advec_rhs1d(u0, t, a, S, inflow)[0], m.array(m.rhs(um, m.uin(t))))
  # three LSERK4 steps (the first is "one step"; the indicator needs the states)
  sx, tx = ox.forward_sweep(u0, t0, dt, nsteps, a, SX, inflow)
  sd, _ = oadv.forward_sweep(u0, t0, dt, nsteps, a, S, inflow)
  assert tx == times
  sm = [um]
  for n in range(nsteps):
    sm.append(m.step(sm[-1], times[n]))
  both("one LSERK4 step", sx[1], sd[1], m.array(sm[1]))
  both("u^3", sx[3], sd[3], m.array(sm[3]))
  # one adjoint step
  wm = m.adjoint_step(m.field(g))
  both("one adjoint step", ox.adjoint_step(ox.field(g), dt, a, SX), oadj.adjoint_step(g, dt, a, S),
       m.array(wm))
  # the jump indicator, terminal weight g, on each oracle's own states
  ws = [None] * (nsteps + 1)
  ws[nsteps] = m.field(g)
  for n in range(nsteps - 1, -1, -1):
    ws[n] = m.adjoint_step(ws[n + 1])
  eta = [m.zero] * m.K
  for n in range(nsteps):
    R = m.lift(sm[n + 1], m.uin(times[n + 1]))
    eta = [eta[k] + m.dt * sum(ws[n + 1][k][i] * R[k][i] for i in range(m.Np)) for k in range(m.K)]
  eta_d = np.zeros(S["K"])
  wd = oef.adjoint_weights(sd, g, dt, a, S)
  for n in range(nsteps):
    eta_d = eta_d + dt * np.sum(wd[n + 1] * oadv.lift_residual(sd[n + 1], times[n + 1], a, S, inflow), axis=0)
  both("jump indicator", ox.jump_indicator(sx, times, dt, a, SX, ox.field(g), inflow), eta_d,
       np.array(eta, dtype=object))
  for what, (ex, ed) in figures.items():
    assert ex <= 1e-18, (what, ex)
    assert ed <= 2e-15, (what, ed)
  # fp64 is visibly coarser: no quantity of the long-double oracle sits at fp64's level
  assert max(ex for ex, _ in figures.values()) < 0.02 * max(ed for _, ed in figures.values())
  for s in sx:
    assert s.dtype == LD


def test_every_output_is_long_double():
  pkg = load_pkg()
  fwd = xo.forward_ref(pkg, 2, 9, False, 2, xo.AWAY, 3)
  adj = xo.adjoint_ref(pkg, (2, 9, False, 2, xo.AWAY, 3), xo.AWAY, src=0.3)
  for q in fwd["X"]["snaps"] + [fwd["X"]["rec"], adj["X"]["w0"], adj["X"]["eta"]]:
    assert q.dtype == LD
  fwd1 = xo.forward_ref(pkg, 2, 9, False, 1, xo.AWAY, 3)
  p = xo.p_ref(pkg, (2, 9, False, 1, xo.AWAY, 3), xo.AWAY)
  for q in p["X"].values():
    assert q.dtype == LD
  assert fwd1["D"]["snaps"][-1].dtype == np.float64
  nl = xo.nl_forward_ref(pkg, 2, 9, False)
  assert nl["X"]["snaps"][-1].dtype == LD
  on = xo.nl_adjoint_on(nl, nl["D"]["snaps"])
  assert on["X"]["w0"].dtype == LD and on["X"]["eta"].dtype == LD


def test_burgers_adjoint_restatement_equals_the_oracle_in_fp64():
  """oracle.extended.nl_step_vjp sums each coloured column's window directly; in fp64 inputs it
  must give oracle.burgers.step_vjp (limit=False) to rounding."""
  pkg = load_pkg()
  nl = xo.nl_forward_ref(pkg, 2, 30, False)
  on = xo.nl_adjoint_on(nl, nl["D"]["snaps"])
  assert xo.err(on["D"]["w0"], on["X"]["w0"]) <= 1e-14
  assert xo.err(on["D"]["eta"], on["X"]["eta"]) <= 1e-14


# --- the reference-alone condition of every GPU case ----------------------------------------------
LINEAR = xo.linear_case_keys()


@pytest.mark.parametrize("case", LINEAR, ids=[c[0] for c in LINEAR])
def test_reference_alone_condition_linear(case):
  cid, key, scheme, src, p = case
  pkg = load_pkg()
  point = key[4]
  fwd = xo.forward_ref(pkg, *key, scheme=scheme)
  worst = {}
  worst["snapshots"] = max(xo.err(d, x) for d, x in zip(fwd["D"]["snaps"], fwd["X"]["snaps"]))
  worst["record"] = xo.err(fwd["D"]["rec"], fwd["X"]["rec"])
  if src is not None:
    adj = xo.adjoint_ref(pkg, key, point, src, scheme)
    worst["w0"] = xo.err(adj["D"]["w0"], adj["X"]["w0"])
    worst["eta"] = xo.err(adj["D"]["eta"], adj["X"]["eta"])
    top = np.sort(np.abs(adj["X"]["eta"]))[::-1]
    print(f"  {cid}: max|eta| = {float(top[0]):.3g}, top-2 gap = {float((top[0] - top[1]) / top[0]):.2e}")
  if p:
    pr = xo.p_ref(pkg, key, point)
    for q in ("eta", "w0", "prolong"):
      worst["p " + q] = xo.err(pr["D"][q], pr["X"][q])
  print(f"  {cid}: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
  for k, v in worst.items():
    assert v <= xo.CAP, (cid, k, v)


RHS = [(N, K, uni, inflow, "linear") for N in range(1, 9) for inflow in ("a", "a2")
       for K, uni in xo.RHS_MESHES] + \
      [(N, K, uni, "a", "burgers") for N in (1, 2, 4, 8) for K, uni in xo.RHS_MESHES]


def test_reference_alone_condition_rhs():
  pkg = load_pkg()
  for N, K, uni, inflow, flux in RHS:
    r = xo.rhs_ref(pkg, N, K, uni, inflow, flux)
    assert xo.err(r["D"], r["X"]) <= xo.CAP, (N, K, uni, inflow, flux)


@pytest.mark.parametrize("exchange", [0, 1])
@pytest.mark.parametrize("N", [2, 4])
def test_reference_alone_condition_burgers(N, exchange):
  pkg = load_pkg()
  nl = xo.nl_forward_ref(pkg, N, xo.NL_K[exchange], (N + exchange) % 2 == 0)
  worst = max(xo.err(d, x) for d, x in zip(nl["D"]["snaps"], nl["X"]["snaps"]))
  on = xo.nl_adjoint_on(nl, nl["D"]["snaps"])  # (the GPU cases feed the GPU's snapshots)
  figs = dict(snapshots=worst, w0=xo.err(on["D"]["w0"], on["X"]["w0"]),
              eta=xo.err(on["D"]["eta"], on["X"]["eta"]))
  print("  " + ", ".join(f"{k} {v:.2e}" for k, v in figs.items()))
  for k, v in figs.items():
    assert v <= xo.CAP, (k, v)
