"""oracle/extended.py: the long-double oracle really computes in long double, and every case of
tests/test_gpu_extended.py meets the reference-alone condition e64 <= CAP.

The proof that no stage rounds to fp64 is a 40-digit mpmath restatement (explicit loops over
elements, nodes and faces; a dense transpose for the adjoint) of the RHS, one LSERK4 step, one
adjoint step and the jump indicator on a tiny case: the long-double oracle meets it to 1e-18 of
max|ref| (its eps is 1.1e-19), the fp64 oracle only to about 1e-16.

The limited paths (tests/test_gpu_extended_limiter.py) get the same proof with the limiter in the
loop (equal decision codes, both forms of SlopeLimitLin), and per GPU case the conditions that make
its exact comparison of decisions decidable: equal codes in fp64 and long double, every decision
margin >= GAP, e64 <= CAP, and over the set a least share of every code class.
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


# --- the limited paths: the mpmath restatement ------------------------------------------------------
def mp_lim_case():
  """N = 2, K = 8, non-uniform on [0, 1] (max|x| / min h = 11), a sine with a jump and nodal
  noise: one limited step meets every code class (asserted), both fluxes and both inflows."""
  pkg = load_pkg()
  rng = np.random.default_rng(0)
  K = 8
  v_x = np.concatenate(([0.0], np.cumsum(rng.uniform(0.6, 1.4, K))))
  v_x = v_x / v_x[-1]
  v_x[-1] = 1.0
  mesh = pkg.BaseGalerkin1D(n=2, v_x=v_x)
  S, SX = xo.lim_setups(mesh, v_x)
  u0 = np.sin(2 * np.pi * S["x"]) + 0.8 * (S["x"] > 0.5) + 0.05 * rng.standard_normal(S["x"].shape)
  g = rng.standard_normal(S["x"].shape)
  return S, SX, u0, g, 2 * np.pi, 0.02, xo.te.bench_dt(2, v_x, 2 * np.pi)


class MPLim(MP):
  """MP with a flux f(u) (u or u^2/2) and the limiter after every stage, both forms of
  SlopeLimitLin in explicit loops, the tangent with frozen codes and its dense transpose."""

  def __init__(self, S, a, dt, inflow, flux, kind):
    super().__init__(S, a, dt, inflow)
    f = self.mp.mpf
    self.flux, self.kind = flux, kind
    self.V = [[f(float(v)) for v in row] for row in S["V"]]
    self.invV = [[f(float(v)) for v in row] for row in S["invV"]]
    self.r = [f(float(v)) for v in S["r"]]
    self.VX = [f(float(v)) for v in S["VX"]]
    self.eps0 = f(1.0e-8)

  def f(self, u):
    return u * u / 2 if self.flux == "burgers" else u

  def rhs_f(self, u, uin):
    fu = [[self.f(v) for v in e] for e in u]
    R = self.lift(fu, self.f(uin))
    return [[-self.a * self.sc[k] * sum(self.Dr[i][j] * fu[k][j] for j in range(self.Np)) + R[k][i]
             for i in range(self.Np)] for k in range(self.K)]

  def minmod(self, a, b, c):
    if not ((a > 0 and b > 0 and c > 0) or (a < 0 and b < 0 and c < 0)):
      return self.zero, 0
    m, br = abs(a), 1
    if abs(b) < m:
      m, br = abs(b), 2
    if abs(c) < m:
      m, br = abs(c), 3
    return (m if a > 0 else -m), br

  def limit(self, v, coord=False):
    K, Np = self.K, self.Np
    uh = [[sum(self.invV[m][j] * v[k][j] for j in range(Np)) for m in range(2)] for k in range(K)]
    avg = [self.V[0][0] * uh[k][0] for k in range(K)]
    out, codes = [], []
    for k in range(K):
      vm, vp = avg[max(k - 1, 0)], avg[min(k + 1, K - 1)]
      b, c = avg[k] - vm, vp - avg[k]
      if self.kind == "N":
        ve1 = avg[k] - self.minmod(avg[k] - v[k][0], b, c)[0]
        ve2 = avg[k] + self.minmod(v[k][Np - 1] - avg[k], b, c)[0]
        if not (abs(ve1 - v[k][0]) > self.eps0 or abs(ve2 - v[k][Np - 1]) > self.eps0):
          out.append(list(v[k]))
          codes.append(0)
          continue
      ul = [self.V[i][0] * uh[k][0] + self.V[i][1] * uh[k][1] for i in range(Np)]
      d = sum(self.Dr[0][j] * ul[j] for j in range(Np))
      if coord:
        xa, xb = self.VX[k], self.VX[k + 1]
        x = [xa + (self.r[i] + 1) / 2 * (xb - xa) for i in range(Np)]
        h = x[Np - 1] - x[0]
        x0 = x[0] + h / 2
        m, br = self.minmod((2 / h) * d, c / h, b / h)
        out.append([avg[k] + (x[i] - x0) * m for i in range(Np)])
      else:
        hm, br = self.minmod(2 * d, c, b)
        out.append([avg[k] + self.r[i] / 2 * hm for i in range(Np)])
      codes.append(4 | br)
    return out, codes

  def limit_tangent(self, dv, codes):
    K, Np = self.K, self.Np
    duh = [[sum(self.invV[m][j] * dv[k][j] for j in range(Np)) for m in range(2)] for k in range(K)]
    davg = [self.V[0][0] * duh[k][0] for k in range(K)]
    out = []
    for k in range(K):
      if not codes[k] & 4:
        out.append(list(dv[k]))
        continue
      dul = [self.V[i][0] * duh[k][0] + self.V[i][1] * duh[k][1] for i in range(Np)]
      br = codes[k] & 3
      dhm = {0: self.zero, 1: 2 * sum(self.Dr[0][j] * dul[j] for j in range(Np)),
             2: davg[min(k + 1, K - 1)] - davg[k], 3: davg[k] - davg[max(k - 1, 0)]}[br]
      out.append([davg[k] + self.r[i] / 2 * dhm for i in range(Np)])
    return out

  def lim_step(self, u, t, coord=False):
    res = [[self.zero] * self.Np for _ in range(self.K)]
    stages = []
    for s in range(5):
      r = self.rhs_f(u, self.uin(ox.stage_time(t, float(self.dt), s)))
      res = [[self.A[s] * res[k][i] + self.dt * r[k][i] for i in range(self.Np)] for k in range(self.K)]
      v = [[u[k][i] + self.B[s] * res[k][i] for i in range(self.Np)] for k in range(self.K)]
      y, codes = self.limit(v, coord)
      stages.append((u, codes))
      u = y
    return u, stages

  def lim_tangent(self, du, stages):
    dres = [[self.zero] * self.Np for _ in range(self.K)]
    keep, self.inflow = self.inflow, "zero"
    for s, (us, codes) in enumerate(stages):
      df = [[us[k][i] * du[k][i] if self.flux == "burgers" else du[k][i] for i in range(self.Np)]
            for k in range(self.K)]
      R = self.lift(df, self.zero)
      r = [[-self.a * self.sc[k] * sum(self.Dr[i][j] * df[k][j] for j in range(self.Np)) + R[k][i]
            for i in range(self.Np)] for k in range(self.K)]
      dres = [[self.A[s] * dres[k][i] + self.dt * r[k][i] for i in range(self.Np)] for k in range(self.K)]
      du = self.limit_tangent([[du[k][i] + self.B[s] * dres[k][i] for i in range(self.Np)]
                               for k in range(self.K)], codes)
    self.inflow = keep
    return du

  def lim_adjoint_step(self, w, stages):
    n = self.K * self.Np
    cols = []
    for j in range(n):
      e = [self.zero] * n
      e[j] = self.mp.mpf(1)
      cols.append(self.flat(self.lim_tangent(self.unflat(e), stages)))
    wf = self.flat(w)
    return self.unflat([sum(cols[j][i] * wf[i] for i in range(n)) for j in range(n)])

  def jump_residual(self, u, uin):
    return self.lift([[self.f(v) for v in e] for e in u], self.f(uin))


@pytest.mark.parametrize("flux,inflow,kind", [("burgers", "a", "N"), ("burgers", "a2", "N"),
                                              ("linear", "a", "N"), ("linear", "a2", "N"),
                                              ("burgers", "a2", "1"), ("linear", "a", "1")])
def test_limited_oracle_meets_the_mpmath_restatement(flux, inflow, kind):
  """One limited step, its adjoint step and the jump indicator: equal codes, long double within
  1e-18 of max|ref|, the fp64 run of the same code at the 1e-16 level; the mesh-free and the
  coordinate form of SlopeLimitLin state the same function (mpmath: to 1e-36; long double: to
  1e-18, at max|x| / min h = 11)."""
  mpmath = pytest.importorskip("mpmath")
  mpmath.mp.dps = 40
  S, SX, u0, g, a, t0, dt = mp_lim_case()
  m = MPLim(S, a, dt, inflow, flux, kind)
  um, gm = m.field(u0), m.field(g)
  u1m, stages = m.lim_step(um, t0)
  codes_m = np.array([c for _, c in stages])
  if kind == "N":
    assert set(np.unique(codes_m)) == {0, 4, 5, 6, 7}, "a code class is missing from the case"
  else:
    assert set(np.unique(codes_m)) == {4, 5, 6, 7}
  figures = {}

  def both(what, x, d, ref):
    figures[what] = (rel(x, ref), rel(d, ref))
    print(f"  {what}: long double {figures[what][0]:.2e}, fp64 {figures[what][1]:.2e}")

  u1x, cx, mx, _ = ox.lim_step(ox.field(u0), t0, dt, a, SX, flux, inflow, kind)
  u1d, cd, md, _ = ox.lim_step(u0, t0, dt, a, S, flux, inflow, kind)
  np.testing.assert_array_equal(cx, codes_m)
  np.testing.assert_array_equal(cd, codes_m)
  assert u1x.dtype == LD and u1d.dtype == np.float64
  assert min(mx, md) >= 1e-9  # the decisions of this case are far from their thresholds
  both("one limited step", u1x, u1d, m.array(u1m))
  # the adjoint step, linearised at u^0
  wm = m.lim_adjoint_step(gm, stages)
  wx, cx2, _ = ox.lim_step_vjp(ox.field(u0), ox.field(g), t0, dt, a, SX, flux, inflow, kind)
  wd, _, _ = ox.lim_step_vjp(u0, g, t0, dt, a, S, flux, inflow, kind)
  np.testing.assert_array_equal(cx2, codes_m)
  both("one adjoint step", wx, wd, m.array(wm))
  # the jump indicator of that step (terminal weight g, each on its own u^1)
  t1 = ox.times_of(t0, dt, 1)
  Rm = m.jump_residual(u1m, m.uin(t1[1]))
  eta_m = np.array([m.dt * sum(gm[k][i] * Rm[k][i] for i in range(m.Np)) for k in range(m.K)],
                   dtype=object)
  ex = ox.lim_jump_indicator([ox.field(u0), u1x], t1, dt, a, SX, ox.field(g), flux, inflow, kind)
  ed = ox.lim_jump_indicator([u0, u1d], t1, dt, a, S, g, flux, inflow, kind)
  both("jump indicator", ex, ed, eta_m)
  for what, (e_x, e_d) in figures.items():
    assert e_x <= 1e-18, (what, e_x)
    assert e_d <= 2e-15, (what, e_d)
  assert max(e for e, _ in figures.values()) < 0.02 * max(e for _, e in figures.values())
  # the two forms: the limiter alone on the stage-0 input, then the whole step
  u1c, stages_c = m.lim_step(um, t0, coord=True)
  assert [c for _, c in stages_c] == [c for _, c in stages]
  assert max(abs(p - q) for p, q in zip(m.flat(u1c), m.flat(u1m))) <= 1e-36
  v = ox.field(u0)
  yx, cfx, _ = ox.slope_limit(v, SX, kind)
  yc, cfc = ox.slope_limit_coord(v, SX, kind)
  ym, cm = m.limit(um)
  np.testing.assert_array_equal(cfx, cfc)
  np.testing.assert_array_equal(cfx, cm)
  print(f"  forms in long double: mesh-free {rel(yx, m.array(ym)):.2e}, "
        f"coordinate {rel(yc, m.array(ym)):.2e}")
  assert rel(yx, m.array(ym)) <= 1e-18 and rel(yc, m.array(ym)) <= 1e-18


def test_limited_adjoint_restatement_equals_the_oracle_in_fp64():
  """oracle.extended's mesh-free tangent and coloured transpose against oracle.burgers.step_vjp
  (coordinate form, forward differentiation of every stage): the same matrix to rounding."""
  from oracle import burgers as ob
  pkg = load_pkg()
  c = ("BN", 0, 2, False, "HOME", 0.3, 0, "adj", False)
  ref = xo.lim_forward_ref(pkg, c)
  S, dt, p = ref["S"], ref["dt"], ref["point"]
  u0 = setup1d.from_elem_major(ref["u0"], 3)[:, :60]
  g = setup1d.from_elem_major(ref["g"], 3)[:, :60]
  mesh = pkg.BaseGalerkin1D(n=2, v_x=ref["v_x"][:61])
  S, _ = xo.lim_setups(mesh, ref["v_x"][:61])
  for flux, limit in (("burgers", "N"), ("linear", "1")):
    w, codes, _ = ox.lim_step_vjp(u0, g, p["t0"], dt, p["a"], S, flux, "a", limit)
    wo = ob.step_vjp(u0, g, p["t0"], dt, p["a"], S, flux, "a", True if limit == "N" else "1")
    assert xo.err(w, wo) <= 1e-13, (flux, limit, xo.err(w, wo))  # (eps |x| / h of the old form)
    _, ids = ob.limited_step(u0, p["t0"], dt, p["a"], S, flux, "a", True if limit == "N" else "1",
                             return_ids=True)
    for s in range(5):
      np.testing.assert_array_equal(np.nonzero(codes[s] & 4)[0], np.sort(ids[s]))


# --- the conditions on every limited GPU case (proved from the oracles alone) -----------------------
@pytest.mark.parametrize("c", xo.LIM_CASES, ids=[xo.lim_id(c) for c in xo.LIM_CASES])
def test_limited_case_conditions(c):
  """(a) the fp64 and the long-double run decide alike at every step and stage, (b) every
  decision margin is >= GAP, (c) e64 <= CAP for every compared quantity (the adjoint and eta with
  both runs fed the fp64 run's snapshots, as the GPU cases feed the GPU's; the self-contained
  pipelines also on their own states).  And the old fp64 oracle (oracle/burgers.py, coordinate
  form) against the truth: a finding about the 1e-10 bar, asserted only to leave it a factor 8."""
  from oracle import burgers as ob
  pkg = load_pkg()
  ref = xo.lim_forward_ref(pkg, c)
  X, D, p, N = ref["X"], ref["D"], ref["point"], c[2]
  np.testing.assert_array_equal(D["codes"], X["codes"])  # (a)
  on = xo.lim_adjoint_on(ref, D["snaps"], c[5])
  np.testing.assert_array_equal(on["D"]["codes"], on["X"]["codes"])
  np.testing.assert_array_equal(on["X"]["codes"], X["codes"])  # the recompute decides as the forward
  margin = min(X["margin"], D["margin"], on["X"]["margin"], on["D"]["margin"])
  figs = dict(snapshots=max(xo.err(d, x) for d, x in zip(D["snaps"], X["snaps"])),
              w0=xo.err(on["D"]["w0"], on["X"]["w0"]), eta=xo.err(on["D"]["eta"], on["X"]["eta"]))
  if c[8]:
    own = xo.lim_adjoint_own(pkg, c)
    figs["w0 (own states)"] = xo.err(own["D"]["w0"], own["X"]["w0"])
    figs["eta (own states)"] = xo.err(own["D"]["eta"], own["X"]["eta"])
    margin = min(margin, own["X"]["margin"], own["D"]["margin"])
  old, _ = ob.forward_sweep(setup1d.from_elem_major(ref["u0"], N + 1), p["t0"], ref["dt"], xo.NL_STEPS,
                            p["a"], ref["S"], ref["flux"], p["inflow"],
                            limit=True if ref["limit"] == "N" else "1")
  e_old = max(xo.err(xo.em(d), x) for d, x in zip(old, X["snaps"]))
  unit = 2.0 ** -52 * float(np.max(np.abs(ref["v_x"])) / np.min(np.diff(ref["v_x"])))
  print(f"  {xo.lim_id(c)}: margin {margin:.2e}, " + ", ".join(f"{k} {v:.2e}" for k, v in figs.items())
        + f"; fp64 coordinate form {e_old:.2e} = {e_old / unit:.2f} x 2^-52 max|x| / min h")
  assert margin >= xo.GAP, margin  # (b)
  for k, v in figs.items():
    assert v <= xo.CAP, (k, v)  # (c)
  assert e_old <= 1e-10 / 8
  if c[7] == "quiet":  # narrow and wide tiles side by side, in every step
    units = xo.quiet_units(ox.pack_codes(X["codes"]), xo.LIM_UNIT[c[1]])
    assert units.any(axis=1).all() and (~units).any(axis=1).all()


def test_limited_code_class_shares():
  """(d) over the case set and per limiter kind, every code class makes up >= 0.5 % of all
  (step, stage, element) decisions."""
  pkg = load_pkg()
  for kind in ("N", "1"):
    total = {}
    for c in xo.LIM_CASES:
      if xo.PHYSICS[c[0]][1] == kind:
        for k, v in xo.class_counts(xo.lim_forward_ref(pkg, c)["X"]["codes"], kind).items():
          total[k] = total.get(k, 0) + v
    n = sum(total.values())
    print(f"  SlopeLimit{kind}: " + ", ".join(f"code {k}: {v / n:.4f}" for k, v in total.items()))
    assert len(total) == (4 if kind == "1" else 5)
    for k, v in total.items():
      assert v >= xo.SHARE * n, (kind, k, v / n)


@pytest.mark.parametrize("i", range(len(xo.KLIMIT)), ids=["-".join(map(str, s)) for s in xo.KLIMIT])
def test_klimit_case_conditions(i):
  """The stand-alone limiters: equal decisions in both precisions, margins >= GAP, and
  oracle/limiter.py (which shares k_limit's coordinate cancellation) within
  1e-14 + 4 * 2^-52 * max|x| / min h of the truth (two roundings of eps |x| in a difference of
  size <= h / 2)."""
  pkg = load_pkg()
  r = xo.klimit_ref(pkg, i)
  np.testing.assert_array_equal(r["D"]["codes"], r["X"]["codes"])
  np.testing.assert_array_equal(np.nonzero(r["X"]["codes"])[0], r["C"]["ids"])
  e_rest, e_old = xo.err(r["D"]["y"], r["X"]["y"]), xo.err(r["C"]["y"], r["X"]["y"])
  print(f"  k_limit {xo.KLIMIT[i]}: margin {r['X']['margin']:.2e}, restatement in fp64 {e_rest:.2e}, "
        f"oracle/limiter.py {e_old:.2e} against the condition {r['cond']:.2e}")
  assert min(r["X"]["margin"], r["D"]["margin"]) >= xo.GAP
  assert e_old <= r["cond"]
  assert e_rest <= xo.CAP
  if xo.KLIMIT[i][3] == "tvb":
    h = np.diff(r["v_x"]).astype(LD)
    a1 = np.abs(ox._slope_arg(ox.field(setup1d.from_elem_major(r["u"], xo.KLIMIT[i][0] + 1)), r["SX"]))
    over = (a1 > r["M"] * h ** 3)[r["X"]["codes"] != 0]
    assert over.any() and (~over).any()
