"""Helpers of tests/test_oracle_extended.py (CPU), tests/test_gpu_extended.py and
tests/test_gpu_extended_limiter.py: the cases of the extended-precision anchor,
their inputs built on the host, and per case the oracle in long double (oracle/extended.py) next to the fp64 numpy oracle on the same inputs,
cached per case key and read-only.

For a quantity q: qX the long-double result, e64(q) = max|q64 - qX| / max|qX| the fp64 numpy
oracle's distance from it, eg(q) the same ratio for a GPU result.  The bar is

    eg(q) <= MARGIN * max(e64(q), FLOOR)    and    e64(q) <= CAP

with FLOOR = 4 * 2^-52 (below it a ratio of two roundings says nothing), CAP = 1e-14 (a
condition on the case, never a measurement: an ill-conditioned input may not widen its own
tolerance) and MARGIN = 8 (derived in DESIGN.md §3 from the project's 2e-16 per step of Horner
form against the stage loop; not fitted to the kernels).

Every K is 2*TE + 1 of the family (both edge tiles and an interior one), from the formulas
tests/tile_edges.py restates; the GPU tests check them against the plan's queries.
"""
import numpy as np

import tile_edges as te
from oracle import adjoint as oadj
from oracle import advec as oadv
from oracle import burgers as ob
from oracle import extended as ox
from oracle import setup1d

LD = np.longdouble
FLOOR = 4 * 2.0 ** -52
CAP = 1e-14
MARGIN = 8.0

TWO_PI = 2 * np.pi
HOME = dict(a=TWO_PI, x0=0.0, x1=1.0, t0=0.02, inflow="a")  # tests/test_gpu_tile_edges.py
AWAY = dict(a=1.3, x0=-0.7, x1=2.1, t0=3.7, inflow="a2")


def err(q, qx):
  """max|q - qX| / max|qX| in long double."""
  q, qx = np.asarray(q, dtype=LD), np.asarray(qx, dtype=LD)
  return float(np.max(np.abs(q - qx)) / max(np.max(np.abs(qx)), LD(1e-300)))


def bound(e64):
  return MARGIN * max(e64, FLOOR)


class Report:
  """Collects (quantity, eg, e64) of one case, prints each figure, asserts at the end so that a
  failing run still shows every figure."""

  def __init__(self, case_id):
    self.case_id, self.rows = case_id, []

  def add(self, what, got, x, d, margin=MARGIN, cap=CAP):
    """``got`` the GPU's, ``x`` the long-double and ``d`` the fp64 oracle's value; ``cap``: the
    family's reference-alone condition where it is not CAP (k_limit's derived one)."""
    e64, eg = err(d, x), err(got, x)
    self.rows.append((what, eg, e64, margin, cap))
    print(f"  {self.case_id} {what}: eg = {eg:.3e}  e64 = {e64:.3e}  "
          f"eg/max(e64, FLOOR) = {eg / max(e64, FLOOR):.2f}")

  def check(self):
    for what, eg, e64, margin, cap in self.rows:
      assert e64 <= cap, (self.case_id, what, "the reference alone exceeds its condition", e64)
    for what, eg, e64, margin, cap in self.rows:
      assert eg <= margin * max(e64, FLOOR), (self.case_id, what, eg, e64)

  def worst(self):
    """(eg / max(e64, FLOOR), what, eg, e64) of the row nearest its bound."""
    return max((eg / max(e64, FLOOR), what, eg, e64) for what, eg, e64, _, _ in self.rows)


# --- the tile extents, by formula (checked against the plan in the GPU tests) ------------------
def te_stage(N, W, MS, stages=5):
  """csrc/dg_advec.hip launch_step_e / launch_adj_e: TE = 256*W - 2*MS*stages (euler: 1 stage)."""
  MS = min(MS, 2) if N == 8 else MS  # tests/test_gpu_tile_edges.py StageLoop.tune
  return 256 * W - 2 * MS * stages


def te_wave(E, MS):
  return 64 * E - 10 * MS


def te_snap_pairs(tw, ms):
  return 512 * tw - 2 * te.halo_f(ms)


def te_record(lanes, rtw, spl):
  if lanes == 2:
    return min(512 * rtw - 2 * te.halo_f(spl), 512 * rtw - 2 * te.halo_a(spl))
  ms = 1
  while 2 * ms <= spl:
    ms *= 2
  return min(256 * rtw - 2 * (5 * ms + 1), 256 * rtw - 10 * ms)


def te_flow(waves, msf, msa, E, X):
  T = 116 * waves + 12 if X else (256 if E == 4 else 128) * waves
  return min(T - 2 * te.halo_f(msf), T - 2 * te.halo_a(msa))


def te_p(tw, spl):
  return 256 * tw - 10 * spl


# --- inputs ------------------------------------------------------------------------------------
def make_mesh(pkg, N, K, uniform, point):
  v_x = te.make_vx(K, uniform, 1000 * N + K, point["x0"], point["x1"])  # as make_op
  return pkg.BaseGalerkin1D(n=N, v_x=v_x), v_x


def noise(N, ktot, seed):
  """N(0,1) nodal noise, element-major: with the central flux the roughness persists and eta is
  O(10 .. 100), well conditioned."""
  return np.random.default_rng(seed).standard_normal(ktot * (N + 1))


def setups(mesh, v_x, batch):
  """(S64, SX) of ``batch`` trajectories side by side with the mesh object's own Dr and LIFT
  (the ones the plan is created with)."""
  S = ox.with_operators(te.batched_setup(mesh.n, v_x, batch), mesh.d_r, mesh.lift)
  return S, ox.widen(S)


def em(u):
  return setup1d.to_elem_major(u)


def freeze(d):
  for v in d.values():
    if isinstance(v, dict):
      freeze(v)
    for x in (v if isinstance(v, list) else [v]):
      if isinstance(x, np.ndarray):
        x.setflags(write=False)
  return d


_CACHE = {}


def hashable(key):
  return tuple(tuple(sorted(v.items())) if isinstance(v, dict) else v for v in key)


def cached(key, make):
  if key not in _CACHE:
    _CACHE[key] = make()
  return _CACHE[key]


def linear_inputs(pkg, N, K, uniform, batch, point):
  mesh, v_x = make_mesh(pkg, N, K, uniform, point)
  dt = te.bench_dt(N, v_x, point["a"])
  u0 = noise(N, K * batch, 7 * N + 13 * K + batch)
  return mesh, v_x, dt, u0


def forward_ref(pkg, N, K, uniform, batch, point, nsteps, scheme="lserk4"):
  """Both oracles' forward states (element-major lists), records and setups for one input set.
  ``X`` long double, ``D`` fp64."""
  key = ("fwd", hashable((N, K, uniform, batch, point, nsteps)), scheme)

  def make():
    mesh, v_x, dt, u0 = linear_inputs(pkg, N, K, uniform, batch, point)
    S, SX = setups(mesh, v_x, batch)
    a, inflow, t0 = point["a"], point["inflow"], point["t0"]
    u0m = setup1d.from_elem_major(u0, N + 1)
    out = dict(mesh=mesh, v_x=v_x, dt=dt, u0=u0, S=S, SX=SX)
    sx, times = ox.forward_sweep(u0m, t0, dt, nsteps, a, SX, inflow, scheme)
    sd, times_d = oadv.forward_sweep(u0m, t0, dt, nsteps, a, S, inflow, scheme)
    assert times == times_d == te.times_of(t0, dt, nsteps)
    out["times"], out["_sx"], out["_sd"] = times, sx, sd
    out["X"] = dict(snaps=[em(s) for s in sx],
                    rec=np.stack([ox.raw_jumps(sx[n], K, batch, ox.inflow_value(a, times[n], inflow))
                                  for n in range(1, nsteps + 1)]))
    out["D"] = dict(snaps=[em(s) for s in sd],
                    rec=np.stack([te.raw_jumps(sd[n], K, batch, oadv.inflow_value(a, times[n], inflow))
                                  for n in range(1, nsteps + 1)]))
    freeze(out["X"])
    freeze(out["D"])
    return out

  return cached(key, make)


def adjoint_ref(pkg, fwd_key, point, src=0.0, scheme="lserk4"):
  """w^0 and eta of each oracle on its OWN forward states, terminal weight u^N."""
  fwd = forward_ref(pkg, *fwd_key, scheme=scheme)
  key = ("adj", hashable(fwd_key), src, scheme)

  def make():
    a, inflow, dt = point["a"], point["inflow"], fwd["dt"]
    sx, sd, t = fwd["_sx"], fwd["_sd"], fwd["times"]
    wx, ex = ox.adjoint_sweep(sx[-1], sx, t, dt, a, fwd["SX"], inflow, src, scheme)
    wd, ed, _ = oadj.adjoint_sweep(sd[-1], sd, t, dt, a, fwd["S"], inflow, src_coef=src, scheme=scheme)
    return freeze(dict(X=dict(w0=em(wx), eta=ex), D=dict(w0=em(wd), eta=ed)))

  return cached(key, make)


def adjoint_on(fwd, snaps_em, point, src=0.0, scheme="lserk4"):
  """Both oracles' w^0 and eta fed the SAME fp64 snapshots (the GPU's): the project's usual
  convention where snapshots exist.  Not cached (the snapshots are the caller's)."""
  N = fwd["mesh"].n
  sn = [setup1d.from_elem_major(s, N + 1) for s in snaps_em]
  snx = [ox.field(s) for s in sn]
  a, inflow, dt, t = point["a"], point["inflow"], fwd["dt"], fwd["times"]
  wx, ex = ox.adjoint_sweep(snx[-1], snx, t, dt, a, fwd["SX"], inflow, src, scheme)
  wd, ed, _ = oadj.adjoint_sweep(sn[-1], sn, t, dt, a, fwd["S"], inflow, src_coef=src, scheme=scheme)
  return dict(X=dict(w0=em(wx), eta=ex), D=dict(w0=em(wd), eta=ed))


def p_setups(pkg, fwd):
  """The order-(N+1) setups and the prolongation the DWREstimate builds (galerkin.prolongation
  of two meshes on the plan's v_x)."""
  def make():
    mesh = fwd["mesh"]
    hi = pkg.BaseGalerkin1D(n=mesh.n + 1, v_x=fwd["v_x"])
    P = pkg.galerkin.prolongation(pkg.BaseGalerkin1D(n=mesh.n, v_x=fwd["v_x"]), hi)
    Sh, ShX = setups(hi, fwd["v_x"], 1)
    return Sh, ShX, np.array(P, dtype=np.float64)
  return cached(("psetup", id(fwd)), make)


def p_from(pkg, fwd, point, sx, sd):
  """Both oracles' p-estimate (eta, w^0 of order N+1, P u^N) from the given low-order states
  (``sx`` long double, ``sd`` fp64), terminal weight P u^N."""
  from oracle import effectivity as oef
  Sh, ShX, P = p_setups(pkg, fwd)
  a, inflow, dt, t = point["a"], point["inflow"], fwd["dt"], fwd["times"]
  PX = P.astype(LD)
  ex, wx = ox.p_estimate(sx, t, dt, a, ShX, PX, PX @ sx[-1], inflow)
  # (oracle.effectivity.p_estimate with the estimate's own P: prolong_matrix is setup1d's)
  ps = [P @ u for u in sd]
  ws = oef.adjoint_weights(ps, P @ sd[-1], dt, a, Sh)
  ed = np.zeros(Sh["K"])
  for n in range(len(sd) - 1):
    ed -= np.sum(ws[n + 1] * (ps[n + 1] - oadv.step(ps[n], t[n], dt, a, Sh, inflow)), axis=0)
  return dict(X=dict(eta=ex, w0=em(wx), prolong=em(PX @ sx[-1])),
              D=dict(eta=ed, w0=em(ws[0]), prolong=em(P @ sd[-1])))


def p_ref(pkg, fwd_key, point):
  fwd = forward_ref(pkg, *fwd_key)
  return cached(("p", hashable(fwd_key)), lambda: freeze(p_from(pkg, fwd, point, fwd["_sx"], fwd["_sd"])))


def p_on(pkg, fwd, snaps_em, point):
  N = fwd["mesh"].n
  sd = [setup1d.from_elem_major(s, N + 1) for s in snaps_em]
  return p_from(pkg, fwd, point, [ox.field(s) for s in sd], sd)


# --- the cases ---------------------------------------------------------------------------------
def _k(te_):
  return 2 * te_ + 1


# family 3: (N, W, MS, scheme, src, w in place)
STAGE = [(N, W, MS, scheme, src, alias)
         for N, (W, MS) in ((1, (1, 1)), (4, (1, 4)), (8, (2, 8)))
         for scheme, src, alias in (("lserk4", 0.0, False), ("lserk4", 0.3, True),
                                    ("euler", 0.3, False), ("euler", 0.0, True))]
WAVE = [(2, 2, 2), (2, 4, 4)]                       # family 4: (N, E, MS)
SNAP = [(4, 1, 4)]                                  # family 5: (N, tw, ms)
# family 6: (N, lanes, rtw, spl, batch, nsteps)
RECORD = [(1, 2, 1, 10, 1, 20), (4, 2, 2, 20, 1, 40), (8, 2, 2, 10, 1, 20), (4, 1, 1, 5, 1, 20),
          (4, 2, 2, 20, 3, 40)]
# family 7: (N, waves, msf, msa, lane elements, exchange, nsteps)
FLOW = [(4, 12, 20, 10, 2, 0, 40), (8, 12, 20, 10, 2, 0, 40), (1, 4, 20, 10, 4, 0, 40),
        (4, 8, 20, 10, 2, 1, 40)]
P_CASES = [(1, 1, 4), (3, 1, 4), (7, 1, 4)]         # family 8: (N, tw, spl), 20 steps
AWAY_RECORD = (4, 2, 1, 10, 1, 20)                  # family 11


def mesh_kind(i):
  """Alternate a uniform and a make_vx non-uniform mesh along a family's list."""
  return i % 2 == 0


def stage_key(i):
  N, W, MS, scheme = STAGE[i][:4]
  return (N, _k(te_stage(N, W, MS, 5 if scheme == "lserk4" else 1)), mesh_kind(i // 4 + (i % 4) // 2), 1, HOME, 20)


def wave_key(i):
  N, E, MS = WAVE[i]
  return (N, _k(te_wave(E, MS)), mesh_kind(i), 1, HOME, 20)


def snap_key(i):
  N, tw, ms = SNAP[i]
  return (N, _k(te_snap_pairs(tw, ms)), mesh_kind(i + 1), 1, HOME, 20)


def record_key(shape, i, point=HOME):
  N, lanes, rtw, spl, batch, nsteps = shape
  TE = te_record(lanes, rtw, spl)
  K = TE - 1 if batch > 1 else _k(TE)  # batch 3 at TE - 1: trajectory edges inside tiles
  return (N, K, mesh_kind(i), batch, point, nsteps)


def flow_key(i):
  N, waves, msf, msa, E, X, nsteps = FLOW[i]
  return (N, _k(te_flow(waves, msf, msa, E, X)), mesh_kind(i + 1), 1, HOME, nsteps)


def p_key(i):
  N, tw, spl = P_CASES[i]
  return (N, _k(te_p(tw, spl)), mesh_kind(i), 1, HOME, 20)


def linear_case_keys():
  """(id, forward key, scheme, src or None (no adjoint), p-estimate?) of every linear sweep
  case, for the CPU check of the reference-alone condition."""
  out = []
  for i, s in enumerate(STAGE):
    out.append((f"stage-{'-'.join(map(str, s))}", stage_key(i), s[3], s[4], False))
  for i, s in enumerate(WAVE):
    out.append((f"wave-{'-'.join(map(str, s))}", wave_key(i), "lserk4", None, False))
  for i, s in enumerate(SNAP):
    out.append((f"snap-{'-'.join(map(str, s))}", snap_key(i), "lserk4", None, False))
  for i, s in enumerate(RECORD):
    out.append((f"record-{'-'.join(map(str, s))}", record_key(s, i), "lserk4", 0.0, False))
  for i, s in enumerate(FLOW):
    out.append((f"flow-{'-'.join(map(str, s))}", flow_key(i), "lserk4", 0.0, False))
  for i, s in enumerate(P_CASES):
    out.append((f"p-{'-'.join(map(str, s))}", p_key(i), "lserk4", None, True))
  out.append(("away-record", record_key(AWAY_RECORD, 1, AWAY), "lserk4", 0.0, False))
  return out


# --- rhs (families 1, 2) ------------------------------------------------------------------------
RHS_MESHES = [(37, True), (60, False)]


def rhs_ref(pkg, N, K, uniform, inflow, flux, point=HOME):
  def make():
    mesh, v_x = make_mesh(pkg, N, K, uniform, point)
    S, SX = setups(mesh, v_x, 1)
    u = noise(N, K, 31 * N + K)
    um = setup1d.from_elem_major(u, N + 1)
    t, a = point["t0"] + 0.35, point["a"]
    if flux == "burgers":
      x = ox.nl_rhs(ox.field(um), t, a, SX, flux, inflow)
      d, _ = ob.rhs(um, t, a, S, flux, inflow)
    else:
      x, _ = ox.advec_rhs1d(ox.field(um), t, a, SX, inflow)
      d, _ = oadv.advec_rhs1d(um, t, a, S, inflow)
    return freeze(dict(mesh=mesh, u=u, t=t, X=em(x), D=em(d)))
  return cached(("rhs", N, K, uniform, inflow, flux), make)


# --- Burgers without a limiter (family 9) ------------------------------------------------------
NL_STEPS = 4
# 2*TE + 1 of the smallest extent (the adjoint's) per nl_exchange, limiter off: workgroup tiles
# TE = 256 - 2*10, overlapped waves TE = 4 * (64 - 2*10) (tests/tile_edges.nl_extents)
NL_K = {0: 2 * 236 + 1, 1: 2 * 176 + 1}


def nl_inputs(pkg, N, K, uniform):
  mesh, v_x = make_mesh(pkg, N, K, uniform, HOME)
  S, SX = setups(mesh, v_x, 1)
  rng = np.random.default_rng(5 * N + K)
  u0 = np.sin(TWO_PI * S["x"]) + 0.1 * rng.standard_normal(S["x"].shape)
  return mesh, v_x, S, SX, u0, oadv.bench_dt(S)  # dt as tests/test_gpu_nonlinear.py


def nl_forward_ref(pkg, N, K, uniform):
  def make():
    mesh, v_x, S, SX, u0, dt = nl_inputs(pkg, N, K, uniform)
    a, t0 = HOME["a"], HOME["t0"]
    sx, times = ox.nl_forward_sweep(u0, t0, dt, NL_STEPS, a, SX, "burgers", "a")
    sd, _ = ob.forward_sweep(u0, t0, dt, NL_STEPS, a, S, "burgers", "a", limit=False)
    return dict(mesh=mesh, v_x=v_x, S=S, SX=SX, u0=em(u0), dt=dt, times=times,
                X=freeze(dict(snaps=[em(s) for s in sx])), D=freeze(dict(snaps=[em(s) for s in sd])))
  return cached(("nl", N, K, uniform), make)


def nl_adjoint_on(ref, snaps_em):
  """Both oracles' adjoint and eta on the same fp64 snapshots, terminal weight u^N."""
  N = ref["mesh"].n
  sd = [setup1d.from_elem_major(s, N + 1) for s in snaps_em]
  sx = [ox.field(s) for s in sd]
  a, dt, t = HOME["a"], ref["dt"], ref["times"]
  wx, ex = ox.nl_adjoint_sweep(sx[-1], sx, t, dt, a, ref["SX"], "burgers", "a")
  wd, ed, _ = ob.adjoint_sweep(sd[-1], sd, t, dt, a, ref["S"], "burgers", "a", limit=False)
  return dict(X=dict(w0=em(wx), eta=ex), D=dict(w0=em(wd), eta=ed))


# --- transfer (family 10) ----------------------------------------------------------------------
def transfer_ld(u, parent, k_old, A, to_children, batch=1):
  """tests/transfer_oracle.to_children / from_children in long double (same loops, the widened
  matrix)."""
  import transfer_oracle as tor
  A = np.asarray(A, dtype=np.float64).astype(LD)
  AR = np.ascontiguousarray(A[::-1, ::-1])
  Np, K = A.shape[0], len(parent)
  role = tor.roles(parent)
  u = np.asarray(u, dtype=np.float64).astype(LD).reshape(batch, k_old if to_children else K, Np)
  out = np.zeros((batch, K if to_children else k_old, Np), dtype=LD)
  for b in range(batch):
    for n in range(K):
      if to_children:
        src = u[b, parent[n]]
        out[b, n] = src if role[n] == 0 else (A @ src if role[n] == 1 else AR @ src)
      elif role[n] == 0:
        out[b, parent[n]] = u[b, n]
      elif role[n] == 1:
        out[b, parent[n]] = A @ u[b, n] + AR @ u[b, n + 1]
  return out.ravel()


# --- the limited paths (families 12, 13; DESIGN.md §3 "The limiter paths") ------------------------
GAP = 1e-11  # condition (b): every decision margin of a case, in units of max|u|
SHARE = 0.005  # condition (d): each code class's least share of all decisions, per limiter kind
# 2*TE + 1 of the record-driven adjoint's extent per nl_exchange (tests/tile_edges.nl_extents with
# a limiter): workgroup tiles TE = 256 - 2*10, overlapped waves TE = 4 * (64 - 2*10); and of the
# snapshot forward on workgroup tiles, TE = 512 - 2*10 (one step per launch, two cells per stage)
LIM_K = {0: 2 * 236 + 1, 1: 2 * 176 + 1}
LIM_K_FWD = 2 * 492 + 1
# quiet cases: 3*TE + 1, so that an interior tile's halo ends before the last element (the ends of
# a trajectory are always troubled: the replicated neighbour zeroes the minmod)
LIM_K_QUIET = {0: 3 * 236 + 1, 1: 3 * 176 + 1}
LIM_UNIT = {0: 236, 1: 44}  # the record-driven adjoint's unit: a tile / an overlapped-wave window
PHYSICS = {"BN": ("burgers", "N"), "B1": ("burgers", "1"), "LN": ("linear", "N")}


def _lim_cases():
  """(physics, exchange, N, uniform, point, src, seed, shape, own pipeline).  ``shape``: "adj"
  K of the adjoint's extent, "fwd" of the forward's, "quiet" noise and jump only on the first
  elements.  Meshes alternate so that every (physics, exchange) has both kinds."""
  out = []
  for ip, ph in enumerate(PHYSICS):
    for ex in (0, 1):
      for iN, N in enumerate((1, 2, 4, 7)):
        i = len(out)
        out.append((ph, ex, N, (iN + ex + ip) % 2 == 0, "HOME", 0.3 * (i % 2), 0, "adj",
                    N == 2 and ex == ip % 2))
  out.append(("BN", 0, 2, False, "AWAY", 0.3, 0, "adj", False))
  out.append(("BN", 0, 2, True, "HOME", 0.0, 0, "quiet", False))
  out.append(("LN", 1, 4, False, "HOME", 0.3, 0, "quiet", False))
  out.append(("B1", 0, 1, False, "HOME", 0.0, 0, "fwd", False))
  out.append(("BN", 0, 2, True, "HOME", 0.3, 0, "fwd", False))
  return out


LIM_CASES = _lim_cases()
POINTS = dict(HOME=HOME, AWAY=AWAY)


def lim_id(c):
  ph, ex, N, uni, point, src, seed, shape, own = c
  return f"{ph}-x{ex}-N{N}-{'uni' if uni else 'ref'}-{point}-src{src:g}-s{seed}-{shape}"


def lim_k(c):
  ex, shape = c[1], c[7]
  return {"adj": LIM_K[ex], "fwd": LIM_K_FWD, "quiet": LIM_K_QUIET[ex]}[shape]


def refined_vx(K, seed, x0=0.0, x1=1.0):
  """tests/test_gpu_nonlinear.refined_vx (7 random bisections of a uniform mesh) with K elements
  in all, on [x0, x1]."""
  rng = np.random.default_rng(seed)
  v = setup1d.mesh_gen1d(0.0, 1.0, K - 7)[1]
  for _ in range(7):
    j = int(rng.integers(0, len(v) - 1))
    v = np.insert(v, j + 1, 0.5 * (v[j] + v[j + 1]))
  return v if (x0, x1) == (0.0, 1.0) else x0 + (x1 - x0) * v


def lim_mesh(pkg, c):
  N, uni, p, K = c[2], c[3], POINTS[c[4]], lim_k(c)
  v_x = setup1d.mesh_gen1d(p["x0"], p["x1"], K)[1] if uni else \
      refined_vx(K, 100 * N + K, p["x0"], p["x1"])
  return pkg.BaseGalerkin1D(n=N, v_x=v_x), v_x


def lim_setups(mesh, v_x):
  """(S64, SX) with every operator the plan is created with: Dr, LIFT, V, invV and r."""
  S = ox.with_operators(setup1d.startup1d(mesh.n, v_x, metric="element"), mesh.d_r, mesh.lift,
                        mesh.v, mesh.inv_v, mesh.r_gl)
  return S, ox.widen(S)


def lim_u0(c, S):
  """A smooth sine + a jump + N(0, 0.05^2) nodal noise (tests/test_gpu_nonlinear.ic on the
  case's domain).  "quiet": a monotone sine arc, the jump and the noise on the first 3/4 of a
  unit only, so that whole tiles (windows) with their halos have no troubled cell."""
  ph, ex, N, uni, point, src, seed, shape, own = c
  p = POINTS[point]
  rng = np.random.default_rng(1000 * seed + 10 * N + ex + len(ph) + S["K"])
  xi = (S["x"] - p["x0"]) / (p["x1"] - p["x0"])
  z = rng.standard_normal(xi.shape)
  if shape == "quiet":
    k = np.arange(S["K"])[None, :]
    rough = k < 3 * LIM_UNIT[ex] // 4
    return np.sin(0.3 + xi) + np.where(rough, 0.8 * (k > LIM_UNIT[ex] // 3) + 0.05 * z, 0.0)
  return np.sin(TWO_PI * xi) + 0.8 * (xi > 0.5) + 0.05 * z


def lim_weight(c, S):
  """The adjoint's terminal weight: N(0,1) nodal noise.  The weight u^N is piecewise linear after
  the limiter and excites only two functionals per cell of the transposed limiter (sum_i w_i and
  sum_i r_i w_i); noise excites every node, so every coefficient of a0e / a1o / rco shows."""
  rng = np.random.default_rng(77 + 1000 * c[6] + 10 * c[2] + c[1] + S["K"])
  return rng.standard_normal(S["x"].shape)


def lim_forward_ref(pkg, c):
  """Both runs of oracle/extended.py's limited sweep from the case's u^0 (``X`` long double,
  ``D`` the same code in fp64), with codes and margins."""
  def make():
    ph, ex, N, uni, point, src, seed, shape, own = c
    flux, limit = PHYSICS[ph]
    p = POINTS[point]
    mesh, v_x = lim_mesh(pkg, c)
    S, SX = lim_setups(mesh, v_x)
    dt = te.bench_dt(N, v_x, p["a"])
    u0 = lim_u0(c, S)
    g = lim_weight(c, S)
    sx, times, cx, mx = ox.lim_forward_sweep(ox.field(u0), p["t0"], dt, NL_STEPS, p["a"], SX, flux,
                                             p["inflow"], limit)
    sd, _, cd, md = ox.lim_forward_sweep(u0, p["t0"], dt, NL_STEPS, p["a"], S, flux, p["inflow"],
                                         limit)
    assert sd[-1].dtype == np.float64 and sx[-1].dtype == LD
    return dict(mesh=mesh, v_x=v_x, S=S, SX=SX, u0=em(u0), g=em(g), dt=dt, times=times, flux=flux,
                limit=limit, point=p, _sx=sx, _sd=sd,
                X=freeze(dict(snaps=[em(s) for s in sx], codes=cx, margin=mx)),
                D=freeze(dict(snaps=[em(s) for s in sd], codes=cd, margin=md)))
  return cached(("lim", c), make)


def lim_adjoint_on(ref, snaps_em, src):
  """Both runs' w^0, eta, recomputed codes and margin fed the same fp64 snapshots, terminal
  weight ``ref["g"]``."""
  N = ref["mesh"].n
  sd = [setup1d.from_elem_major(s, N + 1) for s in snaps_em]
  sx = [ox.field(s) for s in sd]
  p, dt, t = ref["point"], ref["dt"], ref["times"]
  args = (ref["flux"], p["inflow"], ref["limit"], src)
  g = setup1d.from_elem_major(ref["g"], N + 1)
  wx, ex, cx, mx = ox.lim_adjoint_sweep(ox.field(g), sx, t, dt, p["a"], ref["SX"], *args)
  wd, ed, cd, md = ox.lim_adjoint_sweep(g, sd, t, dt, p["a"], ref["S"], *args)
  return dict(X=dict(w0=em(wx), eta=ex, codes=cx, margin=mx),
              D=dict(w0=em(wd), eta=ed, codes=cd, margin=md))


def lim_adjoint_own(pkg, c):
  """Each run's adjoint on its OWN forward states (the CPU module's e64 of w^0 and eta, and the
  reference of the self-contained pipelines)."""
  ref = lim_forward_ref(pkg, c)

  def make():
    p, dt, t = ref["point"], ref["dt"], ref["times"]
    args = (ref["flux"], p["inflow"], ref["limit"], c[5])
    sx, sd = ref["_sx"], ref["_sd"]
    g = setup1d.from_elem_major(ref["g"], ref["mesh"].n + 1)
    wx, ex, cx, mx = ox.lim_adjoint_sweep(ox.field(g), sx, t, dt, p["a"], ref["SX"], *args)
    wd, ed, cd, md = ox.lim_adjoint_sweep(g, sd, t, dt, p["a"], ref["S"], *args)
    return freeze(dict(X=dict(w0=em(wx), eta=ex, codes=cx, margin=mx),
                       D=dict(w0=em(wd), eta=ed, codes=cd, margin=md)))
  return cached(("lim-adj", c), make)


def class_counts(codes, limit):
  """Decisions per code class (0, 4, 5, 6, 7) of a (..., K) code array."""
  return {k: int(np.count_nonzero(codes == k)) for k in ((4, 5, 6, 7) if limit == "1" else (0, 4, 5, 6, 7))}


def quiet_units(words, unit, halo=10):
  """Per step of a (nsteps, K) record, which adjoint units (tiles, windows) have a troubled cell
  within their halo (tests/test_gpu_decisions.test_troubled_tiles_on_the_wide_cone)."""
  nsteps, K = words.shape
  n = -(-K // unit)
  out = np.zeros((nsteps, n), dtype=bool)
  for t in range(n):
    out[:, t] = words[:, max(t * unit - halo, 0):t * unit + unit + halo].any(axis=1)
  return out


# k_limit (family 13): (N, uniform, kind, M)
KLIMIT_K = 2 * 254 + 1
KLIMIT = [(1, True, "N", None), (4, False, "N", None), (7, True, "N", None),
          (1, False, "1", None), (4, True, "1", None), (7, False, "1", None),
          (4, False, "N", "tvb")]


def klimit_ref(pkg, i):
  """The stand-alone limiters: long-double truth (mesh-free form, coordinates from the widened VX
  and r), the restatement in fp64 (codes, margin), and oracle/limiter.py's coordinate form in
  fp64, which shares k_limit's cancellation and is the ``e64`` of this family."""
  from oracle import limiter as olim

  def make():
    N, uni, kind, M = KLIMIT[i]
    c = ("BN", 0, N, uni, "HOME", 0.0, 3, "adj", False)
    v_x = setup1d.mesh_gen1d(0.0, 1.0, KLIMIT_K)[1] if uni else refined_vx(KLIMIT_K, 7 + N)
    mesh = pkg.BaseGalerkin1D(n=N, v_x=v_x)
    S, SX = lim_setups(mesh, v_x)
    u = lim_u0(c, S)
    h = np.diff(v_x)
    if M == "tvb":  # between the two middle values of |ux| / h^2 over the troubled cells: both
      # sides of |ux| > M h^2 occur, and no cell sits on the threshold
      q = np.sort((np.abs(ox._slope_arg(u, S)) / h ** 3)[ox.slope_limit(u, S, kind)[1] != 0])
      M = float(np.sqrt(q[len(q) // 2 - 1] * q[len(q) // 2]))
    yx, cx, mx = ox.slope_limit(ox.field(u), SX, kind, M)
    yd, cd, md = ox.slope_limit(u, S, kind, M)
    if kind == "1":
      y64, ids = olim.slope_limit_1(u, S, M), np.arange(S["K"])
    else:
      y64, ids = olim.slope_limit_n(u, S, return_ids=True, M=M)
    cond = 1e-14 + 4 * 2.0 ** -52 * float(np.max(np.abs(v_x)) / np.min(h))
    return freeze(dict(mesh=mesh, v_x=v_x, S=S, SX=SX, u=em(u), M=M, kind=kind, cond=cond,
                       X=dict(y=em(yx), codes=cx, margin=mx), D=dict(y=em(yd), codes=cd, margin=md),
                       C=dict(y=em(y64), ids=np.sort(ids))))
  return cached(("klimit", i), make)
