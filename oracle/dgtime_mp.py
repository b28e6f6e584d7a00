"""DG-in-time forward and adjoint marches for du/dt = sin(u) in extended precision
(mpmath, >= 40 digits): the arbiter between oracle/dgtime.py (polyfit/polyval, as
matlab/dg_march.m and adj_march.m are written) and the nodal-basis form the kernels of
csrc/dg_time.hip use.

TEST INFRASTRUCTURE ONLY (see oracle/__init__.py).  Needs mpmath; nothing on the GPU path
imports it (the GPU tests read tests/golden/dgtime_mp_golden.json, written from here by
tests/golden/make_dgtime_golden.py).

Everything is built in extended precision: the LGL nodes and Gauss points (the fp64
values of oracle/setup1d.py polished by Newton on the Legendre polynomials), V, Dr,
S = (V V')\\Dr, Phi, Pext, Ifa and the LU solves.  The slab polynomial is evaluated in
the nodal form; in exact arithmetic polyfit through Np points and nodal interpolation are
the same polynomial, so this is the reference's statement with the rounding taken out.

Semantics kept as oracle/dgtime.py documents them:
* adj_march.m:73's hk = x(1) - x(end) < 0, its evaluation points before the slab (forward
  reference coordinate -2 - r) and the negative hk in the mass terms;
* the Newton loop `while it <= maxit && err > tol` (dg_march.m:53);
* F = M_k * 1 (adj_march.m:96);
* partial pivoting with the first maximal row on ties (MATLAB mldivide / LAPACK dgesv).
The slab width is the fp64 number (ta + (tb - ta)) - ta, which is what fem_setup's
x(end) - x(1) is and what the kernels compute; it enters the mp arithmetic exactly.

What it settled (tests/golden/make_dgtime_golden.py, floors (a)/(b) of the fixture): at
N >= 6 neither the polyfit form of oracle/dgtime.py nor the nodal form carries the
adjoint's error.  Both sit at the same distance from this reference at every order (err at
N = 7: 2e-10 relative for y0 = 1, 2e-9 for y0 = 40) and within 1e-11 of each other; on
the same Y both are within 2e-12 of it.  The common error is the 5e-15 an fp64 forward
march has in Y (from the fp64 stiffness S = (V V')\\Dr), amplified by adj_march.m:79's
evaluation of u_h before the slab (max|Pext| = 2e4 at N = 7).  DESIGN.md 6b has the table.
"""
import mpmath

from . import setup1d

DPS = 50


def _legendre(n, x):
  """P_n(x), P_n'(x), P_n''(x) (Legendre) by the three-term recurrence and the ODE."""
  one = mpmath.mpf(1)
  if n == 0:
    return one, 0 * one, 0 * one
  p0, p1 = one, x
  for k in range(1, n):
    p0, p1 = p1, ((2 * k + 1) * x * p1 - k * p0) / (k + 1)
  if abs(x) == 1:  # P_n'(+-1) = (+-1)^(n-1) n(n+1)/2; P'' is not needed at the end points
    return p1, (1 if (x > 0 or n % 2 == 1) else -1) * mpmath.mpf(n * (n + 1)) / 2, None
  d1 = n * (x * p1 - p0) / (x * x - 1)
  d2 = (2 * x * d1 - n * (n + 1) * p1) / (1 - x * x)
  return p1, d1, d2


def _polish(seed, fun):
  """Newton from an fp64 seed; fun(x) -> (f, f')."""
  x = mpmath.mpf(float(seed))
  for _ in range(12):
    f, df = fun(x)
    dx = f / df
    x -= dx
    if abs(dx) < mpmath.mpf(10) ** (-(mpmath.mp.dps - 5)):
      break
  return x


def lgl_nodes(n):
  """Legendre-Gauss-Lobatto nodes of order n: -1, the roots of P_n', +1."""
  seeds = setup1d.jacobi_gl(0, 0, n)
  inner = [_polish(s, lambda x: _legendre(n, x)[1:3]) for s in seeds[1:-1]]
  return [mpmath.mpf(-1)] + inner + [mpmath.mpf(1)]


def gauss_rule(n_gq):
  """The n_gq+1 point Gauss-Legendre rule (JacobiGQ(0, 0, n_gq)): points and weights."""
  m = n_gq + 1
  seeds, _ = setup1d.jacobi_gq(0, 0, n_gq)
  r = [_polish(s, lambda x: _legendre(m, x)[0:2]) for s in seeds]
  w = [2 / ((1 - x * x) * _legendre(m, x)[1] ** 2) for x in r]
  return r, w


def _vander(n, pts):
  """Orthonormal Legendre Vandermonde: V[i][j] = sqrt((2j+1)/2) P_j(pts[i])."""
  return mpmath.matrix([[mpmath.sqrt(mpmath.mpf(2 * j + 1) / 2) * _legendre(j, x)[0]
                         for j in range(n + 1)] for x in pts])


def _grad_vander(n, pts):
  return mpmath.matrix([[mpmath.sqrt(mpmath.mpf(2 * j + 1) / 2) * _legendre(j, x)[1]
                         for j in range(n + 1)] for x in pts])


def basis_at(n, pts):
  """Nodal (LGL, order n) basis at pts: P(pts) inv(V)  (fem_setup.m:30-38)."""
  return _vander(n, pts) * mpmath.inverse(_vander(n, lgl_nodes(n)))


def _rows(M):
  return [[M[i, j] for j in range(M.cols)] for i in range(M.rows)]


_cache = {}


def forward_ops(n):
  """S = (V V')\\Dr, Phi at the 30n+1 Gauss points, w (dg_march.m:38, :57), as nested lists."""
  key = ("f", n, mpmath.mp.dps)
  if key not in _cache:
    r = lgl_nodes(n)
    V = _vander(n, r)
    Minv = mpmath.inverse(V * V.T)
    Dr = _grad_vander(n, r) * mpmath.inverse(V)
    rq, wq = gauss_rule(30 * n)
    _cache[key] = dict(n=n, r=r, S=_rows(Minv * Dr), Phi=_rows(basis_at(n, rq)), wq=wq, rq=rq)
  return _cache[key]


def adjoint_ops(n_fwd):
  """Order n_fwd+1 adjoint operators on the 2(n_fwd+1)+1 point rule (adj_march.m:71-85),
  Pext (forward basis at -2 - r) and Ifa (forward basis at the adjoint nodes)."""
  key = ("a", n_fwd, mpmath.mp.dps)
  if key not in _cache:
    na = n_fwd + 1
    r = lgl_nodes(na)
    V = _vander(na, r)
    Minv = mpmath.inverse(V * V.T)
    Dr = _grad_vander(na, r) * mpmath.inverse(V)
    rq, wq = gauss_rule(2 * na)
    _cache[key] = dict(n=na, r=r, Sa=_rows(Minv * Dr), Ma=_rows(Minv),
                       Phia=_rows(basis_at(na, rq)), wq=wq, rq=rq,
                       Pext=_rows(basis_at(n_fwd, [-2 - x for x in rq])),
                       Ifa=_rows(basis_at(n_fwd, r)))
  return _cache[key]


def lu_solve(A, b):
  """A x = b by Gaussian elimination with partial pivoting, first maximal row on ties."""
  n = len(b)
  A = [row[:] for row in A]
  b = b[:]
  for c in range(n):
    p = c
    for r in range(c + 1, n):
      if abs(A[r][c]) > abs(A[p][c]):
        p = r
    if p != c:
      A[c], A[p] = A[p], A[c]
      b[c], b[p] = b[p], b[c]
    for r in range(c + 1, n):
      f = A[r][c] / A[c][c]
      for j in range(c + 1, n):
        A[r][j] -= f * A[c][j]
      b[r] -= f * b[c]
  for c in range(n - 1, -1, -1):
    s = b[c]
    for j in range(c + 1, n):
      s -= A[c][j] * b[j]
    b[c] = s / A[c][c]
  return b


def slab_width(ta, tb):
  """fem_setup's x(end) - x(1) on [ta, tb], evaluated in fp64 (StartUp1D.m:21)."""
  ta, tb = float(ta), float(tb)
  return (ta + (tb - ta)) - ta


def _quad(Pe, Pa, wq, U):
  """sum_q w_q sin(u_q) Pa[q][:], sum_q w_q cos(u_q) Pa[q][:] Pa[q][:]' with u_q = Pe[q] . U."""
  na = len(Pa[0])
  Mt = [mpmath.mpf(0)] * na
  J = [[mpmath.mpf(0)] * na for _ in range(na)]
  for q in range(len(wq)):
    ur = mpmath.fdot(Pe[q], U)
    ws, wc = wq[q] * mpmath.sin(ur), wq[q] * mpmath.cos(ur)
    pa = Pa[q]
    for i in range(na):
      Mt[i] += pa[i] * ws
      pw = pa[i] * wc
      for j in range(i, na):
        J[i][j] += pw * pa[j]
  for i in range(na):
    for j in range(i):
      J[i][j] = J[j][i]
  return Mt, J


def dg_march(N, times, y0, tol=1e-7, maxit=500):
  """matlab/dg_march.m:36-77 (nonlinear branch) at mp precision.
  Returns (Y, iterations, errors): per slab the nodal values, the Newton iteration count
  and the list of every Newton error ||U_old - U_next||."""
  with mpmath.workdps(DPS):
    ops = forward_ops(N)
    S, Phi, wq = ops["S"], ops["Phi"], ops["wq"]
    Np = N + 1
    tol = mpmath.mpf(float(tol))
    uR = mpmath.mpf(float(y0))
    Y, its, errs = [], [], []
    for k in range(len(times) - 1):
      hh = mpmath.mpf(slab_width(times[k], times[k + 1])) / 2
      U = [uR] * Np
      it, err, elist = 0, mpmath.mpf(1), []
      while it <= maxit and err > tol:
        Mt, J = _quad(Phi, Phi, wq, U)
        R, D = [], []
        for i in range(Np):
          a = hh * Mt[i] + (uR if i == 0 else 0)
          row = []
          for j in range(Np):
            Aij = S[j][i] + (-1 if (i == Np - 1 and j == Np - 1) else 0)
            a += Aij * U[j]
            row.append(Aij + hh * J[i][j])
          R.append(a)
          D.append(row)
        delta = lu_solve(D, R)
        Un = [U[i] - delta[i] for i in range(Np)]
        err = mpmath.sqrt(sum((U[i] - Un[i]) ** 2 for i in range(Np)))
        elist.append(err)
        U = Un
        it += 1
      Y.append(U)
      its.append(it)
      errs.append(elist)
      uR = U[-1]
    return Y, its, errs


def adj_march(Na, times, Y, y0):
  """matlab/adj_march.m:61-119 (nonlinear branch, J = integral of u) at mp precision, on
  the forward march Y of order Na - 1.  Returns (V, err)."""
  with mpmath.workdps(DPS):
    Nf = Na - 1
    ops = adjoint_ops(Nf)
    Sa, Ma, Phia, Pext, Ifa, wq = (ops[k] for k in ("Sa", "Ma", "Phia", "Pext", "Ifa", "wq"))
    NA = Na + 1
    Ks = len(times) - 1
    V, err = [None] * Ks, [None] * Ks
    vL = mpmath.mpf(0)
    for k in range(Ks - 1, -1, -1):
      U = [mpmath.mpf(u) for u in Y[k]]
      hh = -mpmath.mpf(slab_width(times[k], times[k + 1])) / 2  # hk/2, hk < 0 (:73)
      uh = [mpmath.fdot(Ifa[j], U) for j in range(NA)]
      Mt, Mv = _quad(Pext, Phia, wq, U)
      A, F = [], []
      for i in range(NA):
        A.append([-Sa[j][i] + (-1 if (i == 0 and j == 0) else 0) - hh * Mv[i][j]
                  for j in range(NA)])
        F.append(hh * sum(Ma[i]))
      F[-1] -= vL
      v = lu_solve(A, F)
      vL = v[0]
      uprev = mpmath.mpf(float(y0)) if k == 0 else mpmath.mpf(Y[k - 1][-1])
      e = mpmath.mpf(0)
      for i in range(NA):
        res = -hh * Mt[i] + (uprev if i == 0 else 0)
        for j in range(NA):
          a2 = -Sa[j][i] + (1 if (i == NA - 1 and j == NA - 1) else 0)
          res -= a2 * uh[j]
        e += v[i] * res
      V[k] = v
      err[k] = e
    return V, err
