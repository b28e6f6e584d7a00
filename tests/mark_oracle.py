"""numpy statement of the marking contract (include/dg_advec.h, dg_plan_mark and
dg_plan_refine_marked): the rank order, the two strategies and the multi-element split."""
import numpy as np

NAN_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)
INF_KEY = np.uint64(0x7FF0000000000000)


def keys(eta):
  """The 64 bits of |x| as an unsigned integer; all ones for NaN."""
  eta = np.ascontiguousarray(eta, dtype=np.float64)
  k = np.abs(eta).view(np.uint64).copy()
  k[np.isnan(eta)] = NAN_KEY
  return k


def rank_order(eta):
  """Indices by rank: larger key first, equal keys by the lower index."""
  return np.argsort(~keys(eta), kind="stable")


def _marks(n, idx):
  m = np.zeros(n, dtype=np.uint8)
  m[idx] = 1
  return m


def top_count(eta, m, cap=None, order=None):
  """uint8 marks of the first min(m, K, cap) elements in rank order."""
  n = len(eta)
  m = min(int(m), n, n if cap is None or cap < 0 else int(cap))
  order = rank_order(eta) if order is None else order
  return _marks(n, order[:m])


def max_fraction(eta, theta, cap=None, order=None):
  """uint8 marks of {|eta_k| >= theta*M and |eta_k| > 0} (M = the top-ranked |eta|, finite) or
  of the non-finite entries (M not finite); the top `cap` of them in rank order when they
  number more."""
  eta = np.ascontiguousarray(eta, dtype=np.float64)
  n = len(eta)
  order = rank_order(eta) if order is None else order
  a = np.abs(eta)
  M = a[order[0]]
  if np.isfinite(M):
    cand = (a >= np.float64(theta) * M) & (a > 0)
  else:
    cand = ~np.isfinite(eta)
  count = int(np.count_nonzero(cand))
  if cap is not None and 0 <= cap < count:
    return _marks(n, order[:int(cap)])
  return cand.astype(np.uint8)


def info(eta, marks, vx):
  """(count marked, count non-finite, minimum marked width or +inf)."""
  marks = np.asarray(marks) != 0
  w = np.diff(np.asarray(vx, dtype=np.float64))[marks]
  return (int(np.count_nonzero(marks)), int(np.count_nonzero(~np.isfinite(eta))),
          float(w.min()) if w.size else float("inf"))


def split_marked(vx, marks):
  """(new vertices, parent map): every marked interval split at its midpoint."""
  vx = np.asarray(vx, dtype=np.float64)
  marks = np.asarray(marks) != 0
  idx = np.flatnonzero(marks)
  new = np.insert(vx, idx + 1, 0.5 * (vx[idx] + vx[idx + 1]))
  parent = np.repeat(np.arange(len(marks), dtype=np.int32), 1 + marks.astype(np.int64))
  return new, parent
