"""numpy statement of the field transfer across one level of midpoint splits
(include/dg_advec.h, dg_field_to_children / dg_field_from_children): explicit loops over the
elements, the caller's left-child matrix A and its image J A J for the right child."""
import numpy as np


def reversed_matrix(A):
  """J A J with J the node reversal."""
  return np.ascontiguousarray(np.asarray(A)[::-1, ::-1])


def roles(parent):
  """Per new element: 0 unsplit, 1 left child, 2 right child."""
  parent = np.asarray(parent)
  K = len(parent)
  out = np.zeros(K, dtype=np.int64)
  for n in range(K):
    if n > 0 and parent[n - 1] == parent[n]:
      out[n] = 2
    elif n + 1 < K and parent[n + 1] == parent[n]:
      out[n] = 1
  return out


def to_children(u, parent, k_old, A, batch=1):
  """u (batch * k_old * Np, device layout) on the refined mesh: a copy for an unsplit element,
  A u / J A J u for a left / right child."""
  A = np.asarray(A, dtype=np.float64)
  AR = reversed_matrix(A)
  Np, K = A.shape[0], len(parent)
  u = np.asarray(u, dtype=np.float64).reshape(batch, k_old, Np)
  role = roles(parent)
  out = np.empty((batch, K, Np))
  for b in range(batch):
    for n in range(K):
      src = u[b, parent[n]]
      out[b, n] = src if role[n] == 0 else (A @ src if role[n] == 1 else AR @ src)
  return out.ravel()


def from_children(u, parent, k_old, A, batch=1):
  """u (batch * K_new * Np) back on the k_old-element mesh: a copy for an unsplit element,
  A u[n] + J A J u[n + 1] for an element split into n, n + 1."""
  A = np.asarray(A, dtype=np.float64)
  AR = reversed_matrix(A)
  Np, K = A.shape[0], len(parent)
  u = np.asarray(u, dtype=np.float64).reshape(batch, K, Np)
  role = roles(parent)
  out = np.empty((batch, k_old, Np))
  for b in range(batch):
    for n in range(K):
      if role[n] == 0:
        out[b, parent[n]] = u[b, n]
      elif role[n] == 1:
        out[b, parent[n]] = A @ u[b, n] + AR @ u[b, n + 1]
  return out.ravel()


def mass(mesh, v_x, u, batch=1):
  """sum_k h_k/2 1^T M u_k per trajectory (M = (V V^T)^-1)."""
  w = np.linalg.inv(mesh.v @ mesh.v.T).sum(axis=0)
  h = np.diff(np.asarray(v_x, dtype=np.float64))
  u = np.asarray(u).reshape(batch, len(h), mesh.n_p)
  return np.einsum("k,i,bki->b", 0.5 * h, w, u)
