"""Numpy statement of the ResNet-as-ODE ensemble loop of python/Main_width_ref.py with scalar
state, vectorised over the ensemble members, in any floating dtype (float64 is the oracle of
the GPU tests; np.longdouble measures the oracle's own rounding error).

Layer l, parameters (b, W1, W2) of F_l neurons (models.py:60-64):
  Phi_l(u, dt) = u + dt * sum_f W2[f] relu(W1[f] (u - b[f])).
forwardSolve :48-68; refineTime / refineSolution :108-122 (np.interp); adjointSolve :77-105 as
its backward recursion (forwardFn reads only u[-1]); errorIndicator :126-139; the depth
decision :479-494 with adaptDepth :185-211; lossFn :142-145 and trainStep's means :164-169.
Members run along axis 0 of every per-member array; time / layer nodes along axis 0 of U, V.
"""
import numpy as np


def make_case(seed, widths, n_ics, T=1.0):
  """A random net and ensemble: a non-uniform mesh of len(widths) intervals on [0, T], biases
  and W1 ~ N(0, 1), W2 ~ N(0, 1/F), members uniform in [-1, 1], target u0 + 0.3 cos(3 u0)."""
  rng = np.random.default_rng(seed)
  n_layers = len(widths)
  times = np.sort(np.concatenate(([0.0, T], rng.uniform(0.05 * T, 0.95 * T, n_layers - 1))))
  params = []
  for width in widths:
    bias = rng.normal(0.0, 1.0, width)
    w1 = rng.normal(0.0, 1.0, width)
    w2 = rng.normal(0.0, 1.0 / np.sqrt(width), width)
    params.append((bias, w1, w2))
  u0 = rng.uniform(-1.0, 1.0, n_ics)
  return times, params, u0, u0 + 0.3 * np.cos(3.0 * u0)


def cast(params, dtype):
  return [tuple(np.asarray(x).astype(dtype) for x in p) for p in params]


def pre_activation(u, layer):
  """z[ic, f] = W1[f] (u[ic] - b[f])."""
  bias, w1, _ = layer
  return w1[None, :] * (u[:, None] - bias[None, :])


def phi(u, dt, layer):
  return u + dt * (layer[2][None, :] * np.maximum(pre_activation(u, layer), 0)).sum(axis=1)


def dphi_du(u, dt, layer):
  """d Phi / d u with relu'(0) = 0 (jax's convention)."""
  active = pre_activation(u, layer) > 0
  return 1 + dt * ((layer[2] * layer[1])[None, :] * active).sum(axis=1)


def forward(dt, params, u0):
  """U[l] = the ensemble after l layers (forwardSolve)."""
  U = [u0]
  for dt_l, layer in zip(dt, params):
    U.append(phi(U[-1], dt_l, layer))
  return np.array(U)


def grids(times, ref_factor, dtype=np.float64):
  """dt, the cumulative coarse times, dt_fine and the cumulative fine times (refineTime)."""
  dt = np.diff(np.asarray(times, dtype=np.float64)).astype(dtype)
  t_coarse = np.concatenate((np.zeros(1, dtype), np.cumsum(dt)))
  dt_fine = np.repeat(dt / ref_factor, ref_factor)
  t_fine = np.concatenate((np.zeros(1, dtype), np.cumsum(dt_fine)))
  return dt, t_coarse, dt_fine, t_fine


def interp_members(t_fine, t_coarse, U):
  """np.interp(t_fine, t_coarse, U[:, ic]) for every member, with numpy's own arithmetic
  (compiled_base.c arr_interp: slope * (x - xp[j]) + fp[j], the node itself where x == xp[j],
  fp[-1] at and beyond the last node) in U's dtype; the interval is chosen in float64, where
  the device's interval codes are computed too."""
  xp = t_coarse.astype(np.float64)
  out = np.empty((t_fine.size, U.shape[1]), U.dtype)
  for n, x in enumerate(t_fine):
    j = int(np.clip(np.searchsorted(xp, np.float64(x), side="right") - 1, 0, xp.size - 1))
    if j == xp.size - 1 or xp[j] == np.float64(x):
      out[n] = U[j]
    else:
      slope = (U[j + 1] - U[j]) / (t_coarse[j + 1] - t_coarse[j])
      out[n] = slope * (x - t_coarse[j]) + U[j]
  return out


def sweep(times, params, u0, target, ref_factor, dtype=np.float64):
  """One adapt sweep.  Returns a dict: U [L+1, n], V [L rf + 1, n], err [n, L] and the
  conditioning figures zmin = min |z| over members, fine nodes and neurons and
  smin = min |u_fine[nf] - target|."""
  params = cast(params, dtype)
  u0, target = np.asarray(u0).astype(dtype), np.asarray(target).astype(dtype)
  dt, t_coarse, dt_fine, t_fine = grids(times, ref_factor, dtype)
  n_layers, nf = dt.size, dt.size * ref_factor
  U = forward(dt, params, u0)
  Uf = interp_members(t_fine, t_coarse, U)
  V = np.zeros_like(Uf)
  res = np.zeros_like(Uf)
  V[nf] = np.sign(Uf[nf] - target)
  zmin = np.inf
  for n in range(nf, 0, -1):
    layer = params[(n - 1) // ref_factor]
    zmin = min(zmin, float(np.abs(pre_activation(Uf[n - 1], layer)).min()))
    res[n] = Uf[n] - phi(Uf[n - 1], dt_fine[n - 1], layer)
    V[n - 1] = V[n] * dphi_du(Uf[n - 1], dt_fine[n - 1], layer)
  weighted = res * V
  err = np.abs(np.array([weighted[i * ref_factor + 1:(i + 1) * ref_factor + 1].sum(axis=0)
                         for i in range(n_layers)])).T
  return dict(U=U, V=V, err=err, zmin=zmin, smin=float(np.abs(Uf[nf] - target).min()))


def loss_grad(times, params, u0, target, dtype=np.float64):
  """The mean over members of (u_L - target)^2, its gradient per layer (d b, d W1, d W2) by
  backpropagation, and the members' losses."""
  params = cast(params, dtype)
  u0, target = np.asarray(u0).astype(dtype), np.asarray(target).astype(dtype)
  dt = np.diff(np.asarray(times, dtype=np.float64)).astype(dtype)
  U = forward(dt, params, u0)
  r = U[-1] - target
  lam = 2 * r
  grads = [None] * dt.size
  for l in range(dt.size - 1, -1, -1):
    bias, w1, w2 = params[l]
    z = pre_activation(U[l], params[l])
    active = z > 0
    q = (lam * dt[l])[:, None]
    shifted = U[l][:, None] - bias[None, :]
    grads[l] = ((-q * w2[None, :] * w1[None, :] * active).mean(axis=0),
                (q * w2[None, :] * active * shifted).mean(axis=0),
                (q * np.maximum(z, 0)).mean(axis=0))
    lam = lam * dphi_du(U[l], dt[l], params[l])
  return (r * r).mean(), grads, r * r


def mean_loss(times, params, u0, target):
  dt = np.diff(np.asarray(times, dtype=np.float64))
  return float(np.mean((forward(dt, params, u0)[-1] - target) ** 2))


def split_layer(times, params, idx):
  """adaptDepth: the midpoint of times[idx-1], times[idx] and a copy of layer idx-1 at idx."""
  times = np.asarray(times, dtype=np.float64)
  t_new = np.concatenate((times[:idx], [0.5 * (times[idx - 1] + times[idx])], times[idx:]))
  new = list(params[:idx]) + [tuple(x.copy() for x in params[idx - 1])] + list(params[idx:])
  return t_new, new


def adapt_loop(times, params, u0, target, ref_factor, iterations):
  """The depth branch (:466-494) `iterations` times.  Per iteration a dict: times and params
  before the split, the sweep, mean = the mean indicator over members, idx = argmax + 1."""
  out = []
  for _ in range(iterations):
    s = sweep(times, params, u0, target, ref_factor)
    mean = s["err"].mean(axis=0)
    idx = int(np.argmax(mean) + 1)
    out.append(dict(times=times, params=params, sweep=s, mean=mean, idx=idx))
    times, params = split_layer(times, params, idx)
  out.append(dict(times=times, params=params))
  return out


def adam_train(times, params, u0, target, epochs, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8):
  """optax.adam's update with loss_grad's gradient, `epochs` times.  Returns the parameters
  after the last update, the mean loss before each update and each epoch's gradient."""
  params = cast(params, np.float64)
  m = [[np.zeros_like(x) for x in p] for p in params]
  v = [[np.zeros_like(x) for x in p] for p in params]
  losses, all_grads = [], []
  for step in range(1, epochs + 1):
    loss, grads, _ = loss_grad(times, params, u0, target)
    losses.append(loss)
    all_grads.append(grads)
    new = []
    for l, layer in enumerate(params):
      upd = []
      for k, x in enumerate(layer):
        m[l][k] = b1 * m[l][k] + (1 - b1) * grads[l][k]
        v[l][k] = b2 * v[l][k] + (1 - b2) * grads[l][k] ** 2
        m_hat, v_hat = m[l][k] / (1 - b1 ** step), v[l][k] / (1 - b2 ** step)
        upd.append(x - lr * m_hat / (np.sqrt(v_hat) + eps))
      new.append(tuple(upd))
    params = new
  return params, np.array(losses), all_grads


def rel(x, ref):
  """max |x - ref| relative to max |ref|."""
  x, ref = np.asarray(x), np.asarray(ref)
  return float(np.max(np.abs(x - ref)) / max(float(np.max(np.abs(ref))), 1e-300))


# The input sets of tests/test_gpu_resnet_ensemble.py: name -> (seed, widths, members,
# ref_factors[, T]).  tests/test_resnet_host.py checks the conditioning of every one of them on
# the CPU; the seeds were chosen so that they pass.  "wide129" has layers wider than the 128
# lanes k_resnet_grad_b strides over; "deep256" has DG_RESNET_MAX_LAYERS layers (on [0, 32]: on
# [0, 1] its 256 residuals are differences of nearly equal states and the oracle's own rounding
# in err exceeds 1e-12).
CASES = {
    "main": (0, (5, 7, 4), 4097, (4,)),
    "wide": (3, (100, 100), 1025, (4,)),
    "rf": (0, (3, 1), 300, (2, 3, 16)),
    "one_layer": (0, (6,), 257, (4,)),
    "one_member": (2, (5, 7, 4), 1, (4,)),
    "edge255": (0, (5, 7, 4), 255, (4,)),
    "edge256": (0, (5, 7, 4), 256, (4,)),
    "edge257": (0, (5, 7, 4), 257, (4,)),
    "wide129": (1, (129, 300), 513, (4,)),
    "deep256": (8, (2,) * 256, 300, (4,), 32.0),
}
ADAPT_ITERATIONS = 5
TRAIN_EPOCHS = 5
_cases = {}


def case(name):
  """(times, params, u0, target) of CASES[name], built once."""
  if name not in _cases:
    seed, widths, n_ics, _, *horizon = CASES[name]
    _cases[name] = make_case(seed, widths, n_ics, *horizon)
  return _cases[name]
