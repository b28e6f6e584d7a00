"""The ResNet-as-ODE loop of python/Main_width_ref.py for ensembles of initial conditions with
scalar state, one ensemble member per lane on the device (csrc/dg_resnet.hip).

Layer l is ``ResBlockSimple`` (python/models.py:60-64) with F_l neurons,
Phi_l(u, dt) = u + dt * sum_f W2_l[f] relu(W1_l[f] (u - b_l[f])).  The reference's three
``vmap`` calls of the adapt step (:466-478: ``forwardSolve``, ``adjointSolve``,
``errorIndicator``) are one kernel launch (``sweep``); the mean over members (:479) is the
fixed-order member sum (dg_sum_rows) and one division; ``idx = argmax + 1`` and ``adaptDepth``
(:185-211, :491-494) run on the host.  ``trainStep``'s ``vmap(value_and_grad(lossFn))`` and
its means (:164-169) are ``loss_and_grad``; the optimiser is Adam on the device tensors.

The parameters live in one packed device tensor ``theta`` [3, P] (rows bias, w1, w2; layer l
at columns offsets[l]:offsets[l+1]) that the kernels read in place.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from .fd_ensemble import interp_codes


def refine_time(dt, ref_factor):
  """Main_width_ref.py:108-114: every dt split into ref_factor equal parts, and the cumulative
  fine times starting at 0."""
  dt = np.asarray(dt, dtype=np.float64)
  dt_fine = np.repeat(dt / ref_factor, ref_factor)
  return dt_fine, np.concatenate(([0.0], np.cumsum(dt_fine)))


def split_layer(times, params, idx):
  """adaptDepth (Main_width_ref.py:185-211): insert the midpoint of times[idx-1], times[idx] at
  position idx and a copy of layer idx-1's parameters at position idx (1 <= idx <= L)."""
  times = np.asarray(times, dtype=np.float64)
  n_layers = len(times) - 1
  if len(params) != n_layers or not 1 <= idx <= n_layers:
    raise ValueError(f"idx {idx} does not name a layer of a {n_layers}-layer net")
  t_new = np.zeros(len(times) + 1)
  t_new[0:idx] = times[0:idx]
  t_new[idx + 1:] = times[idx:]
  t_new[idx] = np.mean(times[idx - 1:idx + 1])
  params = list(params)
  params.insert(idx, tuple(np.array(x, dtype=np.float64) for x in params[idx - 1]))
  return t_new, params


def _ptr(x):
  return ctypes.c_void_p(x.data_ptr()) if x is not None else None


class ResNetEnsemble:
  """Main_width_ref.py's depth-adaptive ResNet-ODE loop for an ensemble of initial values."""

  def __init__(self, times, params, u0, target, ref_factor=4, device=None):
    if not torch.cuda.is_available():
      raise _lib.DGLibraryError("ResNetEnsemble needs a ROCm GPU (torch.cuda is unavailable)")
    self.dev = torch.device("cuda", torch.cuda.current_device() if device is None else device)
    self.times = np.asarray(times, dtype=np.float64).copy()
    self.rf = int(ref_factor)
    dev_vec = lambda x: torch.as_tensor(np.asarray(x, dtype=np.float64).ravel(),  # noqa: E731
                                        device=self.dev)
    self.u0, self.target = dev_vec(u0), dev_vec(target)
    self.n_ics = int(self.u0.numel())
    if int(self.target.numel()) != self.n_ics:
      raise ValueError("u0 and target differ in length")
    self._lib = _lib.load()
    self.history = []
    self._opt = None
    self._pack(params)

  # ---- parameters -------------------------------------------------------------------------
  def _pack(self, params):
    params = [tuple(np.asarray(x, dtype=np.float64).ravel() for x in p) for p in params]
    if len(params) != len(self.times) - 1:
      raise ValueError("one (bias, weights1, weights2) per interval of times is needed")
    for b, w1, w2 in params:
      if not b.size == w1.size == w2.size:
        raise ValueError("a layer's bias, weights1 and weights2 differ in length")
    self.offsets = np.concatenate(([0], np.cumsum([p[0].size for p in params]))).astype(np.int32)
    host = np.stack([np.concatenate([p[k] for p in params]) if params else np.zeros(0)
                     for k in range(3)])
    self.theta = torch.as_tensor(host, device=self.dev).contiguous()
    self.grad = torch.zeros_like(self.theta)
    self._scratch = None
    self._mesh_cache = None

  @property
  def n_layers(self):
    return len(self.offsets) - 1

  def _views(self, t):
    o = self.offsets
    return [tuple(t[k, o[l]:o[l + 1]] for k in range(3)) for l in range(self.n_layers)]

  def layer_tensors(self):
    """Per layer (bias, weights1, weights2) as views of the packed device tensor."""
    return self._views(self.theta)

  @property
  def params(self):
    """Per layer (bias, weights1, weights2) as host arrays (a copy; synchronises)."""
    host = self.theta.cpu().numpy()
    o = self.offsets
    return [tuple(host[k, o[l]:o[l + 1]].copy() for k in range(3)) for l in range(self.n_layers)]

  def _offs(self):
    return self.offsets.ctypes.data_as(ctypes.c_void_p)

  def _stream(self):
    return ctypes.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)

  def _mesh(self):
    """Device copies of dt, the cumulative coarse / fine times and np.interp's case codes."""
    if self._mesh_cache is None:
      dt_n = np.diff(self.times, 1)
      _, t_fine = refine_time(dt_n, self.rf)
      t_coarse = np.concatenate(([0.0], np.cumsum(dt_n)))  # refineSolution, :118-119
      t = lambda x, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(x), dtype=dt,  # noqa: E731
                                                      device=self.dev)
      self._mesh_cache = (t(dt_n), t(t_coarse), t(t_fine),
                          t(interp_codes(t_coarse, t_fine), torch.int32))
    return self._mesh_cache

  # ---- the adapt step -----------------------------------------------------------------------
  def sweep(self, with_v=False):
    """Forward + fine-grid adjoint + windowed indicator for every member, one launch.
    Returns U [L+1, n_ics], V [L*rf+1, n_ics] (or None), err [n_ics, L]."""
    n = self.n_layers
    dtd, tcd, tfd, codes = self._mesh()
    new = lambda *s: torch.empty(s, dtype=torch.float64, device=self.dev)  # noqa: E731
    U = new(n + 1, self.n_ics)
    V = new(n * self.rf + 1, self.n_ics) if with_v else None
    err = new(self.n_ics, max(n, 0))
    rc = self._lib.dg_resnet_adapt_sweep(
        n, self.rf, self._offs(), _ptr(self.theta[0]), _ptr(self.theta[1]), _ptr(self.theta[2]),
        _ptr(dtd), _ptr(tcd), _ptr(tfd), _ptr(codes), _ptr(self.u0), _ptr(self.target), self.n_ics,
        _ptr(U), _ptr(V), _ptr(err), self._stream())
    _lib.check(rc, "dg_resnet_adapt_sweep")
    return U, V, err

  def indicator(self):
    """The mean over members of the per-layer indicator (:479) and its sum err_total (:480),
    both on the device."""
    from .operators import sum_rows
    _, _, err = self.sweep()
    mean = sum_rows(err, self.n_ics) / float(self.n_ics)
    return mean, mean.sum()

  def adapt_depth(self):
    """One iteration of the depth branch (:466-494): sweep, mean over members, idx = argmax + 1,
    split the interval and copy the layer.  The new layer starts with a fresh optimiser state,
    the others keep theirs (adaptDepth, :207-209)."""
    mean, total = self.indicator()
    mean = mean.cpu().numpy()
    idx = int(np.argmax(mean) + 1)
    states = self._opt_states()
    times, params = split_layer(self.times, self.params, idx)
    self.times = times
    self._pack(params)
    if states is not None:
      states.insert(idx, None)
      self._new_opt(self._lr, states)
    self.history.append(dict(idx=idx, err=mean, err_total=float(total)))
    return idx

  # ---- training -----------------------------------------------------------------------------
  def _launch_loss_grad(self, loss_mean, loss_ic=None):
    if self._scratch is None:
      nbytes = ctypes.c_int64()
      _lib.check(self._lib.dg_resnet_grad_scratch(self.n_layers, self._offs(), self.n_ics,
                                                  ctypes.byref(nbytes)), "dg_resnet_grad_scratch")
      self._scratch = torch.empty((nbytes.value + 7) // 8, dtype=torch.float64, device=self.dev)
    rc = self._lib.dg_resnet_loss_grad(
        self.n_layers, self._offs(), _ptr(self.theta[0]), _ptr(self.theta[1]), _ptr(self.theta[2]),
        _ptr(self._mesh()[0]), _ptr(self.u0), _ptr(self.target), self.n_ics, _ptr(loss_ic),
        _ptr(loss_mean), _ptr(self.grad), _ptr(self._scratch), self._scratch.numel() * 8,
        self._stream())
    _lib.check(rc, "dg_resnet_loss_grad")

  def loss_and_grad(self, per_member=False):
    """The mean over members of lossFn (:142-145) and of its gradient (trainStep, :164-169):
    a 0-d device tensor and per layer (d bias, d weights1, d weights2) device tensors; with
    per_member also the members' losses."""
    loss = torch.empty((), dtype=torch.float64, device=self.dev)
    loss_ic = (torch.empty(self.n_ics, dtype=torch.float64, device=self.dev) if per_member
               else None)
    self._launch_loss_grad(loss, loss_ic)
    grads = self._views(self.grad.clone())
    return (loss, grads, loss_ic) if per_member else (loss, grads)

  def _new_opt(self, lr, states=None):
    """Adam (torch's defaults are optax.adam's: b1 0.9, b2 0.999, eps 1e-8) over per-layer
    views of theta, their .grad views of the gradient the kernel writes."""
    views, gviews = self._views(self.theta), self._views(self.grad)
    ps = []
    for l in range(self.n_layers):
      for k in range(3):
        p = views[l][k].detach()
        p.grad = gviews[l][k]
        ps.append(p)
    self._opt, self._opt_params, self._lr = torch.optim.Adam(ps, lr=lr), ps, lr
    for l, st in enumerate(states or []):
      for k in range(3):
        if st is not None and st[k]:
          self._opt.state[ps[3 * l + k]] = {key: val.clone() for key, val in st[k].items()}

  def _opt_states(self):
    if self._opt is None:
      return None
    ps = self._opt_params
    return [[self._opt.state.get(ps[3 * l + k], {}) for k in range(3)]
            for l in range(self.n_layers)]

  def train(self, epochs, lr=1e-3):
    """`epochs` trainStep iterations (:162-173).  Returns the mean loss before each update as a
    device tensor [epochs]; nothing inside the loop waits for the device."""
    if self._opt is None:
      self._new_opt(lr)
    elif lr != self._lr:
      self._new_opt(lr, self._opt_states())
    losses = torch.empty(epochs, dtype=torch.float64, device=self.dev)
    for e in range(epochs):
      self._launch_loss_grad(losses[e:e + 1])
      self._opt.step()
    return losses
