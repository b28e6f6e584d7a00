"""The ResNet-as-ODE ensemble on the GPU (csrc/dg_resnet.hip via
resnet_ensemble.ResNetEnsemble; SURVEY §8(f)3, the ResNet half).  Needs an MI355X.

Every member is compared with the numpy oracle (tests/resnet_oracle.py, float64) at 1e-12
relative to each array's maximum, the FD ensemble's bar.  The oracle's own rounding error on
these inputs, d = its float64 run against its np.longdouble run, is what that bar stands on:
tests/test_resnet_host.py computes it for every input set used here and holds it to 1e-13;
the figures it prints are d = 9.7e-15 on the 4097-member set (up to 5.8e-14 on the meshes of
the five adapt iterations, whose mean indicator is what is compared there), 3.0e-15 on widths
(100, 100), <= 2.5e-15 on the ref_factor 2 / 3 / 16 set, 9.9e-16 on one layer, 1.1e-14 on one
member and 8.9e-15 on the block-edge sets; 3.7e-15 (4097 members) and 2.9e-16 (one member) on
the gradients.  The same host tests check that no
member of any set sits within 1e-9 of a relu kink or of its target (where the oracle and the
kernel could legitimately take different branches)."""
import ctypes

import numpy as np
import pytest
import torch

import resnet_oracle as ro

pytestmark = pytest.mark.gpu

SENTINEL = -777.25
BAR = 1e-12
_sweeps = {}


def oracle_sweep(name, rf):
  if (name, rf) not in _sweeps:
    _sweeps[name, rf] = ro.sweep(*ro.case(name), rf)
  return _sweeps[name, rf]


def ensemble(pkg, name, rf=4):
  return pkg.resnet_ensemble.ResNetEnsemble(*ro.case(name), ref_factor=rf)


def check_sweep(name, rf, U, V, err):
  ref = oracle_sweep(name, rf)
  assert U.shape == ref["U"].shape and err.shape == ref["err"].shape
  assert ro.rel(U, ref["U"]) <= BAR, (name, rf)
  if V is not None:
    assert V.shape == ref["V"].shape
    assert ro.rel(V, ref["V"]) <= BAR, (name, rf)
  assert ro.rel(err, ref["err"]) <= BAR, (name, rf)


@pytest.mark.parametrize("name,rf", [("main", 4), ("wide", 4), ("rf", 2), ("rf", 3), ("rf", 16),
                                     ("one_layer", 4), ("one_member", 4), ("wide129", 4),
                                     ("deep256", 4)])
def test_every_member_matches_the_oracle(pkg, gpu, name, rf):
  assert rf in ro.CASES[name][3]
  U, V, err = (t.cpu().numpy() for t in ensemble(pkg, name, rf).sweep(with_v=True))
  check_sweep(name, rf, U, V, err)


@pytest.mark.parametrize("name,rf", [("main", 4), ("rf", 16), ("one_member", 4)])
def test_sweep_without_v_is_bit_identical(pkg, gpu, name, rf):
  ens = ensemble(pkg, name, rf)
  U, V, err = ens.sweep(with_v=True)
  U0, V0, err0 = ens.sweep(with_v=False)
  assert V0 is None
  assert torch.equal(U0, U) and torch.equal(err0, err)


class Raw:
  """dg_resnet_adapt_sweep / dg_resnet_loss_grad called directly on sentinel-filled outputs
  with `pad` spare doubles behind each output's extent."""

  def __init__(self, pkg, gpu, name, rf=4, pad=1000):
    self.pkg, self.gpu, self.rf, self.pad = pkg, gpu, rf, pad
    self.lib = pkg._lib.load()
    times, params, u0, target = ro.case(name)
    fe = pkg.fd_ensemble
    dt = np.diff(times)
    _, t_fine = pkg.resnet_ensemble.refine_time(dt, rf)
    t_coarse = np.concatenate(([0.0], np.cumsum(dt)))
    dev = lambda x, d=torch.float64: torch.as_tensor(np.ascontiguousarray(x), dtype=d,  # noqa: E731
                                                     device=gpu)
    self.L, self.n = dt.size, u0.size
    self.offsets = np.concatenate(([0], np.cumsum([p[0].size for p in params]))).astype(np.int32)
    self.P = int(self.offsets[-1])
    self.theta = [dev(np.concatenate([p[k] for p in params])) for k in range(3)]
    self.mesh = [dev(dt), dev(t_coarse), dev(t_fine),
                 dev(fe.interp_codes(t_coarse, t_fine), torch.int32)]
    self.u0, self.target = dev(u0), dev(target)
    self.sizes = dict(U=(self.L + 1) * self.n, V=(self.L * rf + 1) * self.n, err=self.n * self.L)
    self.out = {k: self.full(v + pad) for k, v in self.sizes.items()}

  def full(self, k):
    return torch.full((k,), SENTINEL, dtype=torch.float64, device=self.gpu)

  def stream(self):
    return torch.cuda.current_stream(self.gpu).cuda_stream

  def sweep(self, **over):
    """Positional arguments of dg_resnet_adapt_sweep, any of them replaced by name."""
    a = dict(n_layers=self.L, rf=self.rf, offsets=self.offsets.ctypes.data, bias=self.theta[0],
             w1=self.theta[1], w2=self.theta[2], dt=self.mesh[0], tc=self.mesh[1], tf=self.mesh[2],
             code=self.mesh[3], u0=self.u0, target=self.target, n_ics=self.n, U=self.out["U"],
             V=self.out["V"], err=self.out["err"])
    a.update(over)
    args = [x.data_ptr() if isinstance(x, torch.Tensor) else x for x in a.values()]
    rc = self.lib.dg_resnet_adapt_sweep(*args, self.stream())
    torch.cuda.synchronize()
    return rc

  def untouched(self, *names):
    return all(bool((self.out[k] == SENTINEL).all()) for k in (names or self.out))


@pytest.mark.parametrize("name", ["edge255", "edge256", "edge257"])
def test_block_edges_write_nothing_outside_the_outputs(pkg, gpu, name):
  raw = Raw(pkg, gpu, name)
  assert raw.sweep() == pkg._lib.DG_OK
  got = {}
  for k, size in raw.sizes.items():
    assert bool((raw.out[k][size:] == SENTINEL).all()), k
    got[k] = raw.out[k][:size].cpu().numpy()
    assert not np.any(got[k] == SENTINEL), k  # every entry of the extent is written
  check_sweep(name, 4, got["U"].reshape(raw.L + 1, raw.n), got["V"].reshape(-1, raw.n),
              got["err"].reshape(raw.n, raw.L))
  # the gradient entry: outputs and the scratch behind the size it reports
  nbytes = ctypes.c_int64()
  offs = raw.offsets.ctypes.data
  assert raw.lib.dg_resnet_grad_scratch(raw.L, offs, raw.n, ctypes.byref(nbytes)) == pkg._lib.DG_OK
  assert nbytes.value % 8 == 0
  ns = nbytes.value // 8
  scratch, grad, loss_ic, loss = (raw.full(ns + raw.pad), raw.full(3 * raw.P + raw.pad),
                                  raw.full(raw.n + raw.pad), raw.full(1 + raw.pad))
  rc = raw.lib.dg_resnet_loss_grad(raw.L, offs, *(t.data_ptr() for t in raw.theta),
                                   raw.mesh[0].data_ptr(), raw.u0.data_ptr(),
                                   raw.target.data_ptr(), raw.n, loss_ic.data_ptr(),
                                   loss.data_ptr(), grad.data_ptr(), scratch.data_ptr(),
                                   nbytes.value, raw.stream())
  torch.cuda.synchronize()
  assert rc == pkg._lib.DG_OK
  for buf, size in ((scratch, ns), (grad, 3 * raw.P), (loss_ic, raw.n), (loss, 1)):
    assert bool((buf[size:] == SENTINEL).all())
  ref_loss, ref_grads, ref_ic = ro.loss_grad(*ro.case(name))
  g = grad[:3 * raw.P].cpu().numpy().reshape(3, raw.P)
  for l in range(raw.L):
    for k in range(3):
      assert ro.rel(g[k, raw.offsets[l]:raw.offsets[l + 1]], ref_grads[l][k]) <= BAR
  assert ro.rel(loss_ic[:raw.n].cpu().numpy(), ref_ic) <= BAR
  assert abs(float(loss[0]) - ref_loss) <= BAR * ref_loss


def test_depth_adaptation_follows_the_oracle_loop(pkg, gpu):
  """Five adapt_depth() iterations on the 4097-member set: idx and times exactly the oracle
  loop's, the mean indicator to 1e-12; the oracle's two largest mean indicators differ by
  more than 1e-9 relative at every iteration (asserted), so the argmax is no rounding matter."""
  times, params, u0, target = ro.case("main")
  its = ro.adapt_loop(times, params, u0, target, 4, ro.ADAPT_ITERATIONS)
  ens = ensemble(pkg, "main")
  for it in its[:-1]:
    top = np.sort(it["mean"])[::-1]
    assert (top[0] - top[1]) / top[0] > 1e-9
    np.testing.assert_array_equal(ens.times, it["times"])
    mean, total = ens.indicator()
    assert ro.rel(mean.cpu().numpy(), it["mean"]) <= BAR
    assert abs(float(total) - it["mean"].sum()) <= BAR * it["mean"].sum()
    assert ens.adapt_depth() == it["idx"]
    assert ens.history[-1]["idx"] == it["idx"]
    assert ro.rel(ens.history[-1]["err"], it["mean"]) <= BAR
  np.testing.assert_array_equal(ens.times, its[-1]["times"])
  assert ens.n_layers == 3 + ro.ADAPT_ITERATIONS and len(ens.history) == ro.ADAPT_ITERATIONS
  for got, ref in zip(ens.params, its[-1]["params"]):
    for x, y in zip(got, ref):
      np.testing.assert_array_equal(x, y)  # the inserted layers are copies


@pytest.mark.parametrize("name", ["main", "one_member", "wide129", "deep256"])
def test_loss_and_gradient_match_the_oracle_and_repeat_bit_for_bit(pkg, gpu, name):
  ref_loss, ref_grads, ref_ic = ro.loss_grad(*ro.case(name))
  ens = ensemble(pkg, name)
  loss, grads, loss_ic = ens.loss_and_grad(per_member=True)
  assert abs(float(loss) - ref_loss) <= BAR * ref_loss
  assert ro.rel(loss_ic.cpu().numpy(), ref_ic) <= BAR
  assert len(grads) == len(ref_grads)
  for got, ref in zip(grads, ref_grads):
    for g, r in zip(got, ref):
      assert g.shape == r.shape
      assert ro.rel(g.cpu().numpy(), r) <= BAR
  loss2, grads2 = ens.loss_and_grad()
  assert torch.equal(loss2, loss)
  for a, b in zip(grads, grads2):
    for x, y in zip(a, b):
      assert torch.equal(x, y)


def test_training_follows_adam_on_the_oracle_gradient(pkg, gpu):
  """Five train epochs against the oracle's gradient and a numpy Adam: 1e-10 on the
  parameters (tests/test_resnet_host.py checks that no gradient entry of these epochs is
  within rounding of zero, where Adam's +-lr first steps would amplify it)."""
  times, params, u0, target = ro.case("main")
  ref_params, ref_losses, _ = ro.adam_train(times, params, u0, target, ro.TRAIN_EPOCHS, lr=1e-3)
  ens = ensemble(pkg, "main")
  losses = ens.train(ro.TRAIN_EPOCHS, lr=1e-3)
  assert ro.rel(losses.cpu().numpy(), ref_losses) <= BAR
  for got, ref, start in zip(ens.params, ref_params, params):
    for x, y, x0 in zip(got, ref, start):
      assert ro.rel(x, y) <= 1e-10
      assert not np.array_equal(y, x0)  # the oracle's parameters moved: the bar says something


NULLABLE = ("offsets", "bias", "w1", "w2", "dt", "tc", "tf", "code", "u0", "target", "U", "err")
BAD_OFFSETS = {"zero_width": [0, 3, 3], "zero_width_first": [0, 0, 4], "bad_start": [1, 3, 4]}


@pytest.mark.parametrize("what", ["rf=1", "rf=17", "n_layers=0", "n_layers=257", "n_ics=0",
                                  *BAD_OFFSETS, *(f"{k}=NULL" for k in NULLABLE)])
def test_sweep_argument_errors_launch_nothing(pkg, gpu, what):
  raw = Raw(pkg, gpu, "rf", rf=4, pad=0)
  assert pkg._lib.DG_RESNET_MAX_LAYERS == 256
  if what in BAD_OFFSETS:
    keep = np.array(BAD_OFFSETS[what], dtype=np.int32)
    over = dict(offsets=keep.ctypes.data)
  else:
    key, val = what.split("=")
    over = {key: None if val == "NULL" else int(val)}
  assert raw.sweep(**over) == pkg._lib.DG_ERR_ARG
  assert raw.lib.dg_last_error()
  # U=NULL / err=NULL replace the buffer in the call only: all three outputs stay untouched
  assert raw.untouched()


def test_gradient_argument_errors(pkg, gpu):
  raw = Raw(pkg, gpu, "rf", pad=0)
  lib, ERR = raw.lib, pkg._lib.DG_ERR_ARG
  offs = raw.offsets.ctypes.data
  nbytes = ctypes.c_int64()
  assert lib.dg_resnet_grad_scratch(raw.L, offs, raw.n, ctypes.byref(nbytes)) == 0
  assert lib.dg_resnet_grad_scratch(0, offs, raw.n, ctypes.byref(nbytes)) == ERR
  assert lib.dg_resnet_grad_scratch(raw.L, None, raw.n, ctypes.byref(nbytes)) == ERR
  assert lib.dg_resnet_grad_scratch(raw.L, offs, 0, ctypes.byref(nbytes)) == ERR
  assert lib.dg_resnet_grad_scratch(raw.L, offs, raw.n, None) == ERR
  zero_width = np.array([0, 0, 4], dtype=np.int32)
  assert lib.dg_resnet_grad_scratch(2, zero_width.ctypes.data, raw.n, ctypes.byref(nbytes)) == ERR
  assert lib.dg_resnet_grad_scratch(raw.L, offs, raw.n, ctypes.byref(nbytes)) == 0
  scratch, grad, loss = raw.full(nbytes.value // 8), raw.full(3 * raw.P), raw.full(1)
  base = [raw.L, offs, raw.theta[0].data_ptr(), raw.theta[1].data_ptr(), raw.theta[2].data_ptr(),
          raw.mesh[0].data_ptr(), raw.u0.data_ptr(), raw.target.data_ptr(), raw.n, None,
          loss.data_ptr(), grad.data_ptr(), scratch.data_ptr(), nbytes.value]
  bad = [(0, 0), (1, None), (2, None), (3, None), (4, None), (5, None), (6, None), (7, None),
         (8, 0), (10, None), (11, None), (12, None), (13, nbytes.value - 8),
         (1, zero_width.ctypes.data)]
  for pos, val in bad:
    args = list(base)
    args[pos] = val
    assert lib.dg_resnet_loss_grad(*args, raw.stream()) == ERR, pos
  torch.cuda.synchronize()
  for buf in (scratch, grad, loss):
    assert bool((buf == SENTINEL).all())
  # the unmodified call is accepted (loss_ic is optional)
  assert lib.dg_resnet_loss_grad(*base, raw.stream()) == 0
  torch.cuda.synchronize()
  ref_loss = ro.loss_grad(*ro.case("rf"))[0]
  assert abs(float(loss[0]) - ref_loss) <= BAR * ref_loss


def test_class_rejections(pkg, gpu):
  err_t = pkg._lib.DGLibraryError
  times, params, u0, target = ro.case("rf")
  for rf in (1, 17):
    with pytest.raises(err_t):
      pkg.resnet_ensemble.ResNetEnsemble(times, params, u0, target, ref_factor=rf).sweep()
  empty = (np.zeros(0), np.zeros(0), np.zeros(0))
  with pytest.raises(err_t):  # a zero-width layer
    pkg.resnet_ensemble.ResNetEnsemble(times, [params[0], empty], u0, target).sweep()
  with pytest.raises(err_t):
    pkg.resnet_ensemble.ResNetEnsemble(times, [params[0], empty], u0, target).loss_and_grad()
  with pytest.raises(err_t):  # no layer
    pkg.resnet_ensemble.ResNetEnsemble(times[:1], [], u0, target).sweep()
  with pytest.raises(ValueError):  # one layer per interval
    pkg.resnet_ensemble.ResNetEnsemble(times, params[:1], u0, target)
