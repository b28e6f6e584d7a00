"""Time of the ResNet-ODE ensemble's adapt sweep (resnet_ensemble.ResNetEnsemble.sweep, one
dg_resnet_adapt_sweep launch: forward, fine-grid adjoint, windowed indicator) and of its
training gradient (loss_and_grad: the three dg_resnet_loss_grad passes) at the reference's
shape (python/Main_width_ref.py: 100,000 initial conditions, 100 neurons per layer,
ref_factor 4) for 2 to 32 layers, timed with HIP events over windows of many launches.

  python profiles/resnet_probe.py [--ics 100000] [--width 100] [--layers 2 4 8 16 32] [--rf 4]
  python profiles/resnet_probe.py --cpu [--layers 2 8]   # the numpy statement, host clock

Unit: member neuron-steps per second.  The sweep does L*F neuron-steps forward (4 fp64 vector
instructions each: subtract, multiply, max, fma) and L*rf*F on the fine grid (9 each: subtract,
multiply, compare, two selects and two moves for the 64-bit mask, two fma) per member; the
gradient 2*L*F in pass A (one forward, one derivative) and L*F in pass B (8 each).  Algorithmic
bytes per member: sweep 8*(L+1) (U) + 8*L (err) + 16 (u0, target), the fine grid re-reads U
from cache; gradient 32*L (u_l and q_l written, then read once per layer) + 16.  Both are
bound by fp64 vector issue, not by HBM: the probe reports the instruction rate against the
chip's 78.6 TF fp64 vector peak (39.3e12 lane-instructions/s) as `valu_fraction`."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_LANE_INSTR = 39.3e12  # fp64 vector instructions x lanes per second (78.6 TF as FMA)


def make(ics, width, layers, seed=0):
  rng = np.random.default_rng(seed)
  times = np.linspace(0.0, 1.0, layers + 1)
  params = [(rng.normal(0, 1, width), rng.normal(0, 1, width),
             rng.normal(0, 1 / np.sqrt(width), width)) for _ in range(layers)]
  u0 = rng.uniform(-1, 1, ics)
  return times, params, u0, u0 + 0.3 * np.cos(3 * u0)


def counts(ics, width, layers, rf):
  sweep = dict(units=ics * width * layers * (1 + rf), instr=ics * width * layers * (4 + 9 * rf),
               bytes=ics * (8.0 * (layers + 1) + 8.0 * layers + 16.0))
  grad = dict(units=ics * width * layers * 3, instr=ics * width * layers * (4 + 9 + 8),
              bytes=ics * (32.0 * layers + 16.0))
  return sweep, grad


def gpu_time(fn, torch, min_window=0.2, windows=5):
  """Median seconds per call over `windows` event-timed windows of >= min_window seconds."""
  st = torch.cuda.current_stream()

  def window(n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(n):
      fn()
    e1.record(st)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3

  window(3)  # warm-up
  n = max(3, int(np.ceil(min_window / max(window(3) / 3, 1e-7))))
  return float(np.median([window(n) for _ in range(windows)]) / n), n


def main():
  p = argparse.ArgumentParser()
  p.add_argument("--ics", type=int, default=100000)
  p.add_argument("--width", type=int, default=100)
  p.add_argument("--layers", type=int, nargs="+", default=[2, 4, 8, 16, 32])
  p.add_argument("--rf", type=int, default=4)
  p.add_argument("--cpu", action="store_true",
                 help="time the numpy statement (tests/resnet_oracle.py) instead of the device")
  a = p.parse_args()
  for layers in a.layers:
    times, params, u0, target = make(a.ics, a.width, layers)
    c_sweep, c_grad = counts(a.ics, a.width, layers, a.rf)
    row = {"ics": a.ics, "width": a.width, "layers": layers, "ref_factor": a.rf}
    if a.cpu:
      sys.path.insert(0, os.path.join(ROOT, "tests"))
      import resnet_oracle as ro
      t0 = time.perf_counter()
      ro.sweep(times, params, u0, target, a.rf)
      t1 = time.perf_counter()
      ro.loss_grad(times, params, u0, target)
      t2 = time.perf_counter()
      row.update(device="cpu-numpy", sweep_s=t1 - t0, grad_s=t2 - t1)
    else:
      import torch
      pkg = importlib.import_module("adjoint-ode-adaptivity_amd")
      ens = pkg.resnet_ensemble.ResNetEnsemble(times, params, u0, target, ref_factor=a.rf)
      loss = torch.empty((), dtype=torch.float64, device=ens.dev)
      t_sweep, n_sweep = gpu_time(ens.sweep, torch)
      t_grad, n_grad = gpu_time(lambda: ens._launch_loss_grad(loss), torch)
      row.update(device=torch.cuda.get_device_name(ens.dev), sweep_s=t_sweep, grad_s=t_grad,
                 calls_per_window=[n_sweep, n_grad],
                 sweep_valu_fraction=c_sweep["instr"] / t_sweep / PEAK_LANE_INSTR,
                 grad_valu_fraction=c_grad["instr"] / t_grad / PEAK_LANE_INSTR,
                 sweep_algorithmic_GBs=c_sweep["bytes"] / t_sweep / 1e9,
                 grad_algorithmic_GBs=c_grad["bytes"] / t_grad / 1e9)
    row.update(sweep_neuron_steps_per_s=c_sweep["units"] / row["sweep_s"],
               grad_neuron_steps_per_s=c_grad["units"] / row["grad_s"])
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
  main()
