"""The tuning-key table and the shape rules of csrc/dg_shape.h, pinned on the CPU.

tests/shape_host_main.cpp includes that header alone (plain C++17, no HIP; it takes the key
numbers and return codes from include/dg_advec.h) and prints, built here with the host
compiler: what every key does with every value in -2 .. 33 at Np = 2, 3, 4, 5, 6, 9 (return
code, message, the knobs afterwards); what every environment name does with the same values as
text plus "" and "8x", and the ordering cases of "both directions" against the forward's own
override; and the shapes the rules resolve over Np 2 .. 9 x uniform x stages x three sizes
(1000 and both sides of the forward's 3*2^20 rule) x every allowed value of a family's knobs x
13 step counts x the four DG_P_HORNER modes.  The dataflow sweep's family crosses its own four
knobs with the record shapes its blocks come from (both widths, the forward's own width, 5-,
10- and 20-step blocks, the forward by size / as the adjoint / 20, one element per lane once).
Every line is compared with tests/shape_rules.py, an independent restatement, and held to the
invariants the launch ladders rely on.  A second build with -fsanitize=address,undefined runs
the same program (host code with its own main: nothing is preloaded)."""
import os
import subprocess

import pytest

import shape_rules as R
from test_chain_host import compiler

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..")
NPS = (2, 3, 4, 5, 6, 9)
NSTEPS = (0, 1, 4, 5, 7, 8, 10, 20, 32, 36, 40, 41, 60)
KTOTS = (1000, 3 * 2**20, 3 * 2**20 + 1)
# steps per launch each family's ladder instantiates: tile_shape / wstep_e (dg_advec.hip,
# dg_wave.hip), pair_shape (dg_rec.hip), launch_adj_p_t (dg_dwr.hip)
FWD_LADDER = {1: (1, 2, 4), 2: (1, 2, 4, 8)}
PAIR_LADDER = {1: (1, 2, 4, 5, 8, 10), 2: (1, 2, 4, 5, 8, 10, 16, 20)}
P_LADDER = {1: (1, 2, 4), 2: (1, 2, 4, 8)}  # (a 1-step launch runs 256-element tiles)


def build(tmp, name, extra=()):
  exe = os.path.join(tmp, name)
  subprocess.run([compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", *extra,
                  "-I", os.path.join(ROOT, "adjoint-ode-adaptivity_amd", "csrc"),
                  "-I", os.path.join(ROOT, "include"),
                  os.path.join(HERE, "shape_host_main.cpp"), "-o", exe], check=True)
  return exe


def run(exe, mode):
  return subprocess.run([exe, mode], check=True, capture_output=True,
                        text=True).stdout.splitlines()


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
  return build(str(tmp_path_factory.mktemp("shape")), "shape_host")


# --- the expected output ----------------------------------------------------------------------
def expect_tune():
  out = []
  for NP in NPS:
    for key in range(0, 23):
      vals = list(range(-2, 34)) + ([2**30, 2**30 + 1] if key == R.SPIN_LIMIT else [])
      for v in vals:
        s = R.Shape(NP)
        rc, text = s.tune(key, v)
        out.append(f't {NP} {key} {v} {rc} "{text}" | {s.knobs()}')
  return out


def expect_env():
  vals = [str(v) for v in range(-2, 34)] + ["", "8x"]
  out = []
  for NP in NPS:
    for name in R.ENV_NAMES:
      for v in vals:
        out.append(f'e {NP} {name} "{v}" | {R.Shape(NP).environment({name: v}).knobs()}')
    for tag, env in (("steps", {"DG_REC_STEPS_PER_LAUNCH": "8"}),
                     ("steps+fwd", {"DG_REC_STEPS_PER_LAUNCH": "8",
                                    "DG_REC_FWD_STEPS_PER_LAUNCH": "20"}),
                     ("width+fwd", {"DG_REC_TILE_WIDTH": "1", "DG_REC_FWD_TILE_WIDTH": "2"})):
      out.append(f"o {NP} {tag} | {R.Shape(NP).environment(env).knobs()}")
  out.append("names 18")
  return out


def expect_shapes():
  out = []
  for NP in range(2, 10):
    for uni in (1, 0):
      for nst in (5, 1):
        for ktot in KTOTS:
          mk = lambda **kw: R.Shape(NP, bool(uni), nst, ktot, **kw)  # noqa: E731
          out.append(f"c {NP} {uni} {nst} {ktot}")
          for w in (1, 2):
            for wf in (0, 1, 2):
              for m in R.REC_STEP_VALUES:
                for mf in (-1, 0) + R.REC_STEP_VALUES:
                  for le in (1, 2):
                    s = mk(rec_tile_width=w, rec_tile_width_fwd=wf, rec_msteps=m,
                           rec_msteps_fwd=mf, rec_lane_elems=le)
                    out.append(f"r {w} {wf} {m} {mf} {le} | {R.rec_fwd_width(s)} "
                               f"{R.rec_steps(s)} {R.rec_steps_fwd(s)} {int(le == 2)}")
          for tw in (1, 2):
            for ms in (1, 2, 4, 8):
              for le in (0, 2, 4, 8):
                for sp in (0, 1):
                  s = mk(tile_width=tw, msteps=ms, lane_elems=le, snap_pairs=sp)
                  out.append(f"f {tw} {ms} {le} {sp} | {ms} {le} {sp} {R.fwd_steps(s)} "
                             f"{R.fwd_steps(s, 4, 0)}")
          for ms in (1, 2, 4, 8):
            for x in (0, 1):
              s = mk(msteps=ms, nl_exchange=x)
              out.append(f"n {ms} {x} | {R.nl_steps(s, True)} {R.nl_steps(s, False)}")
          for W in (1, 2):
            for m in (1, 2, 4, 8):
              for fl in (0, 1):
                for sw in (0, 1):
                  for le in (0, 2, 4, 8):
                    s = mk(p_tile_width=W, p_msteps=m, p_flow=fl, p_sweep=sw, lane_elems=le)
                    for h in range(4):
                      ln = f"p {W} {m} {fl} {sw} {le} {h} | {R.p_steps(s)}"
                      for n in NSTEPS:
                        items = R.p_trace(s, n, h)
                        ln += f" {int(R.p_flow(s, n, h))} {int(R.p_sweep(s, n, h))} " \
                              f"{items[0]} {items[1]}"
                      out.append(ln)
          for rs in (0, 1):
            for sw in R.allowed(R.SWEEP_WAVES, NP):
              for sl in R.allowed(R.SWEEP_LANE_ELEMENTS, NP):
                for sx in (0, 1):
                  for w in (1, 2):
                    for wf in (0, 3 - w):
                      for m in (5, 10, 20):
                        for mf in (-1, 0, 20):
                          for le in (2, 1):
                            if le == 1 and (m != 10 or mf != -1):
                              continue
                            s = mk(rec_sweep=rs, sweep_waves=sw, sweep_lane_elems=sl,
                                   sweep_exchange=sx, rec_tile_width=w, rec_tile_width_fwd=wf,
                                   rec_msteps=m, rec_msteps_fwd=mf, rec_lane_elems=le)
                            blocks = R.sweep_blocks(s)
                            _, nw, f, a = blocks
                            ln = f"s {rs} {sw} {sl} {sx} {w} {wf} {m} {mf} {le} | {nw} {f} {a} " \
                                 f"{R.sweep_tile(s, nw)}"
                            for n in NSTEPS:
                              q = R.sweep_query(s, n, blocks)
                              ln += f" {q[0]} {q[3]} {R.ceil_div(ktot, q[7])}"
                            out.append(ln)
  return out


_EXPECT = {}


def expected(mode):
  if mode not in _EXPECT:
    _EXPECT[mode] = {"tune": expect_tune, "env": expect_env, "shapes": expect_shapes}[mode]()
  return _EXPECT[mode]


def compare(exe, mode):
  got, want = run(exe, mode), expected(mode)
  assert len(got) == len(want), (mode, len(got), len(want))
  if got != want:
    raise AssertionError((mode, next((g, w) for g, w in zip(got, want) if g != w)))
  return got


# --- the invariants, on the program's own output ------------------------------------------
def check_invariants(lines):
  for ln in lines:
    head, _, tail = ln.partition(" | ")
    h, t = head.split(), [int(x) for x in tail.split()]
    if h[0] == "c":
      NP = int(h[1])
    elif h[0] == "r":  # the record ladders: pair_shape, or tile_shape on one element per lane
      fw, a, f, pairs = t
      ladder = PAIR_LADDER if pairs else FWD_LADDER
      assert a in ladder[int(h[1])] and f in ladder[fw], ln
      assert pairs or NP <= 8 or max(a, f) <= 2, ln
    elif h[0] == "f":  # tile_shape / wstep_e: 8 steps on 512-element tiles or 8-element lanes
      tw, le, eff = int(h[1]), int(h[3]), t[3]
      assert eff in (1, 2, 4, 8) and (eff < 8 or ((tw == 2 or le == 8) and le != 2)), ln
      assert (NP <= 8 or eff <= 2) and t[4] == (4 if NP <= 8 else 2), ln
    elif h[0] == "n":
      assert set(t) <= {1, 2}, ln
    elif h[0] == "p":  # launch_adj_p_t's shapes; a dataflow launch's blocks and tile extent
      W, pm = int(h[1]), t[0]
      assert pm in P_LADDER[W], ln
      for n, (flow, sweep, fi, si) in zip(NSTEPS, zip(*[iter(t[1:])] * 4)):
        if flow:
          assert n % pm == 0 and 2 <= n // pm and n <= 40 and pm in (4, 8), ln
          assert 256 * W - 10 * pm > 0 and fi > 0, ln
        if sweep:
          assert flow and pm == 4 and n <= 32 and si == 2 * fi, ln
        assert (fi > 0) == bool(flow) and (si > 0) == bool(sweep), ln
    elif h[0] == "s":  # the dataflow kernel's instantiated shapes
      nw, f, a, T = t[:4]
      for n, (on, items, tadj) in zip(NSTEPS, zip(*[iter(t[4:])] * 3)):
        if not on:
          assert items == 0, ln
          continue
        assert n % f == 0 and n % a == 0 and 0 < n <= 40, ln
        assert f in (5, 10, 20) and a in (5, 10) and nw in (4, 8, 12, 16), ln
        tef, tea = T - 2 * ((5 * f + 2) & ~1), T - 2 * ((5 * a + 1) & ~1)
        assert tef > 0 and tea > 0 and items > 0 and tadj > 0, ln
        assert nw != 16 or NP <= 5, ln


def test_setter_matches_the_table(plain):
  got = compare(plain, "tune")
  # an accepted value changes at most its knob and its side effect; a refused one nothing
  default = R.Shape(2).knobs()
  for ln in got:
    f = ln.split(" | ")[0].split()
    if f[4] == "-1":
      assert ln.endswith(default), ln


def test_environment_matches_the_table(plain):
  compare(plain, "env")


def test_shapes_match_the_rules(plain):
  check_invariants(compare(plain, "shapes"))


def test_under_sanitizers(tmp_path):
  """The same program built with AddressSanitizer and UBSan, run directly."""
  exe = build(str(tmp_path), "shape_host_san",
              ("-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
  for mode in ("tune", "env", "shapes"):
    compare(exe, mode)
