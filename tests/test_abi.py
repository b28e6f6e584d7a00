"""The C-ABI library loads and exports every entry point include/dg_advec.h declares
(no compute calls: this runs without a GPU)."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "dg_advec.h")


def declared_functions():
  src = open(HEADER).read()
  src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
  return sorted(set(re.findall(r"^\s*(?:const\s+)?[A-Za-z_][\w\s\*]*?\b(dg_\w+)\s*\(", src,
                               flags=re.M)))


def test_header_declares_the_contract():
  names = declared_functions()
  for required in ("dg_plan_create", "dg_plan_destroy", "dg_advec_rhs", "dg_lserk4_fwd",
                   "dg_lserk4_adj", "dg_slope_limit_n", "dg_argmax", "dg_last_error"):
    assert required in names


def test_library_exports_every_declared_symbol(pkg):
  lib = pkg._lib.load()
  raw = ctypes.CDLL(pkg._lib.LIB_PATH)
  missing = [n for n in declared_functions() if not hasattr(raw, n)]
  assert not missing, missing
  assert set(pkg._lib.SIGNATURES) == set(declared_functions())
  assert lib.dg_version().decode().startswith("dg_advec")


def test_library_is_built_for_gfx950(pkg):
  data = open(pkg._lib.LIB_PATH, "rb").read()
  assert b"gfx950" in data


def test_argument_errors_cross_the_abi_as_codes(pkg):
  lib = pkg._lib.load()
  out = ctypes.c_void_p()
  import numpy as np
  bufs = [pkg._lib.dbl_array(np.zeros(4))[1] for _ in range(6)]
  rc = lib.dg_plan_create(0, 10, 1, *bufs, 1.0, 0, 0, ctypes.byref(out))  # N = 0: invalid
  assert rc == pkg._lib.DG_ERR_ARG
  assert b"N must be" in lib.dg_last_error()
  assert lib.dg_plan_destroy(None) == 0
  assert lib.dg_advec_rhs(None, None, None, 0.0, None) == pkg._lib.DG_ERR_ARG


def test_missing_library_fails_loudly(pkg, monkeypatch, tmp_path):
  monkeypatch.setattr(pkg._lib, "_lib", None)
  monkeypatch.setattr(pkg._lib, "LIB_PATH", str(tmp_path / "nope.so"))
  with pytest.raises(pkg._lib.DGLibraryError):
    pkg._lib.load()


def test_operator_refuses_cpu(pkg):
  import torch
  if torch.cuda.is_available():
    pytest.skip("GPU present")
  with pytest.raises(pkg._lib.DGLibraryError):
    pkg.operators.DGAdvection1D(pkg.BaseGalerkin1D(n=2, k=8))


def header_enums():
  """name -> value of every `DG_NAME = value` enumerator in include/dg_advec.h."""
  src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
  out = {}
  for body in re.findall(r"enum\s*\{(.*?)\}", src, flags=re.S):
    for name, val in re.findall(r"\b(DG_[A-Z0-9_]+)\s*=\s*(-?\d+)", body):
      out[name] = int(val)
  return out


def test_python_constants_match_the_header(pkg):
  """The ctypes layer's constants are the header's enumerators (a new tuning key or flag
  added on one side only would pass the wrong integer across the ABI)."""
  enums = header_enums()
  assert len(enums) >= 20
  for name, val in enums.items():
    assert hasattr(pkg._lib, name), f"_lib lacks {name}"
    assert getattr(pkg._lib, name) == val, name


def test_tuning_a_null_plan_is_an_argument_error(pkg):
  lib = pkg._lib.load()
  for key in (pkg._lib.DG_TUNE_REC_LANE_ELEMENTS, pkg._lib.DG_TUNE_REC_STEPS_PER_LAUNCH):
    assert lib.dg_plan_tune(None, key, 2) == pkg._lib.DG_ERR_ARG
  out = (ctypes.c_int64 * 4)()
  assert lib.dg_plan_query_rec(None, out) == pkg._lib.DG_ERR_ARG


def entry_point_comments():
  """name -> (parameter list, the comment block that precedes its declaration) for every
  function of the header; declarations that follow one another share the block above them."""
  src = open(HEADER).read()
  out, comment = {}, ""
  for m in re.finditer(r"/\*(.*?)\*/|^\s*(?:const\s+)?[A-Za-z_][\w\s\*]*?\b(dg_\w+)\s*\(([^;]*?)\)\s*;",
                       src, flags=re.S | re.M):
    if m.group(2) is None:
      comment = m.group(1)
    else:
      out[m.group(2)] = (m.group(3), comment)
  return out


# Entry points whose aliasing differs from the default sentence of the Conventions block: each
# says how in an "Alias:" (or, in a shared comment, "Alias (name):") line.
ALIAS_LINES = {"dg_lserk4_fwd", "dg_lserk4_fwd_ex", "dg_lserk4_adj", "dg_lserk4_adj_ex",
               "dg_lserk4_fwd_rec", "dg_plan_refine_marked", "dg_init_sine", "dg_time_march",
               "dg_time_adjoint", "dg_fd_adapt_sweep", "dg_resnet_adapt_sweep",
               "dg_resnet_loss_grad"}


def test_header_states_the_alias_rule_for_every_entry_point():
  """The Conventions block has the "Aliasing and alignment" paragraph with the default (disjoint
  byte ranges, half-open, DG_ERR_ARG before anything is enqueued), and every compute entry point
  (one with a stream) that takes two or more arrays either has its own Alias line -- exactly the
  entry points listed above -- or falls under that default."""
  src = open(HEADER).read()
  head = src[:src.index("#ifndef DG_ADVEC_H")]
  para = head[head.index("Aliasing and alignment"):]
  flat = " ".join(para.replace("*", " ").split())
  for phrase in ("byte ranges of any two array arguments of one compute call must be disjoint",
                 'unless that entry point\'s comment has an "Alias:" line', "half-open",
                 "exact identity", "DG_ERR_ARG before anything is enqueued", "16 bytes"):
    assert phrase in flat, phrase
  fns = entry_point_comments()
  assert set(fns) == set(declared_functions())
  with_line, default = set(), set()
  for name, (params, comment) in fns.items():
    args = [a.strip() for a in params.split(",")]
    if not any(re.fullmatch(r"void\s*\*\s*stream", a) for a in args):
      continue  # not a compute call
    arrays = [a for a in args if ("*" in a or "[" in a) and "dg_plan" not in a
              and not re.fullmatch(r"void\s*\*\s*stream", a)]
    if len(arrays) < 2:
      continue
    tagged = re.findall(r"Alias(?: \((\w+)\))?:", comment)
    if "" in tagged or name in tagged:
      with_line.add(name)
    else:
      default.add(name)
  assert with_line == ALIAS_LINES, (sorted(with_line - ALIAS_LINES), sorted(ALIAS_LINES - with_line))
  # the default covers the rest: the ones the library checks with its one range helper
  for name in ("dg_advec_rhs", "dg_lserk4_adj_rec", "dg_lserk4_sweep_rec", "dg_lserk4_sweep_refine",
               "dg_slope_limit_n", "dg_slope_limit_1", "dg_prolong", "dg_lserk4_adj_p",
               "dg_lserk4_adj_p_refine", "dg_lserk4_sweep_p", "dg_plan_mark", "dg_sum_rows",
               "dg_slice_candidate", "dg_argmax", "dg_argmax_ex", "dg_candidates_argmax",
               "dg_stream_copy", "dg_plan_refine", "dg_field_to_children",
               "dg_field_from_children"):
    assert name in default, name


# Entry points that are not purely asynchronous: each says in a "Sync:" (or, in a shared comment,
# "Sync (name):") line what it waits for -- "the stream" or "the device" on every call, or "only
# on first use or growth" together with what it allocates.  tests/test_gpu_stream_order.py
# imports this: on a delayed side stream a warmed-up call must come back while the delay is
# still running, unless it is listed here as waiting for the stream or the device on every
# call -- and those must not.
SYNC_LINES = {"dg_plan_destroy": "device", "dg_plan_reserve": "device",
              "dg_plan_get_mesh": "device", "dg_plan_refine_marked": "stream",
              "dg_sweep_status": "stream", "dg_lserk4_adj_ex": "first use",
              "dg_lserk4_sweep_rec": "first use", "dg_lserk4_sweep_refine": "first use",
              "dg_lserk4_adj_p": "first use", "dg_lserk4_adj_p_refine": "first use",
              "dg_lserk4_sweep_p": "first use"}
SYNC_KINDS = {"the stream": "stream", "the device": "device",
              "only on first use or growth": "first use"}


def test_header_says_which_entry_points_wait():
  """The Conventions block promises that compute calls enqueue on `stream` and return without
  waiting, that an entry point that waits says so in a "Sync:" line, and that nothing allocates
  in the steady state; the entry points with such a line, and what each waits for, are exactly
  the ones listed above.  Every one that waits only on first use or growth names what it
  allocates."""
  src = open(HEADER).read()
  head = " ".join(src[:src.index("#ifndef DG_ADVEC_H")].replace("*", " ").split())
  for phrase in ("enqueue every launch, fill and copy on `stream`", "return without waiting",
                 'has a "Sync:" line in its comment', "one without such a line never waits",
                 "in the steady state no compute call allocates",
                 "every compute call that takes a non-const dg_plan uses it, except "
                 "dg_slope_limit_n / dg_slope_limit_1"):
    assert phrase in head, phrase
  assert "never allocates inside compute calls" not in head
  fns = entry_point_comments()
  found = {}
  for name, (params, comment) in fns.items():
    flat = " ".join(comment.replace("*", " ").split())
    for m in re.finditer(r"Sync(?: \((\w+)\))?: (.*?)(?=$| Alias| Sync)", flat):
      if m.group(1) not in (None, name):
        continue
      kinds = [k for text, k in SYNC_KINDS.items() if m.group(2).startswith(text)]
      assert len(kinds) == 1, (name, m.group(2)[:60])
      found[name] = kinds[0]
      if kinds[0] == "first use":
        assert re.search(r"hipMalloc|hipHostMalloc|as dg_lserk4_\w+", m.group(2)), name
  assert found == SYNC_LINES, (sorted(set(found.items()) ^ set(SYNC_LINES.items())))
  # a waiting entry point without a stream parameter waits for the device
  for name, kind in SYNC_LINES.items():
    has_stream = bool(re.search(r"void\s*\*\s*stream", fns[name][0]))
    assert has_stream or kind == "device", name
