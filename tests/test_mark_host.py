"""The marking contract on the host: the oracle of tests/mark_oracle.py against numpy's argmax
and galerkin.split_interval, and the C ABI's declarations (no GPU)."""
import re

import numpy as np

import mark_oracle as mo
from test_abi import HEADER, declared_functions, header_enums

SPECIAL = np.array([0.0, -0.0, 5e-324, -5e-324, 2.2250738585072014e-308, 1.0, -1.0, 1.0, 3.5,
                    -3.5, np.inf, -np.inf, np.nan, 1e300, -1e300, -np.nan, 0.0, 1e-310, np.inf,
                    2.0, -2.0, np.nan])


def argmax_rounds(eta, m):
  """m rounds of np.argmax(|eta|) with removal."""
  a = np.abs(np.asarray(eta, dtype=np.float64))
  alive = np.ones(len(a), dtype=bool)
  picked = []
  for _ in range(m):
    idx = np.flatnonzero(alive)
    j = idx[np.argmax(a[idx])]
    picked.append(j)
    alive[j] = False
  return picked


def test_top_count_is_argmax_with_removal():
  rng = np.random.default_rng(5)
  for eta in (SPECIAL, rng.permutation(SPECIAL), np.zeros(7), SPECIAL[:1]):
    order = mo.rank_order(eta)
    assert list(order) == argmax_rounds(eta, len(eta))
    for m in range(len(eta) + 3):
      want = np.zeros(len(eta), dtype=np.uint8)
      want[argmax_rounds(eta, min(m, len(eta)))] = 1
      np.testing.assert_array_equal(mo.top_count(eta, m), want)
      np.testing.assert_array_equal(mo.top_count(eta, len(eta), cap=m), want)


def test_max_fraction_cases():
  eta = np.array([0.0, -4.0, 2.0, 1.0, -2.0, 4.0, 1.9999999])
  np.testing.assert_array_equal(mo.max_fraction(eta, 1.0), [0, 1, 0, 0, 0, 1, 0])
  np.testing.assert_array_equal(mo.max_fraction(eta, 0.5), [0, 1, 1, 0, 1, 1, 0])
  np.testing.assert_array_equal(mo.max_fraction(eta, 0.5, cap=3), [0, 1, 1, 0, 0, 1, 0])
  np.testing.assert_array_equal(mo.max_fraction(eta, 2.0 ** -60), [0, 1, 1, 1, 1, 1, 1])
  np.testing.assert_array_equal(mo.max_fraction(np.zeros(4), 0.5), [0, 0, 0, 0])
  bad = np.array([1.0, np.inf, 3.0, np.nan, -np.inf])
  np.testing.assert_array_equal(mo.max_fraction(bad, 0.5), [0, 1, 0, 1, 1])
  np.testing.assert_array_equal(mo.max_fraction(bad, 0.5, cap=2), [0, 1, 0, 1, 0])
  assert mo.info(bad, [1, 0, 1, 0, 0], [0.0, 1.0, 1.5, 1.75, 3.0, 4.0]) == (2, 3, 0.25)
  assert mo.info(eta[:2], [0, 0], [0.0, 1.0, 2.0]) == (0, 0, float("inf"))


def test_split_marked_is_split_interval_from_the_top(pkg):
  rng = np.random.default_rng(11)
  vx = np.cumsum(rng.uniform(0.01, 1.0, 41))
  for marks in (np.zeros(40, bool), np.ones(40, bool), rng.random(40) < 0.3,
                np.arange(40) % 2 == 0, np.arange(40) == 39, np.arange(40) == 0):
    want = vx.copy()
    for j in np.flatnonzero(marks)[::-1]:
      want = pkg.split_interval(want, j)
    got, parent = mo.split_marked(vx, marks)
    np.testing.assert_array_equal(got, want)
    assert parent.dtype == np.int32 and len(parent) == 40 + np.count_nonzero(marks)
    # new element e covers a sub-interval of old element parent[e]
    assert np.all(vx[parent] <= got[:-1]) and np.all(got[1:] <= vx[parent + 1])


def test_header_declares_marking_and_lib_mirrors_it(pkg):
  names = declared_functions()
  for fn in ("dg_plan_mark", "dg_plan_refine_marked", "dg_plan_query_mark"):
    assert fn in names
    assert fn in pkg._lib.SIGNATURES
  enums = header_enums()
  assert enums["DG_MARK_TOP_COUNT"] == pkg._lib.DG_MARK_TOP_COUNT == 0
  assert enums["DG_MARK_MAX_FRACTION"] == pkg._lib.DG_MARK_MAX_FRACTION == 1
  src = open(HEADER).read()
  for fn in ("dg_plan_mark", "dg_plan_refine_marked"):
    comment = re.findall(r"/\*(?:(?!\*/).)*?\*/\s*(?:enum[^;]*;\s*)?int " + fn + r"\(", src,
                         flags=re.S)
    assert comment and "Main_finite_difference.py:336-341" in comment[0]
    assert "MAIN.m:137-141" in comment[0]
