// dg_chain.h — the launch chain, once: how a sweep of `nsteps` is cut into launches, which
// buffer each launch reads and writes, and which indicator bits it carries (DESIGN.md §5
// "Launch chains").  Plain C++17 with callables for the launches and copies: no HIP, so a
// host compiler builds it alone (tests/test_chain_host.py pins the schedule on the CPU).
//
// A chunk function maps the steps still to run (`left` >= 1) to the steps of the next launch,
// 1 <= m <= left.  A launch or copy callable returns 0 or an error code, which ends the chain.
#pragma once
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

namespace dgk {

// Indicator accumulation bits of a launch (AdjArgs::has_eta and its kin).
constexpr int kEtaOn = 1, kEtaAssign = 2, kEtaAbs = 4;

namespace chain {

// The nsteps + 1 time levels by repeated addition (time = time + dt, One_code.mlx:139).
inline std::vector<double> time_levels(double t0, double dt, int nsteps) {
  std::vector<double> tn(size_t(nsteps) + 1);
  tn[0] = t0;
  for (int n = 0; n < nsteps; ++n) tn[n + 1] = tn[n] + dt;
  return tn;
}

// Indicator bits of a whole sweep in one launch (the dataflow kernels).
inline int eta_sweep_mode(bool eta, bool assign, bool abs) {
  return eta ? (kEtaOn | (assign ? kEtaAssign : 0) | (abs ? kEtaAbs : 0)) : 0;
}

// Indicator bits of launch l, whose first step is n0, of a reverse chain: the first launch
// assigns eta, the one that reaches step 0 stores |eta|.
inline int eta_launch_mode(int l, int n0, bool assign, bool abs) {
  return ((l == 0 && assign) ? kEtaAssign : 0) | ((n0 == 0 && abs) ? kEtaAbs : 0);
}

// Halving chunk: the largest of m0, m0/2, m0/4, ... that fits, at least 1.
inline int halve(int m0, int left) {
  while (m0 > left) m0 >>= 1;
  return m0 < 1 ? 1 : m0;
}

template <class Chunk> int launches(int nsteps, Chunk chunk) {
  int l = 0;
  for (int left = nsteps; left > 0; left -= chunk(left)) ++l;
  return l;
}

struct Result {
  int rc;
  const double* buf;  // the buffer that holds the chain's result (rc == 0)
};

// Reverse chain from step nsteps down to 0: launch(l, n0, m, in, out, em) covers steps
// n0 .. n0+m-1.  Launch 0 reads w; a launch never writes the buffer it reads: intermediate
// outputs alternate s0, s1 by launch index and the last launch writes w when there is more
// than one.  The result is in `buf` (s0 after a single launch, w after none): the caller
// hands it back.
template <class Chunk, class Launch>
Result reverse(int nsteps, Chunk chunk, double* w, double* s0, double* s1, bool assign, bool abs,
               Launch launch) {
  const int count = launches(nsteps, chunk);
  const double* in = w;
  int l = 0;
  for (int n = nsteps; n > 0; ++l) {
    const int m = chunk(n), n0 = n - m;
    double* out = (l == count - 1 && count > 1) ? w : ((l % 2 == 0) ? s0 : s1);
    if (const int rc = launch(l, n0, m, in, out, eta_launch_mode(l, n0, assign, abs)))
      return {rc, nullptr};
    in = out;
    n = n0;
  }
  return {0, in};
}

// Forward chain out of place: launch(l, n0, m, in, out) from u0; outputs alternate s0, s1 and
// the final launch writes uN unless it would read it (one launch with u0 == uN).  u0 is
// written only where it is uN.
template <class Chunk, class Launch>
Result forward(int nsteps, Chunk chunk, const double* u0, double* uN, double* s0, double* s1,
               Launch launch) {
  const double* in = u0;
  int l = 0;
  for (int n = 0; n < nsteps; ++l) {
    const int m = chunk(nsteps - n);
    double* out = (n + m == nsteps && in != uN) ? uN : ((l % 2 == 0) ? s0 : s1);
    if (const int rc = launch(l, n, m, in, out)) return {rc, nullptr};
    in = out;
    n += m;
  }
  return {0, in};
}

// Forward chain in place: u <-> scratch, the last launch landing in u; with an odd launch
// count the first launch reads a copy(scratch, u).
template <class Chunk, class Copy, class Launch>
int pingpong(int nsteps, Chunk chunk, double* u, double* scratch, Copy copy, Launch launch) {
  double *a = u, *b = scratch;
  if (launches(nsteps, chunk) % 2 == 1) {
    if (const int rc = copy(b, a)) return rc;
    std::swap(a, b);
  }
  int l = 0;
  for (int n = 0; n < nsteps; ++l) {
    const int m = chunk(nsteps - n);
    if (const int rc = launch(l, n, m, a, b)) return rc;
    std::swap(a, b);
    n += m;
  }
  return 0;
}

// Snapshot march: row 0 = u (copied when they differ); launch(l, n0, m, in, rows, last) reads
// row n0 and writes rows n0+1 .. n0+m.  u receives u^nsteps from the final launch (`last` = u
// there, else null) or, where the kernel has no such output (last_out = false), by a copy of
// the last row.
template <class Chunk, class Copy, class Launch>
int march(int nsteps, Chunk chunk, double* u, double* snapshots, int64_t field, bool last_out,
          Copy copy, Launch launch) {
  const bool apart = snapshots != u;
  if (apart)
    if (const int rc = copy(snapshots, u)) return rc;
  int l = 0;
  for (int n = 0; n < nsteps; ++l) {
    const int m = chunk(nsteps - n);
    double* last = (last_out && apart && n + m == nsteps) ? u : nullptr;
    if (const int rc = launch(l, n, m, snapshots + int64_t(n) * field,
                              snapshots + int64_t(n + 1) * field, last))
      return rc;
    n += m;
  }
  if (!last_out && apart && nsteps > 0) return copy(u, snapshots + int64_t(nsteps) * field);
  return 0;
}

}  // namespace chain
}  // namespace dgk
