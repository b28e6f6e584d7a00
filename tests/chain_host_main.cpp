// The launch schedule of csrc/dg_chain.h, printed (tests/test_chain_host.py).  Includes that
// header alone; buffers are named symbolically: w / u / u0 / uN the caller's, s0 / s1 the
// scratch fields, rN snapshot row N, - a null pointer.
//   chain_host_main KIND M0 NMAX
// KIND = halve | min (the chunk function, from M0); every nsteps in 0 .. NMAX, one line per
// launch or copy.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "dg_chain.h"

namespace ch = dgk::chain;

namespace {
constexpr int64_t kField = 3;
constexpr int kMaxSteps = 64;
double w[kField], u[kField], uN[kField], s0[kField], s1[kField];
double rows[(kMaxSteps + 1) * kField];

std::string name(const double* p) {
  if (p == nullptr) return "-";
  if (p == w) return "w";
  if (p == u) return "u";
  if (p == uN) return "uN";
  if (p == s0) return "s0";
  if (p == s1) return "s1";
  if (p >= rows && p < rows + sizeof(rows) / sizeof(double) && (p - rows) % kField == 0)
    return "r" + std::to_string((p - rows) / kField);
  return "?";
}

int copy(double* dst, const double* src) {
  std::printf("copy %s %s\n", name(dst).c_str(), name(src).c_str());
  return 0;
}

void run(bool halve, int m0, int nsteps) {
  std::printf("nsteps %d\n", nsteps);
  auto chunk = [=](int left) { return halve ? ch::halve(m0, left) : (m0 > left ? left : m0); };

  const std::vector<double> tn = ch::time_levels(0.1, 1.0 / 3.0, nsteps);
  std::printf("levels");
  for (double t : tn) {
    uint64_t bits;
    std::memcpy(&bits, &t, sizeof(bits));
    std::printf(" %016" PRIx64, bits);
  }
  std::printf("\nsweep_mode %d %d %d %d %d\n", ch::eta_sweep_mode(false, true, true),
              ch::eta_sweep_mode(true, false, false), ch::eta_sweep_mode(true, true, false),
              ch::eta_sweep_mode(true, false, true), ch::eta_sweep_mode(true, true, true));

  for (int flags = 0; flags < 4; ++flags) {
    std::printf("reverse %d\n", flags);
    const ch::Result r = ch::reverse(
        nsteps, chunk, w, s0, s1, flags & 1, flags & 2,
        [](int l, int n0, int m, const double* in, double* out, int em) {
          std::printf("launch %d %d %d %s %s %d\n", l, n0, m, name(in).c_str(), name(out).c_str(),
                      em);
          return 0;
        });
    std::printf("result %d %s\n", r.rc, name(r.buf).c_str());
  }
  auto launch = [](int l, int n0, int m, const double* in, double* out) {
    std::printf("launch %d %d %d %s %s\n", l, n0, m, name(in).c_str(), name(out).c_str());
    return 0;
  };
  for (double* out : {uN, u}) {  // u0 and uN distinct, then u0 == uN
    std::printf("forward %s\n", out == u ? "alias" : "apart");
    const ch::Result r = ch::forward(nsteps, chunk, u, out, s0, s1, launch);
    std::printf("result %d %s\n", r.rc, name(r.buf).c_str());
  }
  std::printf("pingpong\n");
  std::printf("result %d\n", ch::pingpong(nsteps, chunk, u, s0, copy, launch));
  for (int k = 0; k < 4; ++k) {  // (u apart from / on snapshot row 0) x (`last` output or not)
    double* state = (k & 1) ? rows : u;
    std::printf("march %s %s\n", (k & 1) ? "alias" : "apart", (k & 2) ? "copyback" : "last");
    const int rc = ch::march(
        nsteps, chunk, state, rows, kField, !(k & 2), copy,
        [](int l, int n0, int m, const double* in, double* out, double* last) {
          std::printf("launch %d %d %d %s %s %s\n", l, n0, m, name(in).c_str(), name(out).c_str(),
                      name(last).c_str());
          return 0;
        });
    std::printf("result %d\n", rc);
  }
  // an error ends a chain at once and is returned
  int seen = 0;
  const ch::Result bad = ch::reverse(nsteps, chunk, w, s0, s1, false, false,
                                     [&](int, int, int, const double*, double*, int) {
                                       ++seen;
                                       return -7;
                                     });
  std::printf("error %d %d %s\n", bad.rc, seen, name(bad.buf).c_str());
}
}  // namespace

int main(int argc, char** argv) {
  if (argc < 4) return 2;
  const int nmax = std::atoi(argv[3]);
  if (nmax > kMaxSteps) return 2;
  for (int n = 0; n <= nmax; ++n) run(std::strcmp(argv[1], "halve") == 0, std::atoi(argv[2]), n);
  return 0;
}
