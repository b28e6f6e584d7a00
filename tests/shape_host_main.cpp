// Host driver of csrc/dg_shape.h for tests/test_shape_host.py: prints what the table of tuning
// keys does to the knobs (the setter, the environment pass) and the shapes the rules resolve
// over a grid of plans.  Includes that header alone; built with the host compiler.
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "dg_shape.h"

using namespace dgk;

static const int kNsteps[] = {0, 1, 4, 5, 7, 8, 10, 20, 32, 36, 40, 41, 60};

static void knobs(const Shape& s) {
  std::printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d\n", s.tile_width,
              s.msteps, s.xcd_order, s.lane_elems, s.rec_tile_width, s.rec_tile_width_fwd,
              s.rec_msteps, s.rec_msteps_fwd, s.rec_lane_elems, s.p_tile_width, s.p_msteps,
              s.p_flow, s.p_sweep, s.rec_sweep, s.sweep_spin_limit, s.sweep_waves,
              s.sweep_lane_elems, s.sweep_exchange, s.snap_pairs, s.nl_exchange);
}

static Shape fresh(int np) {
  Shape s;
  s.NP = np;
  return s;
}

static void tune_mode() {
  for (int np : {2, 3, 4, 5, 6, 9})
    for (int key = 0; key <= 22; ++key) {
      std::vector<int64_t> vals;
      for (int v = -2; v <= 33; ++v) vals.push_back(v);
      if (key == DG_TUNE_SWEEP_SPIN_LIMIT) {
        vals.push_back(int64_t(1) << 30);
        vals.push_back((int64_t(1) << 30) + 1);
      }
      for (int64_t v : vals) {
        Shape s = fresh(np);
        const char* text = "";
        const int rc = tune::set(&s, key, v, &text);
        std::printf("t %d %d %lld %d \"%s\" | ", np, key, (long long)v, rc, text);
        knobs(s);
      }
    }
}

static void env_case(int np, const char* tag, const std::map<std::string, std::string>& env) {
  Shape s = fresh(np);
  tune::from_env(&s, [&](const char* name) -> const char* {
    const auto it = env.find(name);
    return it == env.end() ? nullptr : it->second.c_str();
  });
  std::printf("%s | ", tag);
  knobs(s);
}

static void env_mode() {
  std::vector<std::string> vals;
  for (int v = -2; v <= 33; ++v) vals.push_back(std::to_string(v));
  vals.push_back("");
  vals.push_back("8x");
  for (int np : {2, 3, 4, 5, 6, 9}) {
    for (const tune::Row& r : tune::kRows)
      if (r.env)
        for (const std::string& v : vals)
          env_case(np, ("e " + std::to_string(np) + " " + r.env + " \"" + v + "\"").c_str(),
                   {{r.env, v}});
    const std::string o = "o " + std::to_string(np);
    env_case(np, (o + " steps").c_str(), {{"DG_REC_STEPS_PER_LAUNCH", "8"}});
    env_case(np, (o + " steps+fwd").c_str(),
             {{"DG_REC_STEPS_PER_LAUNCH", "8"}, {"DG_REC_FWD_STEPS_PER_LAUNCH", "20"}});
    env_case(np, (o + " width+fwd").c_str(),
             {{"DG_REC_TILE_WIDTH", "1"}, {"DG_REC_FWD_TILE_WIDTH", "2"}});
  }
  int names = 0;
  for (const tune::Row& r : tune::kRows) names += r.env != nullptr;
  std::printf("names %d\n", names);
}

static const int kRecSteps[] = {1, 2, 4, 5, 8, 10, 16, 20};

static void shapes_mode() {
  for (int np = 2; np <= 9; ++np)
    for (int uni = 1; uni >= 0; --uni)
      for (int nst : {5, 1})
        for (int64_t ktot : {int64_t(1000), int64_t(3) << 20, (int64_t(3) << 20) + 1}) {
          Shape b = fresh(np);
          b.uniform = uni != 0;
          b.nstages = nst;
          b.ktot = ktot;
          std::printf("c %d %d %d %lld\n", np, uni, nst, (long long)ktot);
          // the record family
          for (int w : {1, 2})
            for (int wf : {0, 1, 2})
              for (int m : kRecSteps)
                for (int mf : {-1, 0, 1, 2, 4, 5, 8, 10, 16, 20})
                  for (int le : {1, 2}) {
                    Shape s = b;
                    s.rec_tile_width = w, s.rec_tile_width_fwd = wf, s.rec_msteps = m;
                    s.rec_msteps_fwd = mf, s.rec_lane_elems = le;
                    std::printf("r %d %d %d %d %d | %d %d %d %d\n", w, wf, m, mf, le,
                                rec_fwd_width(&s), rec_msteps(&s), rec_msteps_fwd(&s),
                                int(rec_pairs(&s)));
                  }
          // the snapshot forward
          for (int tw : {1, 2})
            for (int ms : {1, 2, 4, 8})
              for (int le : {0, 2, 4, 8})
                for (int sp : {0, 1}) {
                  Shape s = b;
                  s.tile_width = tw, s.msteps = ms, s.lane_elems = le, s.snap_pairs = sp;
                  const FwdShape f = plan_shape(&s);
                  std::printf("f %d %d %d %d | %d %d %d %d %d\n", tw, ms, le, sp, f.msteps,
                              f.lane_elems, f.snap_pairs, effective_msteps(&s, f),
                              effective_msteps(&s, FwdShape{4, 0, 0}));
                }
          // config 3
          for (int ms : {1, 2, 4, 8})
            for (int x : {0, 1}) {
              Shape s = b;
              s.msteps = ms, s.nl_exchange = x;
              std::printf("n %d %d | %d %d\n", ms, x, nl_msteps(&s, true), nl_msteps(&s, false));
            }
          // the p-estimate
          for (int W : {1, 2})
            for (int m : {1, 2, 4, 8})
              for (int fl : {0, 1})
                for (int sw : {0, 1})
                  for (int le : {0, 2, 4, 8})
                    for (int h = 0; h <= 3; ++h) {
                      Shape s = b;
                      s.p_tile_width = W, s.p_msteps = m, s.p_flow = fl, s.p_sweep = sw;
                      s.lane_elems = le;
                      std::printf("p %d %d %d %d %d %d | %d", W, m, fl, sw, le, h, p_msteps(&s));
                      for (int n : kNsteps) {
                        const bool f = p_flow_shape(&s, n, h), q = p_sweep_shape(&s, n, h);
                        std::printf(" %d %d %lld %lld", int(f), int(q),
                                    (long long)(f ? p_flow_items(&s, n, ktot) : 0),
                                    (long long)(q ? p_sweep_items(&s, n, ktot) : 0));
                      }
                      std::printf("\n");
                    }
          // the dataflow sweep: its own knobs, over the record shapes its blocks come from
          for (int rs : {0, 1})
            for (int sw : {0, 4, 8, 12, 16})
              for (int sl : {2, 4})
                for (int sx : {0, 1})
                  for (int w : {1, 2})
                    for (int wf : {0, 3 - w})
                      for (int m : {5, 10, 20})
                        for (int mf : {-1, 0, 20})
                          for (int le : {2, 1}) {
                            if (!tune::waves(sw, np) || !tune::lane24(sl, np)) continue;
                            if (le == 1 && (m != 10 || mf != -1)) continue;
                            Shape s = b;
                            s.rec_sweep = rs, s.sweep_waves = sw, s.sweep_lane_elems = sl;
                            s.sweep_exchange = sx, s.rec_tile_width = w;
                            s.rec_tile_width_fwd = wf, s.rec_msteps = m, s.rec_msteps_fwd = mf;
                            s.rec_lane_elems = le;
                            const SweepShape z = sweep_shape(&s, 20);
                            std::printf("s %d %d %d %d %d %d %d %d %d | %d %d %d %d", rs, sw, sl,
                                        sx, w, wf, m, mf, le, z.waves, z.msf, z.msa,
                                        sweep_tile_elems(&s, z.waves));
                            for (int n : kNsteps) {
                              const SweepShape y = sweep_shape(&s, n);
                              std::printf(" %d %lld %lld", int(y.on),
                                          (long long)(y.on ? sweep_items(&s, y.waves, y.msf,
                                                                         y.msa, n) : 0),
                                          (long long)sweep_tiles_adj(&s, y.waves, y.msa));
                            }
                            std::printf("\n");
                          }
        }
}

int main(int argc, char** argv) {
  const char* mode = argc > 1 ? argv[1] : "";
  if (!std::strcmp(mode, "tune")) tune_mode();
  else if (!std::strcmp(mode, "env")) env_mode();
  else if (!std::strcmp(mode, "shapes")) shapes_mode();
  else return 2;
  return 0;
}
