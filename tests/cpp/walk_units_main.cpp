// csrc/orb_plan.h, walk_unit / walk_grid: the unit order of a walker launch (k_walk) in a stand-alone executable
// (tests/test_walk_units_host.py), never inside python.
//   walk_units W H MAX_SLOTS N      for a W x H plan and a call of N frames, every launch form the pipeline uses -- all
//                                   levels in one launch without finish units and with them in either placement, and one
//                                   launch per level --: the grid decodes onto every unit exactly once, surplus indices
//                                   decode to "none", and every dependency of a unit has a lower workgroup index:
//                                     threshold (f, l)  <- all strips of (f, l - 1)         (same launch only)
//                                     strip (f, l)      <- threshold (f, l)
//                                     non-quarter strip <- the sampled quarter of (f, l)
//                                     finish (f, l)     <- all strips of (f, l)
//                                   one line to stdout, failures to stderr and the exit status
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "orb_plan.h"

using namespace msf;

namespace {

int failures = 0;

#define CHECK(cond, ...)                                                      \
  do {                                                                        \
    if (!(cond)) {                                                            \
      if (failures < 50) {                                                    \
        std::fprintf(stderr, "line %d: %s does not hold: ", __LINE__, #cond); \
        std::fprintf(stderr, __VA_ARGS__);                                    \
        std::fprintf(stderr, "\n");                                           \
      }                                                                       \
      failures++;                                                             \
    }                                                                         \
  } while (0)

// units of one launch; returns the number of workgroups without a unit
long long check_launch(const OrbGeometry& g, int l_lo, int l_hi, int n, int finish) {
  const long long grid = walk_grid(g, l_lo, l_hi, n, finish);
  const int nl = l_hi - l_lo + 1;
  // workgroup index of every unit, -1 = not seen yet
  std::vector<long long> thr((size_t)n * nl, -1), fin((size_t)n * nl, -1);
  std::vector<std::vector<long long>> strip((size_t)n * nl);
  for (int f = 0; f < n; f++)
    for (int l = l_lo; l <= l_hi; l++) strip[(size_t)f * nl + (l - l_lo)].assign((size_t)g.lv[l].wk_nx * g.lv[l].wk_ny, -1);
  long long none = 0;
  for (long long wg = 0; wg < grid; wg++) {
    const WalkUnit u = walk_unit(g, l_lo, l_hi, n, finish, (unsigned)wg);
    if (u.kind == kWalkNone) {
      none++;
      continue;
    }
    CHECK(u.kind == kWalkThreshold || u.kind == kWalkStrip || u.kind == kWalkFinish, "wg %lld kind %d", wg, u.kind);
    CHECK(u.level >= l_lo && u.level <= l_hi && u.frame >= 0 && u.frame < n, "wg %lld level %d frame %d", wg, u.level, u.frame);
    if (u.level < l_lo || u.level > l_hi || u.frame < 0 || u.frame >= n) continue;
    const size_t at = (size_t)u.frame * nl + (u.level - l_lo);
    if (u.kind == kWalkThreshold) {
      CHECK(thr[at] < 0, "threshold unit (%d, %d) twice: %lld and %lld", u.frame, u.level, thr[at], wg);
      thr[at] = wg;
    } else if (u.kind == kWalkFinish) {
      CHECK(finish != kWalkFinishOff, "a finish unit at wg %lld of a launch without them", wg);
      CHECK(fin[at] < 0, "finish unit (%d, %d) twice: %lld and %lld", u.frame, u.level, fin[at], wg);
      fin[at] = wg;
    } else {
      CHECK(u.strip >= 0 && (size_t)u.strip < strip[at].size(), "wg %lld strip %d of %zu", wg, u.strip, strip[at].size());
      if (u.strip < 0 || (size_t)u.strip >= strip[at].size()) continue;
      CHECK(strip[at][u.strip] < 0, "strip %d of (%d, %d) twice: %lld and %lld", u.strip, u.frame, u.level, strip[at][u.strip], wg);
      strip[at][u.strip] = wg;
    }
  }
  // an index past the grid never names a unit
  for (long long wg = grid; wg < grid + 64; wg++)
    CHECK(walk_unit(g, l_lo, l_hi, n, finish, (unsigned)wg).kind == kWalkNone, "wg %lld past the grid of %lld", wg, grid);
  long long units = 0;
  for (int f = 0; f < n; f++)
    for (int l = l_lo; l <= l_hi; l++) {
      const size_t at = (size_t)f * nl + (l - l_lo);
      const long long t = thr[at];
      CHECK(t >= 0, "no threshold unit (%d, %d)", f, l);
      units++;
      long long last_strip = -1, last_quarter = -1;
      for (size_t s = 0; s < strip[at].size(); s++) {
        const long long w = strip[at][s];
        CHECK(w >= 0, "no strip %zu of (%d, %d)", s, f, l);
        units++;
        CHECK(w > t, "strip %zu of (%d, %d) at %lld, its threshold unit at %lld", s, f, l, w, t);
        if (w > last_strip) last_strip = w;
        if (s % 4 == 0 && w > last_quarter) last_quarter = w;
      }
      for (size_t s = 0; s < strip[at].size(); s++)
        if (s % 4 != 0)
          CHECK(strip[at][s] > last_quarter, "strip %zu of (%d, %d) at %lld, a quarter strip at %lld", s, f, l, strip[at][s], last_quarter);
      if (l > l_lo) {
        const size_t up = at - 1;
        for (size_t s = 0; s < strip[up].size(); s++)
          CHECK(strip[up][s] < t, "threshold unit (%d, %d) at %lld, strip %zu of the level above at %lld", f, l, t, s, strip[up][s]);
      }
      if (finish != kWalkFinishOff) {
        CHECK(fin[at] >= 0, "no finish unit (%d, %d)", f, l);
        units++;
        CHECK(fin[at] > last_strip, "finish unit (%d, %d) at %lld, a strip of its level at %lld", f, l, fin[at], last_strip);
      } else {
        CHECK(fin[at] < 0, "a finish unit (%d, %d)", f, l);
      }
    }
  CHECK(units + none == grid, "%lld units + %lld none != grid %lld", units, none, grid);
  // surplus: XCDs with one frame fewer than ceil(n / 8)
  const long long per_frame = grid / (8ll * ((n + 7) / 8));
  CHECK(none == (8ll * ((n + 7) / 8) - n) * per_frame, "%lld workgroups without a unit", none);
  return none;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 5) {
    std::fprintf(stderr, "usage: walk_units W H MAX_SLOTS N\n");
    return 2;
  }
  OrbPlanRequest rq;
  rq.width = std::atoi(argv[1]);
  rq.height = std::atoi(argv[2]);
  rq.max_slots = std::atoi(argv[3]);
  const int n = std::atoi(argv[4]);
  OrbPlan plan;
  const std::string err = plan_orb(rq, &plan);
  if (!err.empty() || n < 1) {
    std::fprintf(stderr, "plan: %s\n", err.c_str());
    return 2;
  }
  const OrbGeometry& g = plan.g;
  long long none = 0, grids = 0;
  const int finishes[3] = {kWalkFinishOff, kWalkFinishThr, kWalkFinishQuarter};
  for (int finish : finishes) {
    none += check_launch(g, 0, g.nlevels - 1, n, finish);
    grids += walk_grid(g, 0, g.nlevels - 1, n, finish);
  }
  for (int l = 0; l < g.nlevels; l++) {     // the per-level form: no finish units
    none += check_launch(g, l, l, n, kWalkFinishOff);
    grids += walk_grid(g, l, l, n, kWalkFinishOff);
  }
  // without finish units the grid is what the kernel's own loop held before the order moved into the header
  CHECK(walk_grid(g, 0, g.nlevels - 1, n, kWalkFinishOff) == 8ll * ((n + 7) / 8) * (g.nlevels + g.total_strips),
        "grid without finish units");
  CHECK(walk_grid(g, 0, g.nlevels - 1, n, kWalkFinishThr) == 8ll * ((n + 7) / 8) * (2 * g.nlevels + g.total_strips),
        "grid with finish units");
  std::printf("walk_units %d x %d n=%d: strips=%d workgroups=%lld none=%lld failures=%d\n", rq.width, rq.height, n,
              g.total_strips, grids, none, failures);
  return failures ? 1 : 0;
}
