// Stand-alone program (its own main; built with -fsanitize=address,undefined by tests/test_new_points_host.py and run
// as an executable): new_point of csrc/triangulate_solve.h on inputs at the edge of its domain must end, with a status
// in 0..7 and without a sanitizer report.  Exit status 0: every case did.
#include <climits>
#include <cmath>
#include <cstdio>
#include <initializer_list>

#include "triangulate_solve.h"

using namespace msf::triangulate;

static View view(float tx) {
  View v{};
  v.Rcw[0] = v.Rcw[4] = v.Rcw[8] = 1.0f;
  v.tcw[0] = tx;
  v.fx = v.fy = 500.0f;
  v.cx = 320.0f;
  v.cy = 240.0f;
  return v;
}

int main() {
  const Match inside{370, 240, 270, 240}, centre{320, 240, 320, 240};
  const Match huge{INT_MAX, INT_MAX, INT_MIN, INT_MIN}, huge_same{INT_MAX, INT_MAX, INT_MAX, INT_MAX};
  View nan_pose = view(-1.0f), nan_t = view(-1.0f), inf_pose = view(-1.0f), zero{};
  nan_pose.Rcw[4] = NAN;
  nan_t.tcw[2] = NAN;
  inf_pose.Rcw[0] = INFINITY;
  struct Case { const char* name; View a, b; Match m; int expect; };   // expect < 0: any status
  const Case cases[] = {
      {"ordinary", view(0.0f), view(-1.0f), inside, kNewPoint},
      {"identical views", view(0.0f), view(0.0f), inside, -1},
      {"identical views, same pixel", view(0.0f), view(0.0f), centre, -1},
      {"parallel rays", view(0.0f), view(-1.0f), centre, kNoPoint},
      {"NaN in Rcw", view(0.0f), nan_pose, inside, -1},
      {"NaN in tcw", view(0.0f), nan_t, inside, kNoPoint},
      {"Inf in Rcw", view(0.0f), inf_pose, inside, -1},
      {"all-zero views", zero, zero, inside, kCosNotPositive},
      {"INT32 extremes", view(0.0f), view(-1.0f), huge, -1},
      {"INT32_MAX twice", view(0.0f), view(-1.0f), huge_same, -1},
  };
  int bad = 0;
  for (const Case& c : cases) {
    for (double max_cos : {1.1, 0.9998, 0.0}) {
      float x3d[3], hom[4];
      double cos = 0.0;
      const int s = new_point(c.m, c.a, c.b, max_cos, 5.991, x3d, hom, &cos);
      const bool zero_point = x3d[0] == 0.0f && x3d[1] == 0.0f && x3d[2] == 0.0f;
      const bool finite_point = std::isfinite(x3d[0]) && std::isfinite(x3d[1]) && std::isfinite(x3d[2]);
      const bool ok = s >= 0 && s <= 7 && (s == kNewPoint ? finite_point : zero_point) &&
                      (c.expect < 0 || max_cos != 1.1 || s == c.expect);
      std::printf("%-28s max_cos %-6g status %d cos %g%s\n", c.name, max_cos, s, cos, ok ? "" : "  <-- BAD");
      bad += ok ? 0 : 1;
    }
  }
  return bad ? 1 : 0;
}
