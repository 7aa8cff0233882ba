// Stand-alone program (its own main; built with -fsanitize=address,undefined by tests/test_pnp_solve_host.py and run as
// an executable): ransac_host of csrc/pnp_solve.h on inputs at the edge of its domain must end, with poses that are
// finite or NaN (never Inf), counts in [0, n] and records within bounds, and without a sanitizer report.
// Exit status 0: every case did.
#include <cmath>
#include <cstdio>
#include <vector>

#include "pnp_solve.h"

using namespace msf::pnp;

struct Case {
  const char* name;
  std::vector<float> p3d, p2d;
  int min_inliers;
};

static const Cam kCam{500.0, 500.0, 320.0, 240.0};

// points in front of an identity camera and their exact projections
static Case make(const char* name, std::vector<float> p3d, int min_inliers) {
  Case c{name, p3d, {}, min_inliers};
  for (size_t i = 0; i < p3d.size() / 3; i++) {
    const float z = p3d[3 * i + 2];
    c.p2d.push_back((float)(kCam.uc + kCam.fu * p3d[3 * i] / z));
    c.p2d.push_back((float)(kCam.vc + kCam.fv * p3d[3 * i + 1] / z));
  }
  return c;
}

int main() {
  std::vector<Case> cases;
  cases.push_back(make("ordinary", {0, 0, 4, 1, 0, 5, 0, 1, 6, 1, 1, 3, -1, 0.5f, 4, 0.5f, -1, 7}, 4));
  cases.push_back(make("four coplanar points", {0, 0, 4, 1, 0, 4, 0, 1, 4, 1, 1, 4}, 4));
  cases.push_back(make("coplanar, six", {0, 0, 4, 1, 0, 4, 0, 1, 4, 1, 1, 4, 2, 1, 4, -1, 2, 4}, 4));
  cases.push_back(make("coincident points", {1, 1, 4, 1, 1, 4, 1, 1, 4, 1, 1, 4, 1, 1, 4}, 4));
  cases.push_back(make("two distinct points", {1, 1, 4, 1, 1, 4, 0, 0, 5, 0, 0, 5}, 4));
  cases.push_back(make("collinear points", {0, 0, 4, 1, 0, 4, 2, 0, 4, 3, 0, 4, 4, 0, 4}, 4));
  cases.push_back(make("n = 4, min_inliers = 4", {0, 0, 4, 1, 0, 5, 0, 1, 6, 1, 1, 3}, 4));
  Case centre = make("a point at the camera centre", {0, 0, 4, 1, 0, 5, 0, 1, 6, 1, 1, 3, 0, 0, 1}, 4);
  centre.p3d[12] = centre.p3d[13] = centre.p3d[14] = 0.0f;
  centre.p2d[8] = 320.0f, centre.p2d[9] = 240.0f;
  cases.push_back(centre);
  Case nan3 = cases[0], inf3 = cases[0], nan2 = cases[0], inf2 = cases[0], zeros = cases[0], huge = cases[0];
  nan3.name = "NaN in p3d", nan3.p3d[4] = NAN;
  inf3.name = "Inf in p3d", inf3.p3d[5] = INFINITY;
  nan2.name = "NaN in p2d", nan2.p2d[3] = NAN;
  inf2.name = "Inf in p2d", inf2.p2d[0] = -INFINITY;
  zeros.name = "all zero";
  for (float& x : zeros.p3d) x = 0.0f;
  for (float& x : zeros.p2d) x = 0.0f;
  huge.name = "FLT_MAX";
  huge.p3d[0] = 3.4e38f, huge.p2d[1] = 3.4e38f;
  for (const Case& c : {nan3, inf3, nan2, inf2, zeros, huge}) cases.push_back(c);

  int bad = 0;
  for (const Case& c : cases) {
    const int n = (int)c.p3d.size() / 3, its = 12, max_records = 2;
    std::vector<int32_t> counts(its, -7), sets(4 * its), iteration(max_records, -7), n_refined(max_records, -7);
    std::vector<double> pose(12 * its), rec_pose(12 * max_records, 0.0);
    std::vector<uint8_t> in_best((size_t)max_records * n, 9), in_refined((size_t)max_records * n, 9);
    std::vector<float> tcw(12 * max_records, 0.0f);
    HostOut o{};
    o.counts = counts.data(), o.sets = sets.data(), o.pose_f64 = pose.data(), o.iteration = iteration.data();
    o.n_refined = n_refined.data(), o.rec_pose_f64 = rec_pose.data(), o.inliers_best = in_best.data();
    o.inliers_refined = in_refined.data(), o.tcw_refined = tcw.data();
    const int records = ransac_host(n, c.p3d.data(), c.p2d.data(), kCam, 5.991f, c.min_inliers, its, max_records, 3, 0,
                                    nullptr, n, o);
    bool ok = records >= 0 && records <= its;
    int best = 0;
    for (int it = 0; it < its; it++) {
      ok = ok && counts[it] >= 0 && counts[it] <= n;
      best = counts[it] > best ? counts[it] : best;
      for (int k = 0; k < 12; k++) ok = ok && !std::isinf(pose[12 * it + k]);
      for (int k = 0; k < 4; k++) ok = ok && sets[4 * it + k] >= 0 && sets[4 * it + k] < n;
    }
    for (int r = 0; r < records && r < max_records; r++) {
      ok = ok && iteration[r] >= 0 && iteration[r] < its && n_refined[r] >= 0 && n_refined[r] <= n;
      for (int k = 0; k < 12; k++) ok = ok && !std::isinf(rec_pose[12 * r + k]);
      for (int i = 0; i < n; i++) ok = ok && in_best[(size_t)r * n + i] <= 1 && in_refined[(size_t)r * n + i] <= 1;
    }
    if (c.name == cases[0].name) ok = ok && best == n && records >= 1;   // the ordinary case is solved
    std::printf("%-30s n %d records %d best count %d%s\n", c.name, n, records, best, ok ? "" : "  <-- BAD");
    bad += ok ? 0 : 1;
  }
  return bad ? 1 : 0;
}
