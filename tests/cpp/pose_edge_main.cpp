// Stand-alone program (its own main; built with -fsanitize=address,undefined by tests/test_pose_solve_host.py and run
// as an executable): optimize_host of csrc/pose_solve.h on inputs at the edge of its domain must end, with n_good in
// [0, n_edges], a pose without Inf, flags of 0 or 1 at the edges and untouched bytes elsewhere, iteration and trial
// counts within their bounds, and without a sanitizer report.  Exit status 0: every case did.
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "pose_solve.h"

using namespace msf::pose;

struct Case {
  std::string name;
  std::vector<float> p3d, p2d;
  std::vector<uint8_t> mask;   // empty: no mask
  float tcw0[12];
};

static const Cam kCam{500.0, 500.0, 320.0, 240.0};

// n points in front of an identity camera, their exact projections, and an entry pose shifted a little
static Case make(const std::string& name, int n) {
  Case c{name, {}, {}, {}, {1, 0, 0, 0.05f, 0, 1, 0, -0.03f, 0, 0, 1, 0.02f}};
  for (int i = 0; i < n; i++) {
    const float x = (float)((i * 37) % 11 - 5) * 0.4f, y = (float)((i * 53) % 7 - 3) * 0.5f, z = 3.0f + (float)((i * 29) % 13) * 0.5f;
    c.p3d.insert(c.p3d.end(), {x, y, z});
    c.p2d.push_back((float)std::floor(kCam.uc + kCam.fu * x / z));
    c.p2d.push_back((float)std::floor(kCam.vc + kCam.fv * y / z));
  }
  return c;
}

int main() {
  std::vector<Case> cases;
  for (int n : {0, 2, 3, 9, 10, 40}) cases.push_back(make("n = " + std::to_string(n), n));
  Case plane = make("points on the camera plane", 12), behind = make("points behind the camera", 12);
  for (int i = 0; i < 12; i++) plane.p3d[3 * i + 2] = -0.02f, behind.p3d[3 * i + 2] = -4.0f - (float)i;
  Case some = make("some points on and behind the plane", 20);
  some.p3d[2] = -0.02f, some.p3d[5] = -3.0f, some.p3d[8] = 0.0f;
  Case same = make("all points identical", 15);
  for (int i = 0; i < 15; i++)
    for (int k = 0; k < 3; k++) same.p3d[3 * i + k] = same.p3d[k];
  for (int i = 0; i < 15; i++)
    for (int k = 0; k < 2; k++) same.p2d[2 * i + k] = same.p2d[k];
  Case nan_pose = make("a NaN pose", 20), zero_pose = make("an all-zero pose", 20);
  nan_pose.tcw0[5] = NAN;
  for (float& x : zero_pose.tcw0) x = 0.0f;
  Case no_mask = make("an all-zero mask", 20), third = make("every third masked out", 40), few = make("a mask that leaves 2", 20);
  no_mask.mask.assign(20, 0);
  for (int i = 0; i < 40; i++) third.mask.push_back(i % 3 ? 1 : 0);
  few.mask.assign(20, 0), few.mask[4] = 1, few.mask[17] = 255;
  Case nan_point = make("NaN in p3d and p2d", 20), outliers = make("half the pixels wrong", 40);
  nan_point.p3d[4] = NAN, nan_point.p2d[9] = NAN;
  for (int i = 0; i < 40; i += 2) outliers.p2d[2 * i] = (float)((i * 97) % 640), outliers.p2d[2 * i + 1] = (float)((i * 61) % 480);
  for (const Case& c : {plane, behind, some, same, nan_pose, zero_pose, no_mask, third, few, nan_point, outliers})
    cases.push_back(c);

  int bad = 0;
  for (const Case& c : cases) {
    for (int emu = 0; emu < 2; emu++) {
      const int n = (int)c.p3d.size() / 3;
      int32_t n_edges = -7, rounds_run = -7;
      float tcw[12];
      double pose[12];
      std::vector<uint8_t> flags(n, 9);
      std::vector<int32_t> trials(40, -7), round_its(4, -7), round_bad(4, -7);
      std::vector<double> round_pose(48, 0.0), lam_in(40), lam_out(40), cost_in(40), cost_out(40), H(40 * 21), b(40 * 6), est(40 * 7);
      HostOut o{&n_edges, &rounds_run, tcw, pose, flags.data(),
                Trace{round_pose.data(), round_bad.data(), round_its.data(), trials.data(), lam_in.data(), lam_out.data(),
                      cost_in.data(), cost_out.data(), H.data(), b.data(), est.data(), true}};
      const uint8_t* mask = c.mask.empty() ? nullptr : c.mask.data();
      const int good = emu ? optimize_host(msf::pnp::Emu64(), n, c.p3d.data(), c.p2d.data(), mask, kCam, 5.991f, c.tcw0, o)
                           : optimize_host(msf::pnp::Serial(), n, c.p3d.data(), c.p2d.data(), mask, kCam, 5.991f, c.tcw0, o);
      int edges = 0;
      for (int i = 0; i < n; i++) edges += !mask || mask[i];
      bool ok = n_edges == edges && good >= 0 && good <= edges;
      ok = ok && rounds_run == (edges < 3 ? 0 : edges < 10 ? 1 : 4);
      if (rounds_run == 0) ok = ok && good == 0;
      int flagged_edges = 0;
      for (int i = 0; i < n; i++) {
        const bool edge = !mask || mask[i];
        ok = ok && (edge ? flags[i] <= 1 : flags[i] == 9);
        flagged_edges += edge && flags[i] == 1;
      }
      if (rounds_run) ok = ok && good == edges - flagged_edges;
      for (int k = 0; k < 12; k++) ok = ok && !std::isinf(pose[k]) && !std::isinf(tcw[k]);
      for (int r = 0; r < 4; r++) {
        ok = ok && round_its[r] >= 0 && round_its[r] <= 10 && round_bad[r] >= 0 && round_bad[r] <= edges;
        if (r >= rounds_run) ok = ok && round_its[r] == 0;
        for (int it = 0; it < 10; it++) {
          const int t = trials[r * 10 + it];
          ok = ok && (it < round_its[r] ? t >= 1 && t <= 10 : t == 0);
        }
      }
      if (c.name == "n = 40") ok = ok && good == 40 && std::fabs(pose[3]) < 0.01 && std::fabs(pose[11]) < 0.02;
      if (c.name == "half the pixels wrong") ok = ok && good >= 20 && good <= 22;
      std::printf("%-36s %s n %d edges %d rounds %d good %d iterations %d %d %d %d%s\n", c.name.c_str(), emu ? "emu64 " : "serial",
                  n, n_edges, rounds_run, good, round_its[0], round_its[1], round_its[2], round_its[3], ok ? "" : "  <-- BAD");
      bad += ok ? 0 : 1;
    }
  }
  return bad ? 1 : 0;
}
