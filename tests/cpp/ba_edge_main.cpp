// Stand-alone program (its own main; built with -fsanitize=address,undefined by tests/test_ba_edge_host.py and run as
// an executable): bundle_adjust of csrc/ba_solve.h on problems at the edge of its domain must end, with a status in its
// range, estimates without Inf, flags of 0 or 1, iteration and trial counts within their bounds, fixed cameras as they
// came, and without a sanitizer report.  The scratch is exactly what ba::layout() asks for, so a write beyond a piece
// is a heap overflow the sanitizer sees.  Exit status 0: every case did.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "ba_solve.h"

using namespace msf::ba;

struct Case {
  std::string name;
  std::vector<float> tcw;
  std::vector<uint8_t> fixed;
  std::vector<float> pts;
  std::vector<int32_t> ec, ep;
  std::vector<float> obs;
  int32_t stop = 0;
  int expect = 2;   // the status
};

static const Cam kCam{500.0, 500.0, 320.0, 240.0};

// n_cams cameras side by side looking down z, the first n_fixed fixed, n_points points in front of them, every point
// seen by `per` cameras with its exact pixels truncated; the free cameras start a little off
static Case make(const std::string& name, int n_cams, int n_fixed, int n_points, int per) {
  Case c;
  c.name = name;
  for (int k = 0; k < n_cams; k++) {
    const float off = k < n_fixed ? 0.0f : 0.02f;
    const float t[12] = {1, 0, 0, -0.25f * (float)k + off, 0, 1, 0, off, 0, 0, 1, -off};
    c.tcw.insert(c.tcw.end(), t, t + 12);
    c.fixed.push_back(k < n_fixed ? 1 : 0);
  }
  for (int i = 0; i < n_points; i++) {
    const float x = (float)((i * 37) % 11 - 5) * 0.4f, y = (float)((i * 53) % 7 - 3) * 0.5f, z = 4.0f + (float)((i * 29) % 13) * 0.5f;
    c.pts.insert(c.pts.end(), {x * 1.01f, y * 0.99f, z * 1.01f});
    for (int j = 0; j < per && j < n_cams; j++) {
      const int cam = (i + j * 7) % n_cams;
      bool seen = false;
      for (size_t e = c.ec.size(); e-- > 0 && c.ep[e] == i;) seen = seen || c.ec[e] == cam;
      if (seen) continue;
      c.ec.push_back(cam), c.ep.push_back(i);
      c.obs.push_back(std::floor((float)kCam.uc + (float)kCam.fu * (x - 0.25f * (float)cam) / z));
      c.obs.push_back(std::floor((float)kCam.vc + (float)kCam.fv * y / z));
    }
  }
  return c;
}

int main() {
  std::vector<Case> cases;
  cases.push_back(make("base 4 + 2 x 60", 6, 2, 60, 4));
  Case no_edges = make("0 edges", 4, 1, 20, 0);
  cases.push_back(no_edges);
  cases.push_back(make("0 free cameras", 3, 3, 30, 3));
  cases.push_back(make("every point with one edge", 4, 1, 40, 1));
  Case lonely = make("a camera with no edge", 5, 1, 40, 3);
  for (size_t e = 0; e < lonely.ec.size(); e++)
    if (lonely.ec[e] == 4) lonely.ec[e] = 3;
  cases.push_back(lonely);
  cases.push_back(make("no fixed camera (free gauge)", 5, 0, 50, 4));
  Case all_flagged = make("every edge flagged after round 0", 4, 2, 40, 3);
  for (size_t e = 0; e < all_flagged.ec.size(); e++)
    all_flagged.obs[2 * e] = (float)((e * 97) % 640), all_flagged.obs[2 * e + 1] = (float)((e * 61) % 480);
  cases.push_back(all_flagged);
  Case behind = make("points at Z <= 0", 4, 2, 40, 3);
  behind.pts[2] = 0.0f, behind.pts[5] = -3.0f, behind.pts[8] = -0.01f;
  cases.push_back(behind);
  Case nan_point = make("NaN in a point, a pose and a pixel", 4, 2, 40, 3);
  nan_point.pts[4] = NAN, nan_point.tcw[3 * 12 + 5] = NAN, nan_point.obs[9] = NAN;
  cases.push_back(nan_point);
  cases.push_back(make("64 free cameras", 66, 2, 200, 4));
  Case many = make("65 free cameras", 67, 2, 200, 4);
  many.expect = -1;
  cases.push_back(many);
  Case stopped = make("a stop word set from the start", 6, 2, 60, 4);
  stopped.stop = 1, stopped.expect = 0;
  cases.push_back(stopped);
  Case bad_index = make("an edge index out of range", 6, 2, 60, 4);
  bad_index.ec[11] = 6, bad_index.expect = -1;
  cases.push_back(bad_index);
  Case unsorted = make("edge_point decreasing", 6, 2, 60, 4);
  unsorted.ep[20] = 0, unsorted.expect = -1;
  cases.push_back(unsorted);

  const Params prm{kCam, 2, {5, 10}, {1, 0}, 5.991, 5.991};
  int bad = 0;
  {
    // The pieces of two problems whose descriptors come in another order than their ranges (problem 0 at cameras
    // 10..14 and points 10..19, problem 1 at cameras 0..9 and points 0..9) are disjoint: an integer array over cameras
    // or points has one row per camera or point and nothing more, and the per-problem words differ.
    msf::Carver measure;
    layout(measure, 2, 15, 20, 30, 4);
    std::vector<uint8_t> block(measure.off + 1);
    msf::Carver place{block.data()};
    const Scratch all = layout(place, 2, 15, 20, 30, 4);
    const Scratch a = piece(all, 0, 10, 10, 20), b = piece(all, 1, 0, 0, 0);
    bool ok = a.cam_start == b.cam_start + 10 && a.cam_end == b.cam_end + 10 && a.cam_active == b.cam_active + 10 &&
              a.free_of == b.free_of + 10 && a.free_cam == b.free_cam + 10 && a.pt_start == b.pt_start + 10 &&
              a.pt_end == b.pt_end + 10 && a.pt_active == b.pt_active + 10 && a.word + 1 == b.word;
    ok = ok && (uint8_t*)(all.cam_start + 15) <= (uint8_t*)all.cam_end && (uint8_t*)(all.pt_start + 20) <= (uint8_t*)all.pt_active;
    std::printf("%-40s%s\n", "pieces of permuted descriptors", ok ? "" : "  <-- BAD");
    bad += ok ? 0 : 1;
  }
  for (const Case& c : cases) {
    const int nc = (int)c.fixed.size(), np = (int)c.pts.size() / 3, ne = (int)c.ec.size();
    int n_free = 0;
    for (uint8_t f : c.fixed) n_free += f == 0;
    const int max_free = c.expect == -1 && n_free > kMaxFreeCams ? kMaxFreeCams : (n_free > 0 ? n_free : 1);
    msf::Carver measure;
    layout(measure, 1, nc, np, ne, max_free);
    uint8_t* block = (uint8_t*)std::malloc(measure.off ? measure.off : 1);   // exactly: the sanitizer guards its end
    msf::Carver place{block};
    const Scratch w = layout(place, 1, nc, np, ne, max_free);
    int32_t status = -7;
    std::vector<float> tcw(nc * 12, 9.0f), pts(np * 3, 9.0f);
    std::vector<uint8_t> flags(ne, 9), round_flags(ne * 2, 9);
    std::vector<double> pose(nc * 12, 9.0), pts64(np * 3, 9.0);
    std::vector<int32_t> round_its(2, -7), trials(kSlots, -7);
    std::vector<double> lam_in(kSlots), lam_out(kSlots), cost_in(kSlots), cost_out(kSlots);
    std::vector<double> cam_in(kSlots * nc * 7), cam_out(kSlots * nc * 7), pt_in(kSlots * np * 3), pt_out(kSlots * np * 3);
    std::vector<double> Hcc(kSlots * nc * 21), bc(kSlots * nc * 6), Hpp(kSlots * np * 6), bp(kSlots * np * 3);
    const Out o{&status,        tcw.data(),     pts.data(),      flags.data(),    pose.data(),    pts64.data(),  round_flags.data(),
                round_its.data(), trials.data(), lam_in.data(),  lam_out.data(),  cost_in.data(), cost_out.data(), cam_in.data(),
                pt_in.data(),   cam_out.data(), pt_out.data(),   Hcc.data(),      bc.data(),      Hpp.data(),    bp.data()};
    const Problem p{nc, np, ne, c.tcw.data(), c.fixed.data(), c.pts.data(), c.ec.data(), c.ep.data(), c.obs.data()};
    status = bundle_adjust(Serial(), p, prm, &c.stop, w, o);
    std::free(block);
    bool ok = status == c.expect;
    if (status == -1) {   // nothing else is written
      for (float x : tcw) ok = ok && x == 9.0f;
      for (uint8_t f : flags) ok = ok && f == 9;
      for (int32_t t : trials) ok = ok && t == -7;
    } else {
      for (int k = 0; k < nc * 12; k++) {
        ok = ok && !std::isinf(pose[k]) && !std::isinf(tcw[k]);
        if (c.fixed[k / 12] || status == 0) ok = ok && (tcw[k] == c.tcw[k] || (std::isnan(tcw[k]) && std::isnan(c.tcw[k])));
      }
      for (int k = 0; k < np * 3; k++) ok = ok && !std::isinf(pts64[k]) && (pts[k] == (float)pts64[k] || std::isnan(pts64[k]));
      for (int e = 0; e < ne; e++) {
        ok = ok && flags[e] <= 1;
        for (int r = 0; r < 2; r++) ok = ok && (r < status ? round_flags[2 * e + r] <= 1 : round_flags[2 * e + r] == 9);
        if (status > 0) ok = ok && flags[e] == round_flags[2 * e + status - 1];
      }
      for (int r = 0; r < 2; r++) {
        ok = ok && round_its[r] >= 0 && round_its[r] <= prm.iterations[r];
        if (r >= status) ok = ok && round_its[r] == 0;
        for (int it = 0; it < kMaxIterations; it++) {
          const int t = trials[r * kMaxIterations + it];
          ok = ok && (it < round_its[r] ? t >= 1 && t <= kTrials : t == 0);
        }
      }
      if (c.name == "base 4 + 2 x 60" || c.name == "64 free cameras") {
        int flagged = 0;
        for (uint8_t f : flags) flagged += f;
        ok = ok && flagged == 0 && cost_out[kMaxIterations + round_its[1] - 1] < cost_in[0];
        for (int k = 0; k < nc; k++) ok = ok && std::fabs(pose[12 * k + 7]) < 0.01;   // the 0.02 offset in y is taken back
      }
      if (c.name == "every edge flagged after round 0") {
        int flagged = 0;
        for (uint8_t f : flags) flagged += f;
        ok = ok && flagged >= ne - 2;
      }
      if (c.name == "0 edges") ok = ok && round_its[0] == 1 && trials[0] == 1;
    }
    std::printf("%-40s cams %d points %d edges %d status %d iterations %d %d%s\n", c.name.c_str(), nc, np, ne, status, round_its[0],
                round_its[1], ok ? "" : "  <-- BAD");
    bad += ok ? 0 : 1;
  }
  return bad ? 1 : 0;
}
