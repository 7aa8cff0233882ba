// Stand-alone program for tests/test_tracking_solve_host.py, built with -fsanitize=address,undefined: the family's
// layout (tracking::layout over plain memory) and the host build of the five steps of csrc/tracking_solve.h on the
// empty, one-element and malformed inputs of the refusal list of include/msf_tracking.h.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "tracking_solve.h"

using namespace msf::tracking;

static int failures = 0;
#define EXPECT(c)                                                 \
  do {                                                            \
    if (!(c)) {                                                   \
      std::printf("line %d: %s does not hold\n", __LINE__, #c);   \
      failures++;                                                 \
    }                                                             \
  } while (0)

static const int W = 64, H = 48;

static Frustum camera() {
  Frustum f{};
  f.view.Rcw[0] = f.view.Rcw[4] = f.view.Rcw[8] = 1.0f;
  f.view.fx = f.view.fy = 50.0f, f.view.cx = 32.0f, f.view.cy = 24.0f;
  f.min_x = 0.0f, f.max_x = (float)W, f.min_y = 0.0f, f.max_y = (float)H, f.cos_limit = 0.5f;
  return f;
}

// runs the layout over plain memory and the five steps on a checked map; returns n_claims
static int run(const Map& m, const std::vector<Match>& matches, int cap, const std::vector<int32_t>& n_out,
               const std::vector<uint8_t>& matched, int corr_cap, std::vector<int32_t>* n_to_match, std::vector<uint8_t>* status,
               int32_t* n_corr) {
  Scratch s;
  msf::Carver measure;
  layout(measure, m.n_points, m.n_kf, (size_t)W * H, cap, &s);
  std::vector<uint8_t> block(measure.off + 1, 0);
  msf::Carver place{block.data()};
  layout(place, m.n_points, m.n_kf, (size_t)W * H, cap, &s);
  EXPECT(place.off == measure.off && s.zeroed_bytes <= measure.off);
  n_to_match->assign((size_t)m.n_kf + 1, -5);
  status->assign((size_t)m.n_points + 1, 77);
  std::vector<float> diag(4 * ((size_t)m.n_points + 1));
  const Frustum f = camera();
  host_frustum(m, f, reinterpret_cast<int32_t*>(s.owner), n_to_match->data(), status->data(), nullptr, nullptr,
               diag.data(), nullptr, nullptr, nullptr);
  for (int p = 0; p < m.n_points; p++) s.owner[p] = 0;
  std::vector<int32_t> n_claimed((size_t)m.n_kf + 1, -5), corr_point((size_t)corr_cap + 1);
  std::vector<float> p3d(3 * ((size_t)corr_cap + 1)), p2d(2 * ((size_t)corr_cap + 1));
  std::vector<uint8_t> claim_status((size_t)m.n_kf * cap + 1, 255);
  const int n = host_claims(m, W, H, matches.data(), cap, n_out.data(), matched.data(), s.pixel_word, n_claimed.data(),
                            s.rows, claim_status.data(), corr_cap, n_corr, p3d.data(), p2d.data(), corr_point.data());
  for (size_t k = 0; k < (size_t)W * H; k++) EXPECT(s.pixel_word[k] == 0);
  EXPECT((*status)[m.n_points] == 77 && (*n_to_match)[m.n_kf] == -5 && n_claimed[m.n_kf] == -5);
  return n;
}

int main() {
  std::vector<int32_t> ntm;
  std::vector<uint8_t> st;
  int32_t n_corr = 0;
  {   // nothing at all
    const Map m{0, 0, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    EXPECT(map_fault(m, W, H) == nullptr);
    EXPECT(run(m, {}, 1, {}, {}, 0, &ntm, &st, &n_corr) == 0 && n_corr == 0);
  }
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
  // one point in front of the camera, seen head-on, and its variations
  std::vector<Point> pts(6, Point{{0.0f, 0.0f, 4.0f}, {0.0f, 0.0f, 1.0f}, 10.0f, 0u});
  pts[1].pos[2] = nan, pts[2].pos[0] = inf, pts[3].pos[2] = 0.0f, pts[4].pos[2] = -0.0f, pts[5].flags = kBad | kSeen;
  std::vector<int32_t> start{0, 6, 6}, key{0, 1, 2, 3, 4, W * H - 1}, point{0, 1, 2, 3, 4, 5}, ckey{7}, cpoint{0};
  {   // one key frame with entries, one without; one list of one match
    const Map m{6, 2, 6, 1, pts.data(), start.data(), key.data(), point.data(), ckey.data(), cpoint.data()};
    EXPECT(map_fault(m, W, H) == nullptr);
    const std::vector<Match> matches{{5, 0, 0, 0}, {0, 0, 0, 0}};
    EXPECT(run(m, matches, 1, {1, 1}, {1, 0}, 2, &ntm, &st, &n_corr) == 1 && n_corr == 2);
    EXPECT(ntm[0] == 1 && ntm[1] == 0);
    EXPECT(st[0] == kVisible && st[1] == kNotFinite && st[2] == kNotFinite && st[3] == kNotFinite && st[4] == kNotFinite && st[5] == kIsBad);
    EXPECT(run(m, matches, 1, {1, 1}, {1, 0}, 1, &ntm, &st, &n_corr) == 1 && n_corr == -1);
    EXPECT(run(m, matches, 1, {-1, 5}, {1, 1}, 8, &ntm, &st, &n_corr) == 0 && n_corr == 1);   // invalid, then clipped: k2 has no entry
  }
  {   // the refusal list
    Map m{6, 2, 6, 1, pts.data(), start.data(), key.data(), point.data(), ckey.data(), cpoint.data()};
    Map neg = m; neg.n_cur = -1;
    EXPECT(map_fault(neg, W, H));
    Map missing = m; missing.kf_key = nullptr;
    EXPECT(map_fault(missing, W, H));
    std::vector<int32_t> s2{0, 7, 6}, s3{1, 6, 6}, s4{0, 6, 5}, k2{0, 1, 1, 3, 4, 5}, k3{0, 1, 2, 3, 4, W * H}, p2{0, 1, 2, 3, 4, 6},
        p3{-1, 1, 2, 3, 4, 5}, ck{-1}, cp{6};
    for (const std::vector<int32_t>* s : {&s2, &s3, &s4}) { Map b = m; b.kf_start = s->data(); EXPECT(map_fault(b, W, H)); }
    for (const std::vector<int32_t>* k : {&k2, &k3}) { Map b = m; b.kf_key = k->data(); EXPECT(map_fault(b, W, H)); }
    for (const std::vector<int32_t>* p : {&p2, &p3}) { Map b = m; b.kf_point = p->data(); EXPECT(map_fault(b, W, H)); }
    { Map b = m; b.cur_key = ck.data(); EXPECT(map_fault(b, W, H)); }
    { Map b = m; b.cur_point = cp.data(); EXPECT(map_fault(b, W, H)); }
    { Map b = m; b.n_kf = 0; EXPECT(map_fault(b, W, H)); }
    std::vector<Point> flagged = pts; flagged[2].flags = 4u;
    { Map b = m; b.points = flagged.data(); EXPECT(map_fault(b, W, H)); }
    Frustum f = camera(); f.min_y = nan;
    EXPECT(frustum_fault(f) && !frustum_fault(camera()));
  }
  // the searches on nothing and on one element, and keys at the ends of int32
  const int32_t one[1] = {5};
  EXPECT(find_key(one, 0, 0, 5) == -1 && find_key(one, 0, 1, 5) == 0 && find_key(one, 0, 1, 2147483647) == -1 && find_key(one, 0, 1, -2147483647 - 1) == -1);
  EXPECT(pixel_key(2147483647, 0, W, H) == -1 && pixel_key(0, -2147483647 - 1, W, H) == -1 && pixel_key(W - 1, H - 1, W, H) == W * H - 1);
  std::printf(failures ? "tracking_edge: %d failure(s)\n" : "tracking_edge: ok\n", failures);
  return failures ? 1 : 0;
}
