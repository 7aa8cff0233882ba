// csrc/frame_tracking_solve.h at the edges of its domain, as a stand-alone program for the sanitizers
// (g++ -fsanitize=address,undefined): an empty list, n_map of 0 / 2 / 3 / 9 / 10, the capacity edge at 8191 / 8192 / 8193
// candidates, and every malformed map.  Every buffer has exactly the size the interface promises, so a write past an
// end is a report.  Exit code 0 and "ok" when every case gave what the header says.
#include <cstdio>
#include <vector>

#include "frame_tracking_solve.h"

namespace ft = msf::ftrack;
namespace tk = msf::tracking;

namespace {

constexpr int W = 640, H = 480;
int failures = 0;

void expect(bool ok, const char* what, int a = 0, int b = 0) {
  if (ok) return;
  std::printf("FAILED: %s (%d, %d)\n", what, a, b);
  failures++;
}

struct Scene {
  std::vector<tk::Point> points;
  std::vector<uint8_t> observed;
  std::vector<int32_t> ref_key, ref_point, cur_key, cur_point;
  std::vector<tk::Match> matches;
  ft::Map map() const {
    return ft::Map{(int32_t)points.size(), (int32_t)ref_key.size(), (int32_t)cur_key.size(), points.data(),
                   observed.empty() ? nullptr : observed.data(), ref_key.data(), ref_point.data(), cur_key.data(),
                   cur_point.data()};
  }
};

// n_ref train entries on the even pixels, n_cur entries of the frame on odd pixels of the upper rows, n_matches
// matches from pixel 2 j + 1 of the lower half to train entry j % n_ref
Scene scene(int n_ref, int n_cur, int n_matches) {
  Scene s;
  s.points.resize(16);
  for (int p = 0; p < 16; p++) s.points[p] = tk::Point{{(float)p, 1.0f, 2.0f}, {0, 0, 1}, 10.0f, 0u};
  for (int i = 0; i < n_ref; i++) s.ref_key.push_back(2 * i), s.ref_point.push_back(i % 16);
  for (int i = 0; i < n_cur; i++) s.cur_key.push_back(2 * i + 1), s.cur_point.push_back((i + 3) % 16);
  const int base = W * (H / 2);
  for (int j = 0; j < n_matches; j++) {
    const int k1 = base + 2 * j + 1, k2 = n_ref ? s.ref_key[j % n_ref] : 0;
    s.matches.push_back(tk::Match{k1 % W, k1 / W, k2 % W, k2 / W});
  }
  return s;
}

struct Run {
  int status, track_status = -99;
  int32_t n_map = -7, n_kept = -7, n_removed = -7, n_seen = -7;
  std::vector<ft::FramePoint> map;
  std::vector<uint8_t> carry_status, cur_status;
  std::vector<int32_t> kept_key, kept_point;
  std::vector<ft::Removed> removed;
};

// carry + cut with every (i % 3 == 0) record flagged; the buffers are exactly [corr_cap], [cap], [n_cur]
Run run(const Scene& s, int32_t n, int cap, int corr_cap, int min_matches, int min_map) {
  Run r;
  const ft::Map m = s.map();
  r.map.assign(corr_cap, ft::FramePoint{-7, -7, -7, -7});
  r.carry_status.assign(cap, 255);
  r.cur_status.assign(s.cur_key.size(), 255);
  std::vector<float> p3d((size_t)corr_cap * 3, -7.0f), p2d((size_t)corr_cap * 2, -7.0f);
  std::vector<int32_t> cp(corr_cap, -7);
  const long long most = (long long)s.cur_key.size() + cap;
  std::vector<uint64_t> words((size_t)ft::pow2_at_least(most < ft::kMaxCandidates ? (int)most : ft::kMaxCandidates));
  r.status = ft::host_carry(m, W, H, s.matches.data(), cap, n, min_matches, corr_cap, words.data(), &r.n_map, r.map.data(),
                            r.carry_status.data(), r.cur_status.data(), p3d.data(), p2d.data(), cp.data());
  if (r.status < 0) {
    expect(r.n_map == -7 && (corr_cap == 0 || r.map[0].key == -7) && (cap == 0 || r.carry_status[0] == 255),
           "a refused call wrote something", r.status);
    return r;
  }
  std::vector<uint8_t> outliers(r.n_map > 0 ? r.n_map : 1, 0);
  for (int i = 0; i < r.n_map; i += 3) outliers[i] = 1;
  r.kept_key.assign(corr_cap, -7);
  r.kept_point.assign(corr_cap, -7);
  r.removed.assign(corr_cap, ft::Removed{-7, -7});
  r.track_status = ft::host_cut(m, r.status, r.n_map, r.map.data(), outliers.data(), min_map, &r.n_kept, r.kept_key.data(),
                                r.kept_point.data(), &r.n_removed, r.removed.data(), &r.n_seen);
  expect(r.n_kept + r.n_removed == r.n_map, "kept + removed != n_map", r.n_kept, r.n_removed);
  for (int i = 1; i < r.n_kept; i++) expect(r.kept_key[i] > r.kept_key[i - 1], "kept keys not increasing", i);
  for (int i = 1; i < r.n_map; i++) expect(r.map[i].key > r.map[i - 1].key, "map keys not increasing", i);
  return r;
}

}  // namespace

int main() {
  // an empty list, with and without entries of the frame
  {
    Run r = run(scene(4, 0, 0), 0, 1, 0, 0, 0);
    expect(r.status == 0 && r.n_map == 0 && r.track_status == 0 && r.n_kept == 0, "empty list, empty frame", r.status, r.n_map);
    r = run(scene(4, 5, 0), 0, 1, 5, 0, 10);
    expect(r.status == 0 && r.n_map == 5 && r.track_status == ft::kFewMapMatches && r.n_removed == 2, "empty list", r.n_map, r.track_status);
    r = run(scene(0, 0, 3), 3, 3, 3, 0, 0);
    expect(r.status == 0 && r.n_map == 0 && r.carry_status[2] == ft::kNoPoint2, "no train entry", r.status, r.n_map);
  }
  // n_map of 0 / 2 / 3 / 9 / 10: the optimiser's thresholds
  for (int n : {0, 2, 3, 9, 10}) {
    Run r = run(scene(12, 0, n), n, 16, 16, 0, 0);
    expect(r.status == 0 && r.n_map == n && r.n_removed == (n + 2) / 3 && r.track_status == 0, "n_map", n, r.n_map);
    for (int j = 0; j < 16; j++) expect(r.carry_status[j] == (j < n ? 0 : 255), "carry_status", n, j);
  }
  // the gate
  {
    Run r = run(scene(12, 4, 14), 14, 16, 20, 15, 0);
    expect(r.status == ft::kFewMatches && r.track_status == ft::kFewMatches && r.n_map == 4 && r.n_kept == 4 && r.n_removed == 0 &&
               r.carry_status[0] == 255,
           "gated", r.status, r.n_map);
    r = run(scene(12, 4, 15), 15, 16, 20, 15, 0);
    expect(r.status == 0 && r.n_map == 19, "at the gate", r.status, r.n_map);
    r = run(scene(12, 4, 15), -1, 16, 20, 15, 0);
    expect(r.status == ft::kNoList, "no list", r.status);
    r = run(scene(12, 4, 15), 15, 16, 18, 15, 0);
    expect(r.status == ft::kNoRoom, "corr_cap one short", r.status);
  }
  // the capacity edge: 8191 / 8192 / 8193 candidates, split between the frame and the list
  for (int total : {8191, 8192, 8193}) {
    const int n_cur = 100, n = total - n_cur;
    Run r = run(scene(500, n_cur, n), n, n, total, 15, 10);
    if (total <= ft::kMaxCandidates)
      expect(r.status == 0 && r.n_map == total && r.track_status == 0, "capacity edge", total, r.n_map);
    else
      expect(r.status == ft::kNoRoom, "beyond the capacity", total, r.status);
  }
  // a list longer than its capacity is clipped
  {
    Run r = run(scene(12, 0, 8), 300, 8, 8, 0, 0);
    expect(r.status == 0 && r.n_map == 8, "clipped", r.status, r.n_map);
  }
  // every malformed map
  {
    const Scene good = scene(6, 4, 5);
    auto refused = [&](const char* what, Scene s) {
      Run r = run(s, 5, 5, 9, 0, 0);
      expect(r.status == ft::kBadMap, what, r.status);
      expect(ft::map_fault(s.map(), W, H) != nullptr, what);
    };
    expect(ft::map_fault(good.map(), W, H) == nullptr, "the good map");
    Scene s = good; s.ref_key[0] = -1; refused("ref key negative", s);
    s = good; s.ref_key[5] = W * H; refused("ref key beyond the image", s);
    s = good; s.ref_key[1] = s.ref_key[0]; refused("ref keys equal", s);
    s = good; s.ref_key[2] = s.ref_key[1] - 1; refused("ref keys decreasing", s);
    s = good; s.ref_point[1] = -1; refused("ref point negative", s);
    s = good; s.ref_point[5] = 16; refused("ref point beyond the table", s);
    s = good; s.cur_key[0] = -1; refused("cur key negative", s);
    s = good; s.cur_key[3] = W * H; refused("cur key beyond the image", s);
    s = good; s.cur_key[1] = s.cur_key[0]; refused("cur keys equal", s);
    s = good; s.cur_key[2] = s.cur_key[1] - 1; refused("cur keys decreasing", s);
    s = good; s.cur_point[1] = -1; refused("cur point negative", s);
    s = good; s.cur_point[3] = 16; refused("cur point beyond the table", s);
    ft::Map m = good.map();
    m.n_ref = -1;
    expect(ft::map_fault(m, W, H) != nullptr, "a negative count");
    m = good.map();
    m.ref_point = nullptr;
    expect(ft::map_fault(m, W, H) != nullptr, "a missing pointer");
  }
  // the bitonic network against itself on every power of two up to 64, reversed input
  for (int n = 1; n <= 64; n <<= 1) {
    std::vector<uint64_t> w(n);
    for (int i = 0; i < n; i++) w[i] = ft::word_of(n - i, i);
    ft::bitonic_sort(w.data(), n);
    for (int i = 1; i < n; i++) expect(w[i] > w[i - 1], "bitonic_sort", n, i);
  }
  std::printf(failures ? "%d failures\n" : "ok\n", failures);
  return failures ? 1 : 0;
}
