// Host build of csrc/frame_tracking_solve.h behind a C interface for tests/frame_tracking_host.py: the carry and the cut
// on plain memory, one thread.  g++ -std=c++17 -ffp-contract=off; no HIP.
#include <vector>

#include "frame_tracking_solve.h"

namespace ft = msf::ftrack;

extern "C" {

// Steps 0-3.  -> the status the carry leaves (0, 1 gated, negative: nothing written)
int frame_tracking_host_carry(const ft::Map* m, int width, int height, const msf::tracking::Match* matches, int cap,
                              int32_t n, int min_matches, int corr_cap, int32_t* n_map, ft::FramePoint* map,
                              uint8_t* carry_status, uint8_t* cur_status, float* corr_p3d, float* corr_p2d,
                              int32_t* corr_point) {
  const long long most = (long long)(m->n_cur > 0 ? m->n_cur : 0) + (cap > 0 ? cap : 0);
  std::vector<uint64_t> words((size_t)ft::pow2_at_least(most < ft::kMaxCandidates ? (int)most : ft::kMaxCandidates));
  return ft::host_carry(*m, width, height, matches, cap, n, min_matches, corr_cap, words.data(), n_map, map, carry_status,
                        cur_status, corr_p3d, corr_p2d, corr_point);
}

// Steps 5-6 behind a carry that left `carried` >= 0.  -> track_status
int frame_tracking_host_cut(const ft::Map* m, int carried, int n_map, ft::FramePoint* map, const uint8_t* outliers,
                            int min_map_matches, int32_t* n_kept, int32_t* kept_key, int32_t* kept_point,
                            int32_t* n_removed, ft::Removed* removed, int32_t* n_matches_map) {
  return ft::host_cut(*m, carried, n_map, map, outliers, min_map_matches, n_kept, kept_key, kept_point, n_removed, removed,
                      n_matches_map);
}

}  // extern "C"
