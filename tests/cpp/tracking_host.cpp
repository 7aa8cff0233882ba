// Host build of csrc/tracking_solve.h (the arithmetic and index rules of tracking_kernels.hip) for
// tests/test_tracking_solve_host.py and the GPU tests: g++ -ffp-contract=off, loaded with ctypes.
#include <vector>

#include "tracking_solve.h"

using namespace msf::tracking;

static_assert(sizeof(View) == 64 && sizeof(Point) == 32 && sizeof(Claim) == 16 && sizeof(Frustum) == 96, "public layouts");

extern "C" {

// 0, or -1 for a malformed map (then nothing is written), as the device entry's status_word
int tracking_host_frustum(const Map* m, int width, int height, const Frustum* f, int32_t* n_to_match, uint8_t* status,
                          uint8_t* visible, int32_t* owner_kf, float* u, float* v, float* dist, float* view_cos) {
  if (map_fault(*m, width, height) || frustum_fault(*f)) return -1;
  std::vector<int32_t> owner((size_t)m->n_points + 1);
  host_frustum(*m, *f, owner.data(), n_to_match, status, visible, owner_kf, u, v, dist, view_cos);
  return 0;
}

// n_claims, or -1 for a malformed map
int tracking_host_claims(const Map* m, int width, int height, const Match* matches, int cap, const int32_t* n_out,
                         const uint8_t* matched, int32_t* n_claimed, Claim* claims, uint8_t* claim_status,
                         int32_t corr_cap, int32_t* n_corr, float* corr_p3d, float* corr_p2d, int32_t* corr_point) {
  if (map_fault(*m, width, height)) return -1;
  std::vector<uint32_t> words((size_t)width * height, 0u);
  return host_claims(*m, width, height, matches, cap, n_out, matched, words.data(), n_claimed, claims, claim_status,
                     corr_cap, n_corr, corr_p3d, corr_p2d, corr_point);
}
}
