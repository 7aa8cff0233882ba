// Host build of csrc/ransac_solve.h (the arithmetic of k_solve_models and k_ransac_sets) for
// tests/test_ransac_solve_host.py: g++ -ffp-contract=off, loaded with ctypes, checked against a float64 SVD.
#include "ransac_solve.h"

using namespace msf::ransac;

extern "C" {

// p1, p2: the 8 normalised points [8][2]; T1, T2 [9]; outputs [9] each (m12: homography only, fn: fundamental only)
void ransac_host_solve(int model, const float* p1, const float* p2, const float* T1, const float* T2, float* null_vec,
                       float* m21, float* m12, float* fn) {
  float w[(16 + 9) * 9];
  Strided s{w, 1};
  if (model == 0) {
    build_a_homography(s, p1, p2);
    null_vector<16>(s, null_vec);
    finish_homography(null_vec, T1, T2, m21, m12);
  } else {
    build_a_fundamental(s, p1, p2);
    null_vector<8>(s, null_vec);
    finish_fundamental(null_vec, T1, T2, fn, m21);
  }
}

void ransac_host_rank2(const float* fpre, float* fn) { rank2(fpre, fn); }

void ransac_host_draw(uint64_t seed, int list, int it, int n, int32_t* set) { draw_set(seed, list, it, n, set); }
}
