// Host build of csrc/reconstruct_solve.h (the arithmetic of reconstruct_kernels.hip) for
// tests/test_reconstruct_host.py: g++ -ffp-contract=off, loaded with ctypes, checked against a float64 reference.
#include <algorithm>
#include <vector>

#include "reconstruct_solve.h"

using namespace msf::reconstruct;

extern "C" {

void reconstruct_host_svd3(const float* a, float* u, float* w, float* v) { svd3(a, u, w, v); }

// ReconstructH (model 0) / ReconstructF (model 1) of one list, sequentially.  matches [n][4], inliers [n].
// Outputs: w [3] singular values; cand_R [8][9], cand_t [8][3]; cand_good [8]; cand_parallax [8];
// flags [8][n] (kCounted | kGood); points [8][n][3]; hom [8][n][4] (the null vector before the division, inliers only).
// Returns ok; *n_cand, *winner, *early (ReconstructH's early return).
int reconstruct_host_run(int model, const float* m21, const float* K, float sigma, int min_triangulated,
                         float min_parallax, int n, const int32_t* matches, const uint8_t* inliers, float* w,
                         int32_t* n_cand, float* cand_R, float* cand_t, int32_t* cand_good, float* cand_parallax,
                         uint8_t* flags, float* points, float* hom, int32_t* winner, int32_t* early) {
  int N = 0;
  for (int i = 0; i < n; i++) N += inliers[i] ? 1 : 0;
  float normals[24];
  *early = 0;
  *winner = -1;
  *n_cand = 0;
  if (model == 0) {
    if (!decompose_h(m21, K, cand_R, cand_t, normals, w)) {
      *early = 1;
      return 0;
    }
    *n_cand = 8;
  } else {
    decompose_e(m21, K, cand_R, cand_t, w);
    *n_cand = 4;
  }
  const float th2 = 4.0f * (sigma * sigma);
  for (int c = 0; c < *n_cand; c++) {
    Pose q;
    make_pose(K, cand_R + 9 * c, cand_t + 3 * c, &q);
    std::vector<uint64_t> keys;
    for (int i = 0; i < n; i++) {
      if (!inliers[i]) continue;
      const float x1 = (float)matches[4 * i], y1 = (float)matches[4 * i + 1];
      const float x2 = (float)matches[4 * i + 2], y2 = (float)matches[4 * i + 3];
      float p[3];
      double cosp = 0;
      const int f = check_match(x1, y1, x2, y2, q, th2, p, &cosp);
      float unused[3];
      triangulate(x1, y1, x2, y2, q.P1, q.P2, hom + ((size_t)c * n + i) * 4, unused);
      flags[(size_t)c * n + i] = (uint8_t)f;
      if (f & kCounted) {
        for (int k = 0; k < 3; k++) points[((size_t)c * n + i) * 3 + k] = p[k];
        keys.push_back(cos_key(cosp));
      }
    }
    cand_good[c] = (int)keys.size();
    cand_parallax[c] = 0.0f;
    if (!keys.empty()) {
      std::sort(keys.begin(), keys.end());
      cand_parallax[c] = parallax_degrees(key_cos(keys[std::min<size_t>(50, keys.size() - 1)]));
    }
  }
  *winner = model == 0 ? pick_homography(cand_good, cand_parallax, N, min_triangulated, min_parallax)
                       : pick_fundamental(cand_good, cand_parallax, N, min_triangulated, min_parallax);
  return *winner >= 0;
}

int reconstruct_host_pick(int model, const int32_t* good, const float* parallax, int N, int min_triangulated,
                          float min_parallax) {
  return model == 0 ? pick_homography(good, parallax, N, min_triangulated, min_parallax)
                    : pick_fundamental(good, parallax, N, min_triangulated, min_parallax);
}

uint64_t reconstruct_host_key(double x) { return cos_key(x); }
double reconstruct_host_unkey(uint64_t k) { return key_cos(k); }
}
