// The arithmetic of one RANSAC hypothesis of Initializer::FindHomography / FindFundamental
// (slam_pipeline/src/Initializer.cc:152-320): the 8-point DLT matrices, their null vector, F's rank-2 projection, the
// denormalisation and the 3 x 3 inverse.  Plain C++ shared by k_solve_models (ransac_kernels.hip) and by a host build
// (tests/cpp/ransac_solve_host.cpp), so the solver can be checked against a float64 SVD without a GPU.  Both builds use
// -ffp-contract=off: every expression rounds once per operation, in the order written.
//
// Null vector: one-sided (Hestenes) Jacobi on A itself.  Column pairs (p, q) of W = [A; V] (V starts as I) are rotated
// until the A parts of all columns are mutually orthogonal: then A V = U S, and the column of smallest norm carries the
// right singular vector of the smallest singular value in its V part -- vt.row(8) of the reference's FULL_UV cv::SVD, up
// to sign.  Working on A keeps the error at eps * s1 / (s8 - s9); the eigenvector of A'A in f32 squares the condition
// number and misses that by two to three orders of magnitude on the 8 x 9 matrices of F.
// Termination: at most kMaxSweeps sweeps of the 36 pairs; a sweep that rotates nothing ends the loop; a NaN makes every
// comparison false, so nothing rotates.  A matrix with a non-finite entry yields an all-NaN vector.
#ifndef MSF_RANSAC_SOLVE_H
#define MSF_RANSAC_SOLVE_H

#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#define MSF_HD __host__ __device__ inline
#else
#define MSF_HD inline
#endif

namespace msf {
namespace ransac {

constexpr int kMaxSweeps = 12;
constexpr float kEps = 5.9604644775390625e-08f;   // 2^-24: a pair whose cosine is below it counts as orthogonal

// element i of a per-problem array: LDS [element][lane] on the device (stride = lanes, conflict-free), stride 1 on the host
struct Strided {
  float* p;
  int stride;
  MSF_HD float& operator[](int i) const { return p[(long long)i * stride]; }
};

// W: N columns of ROWS + N entries each, column-major: W[c * (ROWS + N) + r]; r < ROWS is A, the rest V.
// The caller has stored A; V is set here.  Returns the index of the column of smallest norm.
template <int ROWS, int N, class Store>
MSF_HD int jacobi_smallest(Store w) {
  constexpr int R = ROWS + N;
  for (int c = 0; c < N; c++)
    for (int r = 0; r < N; r++) w[c * R + ROWS + r] = r == c ? 1.0f : 0.0f;
  for (int sweep = 0; sweep < kMaxSweeps; sweep++) {
    int rotated = 0;
    for (int p = 0; p < N - 1; p++) {
      for (int q = p + 1; q < N; q++) {
        float alpha = 0.0f, beta = 0.0f, gamma = 0.0f;
        for (int r = 0; r < ROWS; r++) {
          const float x = w[p * R + r], y = w[q * R + r];
          alpha += x * x;
          beta += y * y;
          gamma += x * y;
        }
        if (!(fabsf(gamma) > kEps * sqrtf(alpha * beta))) continue;   // orthogonal already, or NaN
        const float zeta = (beta - alpha) / (2.0f * gamma);
        const float t = copysignf(1.0f, zeta) / (fabsf(zeta) + sqrtf(1.0f + zeta * zeta));
        const float c = 1.0f / sqrtf(1.0f + t * t), s = c * t;
        for (int r = 0; r < R; r++) {
          const float x = w[p * R + r], y = w[q * R + r];
          w[p * R + r] = c * x - s * y;
          w[q * R + r] = s * x + c * y;
        }
        rotated++;
      }
    }
    if (!rotated) break;
  }
  int k = 0;
  float least = 0.0f;
  for (int c = 0; c < N; c++) {
    float norm2 = 0.0f;
    for (int r = 0; r < ROWS; r++) norm2 += w[c * R + r] * w[c * R + r];
    if (c == 0 || norm2 < least) { least = norm2; k = c; }
  }
  return k;
}

// ComputeH21's A (Initializer.cc:246-277): two rows per point pair; p1 / p2: the 8 normalised points (x, y)
template <class Store>
MSF_HD void build_a_homography(Store w, const float* p1, const float* p2) {
  constexpr int R = 16 + 9;
  for (int i = 0; i < 8; i++) {
    const float u1 = p1[2 * i], v1 = p1[2 * i + 1], u2 = p2[2 * i], v2 = p2[2 * i + 1];
    const float even[9] = {0.0f, 0.0f, 0.0f, -u1, -v1, -1.0f, v2 * u1, v2 * v1, v2};
    const float odd[9] = {u1, v1, 1.0f, 0.0f, 0.0f, 0.0f, -u2 * u1, -u2 * v1, -u2};
    for (int c = 0; c < 9; c++) {
      w[c * R + 2 * i] = even[c];
      w[c * R + 2 * i + 1] = odd[c];
    }
  }
}

// ComputeF21's A (:286-307): one row per point pair
template <class Store>
MSF_HD void build_a_fundamental(Store w, const float* p1, const float* p2) {
  constexpr int R = 8 + 9;
  for (int i = 0; i < 8; i++) {
    const float u1 = p1[2 * i], v1 = p1[2 * i + 1], u2 = p2[2 * i], v2 = p2[2 * i + 1];
    const float row[9] = {u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, 1.0f};
    for (int c = 0; c < 9; c++) w[c * R + i] = row[c];
  }
}

// the unit null vector of the A stored in w (ROWS = 16: homography, 8: fundamental); all NaN for a non-finite A
template <int ROWS, class Store>
MSF_HD void null_vector(Store w, float* h) {
  constexpr int R = ROWS + 9;
  float poison = 0.0f;   // 0 for a finite A, NaN otherwise
  for (int c = 0; c < 9; c++)
    for (int r = 0; r < ROWS; r++) poison += w[c * R + r] * 0.0f;
  const int k = jacobi_smallest<ROWS, 9>(w);
  float norm2 = 0.0f;
  for (int r = 0; r < 9; r++) {
    h[r] = w[k * R + ROWS + r];
    norm2 += h[r] * h[r];
  }
  const float norm = sqrtf(norm2);   // V is orthogonal up to the rounding of its rotations: one division makes h unit
  for (int r = 0; r < 9; r++) h[r] = poison == 0.0f ? h[r] / norm : poison;
}

// ComputeF21's second SVD (:313-319): Fpre with its smallest singular value set to 0.  Fpre V = B with orthogonal
// columns (B = U S), so u diag(w1, w2, 0) vt is the sum of b_j v_j' over the two columns of larger norm.
MSF_HD void rank2(const float* fpre, float* fn) {
  float w3[18];
  Strided w{w3, 1};
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) w[c * 6 + r] = fpre[3 * r + c];
  const int k = jacobi_smallest<3, 3>(w);
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) {
      float sum = 0.0f;
      for (int j = 0; j < 3; j++)
        if (j != k) sum += w3[j * 6 + r] * w3[j * 6 + 3 + c];
      fn[3 * r + c] = sum;
    }
}

MSF_HD void mul3(const float* a, const float* b, float* out) {
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) {
      float sum = 0.0f;
      for (int k = 0; k < 3; k++) sum += a[3 * r + k] * b[3 * k + c];
      out[3 * r + c] = sum;
    }
}

// cv::Mat::inv() of a 3 x 3 CV_32F matrix: cofactors and determinant in f64, one rounding to f32; a singular matrix
// gives the zero matrix (cv::invert returns false and clears its output).  NaN in, NaN out.
MSF_HD void inv3(const float* m, float* out) {
  const double a = m[0], b = m[1], c = m[2], d = m[3], e = m[4], f = m[5], g = m[6], h = m[7], i = m[8];
  const double det = a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g);
  if (det == 0.0) {
    for (int k = 0; k < 9; k++) out[k] = 0.0f;
    return;
  }
  const double s = 1.0 / det;
  out[0] = (float)((e * i - f * h) * s);
  out[1] = (float)((c * h - b * i) * s);
  out[2] = (float)((b * f - c * e) * s);
  out[3] = (float)((f * g - d * i) * s);
  out[4] = (float)((a * i - c * g) * s);
  out[5] = (float)((c * d - a * f) * s);
  out[6] = (float)((d * h - e * g) * s);
  out[7] = (float)((b * g - a * h) * s);
  out[8] = (float)((a * e - b * d) * s);
}

// FindHomography's loop body (:185-187): H21 = T2^-1 Hn T1, H12 = H21^-1
MSF_HD void finish_homography(const float* hn, const float* t1, const float* t2, float* h21, float* h12) {
  float t2inv[9], left[9];
  inv3(t2, t2inv);
  mul3(t2inv, hn, left);
  mul3(left, t1, h21);
  inv3(h21, h12);
}

// FindFundamental's loop body (:232-234): F21 = T2' Fn T1, Fn = the rank-2 projection of the null vector
MSF_HD void finish_fundamental(const float* fpre, const float* t1, const float* t2, float* fn, float* f21) {
  float t2t[9], left[9];
  rank2(fpre, fn);
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) t2t[3 * r + c] = t2[3 * c + r];
  mul3(t2t, fn, left);
  mul3(left, t1, f21);
}

// ---- the draw of the minimum sets (Initializer.cc:106-120), with a counter-based generator ----
// The reference seeds std::mt19937 from std::random_device: no sequence exists to reproduce, only the procedure.  Here
// draw j of iteration `it` of list `list` is mix64 (the splitmix64 finaliser) applied twice to the key
//   seed ^ mix64(((list * 2^20 + it) * 8 + j) + 0x9E3779B97F4A7C15)
// and randi = the high 64 bits of (that word * size): uniform on [0, size) up to a bias below 2^-50.
MSF_HD uint64_t mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

MSF_HD uint64_t mulhi64(uint64_t a, uint64_t b) {
  const uint64_t al = a & 0xFFFFFFFFull, ah = a >> 32, bl = b & 0xFFFFFFFFull, bh = b >> 32;
  const uint64_t mid = ah * bl + ((al * bl) >> 32);
  const uint64_t mid2 = al * bh + (mid & 0xFFFFFFFFull);
  return ah * bh + (mid >> 32) + (mid2 >> 32);
}

// vAvailableIndices = all indices; eight times: randi, idx = avail[randi], avail[randi] = avail.back(), pop_back.
// Only eight entries of the list ever change, so they are kept as (position, value) pairs instead of a copy of the list.
MSF_HD void draw_set(uint64_t seed, int list, int it, int n, int32_t* set) {
  int pos[8], val[8];
  int size = n;
  for (int j = 0; j < 8; j++) {
    const uint64_t counter = (((uint64_t)(uint32_t)list << 20) + (uint64_t)(uint32_t)it) * 8 + (uint64_t)j;
    const uint64_t word = mix64(seed ^ mix64(counter + 0x9E3779B97F4A7C15ull));
    const int randi = (int)mulhi64(word, (uint64_t)size);
    int idx = randi, last = size - 1;
    for (int k = 0; k < j; k++) {   // later changes of a position override earlier ones
      if (pos[k] == randi) idx = val[k];
      if (pos[k] == size - 1) last = val[k];
    }
    set[j] = idx;
    pos[j] = randi;
    val[j] = last;
    size--;
  }
}

}  // namespace ransac
}  // namespace msf

#endif  // MSF_RANSAC_SOLVE_H
