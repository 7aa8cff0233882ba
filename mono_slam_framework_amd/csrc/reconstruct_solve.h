// The arithmetic of the tail of Initializer::Initialize (slam_pipeline/src/Initializer.cc:489-934): ReconstructF /
// ReconstructH with DecomposeE, Triangulate and the loop body of CheckRT, and the two selection rules.  Plain C++ shared
// by reconstruct_kernels.hip and by a host build (tests/cpp/reconstruct_host.cpp), so every step can be checked against a
// float64 SVD without a GPU.  Both builds use -ffp-contract=off: every expression rounds once per operation, in the
// order written; f32 where the reference is CV_32F, f64 where cv::norm / Mat::dot / acos return double.
//
// svd3: the full SVD of a 3 x 3 matrix by the one-sided (Hestenes) Jacobi of ransac_solve.h on W = [A; V]: after the
// sweeps A V = B has orthogonal columns, so w_j = |b_j|, u_j = b_j / w_j, and the columns are reordered to descending w.
// Sign convention (the routine's own; cv::SVD's differs, and any valid choice permutes the hypotheses below):
//   * V is the product of the plane rotations, so det(V) = +1 up to rounding before the reordering; an odd reordering
//     makes it -1.  Each v_j is divided by its norm once.
//   * u_1, u_2 = b_j / |b_j|.  u_3 = u_1 x u_2, negated when its dot product with b_3 is negative: for a matrix whose
//     smallest singular value is at rounding level (an essential matrix) b_3 / |b_3| is noise, the cross product is not,
//     and A = U diag(w) V' holds either way.  b_3 = 0 exactly keeps the cross product: det(U) = +1.
// A non-finite entry makes the affected singular values and vectors NaN; every routine here is loop-bounded
// (ransac::kMaxSweeps sweeps) and ends on any input.
#ifndef MSF_RECONSTRUCT_SOLVE_H
#define MSF_RECONSTRUCT_SOLVE_H

#include "ransac_solve.h"

namespace msf {
namespace reconstruct {

using ransac::inv3;
using ransac::mul3;

constexpr int kMaxCandidates = 8;   // ReconstructH: 8 motion hypotheses, ReconstructF: 4

// element i of a private array (registers on the device once the loops over it are unrolled)
struct Flat {
  float* p;
  MSF_HD float& operator[](int i) const { return p[i]; }
};

MSF_HD bool finite32(float x) { return fabsf(x) <= 3.4028234663852886e+38f; }   // false for NaN and +-Inf

MSF_HD float det3(const float* m) {
  return m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
}

MSF_HD void transpose3(const float* m, float* out) {
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) out[3 * r + c] = m[3 * c + r];
}

// a = u diag(w) v', all row-major [9]; w descending.  See the file comment for the signs.
MSF_HD void svd3(const float* a, float* u, float* w, float* v) {
  float buf[18];
  Flat s{buf};
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) buf[c * 6 + r] = a[3 * r + c];
  ransac::jacobi_smallest<3, 3>(s);
  float n2[3];
  for (int c = 0; c < 3; c++) n2[c] = buf[c * 6] * buf[c * 6] + buf[c * 6 + 1] * buf[c * 6 + 1] + buf[c * 6 + 2] * buf[c * 6 + 2];
  int o0 = 0, o1 = 1, o2 = 2, tmp;
  if (n2[o1] > n2[o0]) { tmp = o0; o0 = o1; o1 = tmp; }
  if (n2[o2] > n2[o1]) { tmp = o1; o1 = o2; o2 = tmp; }
  if (n2[o1] > n2[o0]) { tmp = o0; o0 = o1; o1 = tmp; }
  const int order[3] = {o0, o1, o2};
  float b3[3] = {0.0f, 0.0f, 0.0f};
  for (int j = 0; j < 3; j++) {
    const float* col = buf + order[j] * 6;
    const float norm = sqrtf(n2[order[j]]);
    const float vnorm = sqrtf(col[3] * col[3] + col[4] * col[4] + col[5] * col[5]);
    w[j] = norm;
    for (int r = 0; r < 3; r++) {
      u[3 * r + j] = col[r] / norm;
      v[3 * r + j] = col[3 + r] / vnorm;
      if (j == 2) b3[r] = col[r];
    }
  }
  float c3[3] = {u[3] * u[7] - u[6] * u[4], u[6] * u[1] - u[0] * u[7], u[0] * u[4] - u[3] * u[1]};   // u_1 x u_2
  const float side = c3[0] * b3[0] + c3[1] * b3[1] + c3[2] * b3[2];
  for (int r = 0; r < 3; r++) u[3 * r + 2] = side < 0.0f ? -c3[r] : c3[r];
}

// ReconstructF's E21 = K' F21 K (:499) and DecomposeE (:916-934).  R [4][9], t [4][3] in the order the reference tries
// them: (R1, t) (R2, t) (R1, -t) (R2, -t).  w [3]: the singular values of E21 (for tests).
MSF_HD void decompose_e(const float* f21, const float* K, float* R, float* t, float* w) {
  float kt[9], left[9], e21[9], u[9], v[9], vt[9], uw[9];
  transpose3(K, kt);
  mul3(kt, f21, left);
  mul3(left, K, e21);
  svd3(e21, u, w, v);
  transpose3(v, vt);
  const double norm = sqrt((double)u[2] * u[2] + (double)u[5] * u[5] + (double)u[8] * u[8]);   // cv::norm: f64
  const float tv[3] = {(float)(u[2] / norm), (float)(u[5] / norm), (float)(u[8] / norm)};
  const float W[9] = {0.0f, -1.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f};
  float Wt[9], r1[9], r2[9];
  transpose3(W, Wt);
  mul3(u, W, uw);
  mul3(uw, vt, r1);
  if (det3(r1) < 0.0f)
    for (int k = 0; k < 9; k++) r1[k] = -r1[k];
  mul3(u, Wt, uw);
  mul3(uw, vt, r2);
  if (det3(r2) < 0.0f)
    for (int k = 0; k < 9; k++) r2[k] = -r2[k];
  for (int c = 0; c < 4; c++) {
    for (int k = 0; k < 9; k++) R[9 * c + k] = (c & 1) ? r2[k] : r1[k];
    for (int k = 0; k < 3; k++) t[3 * c + k] = c < 2 ? tv[k] : -tv[k];
  }
}

// ReconstructH's eight hypotheses by the method of Faugeras (:599-698).  Returns false on the reference's early
// `return false` (d1 / d2 < 1.00001 || d2 / d3 < 1.00001); R [8][9], t [8][3] (unit), n [8][3], w [3] = d1, d2, d3.
MSF_HD bool decompose_h(const float* h21, const float* K, float* R, float* t, float* n, float* w) {
  float invk[9], left[9], A[9], U[9], V[9], Vt[9];
  inv3(K, invk);
  mul3(invk, h21, left);
  mul3(left, K, A);
  svd3(A, U, w, V);
  transpose3(V, Vt);
  const float s = (float)((double)det3(U) * (double)det3(Vt));
  const float d1 = w[0], d2 = w[1], d3 = w[2];
  if ((double)(d1 / d2) < 1.00001 || (double)(d2 / d3) < 1.00001) return false;

  // n' = [x1 0 x3]: e1 = e3 = 1, e1 = 1 e3 = -1, e1 = -1 e3 = 1, e1 = e3 = -1
  const float aux1 = sqrtf((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3));
  const float aux3 = sqrtf((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3));
  const float x1[4] = {aux1, aux1, -aux1, -aux1};
  const float x3[4] = {aux3, -aux3, aux3, -aux3};
  // case d' = d2, then case d' = -d2
  const float aux_stheta = sqrtf((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2);
  const float ctheta = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2);
  const float stheta[4] = {aux_stheta, -aux_stheta, -aux_stheta, aux_stheta};
  const float aux_sphi = sqrtf((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2);
  const float cphi = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2);
  const float sphi[4] = {aux_sphi, -aux_sphi, -aux_sphi, aux_sphi};
  for (int c = 0; c < 8; c++) {
    const int i = c & 3;
    const bool minus = c >= 4;
    float Rp[9] = {1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f};
    if (!minus) {
      Rp[0] = ctheta; Rp[2] = -stheta[i]; Rp[6] = stheta[i]; Rp[8] = ctheta;
    } else {
      Rp[0] = cphi; Rp[2] = sphi[i]; Rp[4] = -1.0f; Rp[6] = sphi[i]; Rp[8] = -cphi;
    }
    float urp[9];
    mul3(U, Rp, urp);
    for (int k = 0; k < 9; k++) urp[k] = s * urp[k];
    mul3(urp, Vt, R + 9 * c);                       // R = s * U * Rp * Vt

    const float scale = minus ? d1 + d3 : d1 - d3;
    const float tp[3] = {x1[i] * scale, 0.0f * scale, (minus ? x3[i] : -x3[i]) * scale};
    float tv[3];
    for (int r = 0; r < 3; r++) tv[r] = U[3 * r] * tp[0] + U[3 * r + 1] * tp[1] + U[3 * r + 2] * tp[2];
    const double norm = sqrt((double)tv[0] * tv[0] + (double)tv[1] * tv[1] + (double)tv[2] * tv[2]);
    for (int r = 0; r < 3; r++) t[3 * c + r] = (float)(tv[r] / norm);   // t / cv::norm(t)

    const float np[3] = {x1[i], 0.0f, x3[i]};
    float nv[3];
    for (int r = 0; r < 3; r++) nv[r] = V[3 * r] * np[0] + V[3 * r + 1] * np[1] + V[3 * r + 2] * np[2];
    const bool flip = nv[2] < 0.0f;
    for (int r = 0; r < 3; r++) n[3 * c + r] = flip ? -nv[r] : nv[r];
  }
  return true;
}

// What CheckRT sets up before its loop (:814-837) for one (R, t)
struct Pose {
  float R[9], t[3];
  float P1[12];   // K [I | 0]
  float P2[12];   // K [R | t]
  float O2[3];    // -R' t
  float fx, fy, cx, cy;
};

MSF_HD void make_pose(const float* K, const float* R, const float* t, Pose* q) {
  for (int k = 0; k < 9; k++) q->R[k] = R[k];
  for (int k = 0; k < 3; k++) q->t[k] = t[k];
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 4; c++) {
      q->P1[4 * r + c] = c < 3 ? K[3 * r + c] : 0.0f;
      float sum = 0.0f;
      for (int k = 0; k < 3; k++) sum += K[3 * r + k] * (c < 3 ? R[3 * k + c] : t[k]);
      q->P2[4 * r + c] = sum;
    }
    float o = 0.0f;
    for (int k = 0; k < 3; k++) o += R[3 * k + r] * t[k];
    q->O2[r] = -o;
  }
  q->fx = K[0]; q->fy = K[4]; q->cx = K[2]; q->cy = K[5];
}

// Initializer::Triangulate (:744-758): the 4 x 4 matrix, its null vector (the column of V that belongs to the column of
// A V of smallest norm -- vt.row(3) up to sign and scale), and the division by the fourth entry.  hom [4]: the null
// vector before the division, unit up to the rounding of the rotations (all NaN for a non-finite matrix); x3d [3].
MSF_HD void triangulate(float x1, float y1, float x2, float y2, const float* P1, const float* P2, float* hom, float* x3d) {
  float w[32];   // [A; V] column-major, 8 per column
  Flat s{w};
  float poison = 0.0f;
  for (int c = 0; c < 4; c++) {
    w[c * 8] = x1 * P1[8 + c] - P1[c];
    w[c * 8 + 1] = y1 * P1[8 + c] - P1[4 + c];
    w[c * 8 + 2] = x2 * P2[8 + c] - P2[c];
    w[c * 8 + 3] = y2 * P2[8 + c] - P2[4 + c];
    for (int r = 0; r < 4; r++) poison += w[c * 8 + r] * 0.0f;
  }
  const int k = ransac::jacobi_smallest<4, 4>(s);
  for (int r = 0; r < 4; r++) {
    const float x = k == 0 ? w[4 + r] : k == 1 ? w[12 + r] : k == 2 ? w[20 + r] : w[28 + r];   // no runtime index
    hom[r] = poison == 0.0f ? x : poison;
  }
  for (int r = 0; r < 3; r++) x3d[r] = hom[r] / hom[3];
}

constexpr int kCounted = 1;   // the match entered nGood, vCosParallax and vP3D
constexpr int kGood = 2;      // vbGood: counted and cosParallax < 0.99998

// The body of CheckRT's loop (:841-903) for one inlier match: returns 0 where the reference `continue`s, else kCounted,
// plus kGood.  p [3] = p3dC1 and *cos_parallax are what the reference would store (valid when counted).
MSF_HD int check_match(float x1, float y1, float x2, float y2, const Pose& q, float th2, float* p, double* cos_parallax) {
  float hom[4];
  triangulate(x1, y1, x2, y2, q.P1, q.P2, hom, p);
  if (!finite32(p[0]) || !finite32(p[1]) || !finite32(p[2])) return 0;

  // normal1 = p3dC1 - O1 with O1 = 0; cv::norm and Mat::dot work in f64 on the f32 entries
  const double dist1 = sqrt((double)p[0] * p[0] + (double)p[1] * p[1] + (double)p[2] * p[2]);
  const float n2[3] = {p[0] - q.O2[0], p[1] - q.O2[1], p[2] - q.O2[2]};
  const double dist2 = sqrt((double)n2[0] * n2[0] + (double)n2[1] * n2[1] + (double)n2[2] * n2[2]);
  const double cosParallax = ((double)p[0] * n2[0] + (double)p[1] * n2[1] + (double)p[2] * n2[2]) / (dist1 * dist2);
  *cos_parallax = cosParallax;

  if (p[2] <= 0.0f && cosParallax < 0.99998) return 0;
  float p2[3];   // p3dC2 = R * p3dC1 + t
  for (int r = 0; r < 3; r++) {
    float sum = 0.0f;
    for (int k = 0; k < 3; k++) sum += q.R[3 * r + k] * p[k];
    p2[r] = sum + q.t[r];
  }
  if (p2[2] <= 0.0f && cosParallax < 0.99998) return 0;

  const float invZ1 = 1.0f / p[2];
  const float im1x = q.fx * p[0] * invZ1 + q.cx;
  const float im1y = q.fy * p[1] * invZ1 + q.cy;
  const float squareError1 = (im1x - x1) * (im1x - x1) + (im1y - y1) * (im1y - y1);
  if (squareError1 > th2) return 0;

  const float invZ2 = 1.0f / p2[2];
  const float im2x = q.fx * p2[0] * invZ2 + q.cx;
  const float im2y = q.fy * p2[1] * invZ2 + q.cy;
  const float squareError2 = (im2x - x2) * (im2x - x2) + (im2y - y2) * (im2y - y2);
  if (squareError2 > th2) return 0;

  return cosParallax < 0.99998 ? kCounted | kGood : kCounted;
}

// vCosParallax as 64-bit keys whose unsigned order is the order of the doubles (-0 < +0; every NaN becomes one key
// above +Inf, so a list that holds one still has a defined rank order).  ~0 is no key: it marks an empty slot.
MSF_HD uint64_t cos_key(double x) {
  if (x != x) return 0xFFF8000000000000ull;
  union { double d; uint64_t u; } b;
  b.d = x;
  return (b.u >> 63) ? ~b.u : b.u | 0x8000000000000000ull;
}

MSF_HD double key_cos(uint64_t key) {
  union { double d; uint64_t u; } b;
  b.u = (key >> 63) ? key & 0x7FFFFFFFFFFFFFFFull : ~key;
  return b.d;
}

// CheckRT's last lines (:905-911) given the selected entry of the sorted vCosParallax
MSF_HD float parallax_degrees(double cos_selected) { return (float)(acos(cos_selected) * 180 / 3.1415926535897932384626433832795); }

// ReconstructF's selection (:524-582): the candidate index, or -1 for `return false`
MSF_HD int pick_fundamental(const int* nGood, const float* parallax, int N, int minTriangulated, float minParallax) {
  int maxGood = nGood[0];
  for (int k = 1; k < 4; k++) maxGood = nGood[k] > maxGood ? nGood[k] : maxGood;
  const int n90 = (int)(0.9 * N);
  const int nMinGood = n90 > minTriangulated ? n90 : minTriangulated;   // max
  int nsimilar = 0;
  for (int k = 0; k < 4; k++)
    if (nGood[k] > 0.7 * maxGood) nsimilar++;
  if (maxGood < nMinGood || nsimilar > 1) return -1;
  for (int k = 0; k < 4; k++)
    if (maxGood == nGood[k]) return parallax[k] > minParallax ? k : -1;   // the else-if chain: only the first equal one
  return -1;
}

// ReconstructH's selection (:700-741): first strict maximum; min, not max; >=, not >
MSF_HD int pick_homography(const int* nGood, const float* parallax, int N, int minTriangulated, float minParallax) {
  int bestGood = 0, bestIdx = 0;
  float bestParallax = -1.0f;
  for (int k = 0; k < 8; k++)
    if (nGood[k] > bestGood) { bestGood = nGood[k]; bestIdx = k; bestParallax = parallax[k]; }
  const int n90 = (int)(0.9 * N);
  const int minGood = n90 < minTriangulated ? n90 : minTriangulated;   // min
  return bestParallax >= minParallax && bestGood >= minGood ? bestIdx : -1;
}

}  // namespace reconstruct
}  // namespace msf

#endif  // MSF_RECONSTRUCT_SOLVE_H
