// The arithmetic and the index rules of Tracking::SearchLocalPoints (slam_pipeline/src/Tracking.cc:594-632,
// Frame::isInFrustum Frame.cc:48-84) as include/msf_tracking.h states them: one map point -> its frustum status, one
// match -> its claim status.  Plain C++ shared by tracking_kernels.hip and by a host build (tests/cpp/tracking_host.cpp,
// tests/cpp/tracking_edge_main.cpp), so every step can be checked against float64 and run under the sanitizers without a
// GPU.  Both builds use -ffp-contract=off: every expression rounds once per operation, in the order written.
//
// Types are those of the reference's expressions, with triangulate_solve.h's convention for a cv::Mat product:
//   * Pc = mRcw * P + mtcw: per row the f32 products summed left to right from 0.0f, then the f32 add of tcw [M: what
//     cv::gemm does for a 3 x 3 by 3 x 1 CV_32F product is recalled, not read; the convention is the one the other
//     solve headers fixed];
//   * invz = 1.0f / PcZ; u = fx * PcX * invz + cx; v likewise: f32, left to right;
//   * PO = P - mOw in f32; dist = (float)cv::norm(PO): the squares in f64 summed left to right, sqrt in f64 [M: cv::norm
//     of a CV_32F vector accumulates in double], then the cast;
//   * viewCos = (float)(PO.dot(Pn) / dist): Mat::dot returns double -- products of the f32 entries in f64 summed left to
//     right -- divided by (double)dist, then the cast.
// Defined divergence (status 6): a non-finite u, v, dist or viewCos is rejected where it appears; the reference's
// comparisons let a NaN through as visible.  `dist < 0` of the reference never holds for a finite dist and has no code.
// Every loop is bounded: the binary searches by 32 halvings, the host loops by the map's own counts.
#ifndef MSF_TRACKING_SOLVE_H
#define MSF_TRACKING_SOLVE_H

#include <math.h>
#include <stdint.h>
#include <string.h>

#include "carve.h"

#ifndef MSF_HD
#ifdef __HIPCC__
#define MSF_HD __host__ __device__ inline
#else
#define MSF_HD inline
#endif
#endif

namespace msf {
namespace tracking {

// msf_view / msf_map_point / msf_match / msf_local_claim of the public headers, restated so that the host build needs
// no other header
struct View {
  float Rcw[9], tcw[3];
  float fx, fy, cx, cy;
};

struct Point {
  float pos[3], normal[3];
  float max_distance;
  uint32_t flags;
};

struct Match {
  int32_t x1, y1, x2, y2;
};

struct Claim {
  int32_t key, point, kf, match;
};

struct Frustum {
  View view;
  float Ow[3];
  float min_x, max_x, min_y, max_y;
  float cos_limit;
};

// The local map of one call (msf_local_map without its header words)
struct Map {
  int32_t n_points, n_kf, n_entries, n_cur;
  const Point* points;
  const int32_t* kf_start;
  const int32_t* kf_key;
  const int32_t* kf_point;
  const int32_t* cur_key;
  const int32_t* cur_point;
};

constexpr uint32_t kBad = 1u, kSeen = 2u;
constexpr int kVisible = 0, kBehind = 1, kOutsideU = 2, kOutsideV = 3, kTooFar = 4, kViewAngle = 5, kNotFinite = 6,
              kIsBad = 7, kIsSeen = 8, kNoEntry = 9;
constexpr int kClaimed = 0, kNoKey1 = 1, kOccupied = 2, kNoPoint2 = 3, kLost = 4;
// A word that takes the minimum of entry indices or ordinals holds kTop - index and takes the MAXIMUM: 0 is "none", so
// one clear of zeros prepares every word of a call, and the integer max of the complements is the min of the indices.
constexpr uint32_t kTop = 0x7FFFFFFFu;

MSF_HD bool finite32(float x) { return fabsf(x) <= 3.402823466e+38f; }   // false for a NaN

// a NaN leaves as the one quiet NaN, so that the host and the device builds agree on its bits
MSF_HD float canonical(float x) {
  if (x == x) return x;
  const uint32_t q = 0x7FC00000u;
  float f;
  memcpy(&f, &q, sizeof f);
  return f;
}

// Step 2 behind the flags (Frame.cc:48-84) for one point.  diag [4] = u, v, dist, viewCos: what was computed before the
// rejecting stage, 0 behind it.
MSF_HD int frustum_point(const Point& mp, const Frustum& f, float* diag) {
  for (int k = 0; k < 4; k++) diag[k] = 0.0f;
  float pc[3];
  for (int r = 0; r < 3; r++) {
    float sum = 0.0f;
    for (int k = 0; k < 3; k++) sum += f.view.Rcw[3 * r + k] * mp.pos[k];
    pc[r] = sum + f.view.tcw[r];
  }
  if (pc[2] < 0.0f) return kBehind;
  const float invz = 1.0f / pc[2];
  const float u = f.view.fx * pc[0] * invz + f.view.cx;
  const float v = f.view.fy * pc[1] * invz + f.view.cy;
  diag[0] = canonical(u);
  diag[1] = canonical(v);
  if (!finite32(u) || !finite32(v)) return kNotFinite;
  if (u < f.min_x || u > f.max_x) return kOutsideU;
  if (v < f.min_y || v > f.max_y) return kOutsideV;
  float po[3];
  for (int k = 0; k < 3; k++) po[k] = mp.pos[k] - f.Ow[k];
  const float dist = (float)sqrt((double)po[0] * (double)po[0] + (double)po[1] * (double)po[1] + (double)po[2] * (double)po[2]);
  diag[2] = canonical(dist);
  if (!finite32(dist)) return kNotFinite;
  if (dist > mp.max_distance) return kTooFar;
  const double dot = (double)po[0] * (double)mp.normal[0] + (double)po[1] * (double)mp.normal[1] + (double)po[2] * (double)mp.normal[2];
  const float view_cos = (float)(dot / (double)dist);
  diag[3] = canonical(view_cos);
  if (!finite32(view_cos)) return kNotFinite;
  if (view_cos < f.cos_limit) return kViewAngle;
  return kVisible;
}

// index of `key` in the strictly increasing a[lo, hi), or -1.  At most 32 halvings.
MSF_HD int find_key(const int32_t* a, int lo, int hi, int32_t key) {
  for (int it = 0; it < 32 && lo < hi; it++) {
    const int mid = lo + (hi - lo) / 2;
    const int32_t v = a[mid];
    if (v == key) return mid;
    if (v < key) lo = mid + 1; else hi = mid;
  }
  return -1;
}

// the key frame of entry e: the last i in [0, n_kf) with kf_start[i] <= e (empty key frames in front of it share the
// start and are passed over).  kf_start non-decreasing from 0, e in [0, n_entries).
MSF_HD int kf_of_entry(const int32_t* kf_start, int n_kf, int32_t e) {
  int lo = 0, hi = n_kf;   // the answer is in [lo, hi)
  for (int it = 0; it < 32 && hi - lo > 1; it++) {
    const int mid = lo + (hi - lo) / 2;
    if (kf_start[mid] <= e) lo = mid; else hi = mid;
  }
  return lo;
}

// the pixel key of an end point, -1 outside the image
MSF_HD int32_t pixel_key(int32_t x, int32_t y, int width, int height) {
  return (x < 0 || y < 0 || x >= width || y >= height) ? -1 : y * width + x;
}

// Step 4 without the tie: 1..3, or kClaimed for a candidate with *point = the point at k2 and *key = k1.
MSF_HD int claim_candidate(const Map& m, int kf, const Match& q, int width, int height, int32_t* key, int32_t* point) {
  const int32_t k1 = pixel_key(q.x1, q.y1, width, height);
  if (k1 < 0) return kNoKey1;
  if (find_key(m.cur_key, 0, m.n_cur, k1) >= 0) return kOccupied;
  const int32_t k2 = pixel_key(q.x2, q.y2, width, height);
  const int e = k2 < 0 ? -1 : find_key(m.kf_key, m.kf_start[kf], m.kf_start[kf + 1], k2);
  if (e < 0) return kNoPoint2;
  *key = k1;
  *point = m.kf_point[e];
  return kClaimed;
}

// ---- the host build: the five steps on plain memory, one thread ----------------------------------------------------

// nullptr for a usable map, else what is wrong with it: the refusals of the host entry points, and what the checking
// kernel answers with status_word = -1
inline const char* map_fault(const Map& m, int width, int height) {
  if (m.n_points < 0 || m.n_kf < 0 || m.n_entries < 0 || m.n_cur < 0) return "a negative count";
  if ((m.n_points && !m.points) || (m.n_entries && (!m.kf_key || !m.kf_point)) || (m.n_cur && (!m.cur_key || !m.cur_point)) ||
      (m.n_kf && !m.kf_start))
    return "a required pointer is NULL";
  if (m.n_kf == 0 && m.n_entries != 0) return "entries without a key frame";
  const long long n_px = (long long)width * height;
  if (m.n_kf && (m.kf_start[0] != 0 || m.kf_start[m.n_kf] != m.n_entries)) return "kf_start does not run from 0 to n_entries";
  for (int i = 0; i < m.n_kf; i++) {
    const int32_t a = m.kf_start[i], b = m.kf_start[i + 1];
    if (a < 0 || b < a || b > m.n_entries) return "kf_start is not non-decreasing inside [0, n_entries]";
    for (int32_t e = a; e < b; e++) {
      if (m.kf_key[e] < 0 || m.kf_key[e] >= n_px) return "a key frame's key is outside the image";
      if (e > a && m.kf_key[e] <= m.kf_key[e - 1]) return "a key frame's keys are not strictly increasing";
      if (m.kf_point[e] < 0 || m.kf_point[e] >= m.n_points) return "kf_point is out of range";
    }
  }
  for (int i = 0; i < m.n_points; i++)
    if (m.points[i].flags & ~(kBad | kSeen)) return "flag bits above 1 are set";
  for (int i = 0; i < m.n_cur; i++) {
    if (m.cur_key[i] < 0 || m.cur_key[i] >= n_px) return "cur_key is outside the image";
    if (i > 0 && m.cur_key[i] <= m.cur_key[i - 1]) return "cur_key is not strictly increasing";
    if (m.cur_point[i] < 0 || m.cur_point[i] >= m.n_points) return "cur_point is out of range";
  }
  return nullptr;
}

inline const char* frustum_fault(const Frustum& f) {
  if (f.min_x != f.min_x || f.max_x != f.max_x || f.min_y != f.min_y || f.max_y != f.max_y || f.cos_limit != f.cos_limit)
    return "a bound is NaN";
  return nullptr;
}

// Steps 1-2 on a checked map.  owner [n_points] scratch; every output optional except n_to_match [n_kf].
inline void host_frustum(const Map& m, const Frustum& f, int32_t* owner, int32_t* n_to_match, uint8_t* status,
                         uint8_t* visible, int32_t* owner_kf, float* u, float* v, float* dist, float* view_cos) {
  for (int p = 0; p < m.n_points; p++) owner[p] = -1;
  for (int32_t e = m.n_entries - 1; e >= 0; e--) owner[m.kf_point[e]] = e;   // the smallest e stays
  for (int i = 0; i < m.n_kf; i++) n_to_match[i] = 0;
  for (int p = 0; p < m.n_points; p++) {
    float diag[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    const int kf = owner[p] < 0 ? -1 : kf_of_entry(m.kf_start, m.n_kf, owner[p]);
    int s;
    if (kf < 0) s = kNoEntry;
    else if (m.points[p].flags & kBad) s = kIsBad;
    else if (m.points[p].flags & kSeen) s = kIsSeen;
    else s = frustum_point(m.points[p], f, diag);
    if (s == kVisible) n_to_match[kf]++;
    if (status) status[p] = (uint8_t)s;
    if (visible) visible[p] = s == kVisible;
    if (owner_kf) owner_kf[p] = kf;
    if (u) u[p] = diag[0];
    if (v) v[p] = diag[1];
    if (dist) dist[p] = diag[2];
    if (view_cos) view_cos[p] = diag[3];
  }
}

// Steps 4-5 on a checked map.  pixel_word [width * height] scratch, all zero on entry and on return.  Required:
// n_claimed [n_kf]; optional: claims [n_kf * cap], claim_status [n_kf][cap], and the correspondences (all four or none).
// Returns n_claims.
inline int32_t host_claims(const Map& m, int width, int height, const Match* matches, int cap, const int32_t* n_out,
                           const uint8_t* matched, uint32_t* pixel_word, int32_t* n_claimed, Claim* claims,
                           uint8_t* claim_status, int32_t corr_cap, int32_t* n_corr, float* corr_p3d, float* corr_p2d,
                           int32_t* corr_point) {
  auto length = [&](int i) {
    if (!matched[i] || n_out[i] < 0) return 0;
    return n_out[i] < cap ? n_out[i] : cap;
  };
  for (int i = 0; i < m.n_kf; i++)
    for (int j = 0; j < length(i); j++) {
      int32_t key, point;
      if (claim_candidate(m, i, matches[(size_t)i * cap + j], width, height, &key, &point) != kClaimed) continue;
      const uint32_t w = kTop - (uint32_t)(i * cap + j);
      if (w > pixel_word[key]) pixel_word[key] = w;
    }
  int32_t total = 0;
  for (int i = 0; i < m.n_kf; i++) {
    n_claimed[i] = 0;
    for (int j = 0; j < length(i); j++) {
      int32_t key = -1, point = -1;
      int s = claim_candidate(m, i, matches[(size_t)i * cap + j], width, height, &key, &point);
      if (s == kClaimed && pixel_word[key] != kTop - (uint32_t)(i * cap + j)) s = kLost;
      if (claim_status) claim_status[(size_t)i * cap + j] = (uint8_t)s;
      if (s != kClaimed) continue;
      if (claims) claims[total] = Claim{key, point, i, j};
      n_claimed[i]++;
      total++;
    }
  }
  // the words go back to zero, and the correspondences are written behind the count
  const bool corr = n_corr && corr_p3d && corr_p2d && corr_point;
  const bool fits = (long long)m.n_cur + total <= corr_cap;
  if (corr) *n_corr = fits ? m.n_cur + total : -1;
  auto put = [&](int at, int32_t key, int32_t point) {
    corr_p2d[2 * at] = (float)(key % width);
    corr_p2d[2 * at + 1] = (float)(key / width);
    for (int k = 0; k < 3; k++) corr_p3d[3 * at + k] = m.points[point].pos[k];
    corr_point[at] = point;
  };
  if (corr && fits)
    for (int c = 0; c < m.n_cur; c++) put(c, m.cur_key[c], m.cur_point[c]);
  int at = 0;
  for (int i = 0; i < m.n_kf; i++)
    for (int j = 0; j < length(i); j++) {
      int32_t key, point;
      if (claim_candidate(m, i, matches[(size_t)i * cap + j], width, height, &key, &point) != kClaimed) continue;
      if (pixel_word[key] == kTop - (uint32_t)(i * cap + j)) {
        if (corr && fits) put(m.n_cur + at, key, point);
        at++;
        pixel_word[key] = 0;
      }
    }
  return total;
}

// ---- the family's workspace ---------------------------------------------------------------------------------------

// Scratch of one call of the family.  The first zeroed_bytes, from `bad` on, are one run that a single clear of zeros
// prepares: the bad-map word, the owner words, the n_to_match counters and the pixel words.
struct Scratch {
  size_t zeroed_bytes = 0;
  int32_t* bad = nullptr;           // [1]: non-zero once the checking kernel found a fault
  uint32_t* owner = nullptr;        // [n_points]: kTop - the smallest entry index, 0 = none
  int32_t* to_match = nullptr;      // [n_kf]
  uint32_t* pixel_word = nullptr;   // [pixels]: kTop - the smallest ordinal that claims the pixel, 0 = none
  int32_t* cand = nullptr;          // [n_kf * cap]: per match the candidate's point, or -(claim status)
  Claim* rows = nullptr;            // [n_kf * cap]: the winners per key frame, in match order
};

// the one layout of the family: pixels = width * height for a call that claims, 0 for the frustum alone
inline void layout(Carver& c, size_t n_points, size_t n_kf, size_t pixels, size_t cap, Scratch* s) {
  const size_t begin = c.off;
  s->bad = c.take<int32_t>(1);
  s->owner = c.take<uint32_t>(n_points);
  s->to_match = c.take<int32_t>(n_kf);
  s->pixel_word = c.take<uint32_t>(pixels);
  s->zeroed_bytes = c.off - begin;
  s->cand = c.take<int32_t>(n_kf * cap);
  s->rows = c.take<Claim>(n_kf * cap);
}

}  // namespace tracking
}  // namespace msf

#endif  // MSF_TRACKING_SOLVE_H
