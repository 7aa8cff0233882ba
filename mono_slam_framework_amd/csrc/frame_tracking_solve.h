// The index rules of the body of Tracking::TrackWithMotionModel / TrackReferenceKeyFrame (slam_pipeline/src/Tracking.cc
// :434-485, :380-424) as include/msf_frame_tracking.h states them: one match -> its carry status, one sorted run of
// candidates -> its winner, one record + outlier byte -> kept or removed.  Plain C++ shared by
// frame_tracking_kernels.hip and by a host build (tests/cpp/frame_tracking_host.cpp,
// tests/cpp/frame_tracking_edge_main.cpp), so every step can be checked against the reference and run under the
// sanitizers without a GPU.  No floating-point arithmetic in here but the int -> float of a pixel.
//
// The carry as a sort: every entry of the frame and every candidate match becomes one 64-bit word (key << 32) | rank,
// rank = c for entry c and n_cur + j for match j.  In ascending word order the LAST word of every run of equal keys is
// the winner: a match outranks an entry, a later match an earlier one -- SetMapPoint overwriting in list order -- and
// the winners are in ascending key order.  A match that is no candidate is the word kNoWord, behind every key.
#ifndef MSF_FRAME_TRACKING_SOLVE_H
#define MSF_FRAME_TRACKING_SOLVE_H

#include <stdint.h>

#include "tracking_solve.h"

namespace msf {
namespace ftrack {

namespace tk = tracking;

struct FramePoint {
  int32_t key, point, match, flags;
};

struct Removed {
  int32_t key, point;
};

// msfx_frame_map without its header words
struct Map {
  int32_t n_points, n_ref, n_cur;
  const tk::Point* points;
  const uint8_t* observed;
  const int32_t* ref_key;
  const int32_t* ref_point;
  const int32_t* cur_key;
  const int32_t* cur_point;
};

constexpr int kMaxCandidates = 8192;   // MSFX_TRACK_MAX_CANDIDATES
constexpr int kCarried = 0, kNoKey1 = 1, kNoPoint2 = 3, kOverwritten = 4;
constexpr int kTracked = 0, kFewMatches = 1, kFewMapMatches = 2, kBadMap = -1, kNoRoom = -2, kNoList = -3;
constexpr uint64_t kNoWord = ~0ull;

// Step 2 without the tie: kNoKey1, kNoPoint2, or kCarried for a candidate with *key = k1 and *point = the point at k2.
MSF_HD int carry_candidate(const Map& m, const tk::Match& q, int width, int height, int32_t* key, int32_t* point) {
  const int32_t k1 = tk::pixel_key(q.x1, q.y1, width, height);
  if (k1 < 0) return kNoKey1;
  const int32_t k2 = tk::pixel_key(q.x2, q.y2, width, height);
  const int e = k2 < 0 ? -1 : tk::find_key(m.ref_key, 0, m.n_ref, k2);
  if (e < 0) return kNoPoint2;
  *key = k1;
  *point = m.ref_point[e];
  return kCarried;
}

MSF_HD uint64_t word_of(int32_t key, int32_t rank) { return ((uint64_t)(uint32_t)key << 32) | (uint32_t)rank; }
MSF_HD int32_t key_of(uint64_t w) { return (int32_t)(w >> 32); }
MSF_HD int32_t rank_of(uint64_t w) { return (int32_t)(uint32_t)w; }

// is sorted[i] the last word of its run?  `n` words; kNoWord is never a winner.
MSF_HD bool wins(const uint64_t* sorted, int i, int n) {
  const uint64_t w = sorted[i];
  if (w == kNoWord) return false;
  return i + 1 >= n || (sorted[i + 1] >> 32) != (w >> 32);
}

// one entry of a sorted key table, checked: inside the image, above its predecessor, its point in range
MSF_HD bool entry_fault(const int32_t* key, const int32_t* point, int i, long long n_px, int n_points) {
  return key[i] < 0 || key[i] >= n_px || (i > 0 && key[i] <= key[i - 1]) || point[i] < 0 || point[i] >= n_points;
}

// The list's length behind the gate, or a negative status.  *gated: n < min_matches (the list then counts as empty).
MSF_HD int list_length(int32_t n, int cap, int min_matches, int n_cur, int corr_cap, bool* gated) {
  *gated = false;
  if (n < 0) return kNoList;
  int len = n < cap ? n : cap;
  if (n < min_matches) {
    *gated = true;
    len = 0;
  }
  const int room = corr_cap < kMaxCandidates ? corr_cap : kMaxCandidates;
  if ((long long)n_cur + len > room) return kNoRoom;
  return len;
}

MSF_HD bool observed(const Map& m, int32_t point) { return !m.observed || m.observed[point] != 0; }

MSF_HD void put_corr(const Map& m, int width, int at, int32_t key, int32_t point, float* p3d, float* p2d, int32_t* cp) {
  if (p2d) {
    p2d[2 * at] = (float)(key % width);
    p2d[2 * at + 1] = (float)(key / width);
  }
  if (p3d)
    for (int k = 0; k < 3; k++) p3d[3 * at + k] = m.points[point].pos[k];
  if (cp) cp[at] = point;
}

// ---- the host build: the steps on plain memory, one thread --------------------------------------------------------

// nullptr for a usable map, else what is wrong with it: the refusal of msfx_track_frame, and what the carry kernel
// answers with track_status = -1
inline const char* map_fault(const Map& m, int width, int height) {
  if (m.n_points < 0 || m.n_ref < 0 || m.n_cur < 0) return "a negative count";
  if ((m.n_points && !m.points) || (m.n_ref && (!m.ref_key || !m.ref_point)) || (m.n_cur && (!m.cur_key || !m.cur_point)))
    return "a required pointer of map is NULL";
  const long long n_px = (long long)width * height;
  for (int i = 0; i < m.n_ref; i++)
    if (entry_fault(m.ref_key, m.ref_point, i, n_px, m.n_points))
      return "ref_key is outside the image or not strictly increasing, or ref_point is out of range";
  for (int i = 0; i < m.n_cur; i++)
    if (entry_fault(m.cur_key, m.cur_point, i, n_px, m.n_points))
      return "cur_key is outside the image or not strictly increasing, or cur_point is out of range";
  return nullptr;
}

// In-place ascending sort of n words, n a power of two: the bitonic network the kernel runs, one compare-exchange at a
// time.
inline void bitonic_sort(uint64_t* w, int n) {
  for (int k = 2; k <= n; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1)
      for (int i = 0; i < n; i++) {
        const int l = i ^ j;
        if (l <= i) continue;
        const bool up = (i & k) == 0;
        if ((w[i] > w[l]) == up) {
          const uint64_t t = w[i];
          w[i] = w[l];
          w[l] = t;
        }
      }
}

MSF_HD int pow2_at_least(int n) {
  int p = 1;
  for (int it = 0; it < 31 && p < n; it++) p <<= 1;
  return p;
}

// Steps 0-3.  words [pow2_at_least(n_cur + min(n, cap))] scratch.  Every output optional.  Returns the status the
// carry leaves: kTracked, kFewMatches (gated), or a negative one (then nothing was written); *n_map_out is written for
// the first two.
inline int host_carry(const Map& m, int width, int height, const tk::Match* matches, int cap, int32_t n, int min_matches,
                      int corr_cap, uint64_t* words, int32_t* n_map_out, FramePoint* map, uint8_t* carry_status,
                      uint8_t* cur_status, float* corr_p3d, float* corr_p2d, int32_t* corr_point) {
  if (map_fault(m, width, height)) return kBadMap;
  bool gated;
  const int len = list_length(n, cap, min_matches, m.n_cur, corr_cap, &gated);
  if (len < 0) return len;
  const int total = m.n_cur + len, p2 = pow2_at_least(total);
  for (int c = 0; c < m.n_cur; c++) words[c] = word_of(m.cur_key[c], c);
  for (int j = 0; j < len; j++) {
    int32_t key = -1, point = -1;
    const int s = carry_candidate(m, matches[j], width, height, &key, &point);
    words[m.n_cur + j] = s == kCarried ? word_of(key, m.n_cur + j) : kNoWord;
    if (s != kCarried && carry_status) carry_status[j] = (uint8_t)s;
  }
  for (int i = total; i < p2; i++) words[i] = kNoWord;
  bitonic_sort(words, p2);
  int at = 0;
  for (int i = 0; i < total; i++) {
    if (words[i] == kNoWord) break;
    const bool won = wins(words, i, p2);
    const int32_t key = key_of(words[i]), r = rank_of(words[i]);
    if (r < m.n_cur) {
      if (cur_status) cur_status[r] = won ? 0 : 1;
    } else if (carry_status) {
      carry_status[r - m.n_cur] = (uint8_t)(won ? kCarried : kOverwritten);
    }
    if (!won) continue;
    int32_t point = -1, k = -1;
    if (r < m.n_cur) point = m.cur_point[r];
    else carry_candidate(m, matches[r - m.n_cur], width, height, &k, &point);
    if (map) map[at] = FramePoint{key, point, r < m.n_cur ? -1 : r - m.n_cur, 0};
    put_corr(m, width, at, key, point, corr_p3d, corr_p2d, corr_point);
    at++;
  }
  *n_map_out = at;
  return gated ? kFewMatches : kTracked;
}

// Steps 5-6 on the records of host_carry (which returned `carried` >= 0).  outliers [n_map] (ignored when gated).
// Every output optional; returns track_status.
inline int host_cut(const Map& m, int carried, int n_map, FramePoint* map, const uint8_t* outliers, int min_map_matches,
                    int32_t* n_kept, int32_t* kept_key, int32_t* kept_point, int32_t* n_removed, Removed* removed,
                    int32_t* n_matches_map) {
  int kept = 0, gone = 0, seen = 0;
  for (int i = 0; i < n_map; i++) {
    const bool out = carried == kTracked && outliers[i] != 0;
    if (out) {
      map[i].flags |= 1;
      if (removed) removed[gone] = Removed{map[i].key, map[i].point};
      gone++;
    } else {
      if (kept_key) kept_key[kept] = map[i].key;
      if (kept_point) kept_point[kept] = map[i].point;
      kept++;
      seen += observed(m, map[i].point);
    }
  }
  if (n_kept) *n_kept = kept;
  if (n_removed) *n_removed = gone;
  if (n_matches_map) *n_matches_map = seen;
  if (carried == kFewMatches) return kFewMatches;
  return seen >= min_map_matches ? kTracked : kFewMapMatches;
}

// ---- the family's workspace ---------------------------------------------------------------------------------------

// What the launches of one call hand on: written by the carry, read by k_pose_optimize and the cut.
struct Scratch {
  int32_t* state = nullptr;     // [2]: the status the carry leaves; d_n of the optimiser (n_map, or -1)
  int32_t* summary = nullptr;   // [kSummaryWords]: what the cut leaves for the host call's one small copy
};

// The summary: every scalar of a call side by side, so that msfx_track_frame learns them -- and with them how much of
// every array there is to fetch -- from one copy.  Tcw as the bits of its 12 floats.
enum { kSumStatus = 0, kSumMap, kSumKept, kSumRemoved, kSumGood, kSumMatchesMap, kSumNumMatches, kSumTcw = 8, kSummaryWords = 20 };

inline void layout(Carver& c, Scratch* s) {
  s->state = c.take<int32_t>(2);
  s->summary = c.take<int32_t>(kSummaryWords);
}

}  // namespace ftrack
}  // namespace msf

#endif  // MSF_FRAME_TRACKING_SOLVE_H
