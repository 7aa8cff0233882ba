// The body of Tracking::TrackWithMotionModel / TrackReferenceKeyFrame (slam_pipeline/src/Tracking.cc:434-485, :380-424)
// around k_pose_optimize, as include/msf_frame_tracking.h states it.  The index rules are frame_tracking_solve.h, shared
// with a host build.
//   k_carry   one workgroup of 1024: the map checked index by index (nothing of it was seen by the host in a _device
//             call), the gate, one 64-bit word (key << 32) | rank per entry of the frame and per match in LDS (the
//             binary search over ref_key rides in it), a bitonic sort of the words in LDS, the last word of every run of
//             equal keys packed by wave ballot and prefix: the frame's map after the carry, in key order, with its
//             correspondences.  8192 words = 64 KiB of the workgroup's 160 KiB.
//   k_cut     one workgroup of 256 behind k_pose_optimize: kept and removed packed by ballot and prefix, one integer
//             sum (the kept records whose point is observed), the pose, the status word; and every scalar of the call
//             once more side by side (ftrack::Scratch::summary), for the host call's one small copy.
// No global atomics, no per-pixel words, no clear: the launches hand on two words (ftrack::Scratch::state).
//
// Order independence: what crosses threads is one integer OR (the map's fault bit, in LDS), the sorted words -- a
// permutation that does not depend on who compared what: the words are distinct but for kNoWord, which carries
// nothing -- and integer counts of ballots.  No floating-point atomics, no spins, every loop bounded (the counts of the
// call, 13 * 14 / 2 sort stages, 32 halvings).  So a call is bit-identical to its replay.
//
// A call that cannot run (malformed map, no list, no room): k_carry decides that before it writes anything, leaves the
// negative status in state[0] and -1 as the optimiser's length, and the last launch of the call writes track_status --
// nothing else of the outputs is written.
#include <hip/hip_runtime.h>

#include <mutex>
#include <stdint.h>

#include "frame_tracking_pipeline.h"

namespace msf {

namespace ft = ftrack;

static_assert(sizeof(ft::FramePoint) == sizeof(msfx_frame_point) && sizeof(msfx_frame_point) == 16, "msfx_frame_point layout");
static_assert(sizeof(ft::Removed) == sizeof(msfx_removed_point) && sizeof(msfx_removed_point) == 8, "msfx_removed_point layout");
static_assert(ft::kMaxCandidates == MSFX_TRACK_MAX_CANDIDATES, "the interface limit");

namespace {

constexpr int kCarryThreads = 1024, kCarryWaves = kCarryThreads / 64;

// grid: one workgroup of 1024; dynamic LDS: pow2_at_least(min(n_cur + cap, 8192)) words
__global__ __launch_bounds__(kCarryThreads) void k_carry(ft::Map m, int width, int height, CarryIn in, ft::Scratch s,
                                                         CarryOut out, int last) {
  extern __shared__ uint64_t words[];
  __shared__ int wave_count[kCarryWaves];
  __shared__ int bad;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) bad = 0;
  __syncthreads();
  // step 0: every index is checked before any is used
  const long long n_px = (long long)width * height;
  bool fault = false;
  for (int i = tid; i < m.n_ref; i += kCarryThreads) fault |= ft::entry_fault(m.ref_key, m.ref_point, i, n_px, m.n_points);
  for (int i = tid; i < m.n_cur; i += kCarryThreads) fault |= ft::entry_fault(m.cur_key, m.cur_point, i, n_px, m.n_points);
  if (fault) atomicOr(&bad, 1);
  __syncthreads();
  // step 1
  bool gated = false;
  const int len = bad ? ft::kBadMap : ft::list_length(in.n_out[0], in.cap, in.min_matches, m.n_cur, in.corr_cap, &gated);
  if (len < 0) {   // uniform
    if (tid == 0) {
      s.state[0] = len;
      s.state[1] = -1;
      if (last) *out.track_status = len;
    }
    return;
  }
  if (in.tcw0_device && tid < 12) in.tcw0_device[tid] = in.tcw0[tid];
  // step 2: the words.  total <= min(corr_cap, 8192) and total <= n_cur + cap, so p2 words are inside the LDS block.
  const int total = m.n_cur + len, p2 = ft::pow2_at_least(total);
  for (int i = tid; i < p2; i += kCarryThreads) {
    uint64_t w = ft::kNoWord;
    if (i < m.n_cur) {
      w = ft::word_of(m.cur_key[i], i);
    } else if (i < total) {
      const int j = i - m.n_cur;   // < len <= cap
      const msf_match mm = in.matches[j];
      int32_t key = -1, point = -1;
      const int status = ft::carry_candidate(m, tracking::Match{mm.x1, mm.y1, mm.x2, mm.y2}, width, height, &key, &point);
      if (status == ft::kCarried) w = ft::word_of(key, i);
      else out.carry_status[j] = (uint8_t)status;
    }
    words[i] = w;
  }
  __syncthreads();
  for (int k = 2; k <= p2; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < p2; i += kCarryThreads) {
        const int l = i ^ j;
        if (l <= i) continue;
        const uint64_t a = words[i], b = words[l];
        if ((a > b) == ((i & k) == 0)) {
          words[i] = b;
          words[l] = a;
        }
      }
      __syncthreads();
    }
  // step 3: the winners in word order = key order.  A record's place is the number of winners in front of it.
  int offset = 0;
  const int chunks = (total + kCarryThreads - 1) / kCarryThreads;
  for (int chunk = 0; chunk < chunks; chunk++) {
    const int i = chunk * kCarryThreads + tid;
    bool won = false;
    uint64_t w = ft::kNoWord;
    if (i < total) {
      w = words[i];
      won = ft::wins(words, i, p2);
      if (w != ft::kNoWord) {
        const int r = ft::rank_of(w);
        if (r < m.n_cur) out.cur_status[r] = won ? 0 : 1;
        else out.carry_status[r - m.n_cur] = (uint8_t)(won ? ft::kCarried : ft::kOverwritten);
      }
    }
    const unsigned long long ballot = __ballot(won);
    if (lane == 0) wave_count[wave] = __popcll(ballot);
    __syncthreads();
    int before = 0, sum = 0;
    for (int v = 0; v < kCarryWaves; v++) {
      const int c = wave_count[v];
      before += v < wave ? c : 0;
      sum += c;
    }
    if (won) {
      const int at = offset + before + __popcll(ballot & ((1ull << lane) - 1ull));   // < total <= corr_cap
      const int32_t key = ft::key_of(w), r = ft::rank_of(w);
      int32_t point, k1;
      if (r < m.n_cur) {
        point = m.cur_point[r];
      } else {
        const msf_match mm = in.matches[r - m.n_cur];
        ft::carry_candidate(m, tracking::Match{mm.x1, mm.y1, mm.x2, mm.y2}, width, height, &k1, &point);   // a candidate
      }
      out.map[at] = msfx_frame_point{key, point, r < m.n_cur ? -1 : r - m.n_cur, 0};
      ft::put_corr(m, width, at, key, point, out.corr_p3d, out.corr_p2d, out.corr_point);
    }
    offset += sum;
    __syncthreads();   // wave_count is rewritten by the next chunk
  }
  if (tid == 0) {
    *out.n_map = offset;
    s.state[0] = gated ? ft::kFewMatches : ft::kTracked;
    s.state[1] = gated ? -1 : offset;
    if (last) *out.track_status = ft::kTracked;
  }
}

// grid: one workgroup of 256; the records in chunks of 256
__global__ __launch_bounds__(256) void k_cut(ft::Map m, CutIn in, ft::Scratch s, CutOut out) {
  __shared__ int wave_count[3][4];   // kept, removed, kept and observed
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int carried = s.state[0];
  if (carried < 0) {   // uniform
    if (tid == 0) {
      *out.track_status = carried;
      s.summary[ft::kSumStatus] = carried;
      s.summary[ft::kSumNumMatches] = in.n_out[0];
    }
    return;
  }
  const bool gated = carried == ft::kFewMatches;
  const int n_map = *out.n_map;
  int n_kept = 0, n_gone = 0, n_seen = 0;
  const int chunks = (n_map + 255) / 256;
  for (int chunk = 0; chunk < chunks; chunk++) {
    const int i = chunk * 256 + tid;
    bool keep = false, gone = false, seen = false;
    msfx_frame_point rec{};
    if (i < n_map) {
      rec = out.map[i];
      gone = !gated && in.outliers[i] != 0;
      keep = !gone;
      seen = keep && ft::observed(m, rec.point);
    }
    const unsigned long long bk = __ballot(keep), bg = __ballot(gone), bs = __ballot(seen);
    if (lane == 0) {
      wave_count[0][wave] = __popcll(bk);
      wave_count[1][wave] = __popcll(bg);
      wave_count[2][wave] = __popcll(bs);
    }
    __syncthreads();
    int before_k = 0, before_g = 0, sum_k = 0, sum_g = 0, sum_s = 0;
    for (int v = 0; v < 4; v++) {
      before_k += v < wave ? wave_count[0][v] : 0;
      before_g += v < wave ? wave_count[1][v] : 0;
      sum_k += wave_count[0][v];
      sum_g += wave_count[1][v];
      sum_s += wave_count[2][v];
    }
    const unsigned long long below = (1ull << lane) - 1ull;
    if (keep) {
      const int at = n_kept + before_k + __popcll(bk & below);   // < n_map
      out.kept_key[at] = rec.key;
      out.kept_point[at] = rec.point;
    }
    if (gone) {
      const int at = n_gone + before_g + __popcll(bg & below);
      out.removed[at] = msfx_removed_point{rec.key, rec.point};
      out.map[i].flags = rec.flags | 1;
    }
    n_kept += sum_k, n_gone += sum_g, n_seen += sum_s;
    __syncthreads();   // wave_count is rewritten by the next chunk
  }
  if (tid < 12) {
    const float t = gated ? in.tcw0[tid] : in.pose_tcw[tid];
    out.tcw[tid] = t;
    s.summary[ft::kSumTcw + tid] = __float_as_int(t);
  }
  if (tid == 0) {
    const int32_t n_good = gated ? -1 : *in.pose_n_good;
    const int32_t status = gated ? ft::kFewMatches : n_seen >= in.min_map_matches ? ft::kTracked : ft::kFewMapMatches;
    *out.n_good = n_good;
    *out.n_kept = n_kept;
    *out.n_removed = n_gone;
    *out.n_matches_map = n_seen;
    *out.track_status = status;
    s.summary[ft::kSumStatus] = status, s.summary[ft::kSumMap] = n_map, s.summary[ft::kSumKept] = n_kept;
    s.summary[ft::kSumRemoved] = n_gone, s.summary[ft::kSumGood] = n_good, s.summary[ft::kSumMatchesMap] = n_seen;
    s.summary[ft::kSumNumMatches] = in.n_out[0];
  }
}

}  // namespace

hipError_t frame_tracking_carry(const ft::Map& map, int width, int height, const CarryIn& in, const ft::Scratch& s,
                                const CarryOut& out, bool last, hipStream_t st) {
  static std::once_flag attr_once;   // handles on several host threads may arrive here together
  std::call_once(attr_once, [] {
    hipFuncSetAttribute(reinterpret_cast<const void*>(k_carry), hipFuncAttributeMaxDynamicSharedMemorySize,
                        ft::kMaxCandidates * (int)sizeof(uint64_t));
  });
  const long long most = (long long)map.n_cur + in.cap;
  const size_t lds = (size_t)ft::pow2_at_least(most < ft::kMaxCandidates ? (int)most : ft::kMaxCandidates) * sizeof(uint64_t);
  hipLaunchKernelGGL(k_carry, dim3(1), dim3(kCarryThreads), lds, st, map, width, height, in, s, out, last ? 1 : 0);
  return hipGetLastError();
}

hipError_t frame_tracking_cut(const ft::Map& map, const CutIn& in, const ft::Scratch& s, const CutOut& out, hipStream_t st) {
  hipLaunchKernelGGL(k_cut, dim3(1), dim3(256), 0, st, map, in, s, out);
  return hipGetLastError();
}

}  // namespace msf
