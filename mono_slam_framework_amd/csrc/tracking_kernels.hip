// Tracking::SearchLocalPoints (slam_pipeline/src/Tracking.cc:594-632) around the matcher, as include/msf_tracking.h
// states it.  The arithmetic and the index rules are tracking_solve.h, shared with a host build.
//   k_track_check   the local map checked index by index (nothing of it was seen by the host in a _device call); the
//                   owner pass rides in it: one thread per entry, an integer atomic max of kTop - e per point
//   k_frustum       one thread per point: owner -> key frame, the flags, Frame::isInFrustum; n_to_match by wave ballot
//                   and one integer add per wave and key frame
//   k_gate          one workgroup: n_to_match out, the train slots and the matched bytes of the gated match
//   k_claim_mark    one thread per match: the two lookups (binary searches over the sorted keys), an integer atomic max
//                   of kTop - ordinal into the word of the claimed pixel
//   k_claim_pack    one workgroup per key frame: the winners packed in match order (ballot + prefix, as k_new_points)
//   k_claim_finish  a prefix over n_claimed gives each key frame's offset: the records and the correspondences
// The minimum ordinal per pixel lives in one word per pixel of the image inside the family's workspace; the call's one
// clear of zeros (hipMemsetAsync in tracking_check) prepares it together with the owner words and the counters.
//
// Order independence: the only values that cross threads are integer maxima and integer sums (commutative, exact), each
// read by a LATER launch on the same stream; no floating-point atomics, no workgroup waits on another, no spins, every
// loop is bounded (chunks of a list, 32 halvings, 64 distinct key frames in a wave).  A record's place is the number of
// winners in front of it in ordinal order.  So a call is bit-identical to its replay.
//
// A malformed map: k_track_check sets s.bad, every later kernel returns at once when it reads it, and the last kernel
// of the call writes status_word = -1 -- nothing else of the outputs is written.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "tracking_pipeline.h"

namespace msf {

namespace tk = tracking;

static_assert(sizeof(tk::View) == sizeof(msf_view), "msf_view layout");
static_assert(sizeof(tk::Point) == sizeof(msf_map_point) && sizeof(msf_map_point) == 32, "msf_map_point layout");
static_assert(sizeof(tk::Match) == sizeof(msf_match), "msf_match layout");
static_assert(sizeof(tk::Claim) == sizeof(msf_local_claim) && sizeof(msf_local_claim) == 16, "msf_local_claim layout");

namespace {

// grid: n_kf + ceil(n_points / 256) + ceil(n_cur / 256) workgroups of 256.  The first n_kf take one key frame each and
// walk its entries in chunks of 256 (bounded by n_entries: the bounds of the run are checked first); the next check the
// points' flag words; the last the current frame's map.
__global__ __launch_bounds__(256) void k_track_check(tk::Map m, int width, int height, tk::Scratch s) {
  const int tid = threadIdx.x;
  const long long n_px = (long long)width * height;
  int block = blockIdx.x;
  if (block < m.n_kf) {
    const int i = block;
    const int32_t a = m.kf_start[i], b = m.kf_start[i + 1];
    const bool broken = a < 0 || b < a || b > m.n_entries || (i == 0 && a != 0) || (i == m.n_kf - 1 && b != m.n_entries);
    if (broken) {   // uniform
      if (tid == 0) atomicOr(s.bad, 1);
      return;
    }
    for (int32_t e = a + tid; e < b; e += 256) {
      const int32_t key = m.kf_key[e], p = m.kf_point[e];
      const bool fault = key < 0 || key >= n_px || (e > a && key <= m.kf_key[e - 1]) || p < 0 || p >= m.n_points;
      if (fault) atomicOr(s.bad, 1);
      else atomicMax(s.owner + p, tk::kTop - (uint32_t)e);
    }
    return;
  }
  block -= m.n_kf;
  const int point_blocks = (m.n_points + 255) / 256;
  if (block < point_blocks) {
    const int p = block * 256 + tid;
    if (p < m.n_points && (m.points[p].flags & ~(tk::kBad | tk::kSeen))) atomicOr(s.bad, 1);
    return;
  }
  const int c = (block - point_blocks) * 256 + tid;
  if (c < m.n_cur) {
    const int32_t key = m.cur_key[c], p = m.cur_point[c];
    if (key < 0 || key >= n_px || (c > 0 && key <= m.cur_key[c - 1]) || p < 0 || p >= m.n_points) atomicOr(s.bad, 1);
  }
}

// grid: ceil(n_points / 256) workgroups of 256, one thread per point.  The 32-byte record arrives as two 16-byte loads.
__global__ __launch_bounds__(256) void k_frustum(tk::Map m, tk::Frustum f, tk::Scratch s, FrustumOut out) {
  if (*s.bad) return;   // uniform
  const int p = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
  int want = -1;        // the key frame whose n_to_match this point adds to
  if (p < m.n_points) {
    const float4* rec = reinterpret_cast<const float4*>(m.points + p);
    const float4 lo = rec[0], hi = rec[1];
    tk::Point mp;
    mp.pos[0] = lo.x, mp.pos[1] = lo.y, mp.pos[2] = lo.z;
    mp.normal[0] = lo.w, mp.normal[1] = hi.x, mp.normal[2] = hi.y;
    mp.max_distance = hi.z;
    mp.flags = __float_as_uint(hi.w);
    const uint32_t w = s.owner[p];
    const int kf = w ? tk::kf_of_entry(m.kf_start, m.n_kf, (int32_t)(tk::kTop - w)) : -1;
    float diag[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    int status;
    if (kf < 0) status = tk::kNoEntry;
    else if (mp.flags & tk::kBad) status = tk::kIsBad;
    else if (mp.flags & tk::kSeen) status = tk::kIsSeen;
    else status = tk::frustum_point(mp, f, diag);
    if (status == tk::kVisible) want = kf;
    if (out.status) out.status[p] = (uint8_t)status;
    if (out.visible) out.visible[p] = status == tk::kVisible;
    if (out.owner_kf) out.owner_kf[p] = kf;
    if (out.u) out.u[p] = diag[0];
    if (out.v) out.v[p] = diag[1];
    if (out.dist) out.dist[p] = diag[2];
    if (out.view_cos) out.view_cos[p] = diag[3];
  }
  // one integer add per wave and key frame: at most 64 distinct key frames in a wave
  unsigned long long todo = __ballot(want >= 0);
  for (int it = 0; it < 64 && todo; it++) {
    const int leader = __ffsll((long long)todo) - 1;
    const int kf = __shfl(want, leader);
    const unsigned long long same = __ballot(want == kf);
    if (lane == leader) atomicAdd(s.to_match + kf, __popcll(same));
    todo &= ~same;
  }
}

// one workgroup of 256
__global__ __launch_bounds__(256) void k_gate(int n_kf, tk::Scratch s, FrustumOut out, GateOut gate) {
  const int tid = threadIdx.x;
  if (*s.bad) {   // uniform
    if (tid == 0) *out.status_word = -1;
    return;
  }
  for (int i = tid; i < n_kf; i += 256) {
    const int32_t n = s.to_match[i];
    out.n_to_match[i] = n;
    if (gate.train) gate.train[i] = n > 0 ? gate.slots[i] : -1;
    if (gate.matched) gate.matched[i] = n > 0;
  }
  if (tid == 0) *out.status_word = 0;
}

__device__ int list_length(const ClaimLists& in, int i) {
  if (!in.matched[i]) return 0;
  int n = in.n_out[i];
  if (n < 0) return 0;
  n = n < in.cap ? n : in.cap;
  return n < in.limit ? n : in.limit;
}

// grid: (ceil(min(cap, limit) / 256), n_kf) workgroups of 256, one thread per match
__global__ __launch_bounds__(256) void k_claim_mark(tk::Map m, int width, int height, ClaimLists in, tk::Scratch s) {
  if (*s.bad) return;   // uniform
  const int i = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
  if (j >= list_length(in, i)) return;
  const long long at = (long long)i * in.cap + j;   // the ordinal: < 2^31, checked by the entry point
  const msf_match mm = in.matches[at];
  int32_t key = -1, point = -1;
  const int status = tk::claim_candidate(m, i, tk::Match{mm.x1, mm.y1, mm.x2, mm.y2}, width, height, &key, &point);
  if (status == tk::kClaimed) atomicMax(s.pixel_word + key, tk::kTop - (uint32_t)at);   // key in [0, width * height)
  s.cand[at] = status == tk::kClaimed ? point : -status;
}

// grid: n_kf workgroups of 256; the workgroup walks its list in chunks of 256 matches.  A winner's record goes to
// rows[i * cap + (winners in front of it)]: ballot inside a wave, one LDS word per wave across the waves, a running
// offset across the chunks.
__global__ __launch_bounds__(256) void k_claim_pack(int width, int height, ClaimLists in, tk::Scratch s, ClaimOut out) {
  __shared__ int wave_count[4];
  if (*s.bad) return;   // uniform
  const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = list_length(in, i);
  const long long row = (long long)i * in.cap;
  int offset = 0;
  const int chunks = (n + 255) / 256;
  for (int chunk = 0; chunk < chunks; chunk++) {
    const int j = chunk * 256 + tid;
    bool won = false;
    int32_t key = -1, point = -1;
    if (j < n) {
      point = s.cand[row + j];
      int status = point >= 0 ? tk::kClaimed : -point;
      if (point >= 0) {
        const msf_match mm = in.matches[row + j];
        key = tk::pixel_key(mm.x1, mm.y1, width, height);   // a candidate: inside the image
        won = s.pixel_word[key] == tk::kTop - (uint32_t)(row + j);
        if (!won) status = tk::kLost;
      }
      if (out.claim_status) out.claim_status[row + j] = (uint8_t)status;
    }
    const unsigned long long ballot = __ballot(won);
    if (lane == 0) wave_count[wave] = __popcll(ballot);
    __syncthreads();
    int before = 0, total = 0;
    for (int w = 0; w < 4; w++) {
      const int c = wave_count[w];
      before += w < wave ? c : 0;
      total += c;
    }
    if (won) {
      const int at = offset + before + __popcll(ballot & ((1ull << lane) - 1ull));   // < n <= cap
      s.rows[row + at] = tk::Claim{key, point, i, j};
    }
    offset += total;
    __syncthreads();   // wave_count is rewritten by the next chunk
  }
  if (tid == 0) out.n_claimed[i] = offset;
}

__device__ void put_corr(const tk::Map& m, const ClaimOut& out, int width, long long at, int32_t key, int32_t point) {
  out.corr_p2d[2 * at] = (float)(key % width);
  out.corr_p2d[2 * at + 1] = (float)(key / width);
  for (int k = 0; k < 3; k++) out.corr_p3d[3 * at + k] = m.points[point].pos[k];
  out.corr_point[at] = point;
}

// grid: (ceil(max(min(cap, limit), n_cur, 1) / 256), n_kf + 1) workgroups of 256.  Row i < n_kf moves key frame i's
// winners to their place in ordinal order, claims[sum of n_claimed in front + j]; row n_kf writes the current frame's
// own correspondences and the counts.  Every workgroup sums n_claimed itself (integer adds in LDS).
__global__ __launch_bounds__(256) void k_claim_finish(tk::Map m, int width, int cap, tk::Scratch s, ClaimOut out) {
  __shared__ int sums[2];   // claims in front of this key frame, claims in all
  const int tid = threadIdx.x, i = blockIdx.y;
  if (*s.bad) {   // uniform
    if (tid == 0 && blockIdx.x == 0 && i == 0) *out.status_word = -1;
    return;
  }
  if (tid < 2) sums[tid] = 0;
  __syncthreads();
  int front = 0, all = 0;
  for (int k = tid; k < m.n_kf; k += 256) {
    const int c = out.n_claimed[k];
    front += k < i ? c : 0;
    all += c;
  }
  if (front) atomicAdd(&sums[0], front);
  if (all) atomicAdd(&sums[1], all);
  __syncthreads();
  const int offset = sums[0], total = sums[1];
  const bool corr = out.n_corr && out.corr_p3d && out.corr_p2d && out.corr_point;
  const bool fits = (long long)m.n_cur + total <= out.corr_cap;
  const int j = blockIdx.x * 256 + tid;
  if (i < m.n_kf) {
    if (j < out.n_claimed[i]) {
      const tk::Claim rec = s.rows[(long long)i * cap + j];
      if (out.claims) out.claims[offset + j] = msf_local_claim{rec.key, rec.point, rec.kf, rec.match};
      if (corr && fits) put_corr(m, out, width, (long long)m.n_cur + offset + j, rec.key, rec.point);
    }
    return;
  }
  if (corr && fits && j < m.n_cur) put_corr(m, out, width, j, m.cur_key[j], m.cur_point[j]);
  if (blockIdx.x == 0 && tid == 0) {
    *out.status_word = 0;
    *out.n_claims = total;
    if (corr) *out.n_corr = fits ? m.n_cur + total : -1;
  }
}

}  // namespace

hipError_t tracking_check(const tk::Map& map, int width, int height, const tk::Scratch& s, hipStream_t st) {
  const hipError_t e = hipMemsetAsync(s.bad, 0, s.zeroed_bytes, st);
  if (e != hipSuccess) return e;
  const int blocks = map.n_kf + (map.n_points + 255) / 256 + (map.n_cur + 255) / 256;
  if (blocks > 0) hipLaunchKernelGGL(k_track_check, dim3(blocks), dim3(256), 0, st, map, width, height, s);
  return hipGetLastError();
}

hipError_t tracking_frustum(const tk::Map& map, const tk::Frustum& f, const tk::Scratch& s, const FrustumOut& out,
                            const GateOut& gate, hipStream_t st) {
  if (map.n_points > 0)
    hipLaunchKernelGGL(k_frustum, dim3((map.n_points + 255) / 256), dim3(256), 0, st, map, f, s, out);
  hipLaunchKernelGGL(k_gate, dim3(1), dim3(256), 0, st, map.n_kf, s, out, gate);
  return hipGetLastError();
}

hipError_t tracking_claims(const tk::Map& map, int width, int height, const ClaimLists& in, const tk::Scratch& s,
                           const ClaimOut& out, hipStream_t st) {
  const int longest = in.cap < in.limit ? in.cap : in.limit;
  if (map.n_kf > 0) {
    hipLaunchKernelGGL(k_claim_mark, dim3((longest + 255) / 256, map.n_kf), dim3(256), 0, st, map, width, height, in, s);
    hipLaunchKernelGGL(k_claim_pack, dim3(map.n_kf), dim3(256), 0, st, width, height, in, s, out);
  }
  int widest = longest > map.n_cur ? longest : map.n_cur;
  widest = widest > 1 ? widest : 1;
  hipLaunchKernelGGL(k_claim_finish, dim3((widest + 255) / 256, map.n_kf + 1), dim3(256), 0, st, map, width, in.cap, s, out);
  return hipGetLastError();
}

}  // namespace msf
