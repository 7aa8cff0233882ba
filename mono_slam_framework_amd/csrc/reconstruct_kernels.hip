// The tail of Initializer::Initialize (slam_pipeline/src/Initializer.cc:137-147, 489-934) on the device, for one match
// list or a batch of them, behind msf_find_models_device:
//   k_motion_candidates  RH = SH / (SH + SF) picks H or F (:137-147); the 8 / 4 motion hypotheses of ReconstructH /
//                        ReconstructF (:599-698, :499-507 + DecomposeE :916-934) and N, the model's inlier count
//   k_check_rt           CheckRT (:806-914) of every hypothesis: Triangulate (:744-758) per inlier match, nGood, parallax
//   k_pick_motion        the two selection rules (:524-582, :700-741)
//   k_winner_points      vP3D and vbTriangulated of the winning hypothesis only
// The arithmetic is reconstruct_solve.h, shared with a host build that is checked against float64 without a GPU.  Every
// loop is bounded (ransac::kMaxSweeps Jacobi sweeps, 8 radix passes of 256 bins); no kernel waits on another workgroup.
//
// Order independence: nGood is a count and the parallax is one value of the multiset of cosParallax (the entry of rank
// min(50, nGood - 1)), found by radix selection over order-preserving 64-bit keys in LDS -- neither depends on which lane
// handled which match, so a list gives the same bits alone or in any batch.
#include <hip/hip_runtime.h>

#include <mutex>
#include <stdint.h>

#include "msf_abi.h"
#include "reconstruct_pipeline.h"
#include "reconstruct_solve.h"

namespace msf {

namespace rc = reconstruct;

__device__ __forceinline__ int motion_list_len(const MotionLists& in, int list) {
  if (!in.n_out) return in.n_single;
  const int n = in.n_out[list];
  return n < in.cap ? n : in.cap;
}

__device__ __forceinline__ bool motion_list_ok(int n) { return n >= 8 && n <= kMaxReconstructMatches; }

// Initialize's choice (:137-147) and ReconstructH / ReconstructF up to the hypotheses (:494-507, :590-698).
// One thread per list; grid: ceil(n_lists / 64) x 64 threads.  A list shorter than 8 or longer than 8192, or whose chosen
// model kept no hypothesis, gets model = -1 and no candidates; ReconstructH's early return gives model = 0, n_cand = 0.
__global__ __launch_bounds__(64) void k_motion_candidates(int n_lists, MotionLists in, MotionParams prm, MotionOut out) {
  const int list = blockIdx.x * 64 + threadIdx.x;
  if (list >= n_lists) return;
  const int n = motion_list_len(in, list);
  int model = -1, n_cand = 0, N = 0;
  float R[9 * rc::kMaxCandidates], t[3 * rc::kMaxCandidates];
  for (int k = 0; k < 9 * rc::kMaxCandidates; k++) R[k] = 0.0f;
  for (int k = 0; k < 3 * rc::kMaxCandidates; k++) t[k] = 0.0f;
  if (motion_list_ok(n)) {
    int chosen = in.forced_model, kept = 0;
    if (chosen < 0) {
      const int bh = in.best[0][list], bf = in.best[1][list];
      const float SH = bh >= 0 && bh < in.n_hyp ? in.scores[0][(long long)list * in.n_hyp + bh] : 0.0f;
      const float SF = bf >= 0 && bf < in.n_hyp ? in.scores[1][(long long)list * in.n_hyp + bf] : 0.0f;
      const float RH = SH / (SH + SF);
      chosen = (double)RH > 0.40 ? MSF_MODEL_HOMOGRAPHY : MSF_MODEL_FUNDAMENTAL;   // a NaN ratio: F, as `else` does
      kept = chosen == MSF_MODEL_HOMOGRAPHY ? bh : bf;
      if (kept >= in.n_hyp) kept = -1;   // never read outside the list's hypotheses
    }
    if (kept >= 0) {
      model = chosen;
      const uint8_t* inl = in.inliers[chosen] + (long long)list * in.cap;
      for (int i = 0; i < n; i++) N += inl[i] ? 1 : 0;
      const float* src = in.m21[chosen] + ((long long)list * in.n_hyp + kept) * 9;
      float M[9], w[3], normals[3 * rc::kMaxCandidates];
      for (int k = 0; k < 9; k++) M[k] = src[k];
      if (chosen == MSF_MODEL_HOMOGRAPHY) {
        n_cand = rc::decompose_h(M, prm.K, R, t, normals, w) ? 8 : 0;
      } else {
        rc::decompose_e(M, prm.K, R, t, w);
        n_cand = 4;
      }
    }
  }
  out.model[list] = model;
  out.n_inliers[list] = N;
  out.n_cand[list] = n_cand;
  for (int c = 0; c < rc::kMaxCandidates; c++) {
    const bool live = c < n_cand;
    for (int k = 0; k < 9; k++) out.cand_R[((long long)list * 8 + c) * 9 + k] = live ? R[9 * c + k] : 0.0f;
    for (int k = 0; k < 3; k++) out.cand_t[((long long)list * 8 + c) * 3 + k] = live ? t[3 * c + k] : 0.0f;
    out.cand_good[(long long)list * 8 + c] = 0;
    out.cand_parallax[(long long)list * 8 + c] = 0.0f;
  }
}

// CheckRT (:806-914) of one motion hypothesis on one list.  grid: (8 candidates, n_lists), 256 threads; a workgroup
// beyond the list's n_cand leaves at once.  Lane `tid` takes matches tid, tid + 256, ... and skips non-inliers; its
// 4 x 4 [A; V] of Triangulate stays in registers (the Jacobi over 4 columns unrolls completely: no LDS tile, no scratch).
// nGood: ballot + popcount, one LDS add per wave.  Parallax: cosParallax of the counted matches goes to LDS as
// order-preserving 64-bit keys (slot i of match i; ~0 where nothing was counted, which sorts last and is never reached),
// then the key of rank min(50, nGood - 1) is found by 8 passes of 8 bits over a 256-bin LDS histogram.
// Dynamic LDS: 8 bytes per match of the longest list (64 KB at 8192 matches).
// Code object (gfx950, tools/asm_audit.py): 94 vector registers (5 waves per SIMD), 1032 B of static LDS, 0 B of scratch.
__global__ __launch_bounds__(256) void k_check_rt(MotionLists in, MotionParams prm, MotionOut out) {
  extern __shared__ uint64_t keys[];
  __shared__ unsigned hist[256];
  __shared__ int n_good_s;
  const int cand = blockIdx.x, list = blockIdx.y, tid = threadIdx.x;
  if (cand >= out.n_cand[list]) return;
  const int n = motion_list_len(in, list);
  const int model = out.model[list];
  const uint8_t* inl = in.inliers[model] + (long long)list * in.cap;
  const msf_match* m = in.matches + (long long)list * in.cap;
  float R[9], t[3];
  for (int k = 0; k < 9; k++) R[k] = out.cand_R[((long long)list * 8 + cand) * 9 + k];
  for (int k = 0; k < 3; k++) t[k] = out.cand_t[((long long)list * 8 + cand) * 3 + k];
  rc::Pose q;
  rc::make_pose(prm.K, R, t, &q);
  if (tid == 0) n_good_s = 0;
  __syncthreads();
  const int rounds = (n + 255) / 256;
  for (int r = 0; r < rounds; r++) {
    const int i = r * 256 + tid;
    int flag = 0;
    uint64_t key = ~0ull;
    if (i < n && inl[i]) {
      const msf_match mm = m[i];
      float p[3];
      double cosp = 0.0;
      flag = rc::check_match((float)mm.x1, (float)mm.y1, (float)mm.x2, (float)mm.y2, q, prm.th2, p, &cosp);
      if (flag & rc::kCounted) key = rc::cos_key(cosp);
    }
    if (i < n) keys[i] = key;
    const unsigned long long counted = __ballot((flag & rc::kCounted) != 0);
    if ((tid & 63) == 0) atomicAdd(&n_good_s, __popcll(counted));
  }
  __syncthreads();
  const int nGood = n_good_s;
  float parallax = 0.0f;
  if (nGood > 0) {   // uniform
    int k = nGood - 1 < 50 ? nGood - 1 : 50;   // idx = min(50, size - 1)
    uint64_t prefix = 0, mask = 0;
    for (int pass = 0; pass < 8; pass++) {
      const int shift = 56 - 8 * pass;
      hist[tid] = 0;
      __syncthreads();
      for (int i = tid; i < n; i += 256) {
        const uint64_t key = keys[i];
        if ((key & mask) == prefix) atomicAdd(&hist[(unsigned)(key >> shift) & 255u], 1u);
      }
      __syncthreads();
      int below = 0, bin = 255;   // every lane reads the same bins: broadcasts
      for (int b = 0; b < 256; b++) {
        const int c = (int)hist[b];
        if (k < below + c) { bin = b; break; }
        below += c;
      }
      k -= below;
      prefix |= (uint64_t)bin << shift;
      mask |= 0xFFull << shift;
      __syncthreads();
    }
    parallax = rc::parallax_degrees(rc::key_cos(prefix));
  }
  if (tid == 0) {
    out.cand_good[(long long)list * 8 + cand] = nGood;
    out.cand_parallax[(long long)list * 8 + cand] = parallax;
  }
}

// The selection of ReconstructF (:524-582) / ReconstructH (:700-741).  One thread per list; grid: ceil(n_lists / 64) x 64.
__global__ __launch_bounds__(64) void k_pick_motion(int n_lists, MotionParams prm, MotionOut out) {
  const int list = blockIdx.x * 64 + threadIdx.x;
  if (list >= n_lists) return;
  const int n_cand = out.n_cand[list], model = out.model[list];
  int winner = -1;
  if (n_cand > 0) {
    int good[rc::kMaxCandidates];
    float parallax[rc::kMaxCandidates];
    for (int c = 0; c < rc::kMaxCandidates; c++) {
      good[c] = out.cand_good[(long long)list * 8 + c];
      parallax[c] = out.cand_parallax[(long long)list * 8 + c];
    }
    const int N = out.n_inliers[list];
    winner = model == MSF_MODEL_HOMOGRAPHY
                 ? rc::pick_homography(good, parallax, N, prm.min_triangulated, prm.min_parallax)
                 : rc::pick_fundamental(good, parallax, N, prm.min_triangulated, prm.min_parallax);
  }
  out.winner[list] = winner;
  out.ok[list] = winner >= 0 ? 1 : 0;
  const int w = winner >= 0 ? winner : 0;
  if (out.R21)
    for (int k = 0; k < 9; k++) out.R21[(long long)list * 9 + k] = winner >= 0 ? out.cand_R[((long long)list * 8 + w) * 9 + k] : 0.0f;
  if (out.t21)
    for (int k = 0; k < 3; k++) out.t21[(long long)list * 3 + k] = winner >= 0 ? out.cand_t[((long long)list * 8 + w) * 3 + k] : 0.0f;
}

// vP3D and vbTriangulated of the winner: check_match again for that hypothesis only (as k_best_inliers does for the kept
// H / F), instead of 8 x cap x 13 bytes per list that nobody reads.  One workgroup of 256 per list; points [cap][3] are 0
// and triangulated [cap] false beyond the list, for non-inliers, for matches CheckRT does not count, and without a winner.
__global__ __launch_bounds__(256) void k_winner_points(MotionLists in, MotionParams prm, MotionOut out) {
  const int list = blockIdx.x, tid = threadIdx.x;
  const int winner = out.winner[list];
  const int n = winner >= 0 ? motion_list_len(in, list) : 0;
  float* pts = out.points ? out.points + (long long)list * in.cap * 3 : nullptr;
  uint8_t* tri = out.triangulated ? out.triangulated + (long long)list * in.cap : nullptr;
  if (winner >= 0) {
    const int model = out.model[list];
    const uint8_t* inl = in.inliers[model] + (long long)list * in.cap;
    const msf_match* m = in.matches + (long long)list * in.cap;
    float R[9], t[3];
    for (int k = 0; k < 9; k++) R[k] = out.cand_R[((long long)list * 8 + winner) * 9 + k];
    for (int k = 0; k < 3; k++) t[k] = out.cand_t[((long long)list * 8 + winner) * 3 + k];
    rc::Pose q;
    rc::make_pose(prm.K, R, t, &q);
    for (int i = tid; i < n; i += 256) {
      float p[3] = {0.0f, 0.0f, 0.0f};
      int flag = 0;
      if (inl[i]) {
        const msf_match mm = m[i];
        double cosp = 0.0;
        flag = rc::check_match((float)mm.x1, (float)mm.y1, (float)mm.x2, (float)mm.y2, q, prm.th2, p, &cosp);
      }
      const bool counted = (flag & rc::kCounted) != 0;
      if (pts)
        for (int k = 0; k < 3; k++) pts[3 * i + k] = counted ? p[k] : 0.0f;
      if (tri) tri[i] = (flag & rc::kGood) != 0;
    }
  }
  for (int i = n + tid; i < in.cap; i += 256) {
    if (pts)
      for (int k = 0; k < 3; k++) pts[3 * i + k] = 0.0f;
    if (tri) tri[i] = 0;
  }
}

hipError_t reconstruct_motion(int n_lists, const MotionLists& in, const MotionParams& prm, const MotionOut& out,
                              hipStream_t st) {
  if (n_lists <= 0) return hipSuccess;
  const int longest = in.cap < kMaxReconstructMatches ? in.cap : kMaxReconstructMatches;
  const size_t lds = (size_t)(longest > 0 ? longest : 1) * sizeof(uint64_t);
  static std::once_flag attr_once;   // handles on several host threads may arrive here together
  std::call_once(attr_once, [] {
    hipFuncSetAttribute(reinterpret_cast<const void*>(k_check_rt), hipFuncAttributeMaxDynamicSharedMemorySize,
                        kMaxReconstructMatches * (int)sizeof(uint64_t));
  });
  const dim3 per_list((n_lists + 63) / 64);
  hipLaunchKernelGGL(k_motion_candidates, per_list, dim3(64), 0, st, n_lists, in, prm, out);
  hipLaunchKernelGGL(k_check_rt, dim3(rc::kMaxCandidates, n_lists), dim3(256), lds, st, in, prm, out);
  hipLaunchKernelGGL(k_pick_motion, per_list, dim3(64), 0, st, n_lists, prm, out);
  if (out.points || out.triangulated)
    hipLaunchKernelGGL(k_winner_points, dim3(n_lists), dim3(256), 0, st, in, prm, out);
  return hipGetLastError();
}

}  // namespace msf
