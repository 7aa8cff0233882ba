// Match-list consumer: Initializer::FindHomography / FindFundamental
// (slam_pipeline/src/Initializer.cc:152-245) on the device, for one match list or a batch of them:
//   k_ransac_sets       the draw of the minimum sets (:106-120) with a counter-based generator (batch only)
//   k_ransac_normalize  Initializer::Normalize (:760-804) of both point sets of every list
//   k_solve_models      per (list, hypothesis, model): the 8-point DLT matrix, its null vector by a one-sided Jacobi,
//                       F's rank-2 projection, the denormalisation, H12 = H21^-1 (:246-320; arithmetic: ransac_solve.h)
//   k_score_lists       CheckHomography / CheckFundamental (:322-487) of every hypothesis of every list
//   k_ransac_best       the keep loop: first strict maximum above 0 (:190-194, :236-240)
//   k_best_inliers      vbMatchesInliers of the kept hypothesis
//   k_check_hypotheses  the scorer alone, for callers that bring their own hypotheses (msf_check_hypotheses)
//
// Generator of k_ransac_sets: the reference seeds std::mt19937 from std::random_device, so there is no sequence to
// reproduce, only the procedure (copy the index list; eight times: pick randi, take avail[randi], move the last element
// in).  randi of draw j of iteration `it` of list `list` is the high 64 bits of word * size with
//   word = mix64(seed ^ mix64(((list * 2^20 + it) * 8 + j) + 0x9E3779B97F4A7C15)),  mix64 = the splitmix64 finaliser
// (ransac_solve.h: draw_set).  The sets are an output: any result can be replayed through the single-list call.
//
// Bit-exactness: every per-match expression is evaluated in f32 in the reference's operation order (the library is
// built with -ffp-contract=off and correctly rounded division), and the score is accumulated by ONE lane in match
// order, two additions per match, exactly like the reference's `score +=` loop -- f32 addition is not associative.
// Normalize accumulates its four sums the same way: one lane per list and axis, in match order.
#include <hip/hip_runtime.h>

#include <mutex>
#include <stdint.h>

#include "msf_abi.h"
#include "ransac_solve.h"

namespace msf {

constexpr int kMaxRansacMatches = 8192;   // 2 x f32 per match in LDS

// one workgroup per hypothesis
__global__ __launch_bounds__(256) void k_check_hypotheses(int model, const float* __restrict__ m21,
                                                          const float* __restrict__ m12, int n,
                                                          const msf_match* __restrict__ matches, float sigma,
                                                          float* __restrict__ scores, uint8_t* __restrict__ inliers) {
  extern __shared__ float terms[];   // [2 * n]: what the reference adds to `score` for match i (0 when it skips)
  const int hyp = blockIdx.x, tid = threadIdx.x;
  const float* M = m21 + 9 * hyp;
  const float a11 = M[0], a12 = M[1], a13 = M[2], a21 = M[3], a22 = M[4], a23 = M[5], a31 = M[6], a32 = M[7], a33 = M[8];
  const float inv_var = 1.0f / (sigma * sigma);
  if (model == MSF_MODEL_HOMOGRAPHY) {
    const float* I = m12 + 9 * hyp;
    const float i11 = I[0], i12 = I[1], i13 = I[2], i21 = I[3], i22 = I[4], i23 = I[5], i31 = I[6], i32 = I[7], i33 = I[8];
    const float th = 5.991f;
    for (int i = tid; i < n; i += 256) {
      const msf_match q = matches[i];
      const float u1 = (float)q.x1, v1 = (float)q.y1, u2 = (float)q.x2, v2 = (float)q.y2;
      bool consistent = true;
      // reprojection error in the first image, x2in1 = H12 * x2 (Initializer.cc:368-381)
      const float back_w = 1.0f / (i31 * u2 + i32 * v2 + i33);
      const float back_x = (i11 * u2 + i12 * v2 + i13) * back_w;
      const float back_y = (i21 * u2 + i22 * v2 + i23) * back_w;
      const float d2_first = (u1 - back_x) * (u1 - back_x) + (v1 - back_y) * (v1 - back_y);
      const float chi_first = d2_first * inv_var;
      float t1 = 0.f;
      if (chi_first > th) consistent = false; else t1 = th - chi_first;
      // reprojection error in the second image, x1in2 = H21 * x1 (:386-399)
      const float fwd_w = 1.0f / (a31 * u1 + a32 * v1 + a33);
      const float fwd_x = (a11 * u1 + a12 * v1 + a13) * fwd_w;
      const float fwd_y = (a21 * u1 + a22 * v1 + a23) * fwd_w;
      const float d2_second = (u2 - fwd_x) * (u2 - fwd_x) + (v2 - fwd_y) * (v2 - fwd_y);
      const float chi_second = d2_second * inv_var;
      float t2 = 0.f;
      if (chi_second > th) consistent = false; else t2 = th - chi_second;
      terms[2 * i] = t1;
      terms[2 * i + 1] = t2;
      inliers[(long long)hyp * n + i] = consistent;
    }
  } else {
    const float th = 3.841f, gain_cut = 5.991f;
    for (int i = tid; i < n; i += 256) {
      const msf_match q = matches[i];
      const float u1 = (float)q.x1, v1 = (float)q.y1, u2 = (float)q.x2, v2 = (float)q.y2;
      bool consistent = true;
      // l2 = F21 x1 (Initializer.cc:443-456)
      const float l2a = a11 * u1 + a12 * v1 + a13;
      const float l2b = a21 * u1 + a22 * v1 + a23;
      const float l2c = a31 * u1 + a32 * v1 + a33;
      const float line2_dot = l2a * u2 + l2b * v2 + l2c;
      const float d2_first = line2_dot * line2_dot / (l2a * l2a + l2b * l2b);
      const float chi_first = d2_first * inv_var;
      float t1 = 0.f;
      if (chi_first > th) consistent = false; else t1 = gain_cut - chi_first;
      // l1 = x2' F21 (:461-474)
      const float l1a = a11 * u2 + a21 * v2 + a31;
      const float l1b = a12 * u2 + a22 * v2 + a32;
      const float l1c = a13 * u2 + a23 * v2 + a33;
      const float line1_dot = l1a * u1 + l1b * v1 + l1c;
      const float d2_second = line1_dot * line1_dot / (l1a * l1a + l1b * l1b);
      const float chi_second = d2_second * inv_var;
      float t2 = 0.f;
      if (chi_second > th) consistent = false; else t2 = gain_cut - chi_second;
      terms[2 * i] = t1;
      terms[2 * i + 1] = t2;
      inliers[(long long)hyp * n + i] = consistent;
    }
  }
  __syncthreads();
  if (tid == 0) {
    // the reference's accumulation order; a skipped term was stored as +0.0f, and score + 0.0f == score bit for bit
    // (score is never -0: it starts at +0 and only receives th - chi >= 0 or NaN)
    float score = 0.0f;
    for (int i = 0; i < 2 * n; i++) score += terms[i];
    scores[hyp] = score;
  }
}

hipError_t check_hypotheses(int model, int n_hyp, const float* d_m21, const float* d_m12, int n,
                            const msf_match* d_matches, float sigma, float* d_scores, uint8_t* d_inliers,
                            hipStream_t st) {
  if (n_hyp <= 0) return hipSuccess;
  if (n > kMaxRansacMatches) return hipErrorInvalidValue;
  const size_t lds = (size_t)2 * (n > 0 ? n : 1) * sizeof(float);
  static std::once_flag attr_once;     // handles on several host threads (msf_multi) may arrive here together
  std::call_once(attr_once, [] {
    hipFuncSetAttribute(reinterpret_cast<const void*>(k_check_hypotheses), hipFuncAttributeMaxDynamicSharedMemorySize,
                        2 * kMaxRansacMatches * (int)sizeof(float));
  });
  hipLaunchKernelGGL(k_check_hypotheses, dim3(n_hyp), dim3(256), lds, st, model, d_m21, d_m12, n, d_matches, sigma,
                     d_scores, d_inliers);
  return hipGetLastError();
}


// ---------------------------------------------------------------------------------------------------------------------
// FindHomography + FindFundamental for n_lists match lists.  List l is matches + l * cap, its length n_out[l] clamped to
// cap (n_out == nullptr: one list of n_single matches).  A list takes part when 8 <= length <= kMaxRansacMatches; every
// other list gets best = -1, all-false inliers and zero scores, and its matrices are left untouched.

__device__ __forceinline__ int list_len(const int32_t* __restrict__ n_out, int n_single, int cap, int list) {
  if (!n_out) return n_single;
  const int n = n_out[list];
  return n < cap ? n : cap;
}

__device__ __forceinline__ bool list_ok(int n) { return n >= 8 && n <= kMaxRansacMatches; }

// one thread per (iteration, list)
__global__ __launch_bounds__(64) void k_ransac_sets(int n_lists, int n_hyp, const int32_t* __restrict__ n_out, int cap,
                                                    unsigned long long seed, int32_t* __restrict__ sets) {
  const int it = blockIdx.x * 64 + threadIdx.x, list = blockIdx.y;
  if (it >= n_hyp) return;
  const int n = list_len(n_out, 0, cap, list);
  int32_t set[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (list_ok(n)) ransac::draw_set(seed, list, it, n, set);
  int32_t* out = sets + ((long long)list * n_hyp + it) * 8;
  for (int j = 0; j < 8; j++) out[j] = set[j];
}

constexpr int kNormChunk = 1024;   // matches staged in LDS per step

// one workgroup per list.  Lane a < 4 owns axis a (x1, y1, x2, y2) and adds in match order, as the reference's loops do;
// the other lanes stage the coordinates into LDS and write the normalised points.
// pn: [n_lists][cap] float4 (x1, y1, x2, y2 normalised); T: [n_lists][2][9]
__global__ __launch_bounds__(256) void k_ransac_normalize(const msf_match* __restrict__ matches, int cap,
                                                          const int32_t* __restrict__ n_out, int n_single,
                                                          float4* __restrict__ pn, float* __restrict__ T) {
  __shared__ float stage[kNormChunk * 4];
  __shared__ float mean_s[4], scale_s[4];
  const int list = blockIdx.x, tid = threadIdx.x;
  const int n = list_len(n_out, n_single, cap, list);
  if (!list_ok(n)) return;
  const msf_match* m = matches + (long long)list * cap;
  float acc = 0.0f;
  for (int base = 0; base < n; base += kNormChunk) {
    const int cnt = n - base < kNormChunk ? n - base : kNormChunk;
    for (int i = tid; i < cnt; i += 256) {
      const msf_match q = m[base + i];
      stage[4 * i] = (float)q.x1;
      stage[4 * i + 1] = (float)q.y1;
      stage[4 * i + 2] = (float)q.x2;
      stage[4 * i + 3] = (float)q.y2;
    }
    __syncthreads();
    if (tid < 4)
      for (int i = 0; i < cnt; i++) acc += stage[4 * i + tid];          // meanX += vKeys[i].x
    __syncthreads();
  }
  if (tid < 4) mean_s[tid] = acc / (float)n;                             // meanX = meanX / N
  __syncthreads();
  acc = 0.0f;
  for (int base = 0; base < n; base += kNormChunk) {
    const int cnt = n - base < kNormChunk ? n - base : kNormChunk;
    for (int i = tid; i < cnt; i += 256) {
      const msf_match q = m[base + i];
      stage[4 * i] = fabsf((float)q.x1 - mean_s[0]);
      stage[4 * i + 1] = fabsf((float)q.y1 - mean_s[1]);
      stage[4 * i + 2] = fabsf((float)q.x2 - mean_s[2]);
      stage[4 * i + 3] = fabsf((float)q.y2 - mean_s[3]);
    }
    __syncthreads();
    if (tid < 4)
      for (int i = 0; i < cnt; i++) acc += stage[4 * i + tid];          // meanDevX += fabs(x - meanX)
    __syncthreads();
  }
  if (tid < 4) scale_s[tid] = 1.0f / (acc / (float)n);                   // sX = 1.0f / (meanDevX / N)
  __syncthreads();
  const float m0 = mean_s[0], m1 = mean_s[1], m2 = mean_s[2], m3 = mean_s[3];
  const float s0 = scale_s[0], s1 = scale_s[1], s2 = scale_s[2], s3 = scale_s[3];
  for (int i = tid; i < n; i += 256) {
    const msf_match q = m[i];
    pn[(long long)list * cap + i] = make_float4(((float)q.x1 - m0) * s0, ((float)q.y1 - m1) * s1,
                                                ((float)q.x2 - m2) * s2, ((float)q.y2 - m3) * s3);
  }
  if (tid < 2) {   // T1 (tid 0) from axes 0, 1; T2 from axes 2, 3
    float* t = T + ((long long)list * 2 + tid) * 9;
    const float sx = scale_s[2 * tid], sy = scale_s[2 * tid + 1];
    t[0] = sx;   t[1] = 0.0f; t[2] = -mean_s[2 * tid] * sx;
    t[3] = 0.0f; t[4] = sy;   t[5] = -mean_s[2 * tid + 1] * sy;
    t[6] = 0.0f; t[7] = 0.0f; t[8] = 1.0f;
  }
}

// One thread per hypothesis, one wave per workgroup; the thread's [A; V] lives in LDS as [element][lane], so the
// runtime-indexed column rotations of the Jacobi cost no scratch memory and no bank conflicts.
// grid: (ceil(n_hyp / 64), n_lists).  MODEL 0: m21 = H21, aux = H12; MODEL 1: m21 = F21, aux = Fn (rank 2, normalised).
template <int MODEL>
__global__ __launch_bounds__(64) void k_solve_models(int n_hyp, int cap, const int32_t* __restrict__ n_out, int n_single,
                                                     const float4* __restrict__ pn, const int32_t* __restrict__ sets,
                                                     const float* __restrict__ T, float* __restrict__ m21,
                                                     float* __restrict__ aux, float* __restrict__ null_vec) {
  constexpr int ROWS = MODEL == MSF_MODEL_HOMOGRAPHY ? 16 : 8;
  __shared__ float lds[(ROWS + 9) * 9 * 64];
  const int list = blockIdx.y, hyp = blockIdx.x * 64 + threadIdx.x;
  const int n = list_len(n_out, n_single, cap, list);
  if (!list_ok(n) || hyp >= n_hyp) return;
  const long long slot = (long long)list * n_hyp + hyp;
  const int32_t* set = sets + slot * 8;
  float p1[16], p2[16];
  for (int j = 0; j < 8; j++) {
    int idx = set[j];
    idx = idx < 0 ? 0 : (idx >= n ? n - 1 : idx);   // the host entry point rejects such sets; never read outside the list
    const float4 q = pn[(long long)list * cap + idx];
    p1[2 * j] = q.x; p1[2 * j + 1] = q.y; p2[2 * j] = q.z; p2[2 * j + 1] = q.w;
  }
  const float* t1 = T + (long long)list * 18;
  const float* t2 = t1 + 9;
  float T1[9], T2[9], h[9], out21[9], outaux[9];
  for (int k = 0; k < 9; k++) { T1[k] = t1[k]; T2[k] = t2[k]; }
  ransac::Strided w{lds + threadIdx.x, 64};
  if (MODEL == MSF_MODEL_HOMOGRAPHY) {
    ransac::build_a_homography(w, p1, p2);
    ransac::null_vector<ROWS>(w, h);
    ransac::finish_homography(h, T1, T2, out21, outaux);
  } else {
    ransac::build_a_fundamental(w, p1, p2);
    ransac::null_vector<ROWS>(w, h);
    ransac::finish_fundamental(h, T1, T2, outaux, out21);
  }
  for (int k = 0; k < 9; k++) {
    m21[slot * 9 + k] = out21[k];
    if (aux) aux[slot * 9 + k] = outaux[k];
    if (null_vec) null_vec[slot * 9 + k] = h[k];
  }
}

// The per-match part of k_check_hypotheses, expression for expression: what the reference adds to `score` for match i
// goes to terms[2 i], terms[2 i + 1] (when terms != nullptr) and its vbMatchesInliers entry to flags[i] (when != nullptr).
__device__ __forceinline__ void check_matches(int model, const float* __restrict__ M, const float* __restrict__ I, int n,
                                              const msf_match* __restrict__ matches, float sigma, float* terms,
                                              uint8_t* __restrict__ flags, int tid, int nthreads) {
  const float a11 = M[0], a12 = M[1], a13 = M[2], a21 = M[3], a22 = M[4], a23 = M[5], a31 = M[6], a32 = M[7], a33 = M[8];
  const float inv_var = 1.0f / (sigma * sigma);
  if (model == MSF_MODEL_HOMOGRAPHY) {
    const float i11 = I[0], i12 = I[1], i13 = I[2], i21 = I[3], i22 = I[4], i23 = I[5], i31 = I[6], i32 = I[7], i33 = I[8];
    const float th = 5.991f;
    for (int i = tid; i < n; i += nthreads) {
      const msf_match q = matches[i];
      const float u1 = (float)q.x1, v1 = (float)q.y1, u2 = (float)q.x2, v2 = (float)q.y2;
      bool consistent = true;
      const float back_w = 1.0f / (i31 * u2 + i32 * v2 + i33);
      const float back_x = (i11 * u2 + i12 * v2 + i13) * back_w;
      const float back_y = (i21 * u2 + i22 * v2 + i23) * back_w;
      const float d2_first = (u1 - back_x) * (u1 - back_x) + (v1 - back_y) * (v1 - back_y);
      const float chi_first = d2_first * inv_var;
      float t1 = 0.f;
      if (chi_first > th) consistent = false; else t1 = th - chi_first;
      const float fwd_w = 1.0f / (a31 * u1 + a32 * v1 + a33);
      const float fwd_x = (a11 * u1 + a12 * v1 + a13) * fwd_w;
      const float fwd_y = (a21 * u1 + a22 * v1 + a23) * fwd_w;
      const float d2_second = (u2 - fwd_x) * (u2 - fwd_x) + (v2 - fwd_y) * (v2 - fwd_y);
      const float chi_second = d2_second * inv_var;
      float t2 = 0.f;
      if (chi_second > th) consistent = false; else t2 = th - chi_second;
      if (terms) { terms[2 * i] = t1; terms[2 * i + 1] = t2; }
      if (flags) flags[i] = consistent;
    }
  } else {
    const float th = 3.841f, gain_cut = 5.991f;
    for (int i = tid; i < n; i += nthreads) {
      const msf_match q = matches[i];
      const float u1 = (float)q.x1, v1 = (float)q.y1, u2 = (float)q.x2, v2 = (float)q.y2;
      bool consistent = true;
      const float l2a = a11 * u1 + a12 * v1 + a13;
      const float l2b = a21 * u1 + a22 * v1 + a23;
      const float l2c = a31 * u1 + a32 * v1 + a33;
      const float line2_dot = l2a * u2 + l2b * v2 + l2c;
      const float d2_first = line2_dot * line2_dot / (l2a * l2a + l2b * l2b);
      const float chi_first = d2_first * inv_var;
      float t1 = 0.f;
      if (chi_first > th) consistent = false; else t1 = gain_cut - chi_first;
      const float l1a = a11 * u2 + a21 * v2 + a31;
      const float l1b = a12 * u2 + a22 * v2 + a32;
      const float l1c = a13 * u2 + a23 * v2 + a33;
      const float line1_dot = l1a * u1 + l1b * v1 + l1c;
      const float d2_second = line1_dot * line1_dot / (l1a * l1a + l1b * l1b);
      const float chi_second = d2_second * inv_var;
      float t2 = 0.f;
      if (chi_second > th) consistent = false; else t2 = gain_cut - chi_second;
      if (terms) { terms[2 * i] = t1; terms[2 * i + 1] = t2; }
      if (flags) flags[i] = consistent;
    }
  }
}

// grid: (n_hyp, n_lists); one workgroup scores one hypothesis on its list; dynamic LDS: 2 * (longest list) floats
__global__ __launch_bounds__(256) void k_score_lists(int model, const float* __restrict__ m21,
                                                     const float* __restrict__ m12, int n_hyp, int cap,
                                                     const int32_t* __restrict__ n_out, int n_single,
                                                     const msf_match* __restrict__ matches, float sigma,
                                                     float* __restrict__ scores) {
  extern __shared__ float terms[];
  const int hyp = blockIdx.x, list = blockIdx.y, tid = threadIdx.x;
  const long long slot = (long long)list * n_hyp + hyp;
  const int n = list_len(n_out, n_single, cap, list);
  if (!list_ok(n)) {
    if (tid == 0) scores[slot] = 0.0f;
    return;
  }
  check_matches(model, m21 + slot * 9, m12 ? m12 + slot * 9 : nullptr, n, matches + (long long)list * cap, sigma, terms,
                nullptr, tid, 256);
  __syncthreads();
  if (tid == 0) {
    float score = 0.0f;
    for (int i = 0; i < 2 * n; i++) score += terms[i];
    scores[slot] = score;
  }
}

// one thread per list: currentScore > score keeps the first strict maximum above 0 (a NaN score is never kept)
__global__ __launch_bounds__(64) void k_ransac_best(int n_lists, int n_hyp, int cap, const int32_t* __restrict__ n_out,
                                                    int n_single, const float* __restrict__ scores,
                                                    int32_t* __restrict__ best) {
  const int list = blockIdx.x * 64 + threadIdx.x;
  if (list >= n_lists) return;
  int kept = -1;
  if (list_ok(list_len(n_out, n_single, cap, list))) {
    float score = 0.0f;
    for (int i = 0; i < n_hyp; i++) {
      const float s = scores[(long long)list * n_hyp + i];
      if (s > score) { score = s; kept = i; }
    }
  }
  best[list] = kept;
}

// one workgroup per list: inliers[list][0 .. cap) = vbMatchesInliers of the kept hypothesis, false beyond the list and
// everywhere when nothing was kept
__global__ __launch_bounds__(256) void k_best_inliers(int model, const float* __restrict__ m21,
                                                      const float* __restrict__ m12, int n_hyp, int cap,
                                                      const int32_t* __restrict__ n_out, int n_single,
                                                      const msf_match* __restrict__ matches, float sigma,
                                                      const int32_t* __restrict__ best, uint8_t* __restrict__ inliers) {
  const int list = blockIdx.x, tid = threadIdx.x;
  const int kept = best[list];
  int n = 0;
  uint8_t* out = inliers + (long long)list * cap;
  if (kept >= 0) {
    n = list_len(n_out, n_single, cap, list);
    const long long slot = (long long)list * n_hyp + kept;
    check_matches(model, m21 + slot * 9, m12 ? m12 + slot * 9 : nullptr, n, matches + (long long)list * cap, sigma,
                  nullptr, out, tid, 256);
  }
  for (int i = n + tid; i < cap; i += 256) out[i] = 0;
}

size_t find_models_workspace_bytes(int n_lists, int cap, int n_hyp) {
  const size_t L = (size_t)n_lists, Hn = (size_t)n_hyp;
  // pn, T, sets, then per model: m21, aux, null_vec, scores; best; inliers
  return L * cap * sizeof(float4) + L * 18 * sizeof(float) + L * Hn * 8 * sizeof(int32_t) +
         2 * (L * Hn * 28 * sizeof(float) + L * sizeof(int32_t) + L * cap) + 256;
}

// Everything after the sets.  d_pn [n_lists][cap] float4 and d_T [n_lists][2][9] are written here.  Per model (0: H,
// 1: F): m21 / scores / best are required, aux (H12 / Fn), null_vec and inliers optional.
hipError_t find_models(int n_lists, const msf_match* d_matches, int cap, const int32_t* d_n_out, int n_single, int n_hyp,
                       const int32_t* d_sets, float sigma, float4* d_pn, float* d_T, float* const* d_m21,
                       float* const* d_aux, float* const* d_null, float* const* d_scores, int32_t* const* d_best,
                       uint8_t* const* d_inliers, hipStream_t st) {
  if (n_lists <= 0) return hipSuccess;
  const int longest = cap < kMaxRansacMatches ? cap : kMaxRansacMatches;
  const size_t lds = (size_t)2 * (longest > 0 ? longest : 1) * sizeof(float);
  static std::once_flag attr_once;
  std::call_once(attr_once, [] {
    hipFuncSetAttribute(reinterpret_cast<const void*>(k_score_lists), hipFuncAttributeMaxDynamicSharedMemorySize,
                        2 * kMaxRansacMatches * (int)sizeof(float));
  });
  if (n_hyp > 0) {
    hipLaunchKernelGGL(k_ransac_normalize, dim3(n_lists), dim3(256), 0, st, d_matches, cap, d_n_out, n_single, d_pn, d_T);
    const dim3 grid((n_hyp + 63) / 64, n_lists);
    hipLaunchKernelGGL(k_solve_models<MSF_MODEL_HOMOGRAPHY>, grid, dim3(64), 0, st, n_hyp, cap, d_n_out, n_single, d_pn,
                       d_sets, d_T, d_m21[0], d_aux[0], d_null[0]);
    hipLaunchKernelGGL(k_solve_models<MSF_MODEL_FUNDAMENTAL>, grid, dim3(64), 0, st, n_hyp, cap, d_n_out, n_single, d_pn,
                       d_sets, d_T, d_m21[1], d_aux[1], d_null[1]);
  }
  for (int model = 0; model < 2; model++) {
    if (n_hyp > 0)
      hipLaunchKernelGGL(k_score_lists, dim3(n_hyp, n_lists), dim3(256), lds, st, model, d_m21[model],
                         model == MSF_MODEL_HOMOGRAPHY ? d_aux[0] : nullptr, n_hyp, cap, d_n_out, n_single, d_matches,
                         sigma, d_scores[model]);
    hipLaunchKernelGGL(k_ransac_best, dim3((n_lists + 63) / 64), dim3(64), 0, st, n_lists, n_hyp, cap, d_n_out, n_single,
                       d_scores[model], d_best[model]);
    if (d_inliers[model])
      hipLaunchKernelGGL(k_best_inliers, dim3(n_lists), dim3(256), 0, st, model, d_m21[model],
                         model == MSF_MODEL_HOMOGRAPHY ? d_aux[0] : nullptr, n_hyp, cap, d_n_out, n_single, d_matches,
                         sigma, d_best[model], d_inliers[model]);
  }
  return hipGetLastError();
}

hipError_t ransac_sets(int n_lists, int n_hyp, const int32_t* d_n_out, int cap, uint64_t seed, int32_t* d_sets,
                       hipStream_t st) {
  if (n_lists <= 0 || n_hyp <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_ransac_sets, dim3((n_hyp + 63) / 64, n_lists), dim3(64), 0, st, n_lists, n_hyp, d_n_out, cap,
                     (unsigned long long)seed, d_sets);
  return hipGetLastError();
}

}  // namespace msf
