// extern "C" boundary of libmsf.so (declarations + the reference interfaces they replace: include/msf_abi.h).
#include "msf_abi.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "ba_arrays.h"
#include "ba_pipeline.h"
#include "carve.h"
#include "dev_buf.h"
#include "frame_tracking_arrays.h"
#include "frame_tracking_pipeline.h"
#include "gba_pipeline.h"
#include "loftr_pipeline.h"
#include "msf_ba.h"
#include "msf_frame_tracking.h"
#include "msf_global_ba.h"
#include "msf_initializer.h"
#include "msf_local_mapping.h"
#include "msf_pnp.h"
#include "msf_pose.h"
#include "msf_tracking.h"
#include "orb_pipeline.h"
#include "pnp_pipeline.h"
#include "pose_pipeline.h"
#include "ransac_solve.h"
#include "reconstruct_pipeline.h"
#include "result_arrays.h"
#include "tracking_arrays.h"
#include "tracking_pipeline.h"
#include "triangulate_pipeline.h"
#include "weights_io.h"

namespace msf {
hipError_t pack_matches(int n, const msf_match* d_in, int cap, const int32_t* d_cnt, msf_match* d_packed,
                        int32_t* d_offsets, hipStream_t st);
hipError_t count_mappoint_matches(int n, const msf_match* d_matches, int cap, const int32_t* d_cnt,
                                  const int32_t* d_map_a, const int32_t* d_map_b, const uint32_t* d_maps, int n_maps,
                                  int map_words, int width, int height, int32_t* d_num_mp, hipStream_t st);
hipError_t render_match_image(const uint8_t* d_f1, const uint8_t* d_f2, int w, int h, long long pitch,
                              const msf_match* d_m, const uint8_t* d_mp1, const uint8_t* d_mp2, int n, uint8_t* d_out,
                              long long out_stride, hipStream_t st);
hipError_t check_hypotheses(int model, int n_hyp, const float* d_m21, const float* d_m12, int n,
                            const msf_match* d_matches, float sigma, float* d_scores, uint8_t* d_inliers,
                            hipStream_t st);
hipError_t find_models(int n_lists, const msf_match* d_matches, int cap, const int32_t* d_n_out, int n_single, int n_hyp,
                       const int32_t* d_sets, float sigma, float4* d_pn, float* d_T, float* const* d_m21,
                       float* const* d_aux, float* const* d_null, float* const* d_scores, int32_t* const* d_best,
                       uint8_t* const* d_inliers, hipStream_t st);
hipError_t ransac_sets(int n_lists, int n_hyp, const int32_t* d_n_out, int cap, uint64_t seed, int32_t* d_sets,
                       hipStream_t st);
}

namespace {
thread_local std::string g_create_error;
using msf::DevBuf;   // dev_buf.h: the handle's device blocks go with their members
}  // namespace

struct msf_handle {
  msf_config cfg{};
  std::mutex mu;
  std::string err;
  hipStream_t stream = nullptr;
  msf::OrbPipeline orb;
  msf::LoftrPipeline loftr;
  // staging for the host-image entry points
  DevBuf<uint8_t> d_stage;       // [2 * max_pairs][H][pitch]
  DevBuf<msf_match> d_out_base;
  msf_match* d_out = nullptr;    // [max_pairs][stage_cap] = d_out_base + 1
  msf_match* h_pin = nullptr;    // pinned: [1 + kPinMatches]
  DevBuf<int32_t> d_n;           // [max_pairs]
  int stage_pitch = 0;
  long long stage_frame = 0;
  int stage_cap = 0;
  // KeyPointMap occupancy bitmaps (allocated by the first msf_set_mappoints): [n_maps][map_words]
  DevBuf<uint32_t> d_maps;
  int n_maps = 0, map_words = 0;
  std::vector<uint32_t> map_stage;
  // resident frame store of the one-vs-many entry points (allocated by the first msf_store_frame): [2*max_pairs] frames
  DevBuf<uint8_t> d_store;
  DevBuf<int32_t> d_idx;         // [3][max_pairs]: query slot per pair, train slot per pair, map-point counts
  std::vector<int32_t> idx_stage;
  // The geometry workspaces, one per family, each carved by that family's layout (carve()) and grown on demand.
  // msf_check_hypotheses workspace (the two matrix arrays, scores, inlier flags, the list)
  DevBuf<uint8_t> d_hyp;
  // msf_find_models / msf_find_models_device workspace (normalised points, sets, matrices, scores, ...), grown on demand
  DevBuf<uint8_t> d_fm;
  // msf_reconstruct / msf_reconstruct_device workspace (candidates, counts, the host call's list and results), grown on demand
  DevBuf<uint8_t> d_rc;
  // msf_new_points / msf_create_map_points workspace: the views, the results and the host call's list.  The first
  // msf_create_map_points sizes it for max_batch_pairs lists of stage_cap matches; a longer msf_new_points list grows it.
  DevBuf<uint8_t> d_lm;
  // msf_pnp_ransac / msf_pnp_ransac_device workspace: the host call's list, sets and results; for the device call the
  // counts and poses that the second launch reads when the caller does not ask for them
  DevBuf<uint8_t> d_pnp;
  // msf_pose_optimize workspace: the host call's list, entry pose, mask and results (the device call needs none)
  DevBuf<uint8_t> d_pose;
  // msf_bundle_adjust / msf_bundle_adjust_device workspace: the per-problem scratch of ba_solve.h (ba::layout); for the
  // host call also the problem, its descriptor, the stop word and the results
  DevBuf<uint8_t> d_ba;
  // msf_global_bundle_adjust / msf_global_bundle_adjust_device workspace: gba::layout (the record and the scratch of
  // one problem, sized by its own free cameras); for the host call also the problem and the results.  The pinned record
  // is what the host reads after every wait of the Levenberg-Marquardt loop (allocated by the first call).
  DevBuf<uint8_t> d_gba;
  msf::gba::Record* h_gba_rec = nullptr;
  // msf_frustum* / msf_claim_points_device / msf_search_local_points workspace: tracking::layout (the checking word, the
  // owner words, the counters, one word per pixel for the claims, the candidates and the per-key-frame rows); for the
  // host calls also the local map, the gate's bytes and the results
  DevBuf<uint8_t> d_track;
  // msfx_carry_points_device / msfx_track_list_device / msfx_track_frame workspace (msf_frame_tracking.h): the two words
  // the launches hand on, the entry pose, what the caller gave no array for; for the host call also the frame's map
  DevBuf<uint8_t> d_ftrack;
  std::vector<msf_view> view_stage;   // [2][n]: the query's view once per pair, then the neighbours'
  // msf_render_match_image workspace: the RGB image (allocated once) and the match list + flags (grown on demand)
  DevBuf<uint8_t> d_render;      // [H][2 * W][3]
  DevBuf<msf_match> d_render_m;  // [cap] matches, then 2 * cap flag bytes; cap = bytes / kRenderRecord
  // Transparent per-frame cache of the drop-in MatchFrames call: the callers loop
  // MatchFrames(X, KF_i) with X fixed (Tracking.cc:595-632, LocalMapping.cc:176,329, KeyFrameDatabase.cc:32,64) and the
  // reference re-extracts both frames every time.  Key = 64-bit content hash of the frame, confirmed by comparing the
  // bytes with the host copy kept per entry (a collision is a miss, never a wrong answer); value = a feature slot (ORB)
  // or token slot (LoFTR) beyond the caller-visible ones; least recently used entry is replaced.  FrameBase::id() is no
  // key: Frame and KeyFrame count separately (Frame.cc:29, KeyFrame.cc:30).
  struct CacheEntry {
    uint64_t hash = 0, used = 0;
    bool valid = false;
    std::vector<uint8_t> bytes;   // [H][W] contiguous
  };
  std::vector<CacheEntry> fc;
  int fc_slot0 = 0;                // first slot of the cache range
  DevBuf<int32_t> d_fc_slots;      // [fc.size()] = fc_slot0 + i: one-element slot arrays for the match call
  uint64_t fc_tick = 0, fc_hits = 0, fc_misses = 0, fc_hash_mask = ~0ull;
};

namespace {

int fail(msf_handle* h, int code, const std::string& msg) {
  if (h) h->err = msg; else g_create_error = msg;
  return code;
}

int hip_fail(msf_handle* h, const char* what, hipError_t e) {
  return fail(h, MSF_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

// The one form of a checked HIP call (runtime calls and the pipelines' launches alike): a failure leaves the enclosing
// function -- or the lambda of an entry point -- with MSF_ERR_HIP and "<what>: <the runtime's text>" as the error.
#define HIP_TRY(h, what, call)                                                \
  do {                                                                        \
    const hipError_t hip_try_e = (call);                                      \
    if (hip_try_e != hipSuccess) return hip_fail((h), (what), hip_try_e);     \
  } while (0)

// No exception crosses the C ABI (msf_abi.h): every entry point that can allocate runs inside guarded() and
// reports a host exception (std::bad_alloc from a std::vector / std::string, ...) as a status.  The message is
// assigned without allocating anything large; if even that throws, the status alone is returned.
int host_exception(msf_handle* h, const char* where) noexcept {
  try {
    fail(h, MSF_ERR_HIP, std::string(where) + ": host exception (out of memory?)");
  } catch (...) {
  }
  return MSF_ERR_HIP;
}

// Entry scaffold.  An entry point that takes a handle is `return guarded(h, "msf_xxx", [&]() -> int { ... });`: a null
// handle is MSF_ERR_INVALID_ARG (no error text: there is no handle to keep it), the body runs under the handle's lock,
// and whatever it throws becomes a status.  The entry points without a handle use the second form.  Templates on the
// callable, so the body is inlined and nothing is allocated on the way in.
template <class Body>
int guarded(const char* name, Body&& body) noexcept {
  try {
    return body();
  } catch (...) {
    return host_exception(nullptr, name);
  }
}

template <class Body>
int guarded(msf_handle* h, const char* name, Body&& body) noexcept {
  if (!h) return MSF_ERR_INVALID_ARG;
  try {
    std::lock_guard<std::mutex> lk(h->mu);
    return body();
  } catch (...) {
    return host_exception(h, name);
  }
}

// Device and stream of one call.  enter() comes after the argument checks; `stream` is what the caller passed (the host
// entry points pass nothing).  finish() waits only when the work went to the handle's own stream: a caller that names a
// stream gets an asynchronous call.
struct CallScope {
  msf_handle* h;
  hipStream_t st = nullptr;
  bool own_stream = true;
  int enter(void* stream = nullptr) {
    HIP_TRY(h, "hipSetDevice", hipSetDevice(h->cfg.device));
    own_stream = !stream;
    st = stream ? (hipStream_t)stream : h->stream;
    return MSF_OK;
  }
  int finish() {
    if (own_stream) HIP_TRY(h, "hipStreamSynchronize", hipStreamSynchronize(st));
    return MSF_OK;
  }
};

// Held by the host entry points that start asynchronous copies from / to the CALLER's buffers: whichever way the call
// leaves -- an error branch included -- the stream is drained first, so the caller may free or reuse them on return.
struct Drain {
  hipStream_t s;
  bool armed = true;
  ~Drain() { if (armed) hipStreamSynchronize(s); }
};

// The workspace of one geometry call.  `layout` is a function of an msf::Carver& (carve.h) that fills the call's plan
// struct; it runs on a null base to measure, `buf` grows to max(needed, floor) if it is too small (a failure is
// MSF_ERR_HIP under `what`), then the same function runs on the block to place the pieces.
template <class Layout>
int carve(msf_handle* h, DevBuf<uint8_t>& buf, size_t floor, const char* what, Layout&& layout) {
  msf::Carver measure;
  layout(measure);
  if (measure.off > buf.bytes) HIP_TRY(h, what, buf.reserve(measure.off, floor));
  msf::Carver place{buf.p};
  layout(place);
  return MSF_OK;
}

// element `i` of an optional array: null stays null
template <class T>
T* from(T* p, size_t i) {
  return p ? p + i : nullptr;
}

// The copy-back of the geometry host entry points, asynchronous on `st`: nothing to do when the caller gave no
// pointer or there is nothing to copy.
int fetch(msf_handle* h, hipStream_t st, void* dst, const void* src, size_t bytes) {
  if (!dst || !bytes) return MSF_OK;
  HIP_TRY(h, "hipMemcpyAsync", hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st));
  return MSF_OK;
}

// The result arrays of one list that `out` has a pointer for, from their device copies `dev`: copy_result()
// (result_arrays.h) over the struct's table, with fetch() as the copier.
template <class S, size_t N>
int fetch_result(msf_handle* h, hipStream_t st, const msf::ResultArray (&table)[N], const S& dev, const S& out,
                 const msf::Extent& e) {
  return msf::copy_result(table, dev, out, e,
                          [&](void* dst, const void* src, size_t bytes) { return fetch(h, st, dst, src, bytes); });
}

// The kernels' Out structs from a result struct of device pointers: the caller's (the _device entry points) or the
// one carve_result() filled (the host entry points).
msf::MotionOut to_out(const msf_motion_result& r) {   // n_inliers is no result: the entry point adds its piece
  return msf::MotionOut{r.model, nullptr, r.n_cand, r.cand_R, r.cand_t, r.cand_good, r.cand_parallax, r.winner, r.ok,
                        r.R21, r.t21, r.points, r.triangulated};
}

msf::NewPointOut to_out(const msf_new_points_result& r) {
  return msf::NewPointOut{r.n_new, r.packed, r.status, r.points, r.hom, r.cos_parallax};
}

msf::PnpOut to_out(const msf_pnp_result& r) {
  return msf::PnpOut{r.n_records, r.counts, r.iteration, r.n_inliers, r.refined_ok, r.n_refined, r.Tcw_best, r.Tcw_refined,
                     r.inliers_best, r.inliers_refined, r.sets, r.pose_f64, r.cws, r.ut_tail, r.betas, r.rep_errors,
                     r.pca, r.rec_pose_f64, r.rec_cws, r.rec_ut_tail, r.rec_betas, r.rec_rep_errors, r.rec_pca};
}

msf::PoseOut to_out(const msf_pose_result& r) {
  return msf::PoseOut{r.n_good, r.Tcw, r.outliers, r.n_edges, r.rounds_run, r.pose_f64, r.round_pose_f64, r.round_n_bad,
                      r.round_iterations, r.it_trials, r.it_lambda_in, r.it_lambda_out, r.it_cost_in, r.it_cost_out,
                      r.it_H, r.it_b, r.it_pose_out};
}

constexpr int kFrameCacheSlots = 64;   // default capacity of the transparent frame cache (MSF_FRAME_CACHE_SLOTS overrides)
constexpr int kPinMatches = 1024;  // matches fetched together with the count by the single-pair call
constexpr int kStageCap = 4096;  // matches per pair kept by the host-image path (ORB <= n1 <= 2048; LoFTR: see below)
constexpr size_t kRenderRecord = sizeof(msf_match) + 2;   // msf_render_match_image: a match and its two map-point flags
const char* const kNoResult = "at least one pair has no valid result (n_out = -1): a fixed-capacity device list "
                              "overflowed, or a unit of the ORB walker launch gave up a bounded wait";

template <class... V>
bool aligned16(V... v) {   // pointers and strides alike
  return ((... | (uintptr_t)v) & 15) == 0;
}

bool image_ok(const msf_handle* h, const msf_image* im) {
  return im && im->data && im->width == h->cfg.image_width && im->height == h->cfg.image_height &&
         im->stride >= h->cfg.image_width;
}

// one host frame into a staging frame (rows h->stage_pitch apart)
int upload_frame(msf_handle* h, uint8_t* dst, const msf_image* im, hipStream_t st) {
  HIP_TRY(h, "hipMemcpy2DAsync", hipMemcpy2DAsync(dst, h->stage_pitch, im->data, im->stride, h->cfg.image_width,
                                                   h->cfg.image_height, hipMemcpyHostToDevice, st));
  return MSF_OK;
}

// per-frame part of n frames (ORB features / LoFTR backbone tokens) into slots slot0 ..
int extract_into_slots(msf_handle* h, const uint8_t* d_frames, int n, long long frame_stride, long long row_stride,
                       int slot0, hipStream_t st) {
  if (h->cfg.kind == MSF_KIND_ORB) {
    msf::FrameSrc src{d_frames, d_frames, n, slot0, frame_stride, (int)row_stride};
    HIP_TRY(h, "orb extract", h->orb.extract(src, n, st));
  } else {
    HIP_TRY(h, "loftr extract", h->loftr.extract(n, d_frames, frame_stride, (int)row_stride, slot0, st));
  }
  return MSF_OK;
}

// pairs of slots -> match lists; slot_limit as in the pipelines (0 = every slot, the handle's private ones included)
int match_slot_pairs(msf_handle* h, int n, const int32_t* d_a, const int32_t* d_b, msf_match* d_out, int cap,
                     int32_t* d_n_out, hipStream_t st, int slot_limit) {
  HIP_TRY(h, "match slots",
          h->cfg.kind == MSF_KIND_ORB
              ? h->orb.match(n, d_a, d_b, h->cfg.threshold, d_out, cap, d_n_out, st, 0, slot_limit)
              : h->loftr.match_slots(n, d_a, d_b, h->cfg.threshold, d_out, cap, d_n_out, st, slot_limit));
  return MSF_OK;
}

int run_device(msf_handle* h, int n_pairs, const uint8_t* d_a, const uint8_t* d_b, long long frame_stride,
               long long row_stride, msf_match* d_out, int cap, int32_t* d_n_out, hipStream_t st) {
  if (n_pairs <= 0) return MSF_OK;
  if (n_pairs > h->cfg.max_batch_pairs) return fail(h, MSF_ERR_INVALID_ARG, "n_pairs exceeds max_batch_pairs");
  if (!aligned16(d_a, d_b, frame_stride, row_stride))
    return fail(h, MSF_ERR_INVALID_ARG, "device frames must be 16-byte aligned with strides multiple of 16");
  if (row_stride < h->cfg.image_width) return fail(h, MSF_ERR_INVALID_ARG, "row_stride < image_width");
  if (frame_stride < row_stride * (long long)h->cfg.image_height)
    return fail(h, MSF_ERR_INVALID_ARG, "frame_stride < row_stride * image_height (frames would overlap)");
  if (h->cfg.kind == MSF_KIND_ORB) {
    // the stateless MatchFrames path works in its own feature slots [2P, 4P): slots [0, 2P) are the per-frame cache of
    // msf_extract_device / msf_store_frame, which a MatchFrames call on the same handle must not disturb
    // (KeyFrameMatchDatabase and Tracking share one matcher, src/main.cpp:77-81)
    const int scratch0 = 2 * h->cfg.max_batch_pairs;
    msf::FrameSrc src{d_a, d_b, n_pairs, scratch0, frame_stride, (int)row_stride};
    HIP_TRY(h, "orb extract", h->orb.extract(src, 2 * n_pairs, st));
    if (h->orb.take_degraded_note())    // not an error of THIS call: the text is there for whoever reads msf_last_error
      h->err = "note: a unit of an earlier ORB walker launch gave up a bounded wait (its pairs reported n_out = -1); "
               "this handle now launches the walker one level at a time";
    HIP_TRY(h, "orb match", h->orb.match(n_pairs, nullptr, nullptr, h->cfg.threshold, d_out, cap, d_n_out, st, scratch0));
    return MSF_OK;
  }
  HIP_TRY(h, "loftr match", h->loftr.match(n_pairs, d_a, d_b, frame_stride, (int)row_stride, h->cfg.threshold, d_out,
                                           cap, d_n_out, st));
  return MSF_OK;
}

int ensure_stage(msf_handle* h) {
  if (h->d_stage) return MSF_OK;
  const int W = h->cfg.image_width, H = h->cfg.image_height, maxp = h->cfg.max_batch_pairs;
  h->stage_pitch = (W + 15) & ~15;
  h->stage_frame = (long long)h->stage_pitch * H;
  h->stage_cap = kStageCap;
  HIP_TRY(h, "hipMalloc stage", h->d_stage.reserve((size_t)2 * maxp * h->stage_frame));
  // one leading record in front of the lists: the single-pair call puts its count there, so count + list come back
  // in ONE device-to-host copy into pinned memory (one synchronisation per MatchFrames call instead of two)
  HIP_TRY(h, "hipMalloc out", h->d_out_base.reserve(((size_t)maxp * h->stage_cap + 1) * sizeof(msf_match)));
  h->d_out = h->d_out_base + 1;
  HIP_TRY(h, "hipHostMalloc", hipHostMalloc(&h->h_pin, (size_t)(kPinMatches + 1) * sizeof(msf_match), hipHostMallocDefault));
  HIP_TRY(h, "hipMalloc n", h->d_n.reserve((size_t)maxp * sizeof(int32_t)));
  return MSF_OK;
}

int32_t* single_count(msf_handle* h) { return reinterpret_cast<int32_t*>(h->d_out_base.p); }   // the leading record

int ensure_maps(msf_handle* h) {
  if (h->d_maps) return MSF_OK;
  const int n_maps = 2 * h->cfg.max_batch_pairs;
  const long long n_px = (long long)h->cfg.image_width * h->cfg.image_height;
  h->map_words = (int)((n_px + 31) / 32);
  const size_t bytes = (size_t)n_maps * h->map_words * sizeof(uint32_t);
  HIP_TRY(h, "hipMalloc(map bitmaps)", h->d_maps.reserve(bytes));
  HIP_TRY(h, "hipMemsetAsync", hipMemsetAsync(h->d_maps, 0, bytes, h->stream));
  h->n_maps = n_maps;
  return MSF_OK;
}

// 64-bit content hash of a W x H frame with row stride: four independent multiply-xorshift lanes over 8-byte words
// (one dependent chain would run at a quarter of the speed), folded at the end.
uint64_t hash_image(const msf_image* im) {
  const uint64_t K0 = 0x9E3779B97F4A7C15ull, K1 = 0xC2B2AE3D27D4EB4Full, K2 = 0x165667B19E3779F9ull, K3 = 0xD6E8FEB86659FD93ull;
  uint64_t h0 = K0 ^ (uint64_t)im->width, h1 = K1 ^ (uint64_t)im->height, h2 = K2, h3 = K3;
  const int W = im->width;
  for (int y = 0; y < im->height; y++) {
    const uint8_t* p = im->data + (size_t)y * (size_t)im->stride;
    int x = 0;
    for (; x + 32 <= W; x += 32) {
      uint64_t a, b, c, d;
      std::memcpy(&a, p + x, 8); std::memcpy(&b, p + x + 8, 8); std::memcpy(&c, p + x + 16, 8); std::memcpy(&d, p + x + 24, 8);
      h0 = (h0 ^ a) * K1; h0 ^= h0 >> 29;
      h1 = (h1 ^ b) * K2; h1 ^= h1 >> 31;
      h2 = (h2 ^ c) * K3; h2 ^= h2 >> 30;
      h3 = (h3 ^ d) * K0; h3 ^= h3 >> 28;
    }
    uint64_t tail = 0;
    for (; x < W; x++) tail = (tail << 8) ^ p[x] ^ (tail >> 56);
    h0 = (h0 ^ tail ^ (uint64_t)y) * K2; h0 ^= h0 >> 32;
  }
  uint64_t h = h0 ^ (h1 * K3) ^ (h2 * K0) ^ (h3 * K1);
  h ^= h >> 33; h *= 0xFF51AFD7ED558CCDull; h ^= h >> 33; h *= 0xC4CEB9FE1A85EC53ull; h ^= h >> 33;
  return h;
}

bool same_bytes(const msf_image* im, const std::vector<uint8_t>& bytes) {
  const size_t W = (size_t)im->width;
  for (int y = 0; y < im->height; y++)
    if (std::memcmp(im->data + (size_t)y * (size_t)im->stride, bytes.data() + (size_t)y * W, W) != 0) return false;
  return true;
}

// Slot of `im` in the frame cache, extracting it first if it is not there.  `keep` = an entry that must not be evicted
// (the other frame of the same call), or -1.  `d_stage_frame` = where to upload the frame for an extraction.
int cached_slot(msf_handle* h, const msf_image* im, int keep, uint8_t* d_stage_frame, hipStream_t st, int* entry_out) {
  const int W = h->cfg.image_width, H = h->cfg.image_height;
  const uint64_t hv = hash_image(im) & h->fc_hash_mask;
  int victim = -1;   // an unused entry, else the least recently used one; never `keep`
  for (int i = 0; i < (int)h->fc.size(); i++) {
    msf_handle::CacheEntry& e = h->fc[i];
    if (e.valid && e.hash == hv && same_bytes(im, e.bytes)) {
      e.used = ++h->fc_tick;
      h->fc_hits++;
      *entry_out = i;
      return MSF_OK;
    }
    if (i == keep) continue;
    const uint64_t age = e.valid ? e.used : 0;            // invalid entries first
    if (victim < 0 || age < (h->fc[victim].valid ? h->fc[victim].used : 0)) victim = i;
  }
  if (victim < 0) return fail(h, MSF_ERR_INVALID_ARG, "frame cache has no replaceable entry");
  msf_handle::CacheEntry& e = h->fc[victim];
  e.valid = false;
  e.bytes.resize((size_t)W * H);
  for (int y = 0; y < H; y++) std::memcpy(e.bytes.data() + (size_t)y * W, im->data + (size_t)y * (size_t)im->stride, (size_t)W);
  const msf_image kept{e.bytes.data(), W, H, W};
  if (int rc = upload_frame(h, d_stage_frame, &kept, st)) return rc;
  if (int rc = extract_into_slots(h, d_stage_frame, 1, h->stage_frame, h->stage_pitch, h->fc_slot0 + victim, st)) return rc;
  e.hash = hv;
  e.used = ++h->fc_tick;
  e.valid = true;
  h->fc_misses++;
  *entry_out = victim;
  return MSF_OK;
}

// What reaches a caller with room for `cap` matches of a pair whose device count is `c`: the staging list keeps
// stage_cap of them.  Sets *capacity when the count is -1 (the pair has no list) or the staging list is shorter than
// what the caller asked for.
int deliverable(const msf_handle* h, int32_t c, int32_t cap, bool* capacity) {
  if (c < 0) {
    *capacity = true;
    return 0;
  }
  const int avail = c < h->stage_cap ? c : h->stage_cap;
  if (avail < c && cap > avail) *capacity = true;
  return avail < cap ? avail : cap;
}

// Lists of the n pairs of one staged call, counts already on the host: pair i to out + i * cap_per_pair (out = NULL:
// the caller wants the counts only).  A pair that sets *capacity does not stop the lists of the others.
int copy_lists_back(msf_handle* h, int n, const int32_t* counts, msf_match* out, int32_t cap_per_pair, bool* capacity) {
  for (int i = 0; i < n; i++) {
    const int w = deliverable(h, counts[i], out ? cap_per_pair : 0, capacity);
    if (w > 0)
      HIP_TRY(h, "hipMemcpy", hipMemcpy(out + (size_t)i * cap_per_pair, h->d_out + (size_t)i * h->stage_cap,
                                        (size_t)w * sizeof(msf_match), hipMemcpyDeviceToHost));
  }
  return MSF_OK;
}

// count (in the record before the list) + list of the single-pair call: one copy, one synchronisation
int fetch_single(msf_handle* h, msf_match* out, int32_t cap_per_pair, int32_t* n_out, hipStream_t st) {
  const int wmax = cap_per_pair < h->stage_cap ? cap_per_pair : h->stage_cap;
  const int wfirst = wmax < kPinMatches ? wmax : kPinMatches;
  HIP_TRY(h, "hipMemcpyAsync", hipMemcpyAsync(h->h_pin, h->d_out_base, (size_t)(1 + wfirst) * sizeof(msf_match),
                                              hipMemcpyDeviceToHost, st));
  HIP_TRY(h, "hipStreamSynchronize", hipStreamSynchronize(st));
  n_out[0] = *reinterpret_cast<const int32_t*>(h->h_pin);
  bool capacity = false;
  const int w = deliverable(h, n_out[0], cap_per_pair, &capacity);
  const int w1 = w < wfirst ? w : wfirst;
  if (w1 > 0) std::memcpy(out, h->h_pin + 1, (size_t)w1 * sizeof(msf_match));
  if (w > w1)   // a list longer than the pinned part: the rest straight from the staging list
    HIP_TRY(h, "hipMemcpy", hipMemcpy(out + w1, h->d_out + w1, (size_t)(w - w1) * sizeof(msf_match), hipMemcpyDeviceToHost));
  return capacity ? fail(h, MSF_ERR_CAPACITY, kNoResult) : MSF_OK;
}

// The front half of the one-vs-many entry points (msf_match_one_to_many, msf_create_map_points), n > 0.
// one_to_many_args: the checks on the slots, with the entry point's name in front of the message.
int one_to_many_args(msf_handle* h, const char* name, int32_t query_slot, int32_t n, const int32_t* slots) {
  const int maxp = h->cfg.max_batch_pairs;
  const std::string who = std::string(name) + ": ";
  if (n > maxp) return fail(h, MSF_ERR_INVALID_ARG, who + "n exceeds max_batch_pairs");
  if (!h->d_store) return fail(h, MSF_ERR_INVALID_ARG, who + "no frame was stored");
  if (query_slot < 0 || query_slot >= 2 * maxp) return fail(h, MSF_ERR_INVALID_ARG, who + "bad query slot");
  for (int i = 0; i < n; i++)
    if (slots[i] < 0 || slots[i] >= 2 * maxp) return fail(h, MSF_ERR_INVALID_ARG, who + "bad slot");
  return MSF_OK;
}

// launch_one_to_many: the slot arrays to the device (h->d_idx: query slot per pair, then train slot per pair), then the
// match of the n pairs into the handle's lists h->d_out [n][stage_cap] and counts h->d_n [n].
int launch_one_to_many(msf_handle* h, int32_t query_slot, int32_t n, const int32_t* slots, hipStream_t st) {
  const int maxp = h->cfg.max_batch_pairs;
  int32_t* d_query = h->d_idx;
  int32_t* d_train = h->d_idx + maxp;
  h->idx_stage.resize((size_t)2 * maxp);
  for (int i = 0; i < n; i++) { h->idx_stage[i] = query_slot; h->idx_stage[maxp + i] = slots[i]; }
  HIP_TRY(h, "hipMemcpyAsync(idx)",
          hipMemcpyAsync(d_query, h->idx_stage.data(), (size_t)2 * maxp * sizeof(int32_t), hipMemcpyHostToDevice, st));
  return match_slot_pairs(h, n, d_query, d_train, h->d_out, h->stage_cap, h->d_n, st, 0);
}

// MatchFrames(a, b) through the frame cache: per frame a hash + byte compare on the host; only frames not seen lately
// are uploaded and extracted; then one slot-pair match.  Same lists as the stateless path (tests/test_frame_cache_gpu.py).
int match_pair_cached(msf_handle* h, const msf_image* a, const msf_image* b, msf_match* out, int32_t cap, int32_t* n_out,
                      hipStream_t st) {
  uint8_t* dA = h->d_stage;
  uint8_t* dB = h->d_stage + (size_t)h->cfg.max_batch_pairs * h->stage_frame;
  int ea = -1, eb = -1;
  if (int rc = cached_slot(h, a, -1, dA, st, &ea)) return rc;
  if (int rc = cached_slot(h, b, ea, dB, st, &eb)) return rc;
  int rc = match_slot_pairs(h, 1, h->d_fc_slots + ea, h->d_fc_slots + eb, h->d_out, h->stage_cap, single_count(h), st, 0);
  if (rc == MSF_OK) rc = fetch_single(h, out, cap, n_out, st);
  if (rc != MSF_OK) {
    // the extractions of this call may not have completed, and a failed (or overflowed) frame must not be served from
    // the cache again: forget both entries
    h->fc[ea].valid = false;
    h->fc[eb].valid = false;
  }
  return rc;
}

}  // namespace

extern "C" {

int msf_abi_version(void) { return MSF_ABI_VERSION; }

void msf_default_config(msf_config* cfg, int kind) {
  if (!cfg) return;
  *cfg = msf_config{};
  cfg->struct_size = sizeof(msf_config);
  cfg->kind = kind;
  cfg->device = 0;
  cfg->threshold = kind == MSF_KIND_LOFTR ? 0.15f : 0.8f;  // dnnfeaturematcher.h:11 / featurematcher.h:9
  cfg->image_width = 640;                                  // dnnfeaturematcher.h:12-13
  cfg->image_height = 480;
  cfg->max_batch_pairs = 1;
  cfg->flags = 0;
  cfg->weights_path = nullptr;
}

int msf_create(const msf_config* cfg, msf_handle** out) {
  return guarded("msf_create", [&]() -> int {
    if (!cfg || !out) return fail(nullptr, MSF_ERR_INVALID_ARG, "msf_create: null argument");
    *out = nullptr;
    if (cfg->struct_size != sizeof(msf_config)) return fail(nullptr, MSF_ERR_INVALID_ARG, "msf_create: struct_size mismatch");
    if (cfg->kind != MSF_KIND_ORB && cfg->kind != MSF_KIND_LOFTR) return fail(nullptr, MSF_ERR_INVALID_ARG, "msf_create: bad kind");
    if (cfg->max_batch_pairs < 1) return fail(nullptr, MSF_ERR_INVALID_ARG, "msf_create: max_batch_pairs < 1");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
      return fail(nullptr, MSF_ERR_HIP, "msf_create: no HIP device (this library has no CPU fallback)");
    if (cfg->device < 0 || cfg->device >= ndev) return fail(nullptr, MSF_ERR_INVALID_ARG, "msf_create: device ordinal out of range");
    HIP_TRY(nullptr, "hipSetDevice", hipSetDevice(cfg->device));
    msf_handle* h = new (std::nothrow) msf_handle();
    if (!h) return fail(nullptr, MSF_ERR_HIP, "out of host memory");
    struct Guard {   // whatever path leaves this function without success (an exception included) frees the handle
      msf_handle* h;
      ~Guard() { if (h) msf_destroy(h); }
    } guard{h};
    h->cfg = *cfg;
    h->cfg.weights_path = nullptr;
    std::string err;
    const bool profile = (cfg->flags & MSF_FLAG_PROFILE) != 0;
    int n_cache = kFrameCacheSlots;
    if (const char* ev = getenv("MSF_FRAME_CACHE_SLOTS")) n_cache = atoi(ev);
    if (cfg->flags & MSF_FLAG_NO_FRAME_CACHE) n_cache = 0;          // the flag wins over the environment
    n_cache = n_cache < 2 ? 0 : n_cache > 4096 ? 4096 : n_cache;   // a pair needs two entries
    if (const char* ev = getenv("MSF_FRAME_CACHE_HASH_BITS")) {    // tests: a few bits make hash collisions the rule
      const int bits = atoi(ev);
      if (bits >= 0 && bits < 64) h->fc_hash_mask = (1ull << bits) - 1ull;
    }
    if (cfg->kind == MSF_KIND_ORB) {
      h->fc_slot0 = 4 * cfg->max_batch_pairs;
      msf::OrbOptions o;
      o.width = cfg->image_width;
      o.height = cfg->image_height;
      o.max_slots = 4 * cfg->max_batch_pairs + n_cache;
      o.work_frames = 2 * cfg->max_batch_pairs;
      o.blur_half_up = (cfg->flags & MSF_FLAG_BLUR_TIE_HALF_UP) != 0;
      o.blur_sum256 = (cfg->flags & MSF_FLAG_BLUR_SUM256) != 0;
      o.profile = profile;
      o.dense_fast = (cfg->flags & MSF_FLAG_FAST_DENSE) != 0;
      o.level_size_mul_inv = (cfg->flags & MSF_FLAG_LEVEL_SIZE_MUL_INV) != 0;
      o.stream_min_frames = (cfg->flags & MSF_FLAG_FAST_STREAM) ? 1 : 8;
      err = h->orb.init(o);
    } else {
      if (cfg->image_width != 640 || cfg->image_height != 480)
        return fail(nullptr, MSF_ERR_UNSUPPORTED, "LoFTR_teacher is a fixed-shape 1x1x480x640 graph (model/LoFTR_teacher.onnx)");
      h->fc_slot0 = 2 * cfg->max_batch_pairs;
      err = h->loftr.init(cfg->weights_path, cfg->max_batch_pairs, profile, (cfg->flags & MSF_FLAG_KEEP_DEBUG) != 0, n_cache,
                          (cfg->flags & MSF_FLAG_LOFTR_F32) != 0);
    }
    if (!err.empty()) {
      const bool io = err.rfind("io:", 0) == 0, arg = err.rfind("arg:", 0) == 0;
      return fail(nullptr, io ? MSF_ERR_IO : arg ? MSF_ERR_INVALID_ARG : MSF_ERR_HIP, err);
    }
    // hipStreamDefault (a "blocking" stream): work on the handle's own stream is ordered against the legacy null stream,
    // which is where a caller that passes stream = NULL (e.g. torch's default stream) has its own work (msf_abi.h)
    HIP_TRY(nullptr, "hipStreamCreate", hipStreamCreateWithFlags(&h->stream, hipStreamDefault));
    if (n_cache > 0) {
      std::vector<int32_t> ids(n_cache);
      for (int i = 0; i < n_cache; i++) ids[i] = h->fc_slot0 + i;
      const size_t bytes = (size_t)n_cache * sizeof(int32_t);
      HIP_TRY(nullptr, "hipMalloc(frame cache slots)", h->d_fc_slots.reserve(bytes));
      HIP_TRY(nullptr, "hipMalloc(frame cache slots)", hipMemcpy(h->d_fc_slots, ids.data(), bytes, hipMemcpyHostToDevice));
      h->fc.resize(n_cache);
    }
    guard.h = nullptr;
    *out = h;
    return MSF_OK;
  });
}

void msf_destroy(msf_handle* h) {
  if (!h) return;
  hipSetDevice(h->cfg.device);
  hipDeviceSynchronize();
  h->orb.destroy();
  h->loftr.destroy();
  if (h->h_pin) hipHostFree(h->h_pin);
  if (h->h_gba_rec) hipHostFree(h->h_gba_rec);
  const hipStream_t stream = h->stream;
  delete h;   // the device buffers go with their DevBuf members, before the stream
  if (stream) hipStreamDestroy(stream);
}

int msf_set_threshold(msf_handle* h, float value) {
  return guarded(h, "msf_set_threshold", [&]() -> int {
    h->cfg.threshold = value;
    return MSF_OK;
  });
}

const char* msf_last_error(const msf_handle* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int msf_match_batch_device(msf_handle* h, int32_t n_pairs, const uint8_t* d_a, const uint8_t* d_b,
                           int64_t frame_stride, int64_t row_stride, msf_match* d_out, int32_t cap_per_pair,
                           int32_t* d_n_out, void* stream) {
  return guarded(h, "msf_match_batch_device", [&]() -> int {
    if (n_pairs < 0 || !d_a || !d_b || !d_out || !d_n_out || cap_per_pair < 1)
      return fail(h, MSF_ERR_INVALID_ARG, "msf_match_batch_device: bad argument");
    CallScope cs{h};
    if (int rc = cs.enter(stream)) return rc;
    if (int rc = run_device(h, n_pairs, d_a, d_b, frame_stride, row_stride, d_out, cap_per_pair, d_n_out, cs.st)) return rc;
    return cs.finish();
  });
}

int msf_match_batch(msf_handle* h, int32_t n_pairs, const msf_image* a, const msf_image* b, msf_match* out,
                    int32_t cap_per_pair, int32_t* n_out) {
  return guarded(h, "msf_match_batch", [&]() -> int {
    if (n_pairs < 0 || !a || !b || !out || !n_out || cap_per_pair < 1)
      return fail(h, MSF_ERR_INVALID_ARG, "msf_match_batch: bad argument");
    CallScope cs{h};
    if (int rc = cs.enter()) return rc;
    for (int i = 0; i < n_pairs; i++)
      if (!image_ok(h, &a[i]) || !image_ok(h, &b[i]))
        return fail(h, MSF_ERR_INVALID_ARG, "msf_match_batch: image size differs from the handle's, or null data");
    if (int rc = ensure_stage(h)) return rc;
    const int maxp = h->cfg.max_batch_pairs;
    hipStream_t st = cs.st;
    uint8_t* dA = h->d_stage;
    uint8_t* dB = h->d_stage + (size_t)maxp * h->stage_frame;
    if (n_pairs == 1) {   // the drop-in call: count in the record before the list, one copy, one synchronisation
      if (!h->fc.empty()) return match_pair_cached(h, &a[0], &b[0], out, cap_per_pair, n_out, st);
      if (int rc = upload_frame(h, dA, &a[0], st)) return rc;
      if (int rc = upload_frame(h, dB, &b[0], st)) return rc;
      if (int rc = run_device(h, 1, dA, dB, h->stage_frame, h->stage_pitch, h->d_out, h->stage_cap, single_count(h), st)) return rc;
      return fetch_single(h, out, cap_per_pair, n_out, st);
    }
    bool capacity = false;
    for (int p0 = 0; p0 < n_pairs; p0 += maxp) {   // chunks of max_batch_pairs: the counts, one wait, then the lists
      const int n = n_pairs - p0 < maxp ? n_pairs - p0 : maxp;
      for (int i = 0; i < n; i++) {
        if (int rc = upload_frame(h, dA + (size_t)i * h->stage_frame, &a[p0 + i], st)) return rc;
        if (int rc = upload_frame(h, dB + (size_t)i * h->stage_frame, &b[p0 + i], st)) return rc;
      }
      if (int rc = run_device(h, n, dA, dB, h->stage_frame, h->stage_pitch, h->d_out, h->stage_cap, h->d_n, st)) return rc;
      HIP_TRY(h, "hipMemcpyAsync", hipMemcpyAsync(n_out + p0, h->d_n, (size_t)n * 4, hipMemcpyDeviceToHost, st));
      HIP_TRY(h, "hipStreamSynchronize", hipStreamSynchronize(st));
      if (int rc = copy_lists_back(h, n, n_out + p0, out + (size_t)p0 * cap_per_pair, cap_per_pair, &capacity)) return rc;
    }
    return capacity ? fail(h, MSF_ERR_CAPACITY, kNoResult) : MSF_OK;
  });
}

int msf_match_pair(msf_handle* h, const msf_image* a, const msf_image* b, msf_match* out, int32_t cap,
                   int32_t* n_out) {
  return msf_match_batch(h, 1, a, b, out, cap, n_out);
}

int msf_extract_device(msf_handle* h, int32_t n_frames, const uint8_t* d_frames, int64_t frame_stride,
                       int64_t row_stride, int32_t first_slot, void* stream) {
  return guarded(h, "msf_extract_device", [&]() -> int {
    // both kinds: the caller's slots are [0, 2P); what lies beyond (scratch of the stateless calls, the transparent
    // frame cache) belongs to the handle
    if (n_frames < 0 || !d_frames || first_slot < 0 || (long long)first_slot + n_frames > 2ll * h->cfg.max_batch_pairs)
      return fail(h, MSF_ERR_INVALID_ARG, "msf_extract_device: slot range outside [0, 2*max_batch_pairs)");
    if (!aligned16(d_frames, frame_stride, row_stride))
      return fail(h, MSF_ERR_INVALID_ARG, "device frames must be 16-byte aligned with strides multiple of 16");
    CallScope cs{h};
    if (int rc = cs.enter(stream)) return rc;
    if (row_stride < h->cfg.image_width ||
        (n_frames > 1 && frame_stride < row_stride * (long long)h->cfg.image_height))   // one frame: its stride is unused
      return fail(h, MSF_ERR_INVALID_ARG, "msf_extract_device: strides smaller than the frame");
    if (int rc = extract_into_slots(h, d_frames, n_frames, frame_stride, row_stride, first_slot, cs.st)) return rc;
    return cs.finish();
  });
}

int msf_match_slots_device(msf_handle* h, int32_t n_pairs, const int32_t* d_slot_a, const int32_t* d_slot_b,
                           msf_match* d_out, int32_t cap_per_pair, int32_t* d_n_out, void* stream) {
  return guarded(h, "msf_match_slots_device", [&]() -> int {
    if (n_pairs < 0 || !d_slot_a || !d_slot_b || !d_out || !d_n_out || cap_per_pair < 1)
      return fail(h, MSF_ERR_INVALID_ARG, "msf_match_slots_device: bad argument");
    CallScope cs{h};
    if (int rc = cs.enter(stream)) return rc;
    if (h->cfg.kind != MSF_KIND_ORB && n_pairs > h->cfg.max_batch_pairs)   // LoFTR works on per-pair token buffers
      return fail(h, MSF_ERR_INVALID_ARG, "n_pairs exceeds max_batch_pairs");
    if (int rc = match_slot_pairs(h, n_pairs, d_slot_a, d_slot_b, d_out, cap_per_pair, d_n_out, cs.st,
                                  2 * h->cfg.max_batch_pairs))   // the caller's slots only
      return rc;
    return cs.finish();
  });
}

int msf_pack_matches_device(msf_handle* h, int32_t n_pairs, const msf_match* d_in, int32_t cap_per_pair,
                            const int32_t* d_n_out, msf_match* d_packed, int32_t* d_offsets, void* stream) {
  return guarded(h, "msf_pack_matches_device", [&]() -> int {
    if (n_pairs < 0 || !d_in || !d_n_out || !d_packed || !d_offsets || cap_per_pair < 1)
      return fail(h, MSF_ERR_INVALID_ARG, "msf_pack_matches_device: bad argument");
    CallScope cs{h};
    if (int rc = cs.enter(stream)) return rc;
    HIP_TRY(h, "pack_matches", msf::pack_matches(n_pairs, d_in, cap_per_pair, d_n_out, d_packed, d_offsets, cs.st));
    return cs.finish();
  });
}

int msf_set_mappoints(msf_handle* h, int32_t map_slot, const int32_t* keys, int32_t n_keys) {
  return guarded(h, "msf_set_mappoints", [&]() -> int {
    const int n_maps = 2 * h->cfg.max_batch_pairs;
    const long long n_px = (long long)h->cfg.image_width * h->cfg.image_height;
    if (map_slot < 0 || map_slot >= n_maps || n_keys < 0 || (n_keys > 0 && !keys))
      return fail(h, MSF_ERR_INVALID_ARG, "msf_set_mappoints: bad argument");
    CallScope cs{h};
    if (int rc = cs.enter()) return rc;
    if (int rc = ensure_maps(h)) return rc;
    h->map_stage.assign(h->map_words, 0u);
    for (int i = 0; i < n_keys; i++) {
      // KeyPointMap::SetMapPoint ignores points outside the image (KeyPointMap.cc:38-39); a key is y*cols + x
      if (keys[i] < 0 || keys[i] >= n_px) continue;
      h->map_stage[keys[i] >> 5] |= 1u << (keys[i] & 31);
    }
    HIP_TRY(h, "hipMemcpyAsync(map bitmap)",
            hipMemcpyAsync(h->d_maps + (size_t)map_slot * h->map_words, h->map_stage.data(),
                           (size_t)h->map_words * sizeof(uint32_t), hipMemcpyHostToDevice, cs.st));
    return cs.finish();
  });
}

int msf_count_mappoint_matches_device(msf_handle* h, int32_t n_pairs, const msf_match* d_matches,
                                      int32_t cap_per_pair, const int32_t* d_n_matches, const int32_t* d_map_a,
                                      const int32_t* d_map_b, int32_t* d_num_mp, void* stream) {
  return guarded(h, "msf_count_mappoint_matches_device", [&]() -> int {
    if (n_pairs < 0 || !d_matches || !d_n_matches || !d_map_a || !d_map_b || !d_num_mp || cap_per_pair < 1)
      return fail(h, MSF_ERR_INVALID_ARG, "msf_count_mappoint_matches_device: bad argument");
    if (!h->d_maps) return fail(h, MSF_ERR_INVALID_ARG, "msf_count_mappoint_matches_device: no map slot was ever set");
    CallScope cs{h};
    if (int rc = cs.enter(stream)) return rc;
    HIP_TRY(h, "count_mappoint_matches",
            msf::count_mappoint_matches(n_pairs, d_matches, cap_per_pair, d_n_matches, d_map_a, d_map_b, h->d_maps, h->n_maps,
                                        h->map_words, h->cfg.image_width, h->cfg.image_height, d_num_mp, cs.st));
    return cs.finish();
  });
}

int msf_store_frame(msf_handle* h, int32_t slot, const msf_image* img) {
  return guarded(h, "msf_store_frame", [&]() -> int {
    const int maxp = h->cfg.max_batch_pairs;
    if (slot < 0 || slot >= 2 * maxp || !image_ok(h, img))
      return fail(h, MSF_ERR_INVALID_ARG, "msf_store_frame: slot outside [0, 2*max_batch_pairs) or image size differs from the handle's");
    CallScope cs{h};
    if (int rc = cs.enter()) return rc;
    if (int rc = ensure_stage(h)) return rc;
    if (!h->d_store) {
      HIP_TRY(h, "hipMalloc(frame store)", h->d_store.reserve((size_t)2 * maxp * h->stage_frame));
      HIP_TRY(h, "hipMalloc(idx)", h->d_idx.reserve((size_t)3 * maxp * sizeof(int32_t)));
    }
    uint8_t* dst = h->d_store + (size_t)slot * h->stage_frame;
    if (int rc = upload_frame(h, dst, img, cs.st)) return rc;
    // features (ORB) / backbone tokens (LoFTR) of the frame are extracted once, here
    if (int rc = extract_into_slots(h, dst, 1, h->stage_frame, h->stage_pitch, slot, cs.st)) return rc;
    return cs.finish();
  });
}

int msf_match_one_to_many(msf_handle* h, int32_t query_slot, int32_t n, const int32_t* slots, int32_t* num_matches,
                          int32_t* num_mp, msf_match* out, int32_t cap_per_pair) {
  return guarded(h, "msf_match_one_to_many", [&]() -> int {
    const char* const name = "msf_match_one_to_many";
    if (n < 0 || (n > 0 && (!slots || !num_matches)) || (out && cap_per_pair < 1))
      return fail(h, MSF_ERR_INVALID_ARG, std::string(name) + ": bad argument");
    if (n == 0) return MSF_OK;
    if (int rc = one_to_many_args(h, name, query_slot, n, slots)) return rc;
    if (num_mp && !h->d_maps) return fail(h, MSF_ERR_INVALID_ARG, "msf_match_one_to_many: no map slot was ever set");
    CallScope cs{h};
    if (int rc = cs.enter()) return rc;
    hipStream_t st = cs.st;
    if (int rc = launch_one_to_many(h, query_slot, n, slots, st)) return rc;
    if (num_mp) {
      const int maxp = h->cfg.max_batch_pairs;
      int32_t* d_num_mp = h->d_idx + 2 * maxp;
      HIP_TRY(h, "count_mappoint_matches",
              msf::count_mappoint_matches(n, h->d_out, h->stage_cap, h->d_n, h->d_idx, h->d_idx + maxp, h->d_maps,
                                          h->n_maps, h->map_words, h->cfg.image_width, h->cfg.image_height, d_num_mp, st));
      HIP_TRY(h, "hipMemcpyAsync", hipMemcpyAsync(num_mp, d_num_mp, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(h, "hipMemcpyAsync", hipMemcpyAsync(num_matches, h->d_n, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    if (int rc = cs.finish()) return rc;
    bool capacity = false;
    if (int rc = copy_lists_back(h, n, num_matches, out, cap_per_pair, &capacity)) return rc;
    return capacity ? fail(h, MSF_ERR_CAPACITY, kNoResult) : MSF_OK;
  });
}

namespace {

// The device arrays of one msf_check_hypotheses call, all pieces of the workspace: m21 / m12 [hc][9], scores [hc],
// inliers [hc * mc] (the call indexes it with its own n_matches), matches [mc].
struct HypothesesPlan {
  float* m21 = nullptr, *m12 = nullptr, *scores = nullptr;
  uint8_t* inliers = nullptr;
  msf_match* matches = nullptr;
};

}  // namespace

int msf_check_hypotheses(msf_handle* h, int32_t model, int32_t n_hyp, const float* m21, const float* m12,
                         int32_t n_matches, const msf_match* matches, float sigma, float* scores, int32_t* best,
                         uint8_t* best_inliers) {
  return guarded(h, "msf_check_hypotheses", [&]() -> int {
    const bool homography = model == MSF_MODEL_HOMOGRAPHY;
    if ((!homography && model != MSF_MODEL_FUNDAMENTAL) || n_hyp < 0 || n_matches < 0 || n_matches > 8192 ||
        (n_hyp > 0 && (!m21 || !scores || (homography && !m12))) || (n_matches > 0 && !matches) || !best ||
        (n_matches > 0 && !best_inliers))
      return fail(h, MSF_ERR_INVALID_ARG, "msf_check_hypotheses: bad argument (models 0/1, at most 8192 matches)");
    *best = -1;
    for (int i = 0; i < n_matches; i++) best_inliers[i] = 0;   // FindHomography: vbMatchesInliers(N, false) (Initializer.cc:167)
    if (n_hyp == 0) return MSF_OK;
    CallScope cs{h};
    if (int rc = cs.enter()) return rc;
    // sized for at least 256 hypotheses and 2048 matches: no allocation in the steady state
    const size_t hc = n_hyp > 256 ? n_hyp : 256, mc = n_matches > 2048 ? n_matches : 2048;
    HypothesesPlan p;
    if (int rc = carve(h, h->d_hyp, 0, "hipMalloc", [&](msf::Carver& c) {
          p.m21 = c.take<float>(hc * 9);
          p.m12 = c.take<float>(hc * 9);
          p.scores = c.take<float>(hc);
          p.inliers = c.take<uint8_t>(hc * mc);
          p.matches = c.take<msf_match>(mc);
        }))
      return rc;
    hipStream_t st = cs.st;
    const size_t mat_bytes = (size_t)n_hyp * 9 * sizeof(float);
    HIP_TRY(h, "hipMemcpyAsync", hipMemcpyAsync(p.m21, m21, mat_bytes, hipMemcpyHostToDevice, st));
    if (homography) HIP_TRY(h, "hipMemcpyAsync", hipMemcpyAsync(p.m12, m12, mat_bytes, hipMemcpyHostToDevice, st));
    if (n_matches)
      HIP_TRY(h, "hipMemcpyAsync", hipMemcpyAsync(p.matches, matches, (size_t)n_matches * sizeof(msf_match), hipMemcpyHostToDevice, st));
    HIP_TRY(h, "check_hypotheses", msf::check_hypotheses(model, n_hyp, p.m21, p.m12, n_matches, p.matches, sigma, p.scores, p.inliers, st));
    if (int rc = fetch(h, st, scores, p.scores, (size_t)n_hyp * sizeof(float))) return rc;
    if (int rc = cs.finish()) return rc;
    // FindHomography / FindFundamental keep the first hypothesis whose score beats every earlier one (:190-194, :236-240)
    float score = 0.0f;
    for (int i = 0; i < n_hyp; i++)
      if (scores[i] > score) { score = scores[i]; *best = i; }
    if (*best >= 0 && n_matches)
      HIP_TRY(h, "hipMemcpy", hipMemcpy(best_inliers, p.inliers + (size_t)*best * n_matches, (size_t)n_matches, hipMemcpyDeviceToHost));
    return MSF_OK;
  });
}

namespace {

// The device arrays of one find-models call: the caller's where it gave one, else a piece of the handle's workspace.
struct FindModelsPlan {
  float4* pn = nullptr;
  float* T = nullptr;
  int32_t* sets = nullptr;
  msf_match* matches = nullptr;   // single-list call only
  float* m21[2] = {}, *aux[2] = {}, *null_vec[2] = {}, *scores[2] = {};
  int32_t* best[2] = {};
  uint8_t* inliers[2] = {};
};

// user: the device pointers the caller supplied.  host_call: the host entry point -- `user` is empty, and the match list
// and every output get a piece of the workspace.  Returns MSF_OK or an error.
int plan_find_models(msf_handle* h, int n_lists, int cap, int n_hyp, bool host_call, const msf_ransac_batch* user,
                     FindModelsPlan* p) {
  const size_t L = (size_t)n_lists, LH = L * (size_t)n_hyp;
  const msf_ransac_result* res[2] = {&user->homography, &user->fundamental};
  return carve(h, h->d_fm, (size_t)1 << 20, "hipMalloc(find-models workspace)", [&](msf::Carver& c) {
    p->pn = c.take<float4>(L * cap);
    p->T = c.take<float>(L * 18);
    p->sets = c.take(user->sets, LH * 8);
    p->matches = host_call ? c.take<msf_match>(cap) : nullptr;
    for (int m = 0; m < 2; m++) {
      p->m21[m] = c.take(res[m]->m21, LH * 9);
      p->aux[m] = c.take(m == 0 ? res[m]->m12 : res[m]->fn, LH * 9);
      p->null_vec[m] = host_call ? c.take<float>(LH * 9) : res[m]->null_vec;
      p->scores[m] = c.take(res[m]->scores, LH ? LH : 1);
      p->best[m] = host_call ? c.take<int32_t>(1) : res[m]->best;
      p->inliers[m] = host_call ? c.take<uint8_t>(cap) : res[m]->best_inliers;
    }
  });
}

bool ransac_result_ok(const msf_ransac_result* r) {
  return r && r->struct_size == sizeof(msf_ransac_result) && r->best;
}

}  // namespace

int msf_find_models(msf_handle* h, int32_t n_matches, const msf_match* matches, int32_t n_hyp, const int32_t* sets,
                    float sigma, msf_ransac_result* homography, msf_ransac_result* fundamental) {
  return guarded(h, "msf_find_models", [&]() -> int {
    if (!ransac_result_ok(homography) || !ransac_result_ok(fundamental) || n_hyp < 0 || n_hyp > (1 << 20) ||
        n_matches < 0 || n_matches > 8192 || (n_matches > 0 && !matches) ||
        (n_hyp > 0 && (n_matches < 8 || !sets || !homography->scores || !fundamental->scores)))
      return fail(h, MSF_ERR_INVALID_ARG, "msf_find_models: bad argument (8 to 8192 matches, sets, best and scores "
                                          "required, struct_size = sizeof(msf_ransac_result))");
    for (long long i = 0; i < 8ll * n_hyp; i++)
      if (sets[i] < 0 || sets[i] >= n_matches)
        return fail(h, MSF_ERR_INVALID_ARG, "msf_find_models: a set holds an index outside [0, n_matches)");
    msf_ransac_result* res[2] = {homography, fundamental};
    for (int m = 0; m < 2; m++) {
      *res[m]->best = -1;
      if (res[m]->best_inliers)
        for (int i = 0; i < n_matches; i++) res[m]->best_inliers[i] = 0;
    }
    if (n_hyp == 0) return MSF_OK;
    CallScope cs{h};
    if (int rc = cs.enter()) return rc;
    // device side: every array is a piece of the workspace
    msf_ransac_batch dev{};
    FindModelsPlan p;
    if (int rc = plan_find_models(h, 1, n_matches, n_hyp, true, &dev, &p)) return rc;
    hipStream_t st = cs.st;
    Drain drain{st};
    HIP_TRY(h, "hipMemcpyAsync", hipMemcpyAsync(p.matches, matches, (size_t)n_matches * sizeof(msf_match), hipMemcpyHostToDevice, st));
    HIP_TRY(h, "hipMemcpyAsync", hipMemcpyAsync(p.sets, sets, (size_t)n_hyp * 8 * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(h, "find_models", msf::find_models(1, p.matches, n_matches, nullptr, n_matches, n_hyp, p.sets, sigma, p.pn, p.T, p.m21,
                                               p.aux, p.null_vec, p.scores, p.best, p.inliers, st));
    const size_t mat_bytes = (size_t)n_hyp * 9 * sizeof(float);
    for (int m = 0; m < 2; m++) {
      if (int rc = fetch(h, st, res[m]->m21, p.m21[m], mat_bytes)) return rc;
      if (int rc = fetch(h, st, m == 0 ? res[m]->m12 : res[m]->fn, p.aux[m], mat_bytes)) return rc;
      if (int rc = fetch(h, st, res[m]->null_vec, p.null_vec[m], mat_bytes)) return rc;
      if (int rc = fetch(h, st, res[m]->scores, p.scores[m], (size_t)n_hyp * sizeof(float))) return rc;
      if (int rc = fetch(h, st, res[m]->best, p.best[m], sizeof(int32_t))) return rc;
      if (int rc = fetch(h, st, res[m]->best_inliers, p.inliers[m], (size_t)n_matches)) return rc;
      if (int rc = fetch(h, st, res[m]->T1, p.T, 9 * sizeof(float))) return rc;
      if (int rc = fetch(h, st, res[m]->T2, p.T + 9, 9 * sizeof(float))) return rc;
    }
    drain.armed = false;
    return cs.finish();   // the one wait of the call
  });
}

int msf_find_models_device(msf_handle* h, int32_t n_lists, const msf_match* d_matches, int32_t cap_per_pair,
                           const int32_t* d_n_out, int32_t n_hyp, uint64_t seed, float sigma, msf_ransac_batch* out,
                           void* stream) {
  return guarded(h, "msf_find_models_device", [&]() -> int {
    if (!out || out->struct_size != sizeof(msf_ransac_batch) || !ransac_result_ok(&out->homography) ||
        !ransac_result_ok(&out->fundamental) || n_lists < 0 || n_lists > 65535 || n_hyp < 0 || n_hyp > (1 << 20) ||
        cap_per_pair < 1 || (n_lists > 0 && (!d_matches || !d_n_out)))
      return fail(h, MSF_ERR_INVALID_ARG, "msf_find_models_device: bad argument (at most 65535 lists, best required, "
                                          "struct_size = sizeof(msf_ransac_batch))");
    if (n_lists == 0) return MSF_OK;
    CallScope cs{h};
    if (int rc = cs.enter(stream)) return rc;
    FindModelsPlan p;
    if (int rc = plan_find_models(h, n_lists, cap_per_pair, n_hyp, false, out, &p)) return rc;
    hipStream_t st = cs.st;
    HIP_TRY(h, "ransac_sets", msf::ransac_sets(n_lists, n_hyp, d_n_out, cap_per_pair, seed, p.sets, st));
    HIP_TRY(h, "find_models", msf::find_models(n_lists, d_matches, cap_per_pair, d_n_out, 0, n_hyp, p.sets, sigma, p.pn, p.T, p.m21,
                                               p.aux, p.null_vec, p.scores, p.best, p.inliers, st));
    const msf_ransac_result* res[2] = {&out->homography, &out->fundamental};
    for (int m = 0; m < 2; m++) {   // T lives as [n_lists][2][9] in the workspace; the caller's T1 / T2 are [n_lists][9] each
      if (res[m]->T1) HIP_TRY(h, "hipMemcpy2DAsync", hipMemcpy2DAsync(res[m]->T1, 36, p.T, 72, 36, n_lists, hipMemcpyDeviceToDevice, st));
      if (res[m]->T2) HIP_TRY(h, "hipMemcpy2DAsync", hipMemcpy2DAsync(res[m]->T2, 36, p.T + 9, 72, 36, n_lists, hipMemcpyDeviceToDevice, st));
    }
    return cs.finish();
  });
}

// ---- msf_initializer.h: the tail of Initializer::Initialize ----
namespace {

// What a reconstruct call keeps in the workspace besides its result arrays (result_arrays.h: kMotionArrays).
struct ReconstructPlan {
  int32_t* n_inliers = nullptr;   // MotionOut::n_inliers [n_lists]: handed from launch to launch, no result
  msf_match* matches = nullptr;   // host call only: the list, its inlier flags and its matrix
  uint8_t* inliers = nullptr;
  float* m21 = nullptr;
};

// nullptr when the parameters are usable, else what is wrong with them
const char* motion_params_fault(const msf_motion_params* prm) {
  if (!prm) return "params is NULL";
  if (prm->struct_size != sizeof(msf_motion_params)) return "params->struct_size is not sizeof(msf_motion_params)";
  bool finite = std::isfinite(prm->sigma) && std::isfinite(prm->min_parallax);
  for (int k = 0; k < 9; k++) finite = finite && std::isfinite(prm->K[k]);
  if (!finite) return "K, sigma and min_parallax must be finite";
  float inv[9];
  msf::ransac::inv3(prm->K, inv);
  bool zero = true;
  for (int k = 0; k < 9; k++) zero = zero && inv[k] == 0.0f;
  if (zero) return "K is singular";
  return nullptr;
}

msf::MotionParams motion_params(const msf_motion_params* prm) {
  msf::MotionParams d{};
  for (int k = 0; k < 9; k++) d.K[k] = prm->K[k];
  d.th2 = 4.0f * (prm->sigma * prm->sigma);   // 4.0f * mSigma2
  d.min_triangulated = prm->min_triangulated;
  d.min_parallax = prm->min_parallax;
  return d;
}

msf::NewPointParams new_point_params(const msf_new_points_params* prm) {
  return msf::NewPointParams{prm->max_cos_parallax, prm->chi2};
}

}  // namespace

int msf_initializer_version(void) { return MSF_INITIALIZER_VERSION; }

int msf_reconstruct(msf_handle* h, int32_t model, const float* m21, int32_t n_matches, const msf_match* matches,
                    const uint8_t* inliers, const msf_motion_params* params, msf_motion_result* out) {
  return guarded(h, "msf_reconstruct", [&]() -> int {
    if (!out || out->struct_size != sizeof(msf_motion_result))
      return fail(h, MSF_ERR_INVALID_ARG, "msf_reconstruct: out is NULL or out->struct_size is not sizeof(msf_motion_result)");
    if (!out->ok || !m21 || (n_matches > 0 && (!matches || !inliers)))
      return fail(h, MSF_ERR_INVALID_ARG, "msf_reconstruct: a required pointer is NULL (m21, matches, inliers, out->ok)");
    if (n_matches < 0 || n_matches > msf::kMaxReconstructMatches)
      return fail(h, MSF_ERR_INVALID_ARG, "msf_reconstruct: n_matches outside [0, 8192]");
    if (model != MSF_MODEL_HOMOGRAPHY && model != MSF_MODEL_FUNDAMENTAL)
      return fail(h, MSF_ERR_INVALID_ARG, "msf_reconstruct: model is neither MSF_MODEL_HOMOGRAPHY nor MSF_MODEL_FUNDAMENTAL");
    if (const char* fault = motion_params_fault(params))
      return fail(h, MSF_ERR_INVALID_ARG, std::string("msf_reconstruct: ") + fault);
    CallScope cs{h};
    if (int rc = cs.enter()) return rc;
    const int cap = n_matches > 0 ? n_matches : 1;
    const size_t units[] = {1};
    msf_motion_result dev{};
    ReconstructPlan p;
    if (int rc = carve(h, h->d_rc, (size_t)1 << 16, "hipMalloc(reconstruct workspace)", [&](msf::Carver& c) {
          msf::carve_result(c, msf::kMotionArrays, units, (size_t)cap, nullptr, *out, &dev);
          p.n_inliers = c.take<int32_t>(1);
          p.matches = c.take<msf_match>(cap);
          p.inliers = c.take<uint8_t>(cap);
          p.m21 = c.take<float>(9);
        }))
      return rc;
    msf::MotionOut o = to_out(dev);
    o.n_inliers = p.n_inliers;
    hipStream_t st = cs.st;
    Drain drain{st};
    if (n_matches > 0) {
      HIP_TRY(h, "hipMemcpyAsync", hipMemcpyAsync(p.matches, matches, (size_t)n_matches * sizeof(msf_match), hipMemcpyHostToDevice, st));
      HIP_TRY(h, "hipMemcpyAsync", hipMemcpyAsync(p.inliers, inliers, (size_t)n_matches, hipMemcpyHostToDevice, st));
    }
    HIP_TRY(h, "hipMemcpyAsync", hipMemcpyAsync(p.m21, m21, 9 * sizeof(float), hipMemcpyHostToDevice, st));
    msf::MotionLists in{};
    in.matches = p.matches;
    in.cap = cap;
    in.n_single = n_matches;
    in.n_hyp = 1;
    in.forced_model = model;
    in.m21[model] = p.m21;
    in.inliers[model] = p.inliers;
    HIP_TRY(h, "reconstruct_motion", msf::reconstruct_motion(1, in, motion_params(params), o, st));
    const msf::Extent all{0, (size_t)cap, (size_t)cap, (size_t)n_matches, units, units};
    if (int rc = fetch_result(h, st, msf::kMotionArrays, dev, *out, all)) return rc;
    drain.armed = false;
    return cs.finish();   // the one wait of the call
  });
}

int msf_reconstruct_device(msf_handle* h, int32_t n_lists, const msf_match* d_matches, int32_t cap_per_pair,
                           const int32_t* d_n_out, int32_t n_hyp, const msf_ransac_batch* found,
                           const msf_motion_params* params, msf_motion_result* out, void* stream) {
  return guarded(h, "msf_reconstruct_device", [&]() -> int {
    if (!out || out->struct_size != sizeof(msf_motion_result))
      return fail(h, MSF_ERR_INVALID_ARG, "msf_reconstruct_device: out is NULL or out->struct_size is not sizeof(msf_motion_result)");
    if (!found || found->struct_size != sizeof(msf_ransac_batch))
      return fail(h, MSF_ERR_INVALID_ARG, "msf_reconstruct_device: found is NULL or found->struct_size is not sizeof(msf_ransac_batch)");
    const msf_ransac_result* res[2] = {&found->homography, &found->fundamental};
    bool complete = out->ok && (n_lists <= 0 || (d_matches && d_n_out));
    for (int m = 0; m < 2; m++)
      complete = complete && res[m]->m21 && res[m]->scores && res[m]->best && res[m]->best_inliers;
    if (!complete)
      return fail(h, MSF_ERR_INVALID_ARG, "msf_reconstruct_device: a required pointer is NULL (d_matches, d_n_out, out->ok; "
                                          "m21, scores, best and best_inliers of both models of found)");
    if (n_lists < 0 || n_lists > 65535)
      return fail(h, MSF_ERR_INVALID_ARG, "msf_reconstruct_device: n_lists outside [0, 65535]");
    if (cap_per_pair < 1 || n_hyp < 1 || n_hyp > (1 << 20))
      return fail(h, MSF_ERR_INVALID_ARG, "msf_reconstruct_device: cap_per_pair < 1 or n_hyp outside [1, 2^20]");
    if (const char* fault = motion_params_fault(params))
      return fail(h, MSF_ERR_INVALID_ARG, std::string("msf_reconstruct_device: ") + fault);
    if (n_lists == 0) return MSF_OK;
    CallScope cs{h};
    if (int rc = cs.enter(stream)) return rc;
    const size_t units[] = {(size_t)n_lists};
    msf_motion_result dev{};
    ReconstructPlan p;
    if (int rc = carve(h, h->d_rc, (size_t)1 << 16, "hipMalloc(reconstruct workspace)", [&](msf::Carver& c) {
          msf::carve_result(c, msf::kMotionArrays, units, (size_t)cap_per_pair, out, *out, &dev);
          p.n_inliers = c.take<int32_t>(n_lists);
        }))
      return rc;
    msf::MotionOut o = to_out(dev);
    o.n_inliers = p.n_inliers;
    msf::MotionLists in{};
    in.matches = d_matches;
    in.cap = cap_per_pair;
    in.n_out = d_n_out;
    in.n_hyp = n_hyp;
    in.forced_model = -1;
    for (int m = 0; m < 2; m++) {
      in.m21[m] = res[m]->m21;
      in.scores[m] = res[m]->scores;
      in.best[m] = res[m]->best;
      in.inliers[m] = res[m]->best_inliers;
    }
    HIP_TRY(h, "reconstruct_motion", msf::reconstruct_motion(n_lists, in, motion_params(params), o, cs.st));
    return cs.finish();
  });
}

namespace {

// What the host entry points of msf_local_mapping.h keep in the workspace besides their result arrays
// (result_arrays.h: kNewPointsArrays): [lists] views of either side and, for msf_new_points, the list.
struct NewPointsPlan {
  msf_view* view1 = nullptr;
  msf_view* view2 = nullptr;
  msf_match* matches = nullptr;
};

// The copy-back of the host entry points goes in two: n_new and the per-match arrays up to the list's end, then --
// once the count is on the host -- the first n_new records of packed.
struct NewPointsWanted {
  msf_new_points_result rows, records{};
  explicit NewPointsWanted(const msf_new_points_result& out) : rows(out) {
    rows.n_new = nullptr;   // fetched first, by the entry point
    rows.packed = nullptr;
    records.packed = out.packed;
  }
};

// nullptr when params and out are usable, else what is wrong with them
const char* new_points_fault(const msf_new_points_params* prm, const msf_new_points_result* out) {
  if (!out || out->struct_size != sizeof(msf_new_points_result)) return "out is NULL or out->struct_size is not sizeof(msf_new_points_result)";
  if (!prm || prm->struct_size != sizeof(msf_new_points_params)) return "params is NULL or params->struct_size is not sizeof(msf_new_points_params)";
  if (std::isnan(prm->max_cos_parallax) || std::isnan(prm->chi2)) return "max_cos_parallax and chi2 must not be NaN";
  if (!out->n_new) return "a required pointer is NULL (out->n_new)";
  return nullptr;
}

}  // namespace

int msf_local_mapping_version(void) { return MSF_LOCAL_MAPPING_VERSION; }

int msf_new_points(msf_handle* h, int32_t n_matches, const msf_match* matches, const msf_view* view1,
                   const msf_view* view2, const msf_new_points_params* params, msf_new_points_result* out) {
  return guarded(h, "msf_new_points", [&]() -> int {
    if (const char* fault = new_points_fault(params, out))
      return fail(h, MSF_ERR_INVALID_ARG, std::string("msf_new_points: ") + fault);
    if (n_matches < 0) return fail(h, MSF_ERR_INVALID_ARG, "msf_new_points: n_matches is negative");
    if (!view1 || !view2 || (n_matches > 0 && !matches))
      return fail(h, MSF_ERR_INVALID_ARG, "msf_new_points: a required pointer is NULL (matches, view1, view2)");
    CallScope cs{h};
    if (int rc = cs.enter()) return rc;
    const int cap = n_matches > 0 ? n_matches : 1;
    const size_t units[] = {1};
    msf_new_points_result dev{};
    NewPointsPlan p;
    if (int rc = carve(h, h->d_lm, (size_t)1 << 16, "hipMalloc(new points workspace)", [&](msf::Carver& c) {
          p.view1 = c.take<msf_view>(1);
          p.view2 = c.take<msf_view>(1);
          msf::carve_result(c, msf::kNewPointsArrays, units, (size_t)cap, nullptr, *out, &dev);
          p.matches = c.take<msf_match>(cap);
        }))
      return rc;
    hipStream_t st = cs.st;
    Drain drain{st};
    if (n_matches > 0)
      HIP_TRY(h, "hipMemcpyAsync", hipMemcpyAsync(p.matches, matches, (size_t)n_matches * sizeof(msf_match), hipMemcpyHostToDevice, st));
    HIP_TRY(h, "hipMemcpyAsync", hipMemcpyAsync(p.view1, view1, sizeof(msf_view), hipMemcpyHostToDevice, st));
    HIP_TRY(h, "hipMemcpyAsync", hipMemcpyAsync(p.view2, view2, sizeof(msf_view), hipMemcpyHostToDevice, st));
    const msf::NewPointLists in{p.matches, cap, cap, nullptr, n_matches, p.view1, p.view2};
    HIP_TRY(h, "new_points", msf::new_points(1, in, new_point_params(params), to_out(dev), st));
    const NewPointsWanted want(*out);
    msf::Extent e{0, (size_t)cap, (size_t)cap, (size_t)n_matches, units, units};
    if (int rc = fetch(h, st, out->n_new, dev.n_new, sizeof *out->n_new)) return rc;
    if (int rc = fetch_result(h, st, msf::kNewPointsArrays, dev, want.rows, e)) return rc;
    if (out->packed) {   // the first n_new records: the count has to arrive first
      HIP_TRY(h, "hipStreamSynchronize", hipStreamSynchronize(st));
      e.n = out->n_new[0] > 0 ? (size_t)out->n_new[0] : 0;
      if (int rc = fetch_result(h, st, msf::kNewPointsArrays, dev, want.records, e)) return rc;
    }
    drain.armed = false;
    return cs.finish();
  });
}

int msf_new_points_device(msf_handle* h, int32_t n_lists, const msf_match* d_matches, int32_t cap_per_pair,
                          const int32_t* d_n_out, const msf_view* d_view1, const msf_view* d_view2,
                          const msf_new_points_params* params, msf_new_points_result* out, void* stream) {
  return guarded(h, "msf_new_points_device", [&]() -> int {
    if (const char* fault = new_points_fault(params, out))
      return fail(h, MSF_ERR_INVALID_ARG, std::string("msf_new_points_device: ") + fault);
    if (n_lists < 0 || n_lists > 65535)
      return fail(h, MSF_ERR_INVALID_ARG, "msf_new_points_device: n_lists outside [0, 65535]");
    if (cap_per_pair < 1) return fail(h, MSF_ERR_INVALID_ARG, "msf_new_points_device: cap_per_pair < 1");
    if (n_lists > 0 && (!d_matches || !d_n_out || !d_view1 || !d_view2))
      return fail(h, MSF_ERR_INVALID_ARG, "msf_new_points_device: a required pointer is NULL (d_matches, d_n_out, d_view1, d_view2)");
    if (n_lists == 0) return MSF_OK;
    CallScope cs{h};
    if (int rc = cs.enter(stream)) return rc;
    const msf::NewPointLists in{d_matches, cap_per_pair, cap_per_pair, d_n_out, 0, d_view1, d_view2};
    HIP_TRY(h, "new_points", msf::new_points(n_lists, in, new_point_params(params), to_out(*out), cs.st));
    return cs.finish();
  });
}

int msf_create_map_points(msf_handle* h, int32_t query_slot, const msf_view* query_view, int32_t n,
                          const int32_t* slots, const msf_view* views, const msf_new_points_params* params,
                          int32_t* num_matches, msf_match* out_matches, int32_t cap_per_pair,
                          msf_new_points_result* out) {
  return guarded(h, "msf_create_map_points", [&]() -> int {
    const char* const name = "msf_create_map_points";
    if (const char* fault = new_points_fault(params, out))
      return fail(h, MSF_ERR_INVALID_ARG, std::string(name) + ": " + fault);
    if (n < 0 || (n > 0 && (!slots || !num_matches || !query_view || !views)) || cap_per_pair < 1)
      return fail(h, MSF_ERR_INVALID_ARG, std::string(name) + ": bad argument");
    if (n == 0) return MSF_OK;
    if (int rc = one_to_many_args(h, name, query_slot, n, slots)) return rc;
    CallScope cs{h};
    if (int rc = cs.enter()) return rc;
    hipStream_t st = cs.st;
    // sized for max_batch_pairs lists whatever n is: the pieces stay where they are from call to call
    const size_t units[] = {(size_t)h->cfg.max_batch_pairs}, one[] = {1};
    msf_new_points_result dev{};
    NewPointsPlan p;
    if (int rc = carve(h, h->d_lm, (size_t)1 << 16, "hipMalloc(new points workspace)", [&](msf::Carver& c) {
          p.view1 = c.take<msf_view>(units[0]);
          p.view2 = c.take<msf_view>(units[0]);
          msf::carve_result(c, msf::kNewPointsArrays, units, (size_t)h->stage_cap, nullptr, *out, &dev);
        }))
      return rc;
    Drain drain{st};
    h->view_stage.resize((size_t)2 * n);
    for (int i = 0; i < n; i++) { h->view_stage[i] = *query_view; h->view_stage[n + i] = views[i]; }
    HIP_TRY(h, "hipMemcpyAsync(views)", hipMemcpyAsync(p.view1, h->view_stage.data(), (size_t)n * sizeof(msf_view), hipMemcpyHostToDevice, st));
    HIP_TRY(h, "hipMemcpyAsync(views)", hipMemcpyAsync(p.view2, h->view_stage.data() + n, (size_t)n * sizeof(msf_view), hipMemcpyHostToDevice, st));
    if (int rc = launch_one_to_many(h, query_slot, n, slots, st)) return rc;
    const int limit = cap_per_pair < h->stage_cap ? cap_per_pair : h->stage_cap;
    const msf::NewPointLists in{h->d_out, h->stage_cap, limit, h->d_n, 0, p.view1, p.view2};
    HIP_TRY(h, "new_points", msf::new_points(n, in, new_point_params(params), to_out(dev), st));
    if (int rc = fetch(h, st, num_matches, h->d_n, (size_t)n * sizeof *num_matches)) return rc;
    if (int rc = fetch(h, st, out->n_new, dev.n_new, (size_t)n * sizeof *out->n_new)) return rc;
    HIP_TRY(h, "hipStreamSynchronize", hipStreamSynchronize(st));
    // the copy-back: the counts say how much of every list there is to fetch
    bool capacity = false;
    const NewPointsWanted want(*out);
    for (int i = 0; i < n; i++) {
      const int w = deliverable(h, num_matches[i], cap_per_pair, &capacity);
      if (int rc = fetch(h, st, from(out_matches, (size_t)i * cap_per_pair), h->d_out + (size_t)i * h->stage_cap,
                         (size_t)w * sizeof(msf_match)))
        return rc;
      msf::Extent e{(size_t)i, (size_t)h->stage_cap, (size_t)cap_per_pair, (size_t)w, one, one};
      if (int rc = fetch_result(h, st, msf::kNewPointsArrays, dev, want.rows, e)) return rc;
      e.n = out->n_new[i] > 0 ? (size_t)out->n_new[i] : 0;
      if (int rc = fetch_result(h, st, msf::kNewPointsArrays, dev, want.records, e)) return rc;
    }
    drain.armed = false;
    if (int rc = cs.finish()) return rc;
    return capacity ? fail(h, MSF_ERR_CAPACITY, kNoResult) : MSF_OK;
  });
}

namespace {

// What msf_pnp_ransac keeps in the workspace besides its result arrays (result_arrays.h: kPnpArrays): the list and
// the caller's sets.
struct PnpPlan {
  float* p3d = nullptr;
  float* p2d = nullptr;
  int32_t* sets_in = nullptr;
};

// nullptr when params and out are usable, else what is wrong with them
const char* pnp_fault(const msf_pnp_params* prm, const msf_pnp_result* out) {
  if (!out || out->struct_size != sizeof(msf_pnp_result)) return "out is NULL or out->struct_size is not sizeof(msf_pnp_result)";
  if (!prm || prm->struct_size != sizeof(msf_pnp_params)) return "params is NULL or params->struct_size is not sizeof(msf_pnp_params)";
  if (std::isnan(prm->th2)) return "th2 must not be NaN";
  if (prm->min_inliers < 1) return "min_inliers < 1";
  if (prm->n_iterations < 1 || prm->n_iterations >= (1 << 20)) return "n_iterations outside [1, 2^20)";
  if (prm->max_records < 1) return "max_records < 1";
  if (!out->n_records) return "a required pointer is NULL (out->n_records)";
  return nullptr;
}

msf::PnpParams pnp_params(const msf_pnp_params* prm) {
  return msf::PnpParams{prm->fx, prm->fy, prm->cx, prm->cy, prm->th2, prm->min_inliers, prm->n_iterations,
                        prm->max_records, prm->seed};
}

}  // namespace

int msf_pnp_version(void) { return MSF_PNP_VERSION; }

int msf_pnp_ransac(msf_handle* h, int32_t n, const float* p3d, const float* p2d, const msf_pnp_params* params,
                   const int32_t* sets, msf_pnp_result* out) {
  return guarded(h, "msf_pnp_ransac", [&]() -> int {
    if (const char* fault = pnp_fault(params, out)) return fail(h, MSF_ERR_INVALID_ARG, std::string("msf_pnp_ransac: ") + fault);
    if (n < 0) return fail(h, MSF_ERR_INVALID_ARG, "msf_pnp_ransac: n is negative");
    if (n > 0 && (!p3d || !p2d)) return fail(h, MSF_ERR_INVALID_ARG, "msf_pnp_ransac: a required pointer is NULL (p3d, p2d)");
    CallScope cs{h};
    if (int rc = cs.enter()) return rc;
    const size_t cap = n > 0 ? (size_t)n : 1, its = (size_t)params->n_iterations;
    const size_t units[] = {1, its, (size_t)params->max_records};
    msf_pnp_result want = *out, dev{};
    if (sets) want.sets = nullptr;   // the sets come back only when they were drawn here
    PnpPlan p;
    if (int rc = carve(h, h->d_pnp, (size_t)1 << 16, "hipMalloc(pnp workspace)", [&](msf::Carver& c) {
          p.p3d = c.take<float>(cap * 3);
          p.p2d = c.take<float>(cap * 2);
          p.sets_in = sets ? c.take<int32_t>(its * 4) : nullptr;
          msf::carve_result(c, msf::kPnpArrays, units, cap, nullptr, want, &dev);
        }))
      return rc;
    hipStream_t st = cs.st;
    Drain drain{st};
    if (n > 0) {
      HIP_TRY(h, "hipMemcpyAsync", hipMemcpyAsync(p.p3d, p3d, (size_t)n * 12, hipMemcpyHostToDevice, st));
      HIP_TRY(h, "hipMemcpyAsync", hipMemcpyAsync(p.p2d, p2d, (size_t)n * 8, hipMemcpyHostToDevice, st));
    }
    if (sets) HIP_TRY(h, "hipMemcpyAsync", hipMemcpyAsync(p.sets_in, sets, its * 16, hipMemcpyHostToDevice, st));
    const msf::PnpLists in{p.p3d, p.p2d, (int32_t)cap, nullptr, n, p.sets_in};
    HIP_TRY(h, "pnp_ransac", msf::pnp_ransac(1, in, pnp_params(params), to_out(dev), st));
    if (int rc = fetch(h, st, out->n_records, dev.n_records, sizeof *out->n_records)) return rc;
    HIP_TRY(h, "hipStreamSynchronize", hipStreamSynchronize(st));   // the count decides what else there is to copy
    const int32_t records = out->n_records[0];
    if (records >= 0) {
      want.n_records = nullptr;   // has arrived
      const size_t rows[] = {1, its, (size_t)(records < params->max_records ? records : params->max_records)};
      const msf::Extent e{0, cap, cap, (size_t)n, units, rows};   // an inlier row ends with the list
      if (int rc = fetch_result(h, st, msf::kPnpArrays, dev, want, e)) return rc;
    }
    drain.armed = false;
    if (int rc = cs.finish()) return rc;
    if (records > params->max_records)
      return fail(h, MSF_ERR_CAPACITY, "msf_pnp_ransac: the list has more records than max_records; the first max_records are complete");
    return MSF_OK;
  });
}

int msf_pnp_ransac_device(msf_handle* h, int32_t n_lists, const float* d_p3d, const float* d_p2d, int32_t cap,
                          const int32_t* d_n, const msf_pnp_params* params, const int32_t* d_sets, msf_pnp_result* out,
                          void* stream) {
  return guarded(h, "msf_pnp_ransac_device", [&]() -> int {
    if (const char* fault = pnp_fault(params, out))
      return fail(h, MSF_ERR_INVALID_ARG, std::string("msf_pnp_ransac_device: ") + fault);
    if (n_lists < 0 || n_lists > 65535) return fail(h, MSF_ERR_INVALID_ARG, "msf_pnp_ransac_device: n_lists outside [0, 65535]");
    if (cap < 1) return fail(h, MSF_ERR_INVALID_ARG, "msf_pnp_ransac_device: cap < 1");
    if ((long long)n_lists * params->n_iterations > (1ll << 32))   // four hypotheses per workgroup, 2^31 - 1 workgroups
      return fail(h, MSF_ERR_INVALID_ARG, "msf_pnp_ransac_device: n_lists * n_iterations above 2^32");
    if (n_lists > 0 && (!d_p3d || !d_p2d || !d_n))
      return fail(h, MSF_ERR_INVALID_ARG, "msf_pnp_ransac_device: a required pointer is NULL (d_p3d, d_p2d, d_n)");
    if (n_lists == 0) return MSF_OK;
    CallScope cs{h};
    if (int rc = cs.enter(stream)) return rc;
    // the counts and poses that the second launch reads get a piece when the caller does not ask for them
    const size_t units[] = {(size_t)n_lists, (size_t)params->n_iterations, (size_t)params->max_records};
    msf_pnp_result dev{};
    if (int rc = carve(h, h->d_pnp, (size_t)1 << 16, "hipMalloc(pnp workspace)", [&](msf::Carver& c) {
          msf::carve_result(c, msf::kPnpArrays, units, (size_t)cap, out, *out, &dev);
        }))
      return rc;
    const msf::PnpLists in{d_p3d, d_p2d, cap, d_n, 0, d_sets};
    HIP_TRY(h, "pnp_ransac", msf::pnp_ransac(n_lists, in, pnp_params(params), to_out(dev), cs.st));
    return cs.finish();
  });
}

namespace {

// What msf_pose_optimize keeps in the workspace besides its result arrays (result_arrays.h: kPoseArrays): the list,
// its entry pose and mask; base / bytes: the whole of it, for the memset.
struct PosePlan {
  float* p3d = nullptr;
  float* p2d = nullptr;
  float* tcw0 = nullptr;
  uint8_t* mask = nullptr;
  size_t bytes = 0;
  uint8_t* base = nullptr;
};

// nullptr when params and out are usable, else what is wrong with them
const char* pose_fault(const msf_pose_params* prm, const msf_pose_result* out) {
  if (!out || out->struct_size != sizeof(msf_pose_result)) return "out is NULL or out->struct_size is not sizeof(msf_pose_result)";
  if (!prm || prm->struct_size != sizeof(msf_pose_params)) return "params is NULL or params->struct_size is not sizeof(msf_pose_params)";
  if (std::isnan(prm->chi2)) return "chi2 must not be NaN";
  if (!out->n_good) return "a required pointer is NULL (out->n_good)";
  return nullptr;
}

}  // namespace

int msf_pose_version(void) { return MSF_POSE_VERSION; }

int msf_pose_optimize(msf_handle* h, int32_t n, const float* p3d, const float* p2d, const float* Tcw0,
                      const uint8_t* mask, const msf_pose_params* params, msf_pose_result* out) {
  return guarded(h, "msf_pose_optimize", [&]() -> int {
    if (const char* fault = pose_fault(params, out)) return fail(h, MSF_ERR_INVALID_ARG, std::string("msf_pose_optimize: ") + fault);
    if (n < 0) return fail(h, MSF_ERR_INVALID_ARG, "msf_pose_optimize: n is negative");
    if (!Tcw0 || (n > 0 && (!p3d || !p2d))) return fail(h, MSF_ERR_INVALID_ARG, "msf_pose_optimize: a required pointer is NULL (p3d, p2d, Tcw0)");
    CallScope cs{h};
    if (int rc = cs.enter()) return rc;
    const size_t cap = n > 0 ? (size_t)n : 1, count = (size_t)n;
    const size_t units[] = {1, msf::kPoseRounds, msf::kPoseIterations};
    msf_pose_result dev{};
    PosePlan p;
    if (int rc = carve(h, h->d_pose, (size_t)1 << 16, "hipMalloc(pose workspace)", [&](msf::Carver& c) {
          p.base = c.base;
          p.p3d = c.take<float>(cap * 3);
          p.p2d = c.take<float>(cap * 2);
          p.tcw0 = c.take<float>(12);
          p.mask = mask ? c.take<uint8_t>(cap) : nullptr;
          msf::carve_result(c, msf::kPoseArrays, units, cap, nullptr, *out, &dev);
          p.bytes = c.off;
        }))
      return rc;
    hipStream_t st = cs.st;
    Drain drain{st};
    // what the kernel leaves alone comes back as 0, and an outlier byte outside the mask as the caller had it
    HIP_TRY(h, "hipMemsetAsync", hipMemsetAsync(p.base, 0, p.bytes, st));
    if (n > 0) {
      HIP_TRY(h, "hipMemcpyAsync", hipMemcpyAsync(p.p3d, p3d, count * 12, hipMemcpyHostToDevice, st));
      HIP_TRY(h, "hipMemcpyAsync", hipMemcpyAsync(p.p2d, p2d, count * 8, hipMemcpyHostToDevice, st));
      if (mask) HIP_TRY(h, "hipMemcpyAsync", hipMemcpyAsync(p.mask, mask, count, hipMemcpyHostToDevice, st));
      if (mask && out->outliers)
        HIP_TRY(h, "hipMemcpyAsync", hipMemcpyAsync(dev.outliers, out->outliers, count, hipMemcpyHostToDevice, st));
    }
    HIP_TRY(h, "hipMemcpyAsync", hipMemcpyAsync(p.tcw0, Tcw0, 48, hipMemcpyHostToDevice, st));
    const msf::PoseLists in{p.p3d, p.p2d, (int32_t)cap, nullptr, n, p.tcw0, 0, p.mask, 0};
    const msf::PoseParams prm{params->fx, params->fy, params->cx, params->cy, params->chi2};
    HIP_TRY(h, "pose_optimize", msf::pose_optimize(1, in, prm, to_out(dev), st));
    const msf::Extent all{0, cap, cap, count, units, units};
    if (int rc = fetch_result(h, st, msf::kPoseArrays, dev, *out, all)) return rc;
    drain.armed = false;
    return cs.finish();
  });
}

int msf_pose_optimize_device(msf_handle* h, int32_t n_lists, const float* d_p3d, const float* d_p2d, int32_t cap,
                             const int32_t* d_n, const float* d_Tcw0, int64_t Tcw0_stride, const uint8_t* d_mask,
                             int64_t mask_stride, const msf_pose_params* params, msf_pose_result* out, void* stream) {
  return guarded(h, "msf_pose_optimize_device", [&]() -> int {
    if (const char* fault = pose_fault(params, out))
      return fail(h, MSF_ERR_INVALID_ARG, std::string("msf_pose_optimize_device: ") + fault);
    if (n_lists < 0) return fail(h, MSF_ERR_INVALID_ARG, "msf_pose_optimize_device: n_lists is negative");
    if (cap < 1) return fail(h, MSF_ERR_INVALID_ARG, "msf_pose_optimize_device: cap < 1");
    if (Tcw0_stride < 0 || mask_stride < 0) return fail(h, MSF_ERR_INVALID_ARG, "msf_pose_optimize_device: a negative stride");
    if (n_lists > 0 && (!d_p3d || !d_p2d || !d_n || !d_Tcw0))
      return fail(h, MSF_ERR_INVALID_ARG, "msf_pose_optimize_device: a required pointer is NULL (d_p3d, d_p2d, d_n, d_Tcw0)");
    if (n_lists == 0) return MSF_OK;
    CallScope cs{h};
    if (int rc = cs.enter(stream)) return rc;
    const msf::PoseLists in{d_p3d, d_p2d, cap, d_n, 0, d_Tcw0, Tcw0_stride, d_mask, mask_stride};
    const msf::PoseParams prm{params->fx, params->fy, params->cx, params->cy, params->chi2};
    HIP_TRY(h, "pose_optimize", msf::pose_optimize(n_lists, in, prm, to_out(*out), cs.st));
    return cs.finish();
  });
}

namespace {

// What msf_bundle_adjust keeps in the workspace besides its result arrays (ba_arrays.h: kBaArrays) and the scratch:
// the problem, its descriptor and the stop word; base / bytes: what the memset covers (everything but the scratch).
struct BaPlan {
  msf_ba_problem* problem = nullptr;
  float* cam_tcw = nullptr;
  uint8_t* cam_fixed = nullptr;
  float* points = nullptr;
  int32_t* edge_cam = nullptr;
  int32_t* edge_point = nullptr;
  float* edge_obs = nullptr;
  int32_t* stop = nullptr;
  msf::ba::Scratch scratch{};
  size_t bytes = 0;
  uint8_t* base = nullptr;
};

msf::BaOut to_out(const msf_ba_result& r) {
  return msf::BaOut{r.status, r.cam_Tcw, r.points, r.outliers, r.cam_pose_f64, r.points_f64, r.round_flags,
                    r.round_iterations, r.it_trials, r.it_lambda_in, r.it_lambda_out, r.it_cost_in, r.it_cost_out,
                    r.it_cam_in, r.it_point_in, r.it_cam_out, r.it_point_out, r.it_Hcc, r.it_bc, r.it_Hpp, r.it_bp};
}

// nullptr when params and out are usable, else what is wrong with them
const char* ba_fault(const msf_ba_params* prm, const msf_ba_result* out) {
  if (!out || out->struct_size != sizeof(msf_ba_result)) return "out is NULL or out->struct_size is not sizeof(msf_ba_result)";
  if (!prm || prm->struct_size != sizeof(msf_ba_params)) return "params is NULL or params->struct_size is not sizeof(msf_ba_params)";
  if (std::isnan(prm->fx) || std::isnan(prm->fy) || std::isnan(prm->cx) || std::isnan(prm->cy)) return "an intrinsic is NaN";
  if (prm->n_rounds < 1 || prm->n_rounds > 2) return "n_rounds must be 1 or 2";
  for (int r = 0; r < 2; r++) {
    if (prm->iterations[r] < 0 || prm->iterations[r] > MSF_BA_MAX_ITERATIONS) return "iterations must be 0..32";
    if (prm->robust[r] != 0 && prm->robust[r] != 1) return "robust must be 0 or 1";
  }
  if (!(prm->huber_delta2 > 0) || !std::isfinite(prm->huber_delta2)) return "huber_delta2 must be positive and finite";
  if (std::isnan(prm->chi2)) return "chi2 must not be NaN";
  if (!out->status) return "a required pointer is NULL (out->status)";
  return nullptr;
}

msf::ba::Params ba_params(const msf_ba_params* p) {
  return msf::ba::Params{msf::ba::Cam{(double)p->fx, (double)p->fy, (double)p->cx, (double)p->cy},
                         p->n_rounds,
                         {p->iterations[0], p->iterations[1]},
                         {p->robust[0], p->robust[1]},
                         p->huber_delta2,
                         p->chi2};
}

}  // namespace

int msf_ba_version(void) { return MSF_BA_VERSION; }

int msf_bundle_adjust(msf_handle* h, int32_t n_cams, const float* cam_Tcw, const uint8_t* cam_fixed, int32_t n_points,
                      const float* points, int32_t n_edges, const int32_t* edge_cam, const int32_t* edge_point,
                      const float* edge_obs, const int32_t* stop, const msf_ba_params* params, msf_ba_result* out) {
  return guarded(h, "msf_bundle_adjust", [&]() -> int {
    if (const char* fault = ba_fault(params, out)) return fail(h, MSF_ERR_INVALID_ARG, std::string("msf_bundle_adjust: ") + fault);
    if (n_cams < 0 || n_points < 0 || n_edges < 0) return fail(h, MSF_ERR_INVALID_ARG, "msf_bundle_adjust: a count is negative");
    if ((n_cams > 0 && (!cam_Tcw || !cam_fixed)) || (n_points > 0 && !points) || (n_edges > 0 && (!edge_cam || !edge_point || !edge_obs)))
      return fail(h, MSF_ERR_INVALID_ARG, "msf_bundle_adjust: a required pointer is NULL (cam_Tcw, cam_fixed, points, edge_cam, edge_point, edge_obs)");
    for (int32_t e = 0; e < n_edges; e++) {
      if (edge_cam[e] < 0 || edge_cam[e] >= n_cams || edge_point[e] < 0 || edge_point[e] >= n_points)
        return fail(h, MSF_ERR_INVALID_ARG, "msf_bundle_adjust: an edge index is out of range");
      if (e > 0 && edge_point[e - 1] > edge_point[e])
        return fail(h, MSF_ERR_INVALID_ARG, "msf_bundle_adjust: the edges are not sorted by point");
    }
    int n_free = 0;
    for (int32_t c = 0; c < n_cams; c++) n_free += cam_fixed[c] == 0;
    if (n_free > MSF_BA_MAX_FREE_CAMS)
      return fail(h, MSF_ERR_CAPACITY, "msf_bundle_adjust: more than MSF_BA_MAX_FREE_CAMS free cameras");
    CallScope cs{h};
    if (int rc = cs.enter()) return rc;
    const size_t nc = (size_t)n_cams, np = (size_t)n_points, ne = (size_t)n_edges;
    size_t units[msf::kBaUnits];
    msf::ba_units(nc, np, ne, units);
    msf_ba_result dev{};
    BaPlan p;
    if (int rc = carve(h, h->d_ba, (size_t)1 << 20, "hipMalloc(bundle adjustment workspace)", [&](msf::Carver& c) {
          p.base = c.base;
          p.problem = c.take<msf_ba_problem>(1);
          p.cam_tcw = c.take<float>(nc * 12);
          p.cam_fixed = c.take<uint8_t>(nc);
          p.points = c.take<float>(np * 3);
          p.edge_cam = c.take<int32_t>(ne);
          p.edge_point = c.take<int32_t>(ne);
          p.edge_obs = c.take<float>(ne * 2);
          p.stop = c.take<int32_t>(1);
          msf::carve_result(c, msf::kBaArrays, units, 1, nullptr, *out, &dev);
          p.bytes = c.off;
          p.scratch = msf::ba::layout(c, 1, nc, np, ne, n_free > 0 ? n_free : 1);
        }))
      return rc;
    hipStream_t st = cs.st;
    Drain drain{st};
    // what the kernel leaves alone comes back as 0
    HIP_TRY(h, "hipMemsetAsync", hipMemsetAsync(p.base, 0, p.bytes, st));
    const msf_ba_problem desc{n_cams, n_points, n_edges, 0, 0, 0};
    const int32_t stop_now = stop ? *stop : 0;
    HIP_TRY(h, "hipMemcpyAsync", hipMemcpyAsync(p.problem, &desc, sizeof desc, hipMemcpyHostToDevice, st));
    HIP_TRY(h, "hipMemcpyAsync", hipMemcpyAsync(p.stop, &stop_now, sizeof stop_now, hipMemcpyHostToDevice, st));
    if (nc) {
      HIP_TRY(h, "hipMemcpyAsync", hipMemcpyAsync(p.cam_tcw, cam_Tcw, nc * 48, hipMemcpyHostToDevice, st));
      HIP_TRY(h, "hipMemcpyAsync", hipMemcpyAsync(p.cam_fixed, cam_fixed, nc, hipMemcpyHostToDevice, st));
    }
    if (np) HIP_TRY(h, "hipMemcpyAsync", hipMemcpyAsync(p.points, points, np * 12, hipMemcpyHostToDevice, st));
    if (ne) {
      HIP_TRY(h, "hipMemcpyAsync", hipMemcpyAsync(p.edge_cam, edge_cam, ne * 4, hipMemcpyHostToDevice, st));
      HIP_TRY(h, "hipMemcpyAsync", hipMemcpyAsync(p.edge_point, edge_point, ne * 4, hipMemcpyHostToDevice, st));
      HIP_TRY(h, "hipMemcpyAsync", hipMemcpyAsync(p.edge_obs, edge_obs, ne * 8, hipMemcpyHostToDevice, st));
    }
    // `desc` and `stop_now` live in this frame: the stream is drained before the call leaves it
    const msf::BaBatch in{p.problem, p.cam_tcw, p.cam_fixed, p.points, p.edge_cam, p.edge_point, p.edge_obs,
                          n_cams,    n_points,  n_edges,     p.scratch.max_free, p.stop};
    HIP_TRY(h, "bundle_adjust", msf::bundle_adjust(1, in, ba_params(params), p.scratch, to_out(dev), st));
    const msf::Extent all{0, 1, 1, 1, units, units};
    if (int rc = fetch_result(h, st, msf::kBaArrays, dev, *out, all)) return rc;
    drain.armed = false;
    return cs.finish();
  });
}

int msf_bundle_adjust_device(msf_handle* h, int32_t n_problems, const msf_ba_problem* d_problems, const float* d_cam_Tcw,
                             const uint8_t* d_cam_fixed, const float* d_points, const int32_t* d_edge_cam,
                             const int32_t* d_edge_point, const float* d_edge_obs, int64_t total_cams,
                             int64_t total_points, int64_t total_edges, int32_t max_free_cams, const int32_t* d_stop,
                             const msf_ba_params* params, msf_ba_result* out, void* stream) {
  return guarded(h, "msf_bundle_adjust_device", [&]() -> int {
    if (const char* fault = ba_fault(params, out))
      return fail(h, MSF_ERR_INVALID_ARG, std::string("msf_bundle_adjust_device: ") + fault);
    if (n_problems < 0 || total_cams < 0 || total_points < 0 || total_edges < 0)
      return fail(h, MSF_ERR_INVALID_ARG, "msf_bundle_adjust_device: a count is negative");
    if (total_cams > INT32_MAX || total_points > INT32_MAX || total_edges > INT32_MAX)
      return fail(h, MSF_ERR_INVALID_ARG, "msf_bundle_adjust_device: a total above 2^31 - 1");
    if (max_free_cams < 1 || max_free_cams > MSF_BA_MAX_FREE_CAMS)
      return fail(h, MSF_ERR_INVALID_ARG, "msf_bundle_adjust_device: max_free_cams must be 1..MSF_BA_MAX_FREE_CAMS");
    if (n_problems > 0 && (!d_problems || (total_cams > 0 && (!d_cam_Tcw || !d_cam_fixed)) || (total_points > 0 && !d_points) ||
                           (total_edges > 0 && (!d_edge_cam || !d_edge_point || !d_edge_obs))))
      return fail(h, MSF_ERR_INVALID_ARG, "msf_bundle_adjust_device: a required pointer is NULL");
    if (n_problems == 0) return MSF_OK;
    CallScope cs{h};
    if (int rc = cs.enter(stream)) return rc;
    msf::ba::Scratch scratch{};
    if (int rc = carve(h, h->d_ba, (size_t)1 << 20, "hipMalloc(bundle adjustment workspace)", [&](msf::Carver& c) {
          scratch = msf::ba::layout(c, (size_t)n_problems, (size_t)total_cams, (size_t)total_points, (size_t)total_edges,
                                    max_free_cams);
        }))
      return rc;
    const msf::BaBatch in{d_problems,  d_cam_Tcw,   d_cam_fixed,   d_points, d_edge_cam, d_edge_point, d_edge_obs, total_cams,
                          total_points, total_edges, max_free_cams, d_stop};
    HIP_TRY(h, "bundle_adjust", msf::bundle_adjust(n_problems, in, ba_params(params), scratch, to_out(*out), cs.st));
    return cs.finish();
  });
}

namespace {

// What msf_global_bundle_adjust keeps in the workspace besides its result arrays and gba::layout: the problem.
struct GbaPlan {
  float* cam_tcw = nullptr;
  uint8_t* cam_fixed = nullptr;
  float* points = nullptr;
  int32_t* edge_cam = nullptr;
  int32_t* edge_point = nullptr;
  float* edge_obs = nullptr;
  msf::gba::Scratch scratch{};
  size_t bytes = 0;
  uint8_t* base = nullptr;
};

int gba_pinned(msf_handle* h) {
  if (!h->h_gba_rec)
    HIP_TRY(h, "hipHostMalloc(global bundle adjustment record)",
            hipHostMalloc((void**)&h->h_gba_rec, sizeof(msf::gba::Record), hipHostMallocDefault));
  return MSF_OK;
}

}  // namespace

int msf_global_ba_version(void) { return MSF_GLOBAL_BA_VERSION; }

int msf_global_ba_tile_rows(void) { return msf::gba::kTile; }

int msf_global_bundle_adjust(msf_handle* h, int32_t n_cams, const float* cam_Tcw, const uint8_t* cam_fixed,
                             int32_t n_points, const float* points, int32_t n_edges, const int32_t* edge_cam,
                             const int32_t* edge_point, const float* edge_obs, const volatile int32_t* stop,
                             const msf_ba_params* params, msf_ba_result* out) {
  return guarded(h, "msf_global_bundle_adjust", [&]() -> int {
    if (const char* fault = ba_fault(params, out))
      return fail(h, MSF_ERR_INVALID_ARG, std::string("msf_global_bundle_adjust: ") + fault);
    if (n_cams < 0 || n_points < 0 || n_edges < 0)
      return fail(h, MSF_ERR_INVALID_ARG, "msf_global_bundle_adjust: a count is negative");
    if ((n_cams > 0 && (!cam_Tcw || !cam_fixed)) || (n_points > 0 && !points) || (n_edges > 0 && (!edge_cam || !edge_point || !edge_obs)))
      return fail(h, MSF_ERR_INVALID_ARG, "msf_global_bundle_adjust: a required pointer is NULL (cam_Tcw, cam_fixed, points, edge_cam, edge_point, edge_obs)");
    for (int32_t e = 0; e < n_edges; e++) {
      if (edge_cam[e] < 0 || edge_cam[e] >= n_cams || edge_point[e] < 0 || edge_point[e] >= n_points)
        return fail(h, MSF_ERR_INVALID_ARG, "msf_global_bundle_adjust: an edge index is out of range");
      if (e > 0 && edge_point[e - 1] > edge_point[e])
        return fail(h, MSF_ERR_INVALID_ARG, "msf_global_bundle_adjust: the edges are not sorted by point");
    }
    int n_free = 0;
    for (int32_t c = 0; c < n_cams; c++) n_free += cam_fixed[c] == 0;
    if (n_free > MSF_GBA_MAX_FREE_CAMS)
      return fail(h, MSF_ERR_CAPACITY, "msf_global_bundle_adjust: more than MSF_GBA_MAX_FREE_CAMS free cameras");
    CallScope cs{h};
    if (int rc = cs.enter()) return rc;
    if (int rc = gba_pinned(h)) return rc;
    const size_t nc = (size_t)n_cams, np = (size_t)n_points, ne = (size_t)n_edges;
    size_t units[msf::kBaUnits];
    msf::ba_units(nc, np, ne, units);
    msf_ba_result dev{};
    GbaPlan p;
    if (int rc = carve(h, h->d_gba, (size_t)1 << 20, "hipMalloc(global bundle adjustment workspace)", [&](msf::Carver& c) {
          p.base = c.base;
          p.cam_tcw = c.take<float>(nc * 12);
          p.cam_fixed = c.take<uint8_t>(nc);
          p.points = c.take<float>(np * 3);
          p.edge_cam = c.take<int32_t>(ne);
          p.edge_point = c.take<int32_t>(ne);
          p.edge_obs = c.take<float>(ne * 2);
          msf::carve_result(c, msf::kBaArrays, units, 1, nullptr, *out, &dev);
          p.bytes = c.off;
          p.scratch = msf::gba::layout(c, nc, np, ne, n_free);
        }))
      return rc;
    hipStream_t st = cs.st;
    Drain drain{st};
    // what the kernels leave alone comes back as 0
    HIP_TRY(h, "hipMemsetAsync", hipMemsetAsync(p.base, 0, p.bytes, st));
    if (nc) {
      HIP_TRY(h, "hipMemcpyAsync", hipMemcpyAsync(p.cam_tcw, cam_Tcw, nc * 48, hipMemcpyHostToDevice, st));
      HIP_TRY(h, "hipMemcpyAsync", hipMemcpyAsync(p.cam_fixed, cam_fixed, nc, hipMemcpyHostToDevice, st));
    }
    if (np) HIP_TRY(h, "hipMemcpyAsync", hipMemcpyAsync(p.points, points, np * 12, hipMemcpyHostToDevice, st));
    if (ne) {
      HIP_TRY(h, "hipMemcpyAsync", hipMemcpyAsync(p.edge_cam, edge_cam, ne * 4, hipMemcpyHostToDevice, st));
      HIP_TRY(h, "hipMemcpyAsync", hipMemcpyAsync(p.edge_point, edge_point, ne * 4, hipMemcpyHostToDevice, st));
      HIP_TRY(h, "hipMemcpyAsync", hipMemcpyAsync(p.edge_obs, edge_obs, ne * 8, hipMemcpyHostToDevice, st));
    }
    const msf::GbaCall call{msf::ba::Problem{n_cams, n_points, n_edges, p.cam_tcw, p.cam_fixed, p.points, p.edge_cam,
                                             p.edge_point, p.edge_obs},
                            ba_params(params), p.scratch, to_out(dev), nullptr};
    // the same checking launch as the device entry: the device's verdict is the one that counts
    HIP_TRY(h, "global_bundle_adjust(check)", msf::gba_check(call, h->h_gba_rec, st));
    if (h->h_gba_rec->malformed || h->h_gba_rec->n_free != n_free)
      return fail(h, MSF_ERR_INVALID_ARG, "msf_global_bundle_adjust: the problem changed while the call read it");
    int status = 0;
    HIP_TRY(h, "global_bundle_adjust", msf::gba_solve(call, n_free, 0, h->h_gba_rec, stop, st, &status));
    const msf::Extent all{0, 1, 1, 1, units, units};
    if (int rc = fetch_result(h, st, msf::kBaArrays, dev, *out, all)) return rc;
    drain.armed = false;
    return cs.finish();
  });
}

int msf_global_bundle_adjust_device(msf_handle* h, int32_t n_cams, const float* d_cam_Tcw, const uint8_t* d_cam_fixed,
                                    int32_t n_points, const float* d_points, int32_t n_edges, const int32_t* d_edge_cam,
                                    const int32_t* d_edge_point, const float* d_edge_obs, int32_t max_free_cams,
                                    const int32_t* d_stop, const msf_ba_params* params, msf_ba_result* out,
                                    void* stream) {
  return guarded(h, "msf_global_bundle_adjust_device", [&]() -> int {
    if (const char* fault = ba_fault(params, out))
      return fail(h, MSF_ERR_INVALID_ARG, std::string("msf_global_bundle_adjust_device: ") + fault);
    if (n_cams < 0 || n_points < 0 || n_edges < 0)
      return fail(h, MSF_ERR_INVALID_ARG, "msf_global_bundle_adjust_device: a count is negative");
    if (max_free_cams < 1 || max_free_cams > MSF_GBA_MAX_FREE_CAMS)
      return fail(h, MSF_ERR_INVALID_ARG, "msf_global_bundle_adjust_device: max_free_cams must be 1..MSF_GBA_MAX_FREE_CAMS");
    if ((n_cams > 0 && (!d_cam_Tcw || !d_cam_fixed)) || (n_points > 0 && !d_points) ||
        (n_edges > 0 && (!d_edge_cam || !d_edge_point || !d_edge_obs)))
      return fail(h, MSF_ERR_INVALID_ARG, "msf_global_bundle_adjust_device: a required pointer is NULL");
    CallScope cs{h};
    if (int rc = cs.enter(stream)) return rc;
    if (int rc = gba_pinned(h)) return rc;
    const size_t nc = (size_t)n_cams, np = (size_t)n_points, ne = (size_t)n_edges;
    msf::GbaCall call{msf::ba::Problem{n_cams, n_points, n_edges, d_cam_Tcw, d_cam_fixed, d_points, d_edge_cam,
                                       d_edge_point, d_edge_obs},
                      ba_params(params), msf::gba::Scratch{}, to_out(*out), d_stop};
    // the record alone until the checking launch has passed the indices and counted the free cameras
    if (int rc = carve(h, h->d_gba, (size_t)1 << 20, "hipMalloc(global bundle adjustment workspace)",
                       [&](msf::Carver& c) { call.s = msf::gba::layout(c, nc, np, ne, 0); }))
      return rc;
    HIP_TRY(h, "global_bundle_adjust(check)", msf::gba_check(call, h->h_gba_rec, cs.st));
    const int n_free = h->h_gba_rec->n_free;
    if (h->h_gba_rec->malformed || n_free > max_free_cams) {
      HIP_TRY(h, "global_bundle_adjust(refuse)", msf::gba_refuse(call, cs.st));
      if (h->h_gba_rec->malformed) return MSF_OK;   // as a malformed problem of msf_bundle_adjust_device: the status says it
      return fail(h, MSF_ERR_CAPACITY, "msf_global_bundle_adjust_device: more than max_free_cams free cameras");
    }
    const int32_t stop_at_entry = h->h_gba_rec->stop;
    if (int rc = carve(h, h->d_gba, (size_t)1 << 20, "hipMalloc(global bundle adjustment workspace)",
                       [&](msf::Carver& c) { call.s = msf::gba::layout(c, nc, np, ne, n_free); }))
      return rc;
    int status = 0;
    HIP_TRY(h, "global_bundle_adjust", msf::gba_solve(call, n_free, stop_at_entry, h->h_gba_rec, nullptr, cs.st, &status));
    return MSF_OK;   // gba_solve has waited for the stream, whichever it is
  });
}

int msf_render_match_image(msf_handle* h, const msf_image* f1, const msf_image* f2, const msf_match* matches,
                           int32_t n_matches, const uint8_t* has_mp1, const uint8_t* has_mp2, uint8_t* out_rgb,
                           int64_t out_stride) {
  return guarded(h, "msf_render_match_image", [&]() -> int {
    const int W = h->cfg.image_width, H = h->cfg.image_height;
    if (!image_ok(h, f1) || !image_ok(h, f2) || n_matches < 0 || (n_matches > 0 && !matches) || !out_rgb || out_stride < 6ll * W)
      return fail(h, MSF_ERR_INVALID_ARG, "msf_render_match_image: bad argument or image size differs from the handle's");
    CallScope cs{h};
    if (int rc = cs.enter()) return rc;
    if (int rc = ensure_stage(h)) return rc;
    hipStream_t st = cs.st;
    // workspace: the two frames use the staging buffers; the RGB image is allocated by the first call, the list + flags
    // buffer grows when a call brings more matches than any before it (no allocation in the steady state)
    uint8_t* dA = h->d_stage;
    uint8_t* dB = h->d_stage + (size_t)h->cfg.max_batch_pairs * h->stage_frame;
    if (!h->d_render) HIP_TRY(h, "hipMalloc(render image)", h->d_render.reserve((size_t)6 * W * H));
    if ((size_t)n_matches * kRenderRecord > h->d_render_m.bytes) {
      HIP_TRY(h, "hipStreamSynchronize", hipStreamSynchronize(st));
      HIP_TRY(h, "hipMalloc(render list)", h->d_render_m.reserve((size_t)n_matches * kRenderRecord, 4096 * kRenderRecord));
    }
    msf_match* d_m = n_matches ? h->d_render_m.p : nullptr;
    uint8_t* d_flags = n_matches ? reinterpret_cast<uint8_t*>(h->d_render_m + h->d_render_m.bytes / kRenderRecord) : nullptr;
    Drain drain{st};
    if (n_matches) {
      HIP_TRY(h, "hipMemcpyAsync", hipMemcpyAsync(d_m, matches, (size_t)n_matches * sizeof(msf_match), hipMemcpyHostToDevice, st));
      HIP_TRY(h, "hipMemsetAsync", hipMemsetAsync(d_flags, 0, (size_t)2 * n_matches, st));
      if (has_mp1) HIP_TRY(h, "hipMemcpyAsync", hipMemcpyAsync(d_flags, has_mp1, n_matches, hipMemcpyHostToDevice, st));
      if (has_mp2) HIP_TRY(h, "hipMemcpyAsync", hipMemcpyAsync(d_flags + n_matches, has_mp2, n_matches, hipMemcpyHostToDevice, st));
    }
    if (int rc = upload_frame(h, dA, f1, st)) return rc;
    if (int rc = upload_frame(h, dB, f2, st)) return rc;
    HIP_TRY(h, "render_match_image",
            msf::render_match_image(dA, dB, W, H, h->stage_pitch, d_m, d_flags, d_flags ? d_flags + n_matches : nullptr,
                                    n_matches, h->d_render, 6ll * W, st));
    HIP_TRY(h, "hipMemcpy2DAsync",
            hipMemcpy2DAsync(out_rgb, out_stride, h->d_render, (size_t)6 * W, (size_t)6 * W, H, hipMemcpyDeviceToHost, st));
    drain.armed = false;
    return cs.finish();   // the one wait of the call
  });
}

int msf_debug_get(msf_handle* h, int32_t what, int32_t slot, int32_t level, void* host_out, size_t cap_bytes,
                  size_t* n_bytes) {
  if (!n_bytes || (!host_out && cap_bytes)) return MSF_ERR_INVALID_ARG;   // refused before the lock, without a text
  return guarded(h, "msf_debug_get", [&]() -> int {
    CallScope cs{h};
    if (int rc = cs.enter()) return rc;
    std::string err;
    const int rc = h->cfg.kind == MSF_KIND_ORB ? h->orb.debug_get(what, slot, level, host_out, cap_bytes, n_bytes, &err)
                                               : h->loftr.debug_get(what, slot, level, host_out, cap_bytes, n_bytes, &err);
    return rc != 0 ? fail(h, rc, err) : MSF_OK;
  });
}

int msf_debug_loftr_head(msf_handle* h, int32_t n_pairs, const float* d_feat0, const float* d_feat1,
                         msf_match* d_out, int32_t cap_per_pair, int32_t* d_n_out, void* stream) {
  return guarded(h, "msf_debug_loftr_head", [&]() -> int {
    if (h->cfg.kind != MSF_KIND_LOFTR) return fail(h, MSF_ERR_INVALID_ARG, "msf_debug_loftr_head: not a LoFTR handle");
    if (n_pairs < 0 || n_pairs > h->cfg.max_batch_pairs || !d_feat0 || !d_feat1 || !d_out || !d_n_out || cap_per_pair < 1)
      return fail(h, MSF_ERR_INVALID_ARG, "msf_debug_loftr_head: bad argument");
    if (!aligned16(d_feat0, d_feat1, d_out) || ((uintptr_t)d_n_out & 3))
      return fail(h, MSF_ERR_INVALID_ARG, "msf_debug_loftr_head: misaligned pointer");
    CallScope cs{h};
    if (int rc = cs.enter(stream)) return rc;
    HIP_TRY(h, "loftr head", h->loftr.head_only(n_pairs, d_feat0, d_feat1, h->cfg.threshold, d_out, cap_per_pair, d_n_out, cs.st));
    return cs.finish();
  });
}

int msf_debug_loftr_transformer(msf_handle* h, int32_t n_pairs, int32_t first_block, int32_t n_blocks,
                                const float* d_in0, const float* d_in1, float* d_out0, float* d_out1, void* stream) {
  return guarded(h, "msf_debug_loftr_transformer", [&]() -> int {
    if (h->cfg.kind != MSF_KIND_LOFTR) return fail(h, MSF_ERR_INVALID_ARG, "msf_debug_loftr_transformer: not a LoFTR handle");
    if (n_pairs < 0 || n_pairs > h->cfg.max_batch_pairs || first_block < 0 || n_blocks < 1 || first_block + n_blocks > 8 ||
        !d_in0 || !d_in1 || !d_out0 || !d_out1)
      return fail(h, MSF_ERR_INVALID_ARG, "msf_debug_loftr_transformer: bad argument");
    if (!aligned16(d_in0, d_in1, d_out0, d_out1))
      return fail(h, MSF_ERR_INVALID_ARG, "msf_debug_loftr_transformer: misaligned pointer");
    CallScope cs{h};
    if (int rc = cs.enter(stream)) return rc;
    HIP_TRY(h, "loftr transformer", h->loftr.transformer_only(n_pairs, first_block, n_blocks, d_in0, d_in1, d_out0, d_out1, cs.st));
    return cs.finish();
  });
}

int msf_debug_loftr_backbone(msf_handle* h, int32_t n, const uint8_t* d_a, const uint8_t* d_b, int64_t frame_stride,
                             int64_t row_stride, int32_t act_image, float* d_tok_a, float* d_tok_b, void* stream) {
  return guarded(h, "msf_debug_loftr_backbone", [&]() -> int {
    if (h->cfg.kind != MSF_KIND_LOFTR) return fail(h, MSF_ERR_INVALID_ARG, "msf_debug_loftr_backbone: not a LoFTR handle");
    const int images = d_b ? 2 * n : n;
    if (n < 0 || n > h->loftr.backbone_chunk() || !d_a || !d_tok_a || (d_b && !d_tok_b) || act_image < 0 ||
        (n > 0 && act_image >= images))
      return fail(h, MSF_ERR_INVALID_ARG, "msf_debug_loftr_backbone: bad argument");
    if (!aligned16(d_a, d_b, frame_stride, row_stride, d_tok_a, d_tok_b))
      return fail(h, MSF_ERR_INVALID_ARG, "msf_debug_loftr_backbone: misaligned pointer");
    if (row_stride < h->cfg.image_width) return fail(h, MSF_ERR_INVALID_ARG, "row_stride < image_width");
    if (frame_stride < row_stride * (long long)h->cfg.image_height)
      return fail(h, MSF_ERR_INVALID_ARG, "frame_stride < row_stride * image_height (frames would overlap)");
    if (n == 0) return MSF_OK;
    CallScope cs{h};
    if (int rc = cs.enter(stream)) return rc;
    HIP_TRY(h, "loftr backbone", h->loftr.backbone_only(n, d_a, d_b, frame_stride, (int)row_stride, act_image, d_tok_a,
                                                        d_tok_b, cs.st));
    return cs.finish();
  });
}

int msf_debug_orb_set_features(msf_handle* h, int32_t slot, int32_t n, const msf_keypoint* kp, const uint8_t* desc) {
  return guarded(h, "msf_debug_orb_set_features", [&]() -> int {
    if (h->cfg.kind != MSF_KIND_ORB) return fail(h, MSF_ERR_INVALID_ARG, "msf_debug_orb_set_features: not an ORB handle");
    if (slot < 0 || slot >= 2 * h->cfg.max_batch_pairs)
      return fail(h, MSF_ERR_INVALID_ARG, "msf_debug_orb_set_features: slot outside [0, 2*max_batch_pairs)");
    if (n < 0 || n > msf::kKpCap) return fail(h, MSF_ERR_INVALID_ARG, "msf_debug_orb_set_features: n outside [0, 2048]");
    if (n > 0 && (!kp || !desc)) return fail(h, MSF_ERR_INVALID_ARG, "msf_debug_orb_set_features: null pointer with n > 0");
    CallScope cs{h};
    if (int rc = cs.enter()) return rc;
    Drain drain{cs.st};   // the copies read the caller's arrays: never return with one in flight
    HIP_TRY(h, "orb set_features", h->orb.set_features(slot, n, kp, desc, cs.st));
    drain.armed = false;
    return cs.finish();
  });
}

int msf_debug_orb_tail(msf_handle* h, int32_t n_frames, const uint8_t* d_frames, int64_t frame_stride, int64_t row_stride,
                       int32_t first_slot, const int32_t* counts, const int32_t* cands, int32_t form) {
  return guarded(h, "msf_debug_orb_tail", [&]() -> int {
    if (h->cfg.kind != MSF_KIND_ORB) return fail(h, MSF_ERR_INVALID_ARG, "msf_debug_orb_tail: not an ORB handle");
    if (n_frames < 1 || !d_frames || !counts || first_slot < 0 ||
        (long long)first_slot + n_frames > 2ll * h->cfg.max_batch_pairs)
      return fail(h, MSF_ERR_INVALID_ARG, "msf_debug_orb_tail: slot range outside [0, 2*max_batch_pairs), or no frames");
    if (form != 0 && form != 1) return fail(h, MSF_ERR_INVALID_ARG, "msf_debug_orb_tail: form is 0 (dense) or 1 (streaming)");
    if (!aligned16(d_frames, frame_stride, row_stride))
      return fail(h, MSF_ERR_INVALID_ARG, "device frames must be 16-byte aligned with strides multiple of 16");
    if (row_stride < h->cfg.image_width ||
        (n_frames > 1 && frame_stride < row_stride * (long long)h->cfg.image_height))
      return fail(h, MSF_ERR_INVALID_ARG, "msf_debug_orb_tail: strides smaller than the frame");
    // the kernels' loads assume what this checks: nothing is enqueued for lists that fail it
    const std::string why = h->orb.tail_refusal(n_frames, counts, cands);
    if (!why.empty()) return fail(h, MSF_ERR_INVALID_ARG, "msf_debug_orb_tail: " + why);
    CallScope cs{h};
    if (int rc = cs.enter()) return rc;
    Drain drain{cs.st};   // the copies read the caller's arrays: never return with one in flight
    msf::FrameSrc src{d_frames, d_frames, n_frames, first_slot, frame_stride, (int)row_stride};
    HIP_TRY(h, "orb tail", h->orb.tail(src, n_frames, counts, cands, form, cs.st));
    drain.armed = false;
    return cs.finish();
  });
}

int msf_stage_times(msf_handle* h, const char** names, float* ms, int32_t cap) {
  if (!names || !ms || cap < 1) return 0;
  const int n = guarded(h, "msf_stage_times", [&]() -> int {
    hipSetDevice(h->cfg.device);
    return h->cfg.kind == MSF_KIND_ORB ? h->orb.stage_times(names, ms, cap) : h->loftr.stage_times(names, ms, cap);
  });
  return n > 0 ? n : 0;   // a number of stages, not a status: nothing to report is 0
}

int msf_frame_cache_stats(msf_handle* h, uint64_t* hits, uint64_t* misses, int32_t* capacity) {
  return guarded(h, "msf_frame_cache_stats", [&]() -> int {   // host state only: the device is not touched
    if (hits) *hits = h->fc_hits;
    if (misses) *misses = h->fc_misses;
    if (capacity) *capacity = (int32_t)h->fc.size();
    return MSF_OK;
  });
}

/* LoFTR weights, on the host (no GPU needed): reads `path` -- the reference's ONNX model or the MSFLTR01 blob -- and
 * reports the number of tensors / floats and a digest of names, shapes and values; equal digests <=> identical weights. */
int msf_weights_info(const char* path, uint64_t* digest, int32_t* n_tensors, int64_t* n_floats) {
  return guarded("msf_weights_info", [&]() -> int {
    if (!path) return fail(nullptr, MSF_ERR_INVALID_ARG, "msf_weights_info: null path");
    // test hook for the no-exceptions guarantee, armed only by the test's environment
    if (std::strcmp(path, "::throw::") == 0 && getenv("MSF_TEST_HOOKS")) throw std::bad_alloc();
    msf::WeightMap w;
    const std::string err = msf::load_weights(path, &w);
    if (!err.empty()) return fail(nullptr, MSF_ERR_IO, err);
    int64_t nf = 0;
    const uint64_t d = msf::weights_digest(w, &nf);
    if (digest) *digest = d;
    if (n_tensors) *n_tensors = (int32_t)w.size();
    if (n_floats) *n_floats = nf;
    return MSF_OK;
  });
}

/* Writes the weights of `src_path` (ONNX model or blob) as an MSFLTR01 blob: a load-time cache, nothing more. */
int msf_convert_weights(const char* src_path, const char* dst_blob_path) {
  return guarded("msf_convert_weights", [&]() -> int {
    if (!src_path || !dst_blob_path) return fail(nullptr, MSF_ERR_INVALID_ARG, "msf_convert_weights: null path");
    msf::WeightMap w;
    std::string err = msf::load_weights(src_path, &w);
    if (err.empty()) err = msf::save_blob(dst_blob_path, w);
    if (!err.empty()) return fail(nullptr, MSF_ERR_IO, err);
    return MSF_OK;
  });
}

namespace {

namespace tk = msf::tracking;

tk::Map to_map(const msf_local_map& m) {
  return tk::Map{m.n_points, m.n_kf, m.n_entries, m.n_cur, reinterpret_cast<const tk::Point*>(m.points),
                 m.kf_start, m.kf_key, m.kf_point, m.cur_key, m.cur_point};
}

tk::Frustum to_frustum(const msf_frustum_params& p) {
  tk::Frustum f;
  static_assert(sizeof f.view == sizeof p.view, "msf_view layout");
  std::memcpy(&f.view, &p.view, sizeof f.view);
  for (int k = 0; k < 3; k++) f.Ow[k] = p.Ow[k];
  f.min_x = p.min_x, f.max_x = p.max_x, f.min_y = p.min_y, f.max_y = p.max_y;
  f.cos_limit = p.viewing_cos_limit;
  return f;
}

msf::FrustumOut frustum_out(const msf_frustum_result& r) {
  return msf::FrustumOut{r.status_word, r.n_to_match, r.status, r.visible, r.owner_kf, r.u, r.v, r.dist, r.view_cos};
}

msf::ClaimOut claim_out(const msf_claim_result& r, int32_t corr_cap) {
  return msf::ClaimOut{r.status_word, r.n_claims, r.n_claimed, r.claims, r.claim_status, r.n_corr, r.corr_p3d,
                       r.corr_p2d, r.corr_point, corr_cap};
}

// nullptr when the structs of a call are usable, else what is wrong with them.  What the host can see of a map whose
// arrays are in device memory: the counts and the pointers.
const char* local_map_fault(const msf_local_map* map) {
  if (!map || map->struct_size != sizeof(msf_local_map)) return "map is NULL or map->struct_size is not sizeof(msf_local_map)";
  if (map->n_points < 0 || map->n_kf < 0 || map->n_entries < 0 || map->n_cur < 0) return "a negative count";
  if ((map->n_points && !map->points) || (map->n_kf && !map->kf_start) || (map->n_entries && (!map->kf_key || !map->kf_point)) ||
      (map->n_cur && (!map->cur_key || !map->cur_point)))
    return "a required pointer of map is NULL";
  if (map->n_kf == 0 && map->n_entries != 0) return "entries without a key frame";
  return nullptr;
}

const char* frustum_args_fault(const msf_local_map* map, const msf_frustum_params* prm, const msf_frustum_result* out) {
  if (!out || out->struct_size != sizeof(msf_frustum_result)) return "out is NULL or its struct_size is not sizeof(msf_frustum_result)";
  if (!prm || prm->struct_size != sizeof(msf_frustum_params)) return "params is NULL or params->struct_size is not sizeof(msf_frustum_params)";
  if (!out->status_word || (map->n_kf && !out->n_to_match)) return "a required pointer is NULL (status_word, n_to_match)";
  return tk::frustum_fault(to_frustum(*prm));
}

const char* claim_out_fault(const msf_local_map* map, const msf_claim_result* out) {
  if (!out || out->struct_size != sizeof(msf_claim_result)) return "out is NULL or its struct_size is not sizeof(msf_claim_result)";
  if (!out->status_word || !out->n_claims || (map->n_kf && !out->n_claimed)) return "a required pointer is NULL (status_word, n_claims, n_claimed)";
  return nullptr;
}

// What the host entry points of msf_tracking.h keep in the workspace besides the scratch and their result arrays: the
// local map, and for msf_search_local_points the slots and the gate's bytes.
struct TrackPlan {
  tk::Scratch s;
  tk::Point* points = nullptr;
  int32_t *kf_start = nullptr, *kf_key = nullptr, *kf_point = nullptr, *cur_key = nullptr, *cur_point = nullptr;
  int32_t* slots = nullptr;
  uint8_t* matched = nullptr;
};

void take_map(msf::Carver& c, const msf_local_map& m, TrackPlan* p) {
  p->points = c.take<tk::Point>(m.n_points);
  p->kf_start = c.take<int32_t>((size_t)m.n_kf + 1);
  p->kf_key = c.take<int32_t>(m.n_entries);
  p->kf_point = c.take<int32_t>(m.n_entries);
  p->cur_key = c.take<int32_t>(m.n_cur);
  p->cur_point = c.take<int32_t>(m.n_cur);
}

// the host map to its pieces; *dev = the map the kernels read
int upload_map(msf_handle* h, hipStream_t st, const msf_local_map& m, const TrackPlan& p, tk::Map* dev) {
  auto up = [&](void* dst, const void* src, size_t bytes) -> int {
    if (!bytes) return MSF_OK;
    HIP_TRY(h, "hipMemcpyAsync(local map)", hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st));
    return MSF_OK;
  };
  if (int rc = up(p.points, m.points, (size_t)m.n_points * sizeof(msf_map_point))) return rc;
  if (m.n_kf)
    if (int rc = up(p.kf_start, m.kf_start, ((size_t)m.n_kf + 1) * sizeof(int32_t))) return rc;
  if (int rc = up(p.kf_key, m.kf_key, (size_t)m.n_entries * sizeof(int32_t))) return rc;
  if (int rc = up(p.kf_point, m.kf_point, (size_t)m.n_entries * sizeof(int32_t))) return rc;
  if (int rc = up(p.cur_key, m.cur_key, (size_t)m.n_cur * sizeof(int32_t))) return rc;
  if (int rc = up(p.cur_point, m.cur_point, (size_t)m.n_cur * sizeof(int32_t))) return rc;
  *dev = tk::Map{m.n_points, m.n_kf, m.n_entries, m.n_cur, p.points, p.kf_start, p.kf_key, p.kf_point, p.cur_key, p.cur_point};
  return MSF_OK;
}

}  // namespace

int msf_tracking_version(void) { return MSF_TRACKING_VERSION; }

int msf_frustum(msf_handle* h, const msf_local_map* map, const msf_frustum_params* params, msf_frustum_result* out) {
  return guarded(h, "msf_frustum", [&]() -> int {
    const std::string who = "msf_frustum: ";
    if (const char* fault = local_map_fault(map)) return fail(h, MSF_ERR_INVALID_ARG, who + fault);
    if (const char* fault = frustum_args_fault(map, params, out)) return fail(h, MSF_ERR_INVALID_ARG, who + fault);
    if (const char* fault = tk::map_fault(to_map(*map), h->cfg.image_width, h->cfg.image_height))
      return fail(h, MSF_ERR_INVALID_ARG, who + fault);
    CallScope cs{h};
    if (int rc = cs.enter()) return rc;
    const size_t units[msf::kTrUnits] = {1, (size_t)map->n_points, (size_t)map->n_kf};
    msf_frustum_result dev{};
    TrackPlan p;
    if (int rc = carve(h, h->d_track, (size_t)1 << 16, "hipMalloc(tracking workspace)", [&](msf::Carver& c) {
          tk::layout(c, map->n_points, map->n_kf, 0, 0, &p.s);
          take_map(c, *map, &p);
          msf::carve_result(c, msf::kFrustumArrays, units, 1, nullptr, *out, &dev);
        }))
      return rc;
    hipStream_t st = cs.st;
    Drain drain{st};
    tk::Map dmap;
    if (int rc = upload_map(h, st, *map, p, &dmap)) return rc;
    HIP_TRY(h, "tracking_check", msf::tracking_check(dmap, h->cfg.image_width, h->cfg.image_height, p.s, st));
    HIP_TRY(h, "tracking_frustum", msf::tracking_frustum(dmap, to_frustum(*params), p.s, frustum_out(dev), msf::GateOut{}, st));
    const msf::Extent all{0, 1, 1, 1, units, units};
    if (int rc = fetch_result(h, st, msf::kFrustumArrays, dev, *out, all)) return rc;
    drain.armed = false;
    return cs.finish();
  });
}

int msf_frustum_device(msf_handle* h, const msf_local_map* map, const msf_frustum_params* params,
                       msf_frustum_result* out, void* stream) {
  return guarded(h, "msf_frustum_device", [&]() -> int {
    const std::string who = "msf_frustum_device: ";
    if (const char* fault = local_map_fault(map)) return fail(h, MSF_ERR_INVALID_ARG, who + fault);
    if (const char* fault = frustum_args_fault(map, params, out)) return fail(h, MSF_ERR_INVALID_ARG, who + fault);
    if (!aligned16(map->points)) return fail(h, MSF_ERR_INVALID_ARG, who + "map->points must be 16-byte aligned");
    CallScope cs{h};
    if (int rc = cs.enter(stream)) return rc;
    TrackPlan p;
    if (int rc = carve(h, h->d_track, (size_t)1 << 16, "hipMalloc(tracking workspace)",
                       [&](msf::Carver& c) { tk::layout(c, map->n_points, map->n_kf, 0, 0, &p.s); }))
      return rc;
    const tk::Map dmap = to_map(*map);
    HIP_TRY(h, "tracking_check", msf::tracking_check(dmap, h->cfg.image_width, h->cfg.image_height, p.s, cs.st));
    HIP_TRY(h, "tracking_frustum", msf::tracking_frustum(dmap, to_frustum(*params), p.s, frustum_out(*out), msf::GateOut{}, cs.st));
    return cs.finish();
  });
}

int msf_claim_points_device(msf_handle* h, const msf_local_map* map, const msf_match* d_matches, int32_t cap_per_pair,
                            const int32_t* d_n_out, const uint8_t* d_matched, int32_t corr_cap, msf_claim_result* out,
                            void* stream) {
  return guarded(h, "msf_claim_points_device", [&]() -> int {
    const std::string who = "msf_claim_points_device: ";
    if (const char* fault = local_map_fault(map)) return fail(h, MSF_ERR_INVALID_ARG, who + fault);
    if (const char* fault = claim_out_fault(map, out)) return fail(h, MSF_ERR_INVALID_ARG, who + fault);
    if (cap_per_pair < 1 || corr_cap < 0) return fail(h, MSF_ERR_INVALID_ARG, who + "cap_per_pair < 1 or corr_cap < 0");
    if (map->n_kf > 65534 || (long long)map->n_kf * cap_per_pair >= (1ll << 31))
      return fail(h, MSF_ERR_INVALID_ARG, who + "n_kf > 65534 or n_kf * cap_per_pair >= 2^31");
    if (map->n_kf > 0 && (!d_matches || !d_n_out || !d_matched))
      return fail(h, MSF_ERR_INVALID_ARG, who + "a required pointer is NULL (d_matches, d_n_out, d_matched)");
    CallScope cs{h};
    if (int rc = cs.enter(stream)) return rc;
    const int W = h->cfg.image_width, H = h->cfg.image_height;
    TrackPlan p;
    if (int rc = carve(h, h->d_track, (size_t)1 << 16, "hipMalloc(tracking workspace)", [&](msf::Carver& c) {
          tk::layout(c, map->n_points, map->n_kf, (size_t)W * H, cap_per_pair, &p.s);
        }))
      return rc;
    const tk::Map dmap = to_map(*map);
    const msf::ClaimLists in{d_matches, cap_per_pair, cap_per_pair, d_n_out, d_matched};
    HIP_TRY(h, "tracking_check", msf::tracking_check(dmap, W, H, p.s, cs.st));
    HIP_TRY(h, "tracking_claims", msf::tracking_claims(dmap, W, H, in, p.s, claim_out(*out, corr_cap), cs.st));
    return cs.finish();
  });
}

int msf_search_local_points(msf_handle* h, int32_t query_slot, const int32_t* slots, const msf_local_map* map,
                            const msf_frustum_params* params, uint32_t flags, int32_t* num_matches,
                            msf_match* out_matches, int32_t cap_per_pair, msf_frustum_result* frustum,
                            msf_claim_result* claims, msf_device_corr* keep) {
  return guarded(h, "msf_search_local_points", [&]() -> int {
    const char* const name = "msf_search_local_points";
    const std::string who = std::string(name) + ": ";
    if (const char* fault = local_map_fault(map)) return fail(h, MSF_ERR_INVALID_ARG, who + fault);
    if (const char* fault = frustum_args_fault(map, params, frustum)) return fail(h, MSF_ERR_INVALID_ARG, who + fault);
    if (const char* fault = claim_out_fault(map, claims)) return fail(h, MSF_ERR_INVALID_ARG, who + fault);
    const bool on_device = flags & MSF_SEARCH_KEEP_ON_DEVICE;
    if (flags & ~MSF_SEARCH_KEEP_ON_DEVICE) return fail(h, MSF_ERR_INVALID_ARG, who + "unknown flag bits");
    if (on_device && (!keep || keep->struct_size != sizeof(msf_device_corr)))
      return fail(h, MSF_ERR_INVALID_ARG, who + "keep is NULL or keep->struct_size is not sizeof(msf_device_corr)");
    const int n = map->n_kf;
    if (cap_per_pair < 1 || (n > 0 && (!slots || !num_matches)))
      return fail(h, MSF_ERR_INVALID_ARG, who + "cap_per_pair < 1, or slots / num_matches is NULL");
    if (n > 0)
      if (int rc = one_to_many_args(h, name, query_slot, n, slots)) return rc;
    const int W = h->cfg.image_width, H = h->cfg.image_height;
    if (const char* fault = tk::map_fault(to_map(*map), W, H)) return fail(h, MSF_ERR_INVALID_ARG, who + fault);
    const int stage_cap = h->stage_cap > 0 ? h->stage_cap : 1;
    if ((long long)n * stage_cap >= (1ll << 31)) return fail(h, MSF_ERR_INVALID_ARG, who + "n_kf * stage_cap >= 2^31");
    const int limit = cap_per_pair < stage_cap ? cap_per_pair : stage_cap;
    const long long corr_room = (long long)map->n_cur + (long long)n * limit;
    if (corr_room >= (1ll << 31)) return fail(h, MSF_ERR_INVALID_ARG, who + "n_cur + n_kf * cap_per_pair >= 2^31");
    const int32_t corr_cap = (int32_t)corr_room;
    CallScope cs{h};
    if (int rc = cs.enter()) return rc;
    hipStream_t st = cs.st;
    const size_t f_units[msf::kTrUnits] = {1, (size_t)map->n_points, (size_t)n};
    const size_t c_units[msf::kClUnits] = {1, (size_t)n, (size_t)corr_cap};
    msf_frustum_result fdev{};
    msf_claim_result cdev{};
    TrackPlan p;
    if (int rc = carve(h, h->d_track, (size_t)1 << 16, "hipMalloc(tracking workspace)", [&](msf::Carver& c) {
          tk::layout(c, map->n_points, n, (size_t)W * H, stage_cap, &p.s);
          take_map(c, *map, &p);
          p.slots = c.take<int32_t>(n);
          p.matched = c.take<uint8_t>(n);
          msf::carve_result(c, msf::kFrustumArrays, f_units, 1, nullptr, *frustum, &fdev);
          msf::carve_result(c, msf::kClaimArrays, c_units, (size_t)stage_cap, nullptr, *claims, &cdev);
          // the kernel writes the correspondences all four or none: they stay here (keep), or the caller wants some
          if (on_device || claims->n_corr || claims->corr_p3d || claims->corr_p2d || claims->corr_point) {
            // carve_result gave a piece to what the caller asked for: only the others are taken here, in both passes
            if (!claims->n_corr) cdev.n_corr = c.take<int32_t>(1);
            if (!claims->corr_p3d) cdev.corr_p3d = c.take<float>((size_t)corr_cap * 3);
            if (!claims->corr_p2d) cdev.corr_p2d = c.take<float>((size_t)corr_cap * 2);
            if (!claims->corr_point) cdev.corr_point = c.take<int32_t>(corr_cap);
          }
        }))
      return rc;
    Drain drain{st};
    tk::Map dmap;
    if (int rc = upload_map(h, st, *map, p, &dmap)) return rc;
    msf::GateOut gate{};
    if (n > 0) {
      const int maxp = h->cfg.max_batch_pairs;
      HIP_TRY(h, "hipMemcpyAsync(slots)", hipMemcpyAsync(p.slots, slots, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, st));
      h->idx_stage.assign((size_t)maxp, query_slot);
      HIP_TRY(h, "hipMemcpyAsync(idx)",
              hipMemcpyAsync(h->d_idx, h->idx_stage.data(), (size_t)maxp * sizeof(int32_t), hipMemcpyHostToDevice, st));
      gate = msf::GateOut{p.slots, h->d_idx + maxp, p.matched};
    }
    HIP_TRY(h, "tracking_check", msf::tracking_check(dmap, W, H, p.s, st));
    HIP_TRY(h, "tracking_frustum", msf::tracking_frustum(dmap, to_frustum(*params), p.s, frustum_out(fdev), gate, st));
    if (n > 0)   // the train slot of an unmatched key frame is -1: both pipelines answer a negative slot with n_out = -1
      if (int rc = match_slot_pairs(h, n, h->d_idx, gate.train, h->d_out, h->stage_cap, h->d_n, st, 0)) return rc;
    const msf::ClaimLists in{h->d_out, stage_cap, limit, h->d_n, p.matched};
    HIP_TRY(h, "tracking_claims", msf::tracking_claims(dmap, W, H, in, p.s, claim_out(cdev, corr_cap), st));
    // the copy-back: the counts first, they say how much of every list there is to fetch
    const msf::Extent all{0, 1, 1, 1, f_units, f_units};
    if (int rc = fetch_result(h, st, msf::kFrustumArrays, fdev, *frustum, all)) return rc;
    if (int rc = fetch(h, st, num_matches, h->d_n, (size_t)n * sizeof *num_matches)) return rc;
    if (int rc = fetch(h, st, claims->status_word, cdev.status_word, sizeof(int32_t))) return rc;
    if (int rc = fetch(h, st, claims->n_claims, cdev.n_claims, sizeof(int32_t))) return rc;
    if (int rc = fetch(h, st, claims->n_claimed, cdev.n_claimed, (size_t)n * sizeof(int32_t))) return rc;
    int32_t n_corr = 0;
    if (cdev.n_corr)
      if (int rc = fetch(h, st, &n_corr, cdev.n_corr, sizeof n_corr)) return rc;
    HIP_TRY(h, "hipStreamSynchronize", hipStreamSynchronize(st));
    bool capacity = false;
    for (int i = 0; i < n; i++) {
      if (frustum->n_to_match[i] == 0) continue;   // not matched: num_matches = -1 is the gate, no capacity failure
      const int w = deliverable(h, num_matches[i], cap_per_pair, &capacity);
      if (int rc = fetch(h, st, from(out_matches, (size_t)i * cap_per_pair), h->d_out + (size_t)i * h->stage_cap,
                         (size_t)w * sizeof(msf_match)))
        return rc;
      if (int rc = fetch(h, st, from(claims->claim_status, (size_t)i * cap_per_pair),
                         from(cdev.claim_status, (size_t)i * stage_cap), (size_t)w))
        return rc;
    }
    const size_t n_claims = claims->n_claims[0] > 0 ? (size_t)claims->n_claims[0] : 0;
    if (int rc = fetch(h, st, claims->claims, cdev.claims, n_claims * sizeof(msf_local_claim))) return rc;
    if (claims->n_corr) claims->n_corr[0] = n_corr;
    if (on_device) {
      keep->corr_cap = corr_cap;
      keep->d_corr_p3d = cdev.corr_p3d, keep->d_corr_p2d = cdev.corr_p2d;
      keep->d_corr_point = cdev.corr_point, keep->d_n_corr = cdev.n_corr;
    } else if (n_corr > 0 && cdev.n_corr) {
      if (int rc = fetch(h, st, claims->corr_p3d, cdev.corr_p3d, (size_t)n_corr * 3 * sizeof(float))) return rc;
      if (int rc = fetch(h, st, claims->corr_p2d, cdev.corr_p2d, (size_t)n_corr * 2 * sizeof(float))) return rc;
      if (int rc = fetch(h, st, claims->corr_point, cdev.corr_point, (size_t)n_corr * sizeof(int32_t))) return rc;
    }
    drain.armed = false;
    if (int rc = cs.finish()) return rc;
    return capacity ? fail(h, MSF_ERR_CAPACITY, kNoResult) : MSF_OK;
  });
}

namespace {

namespace ft = msf::ftrack;

ft::Map to_frame_map(const msfx_frame_map& m) {
  return ft::Map{m.n_points, m.n_ref, m.n_cur, reinterpret_cast<const tk::Point*>(m.points), m.observed,
                 m.ref_key, m.ref_point, m.cur_key, m.cur_point};
}

// nullptr when the structs of a call are usable, else what is wrong with them: what the host can see of a map whose
// arrays may be in device memory
const char* frame_map_fault(const msfx_frame_map* map, const msfx_track_result* out) {
  if (!map || map->struct_size != sizeof(msfx_frame_map)) return "map is NULL or map->struct_size is not sizeof(msfx_frame_map)";
  if (!out || out->struct_size != sizeof(msfx_track_result)) return "out is NULL or out->struct_size is not sizeof(msfx_track_result)";
  if (!out->track_status) return "a required pointer is NULL (out->track_status)";
  if (map->n_points < 0 || map->n_ref < 0 || map->n_cur < 0) return "a negative count";
  if ((map->n_points && !map->points) || (map->n_ref && (!map->ref_key || !map->ref_point)) ||
      (map->n_cur && (!map->cur_key || !map->cur_point)))
    return "a required pointer of map is NULL";
  return nullptr;
}

const char* track_params_fault(const msfx_track_params* prm, const msf_pose_result* pose) {
  if (!prm || prm->struct_size != sizeof(msfx_track_params)) return "params is NULL or params->struct_size is not sizeof(msfx_track_params)";
  if (prm->pose.struct_size != sizeof(msf_pose_params)) return "params->pose.struct_size is not sizeof(msf_pose_params)";
  if (std::isnan(prm->pose.chi2)) return "chi2 must not be NaN";
  if (prm->min_matches < 0 || prm->min_map_matches < 0) return "min_matches or min_map_matches is negative";
  if (pose && pose->struct_size != sizeof(msf_pose_result)) return "pose->struct_size is not sizeof(msf_pose_result)";
  return nullptr;
}

// What a call of msf_frame_tracking.h keeps in the family's workspace: the words the launches hand on, the entry pose,
// the result arrays the caller gave no pointer for (every one is read by a later launch or by `keep`), the optimiser's
// arrays; for msfx_track_frame also the frame's map.  base / bytes: the whole of it, for the host call's memset.
struct FrameTrackPlan {
  ft::Scratch s;
  float* tcw0 = nullptr;
  msfx_track_result dev{};
  msf_pose_result pdev{};
  tk::Point* points = nullptr;
  uint8_t* observed = nullptr;
  int32_t *ref_key = nullptr, *ref_point = nullptr, *cur_key = nullptr, *cur_point = nullptr;
  uint8_t* base = nullptr;
  size_t bytes = 0;
};

// `given`: the caller's device structs (the _device calls) or null (msfx_track_frame: everything is carved).
void frame_track_layout(msf::Carver& c, const msfx_frame_map& map, int32_t cap, int32_t corr_cap,
                        const msfx_track_result* given, const msfx_track_result& wanted, const msf_pose_result* pose_given,
                        const msf_pose_result& pose_wanted, bool host_map, FrameTrackPlan* p) {
  p->base = c.base;
  ft::layout(c, &p->s);
  p->tcw0 = c.take<float>(12);
  const size_t units[msf::kFtUnits] = {1, (size_t)cap, (size_t)map.n_cur, (size_t)corr_cap};
  msf::carve_result(c, msf::kTrackArrays, units, 1, given, wanted, &p->dev);
  const size_t pcap = corr_cap > 0 ? (size_t)corr_cap : 1;
  const size_t punits[] = {1, msf::kPoseRounds, msf::kPoseIterations};
  msf::carve_result(c, msf::kPoseArrays, punits, pcap, pose_given, pose_wanted, &p->pdev);
  // the cut reads the pose and the outlier bytes whether the caller wants them or not
  if (!p->pdev.Tcw) p->pdev.Tcw = c.take<float>(12);
  if (!p->pdev.outliers) p->pdev.outliers = c.take<uint8_t>(pcap);
  if (host_map) {
    p->points = c.take<tk::Point>(map.n_points);
    p->observed = map.observed ? c.take<uint8_t>(map.n_points) : nullptr;
    p->ref_key = c.take<int32_t>(map.n_ref);
    p->ref_point = c.take<int32_t>(map.n_ref);
    p->cur_key = c.take<int32_t>(map.n_cur);
    p->cur_point = c.take<int32_t>(map.n_cur);
  }
  p->bytes = c.off;
}

msf::CarryOut carry_out(const msfx_track_result& r) {
  return msf::CarryOut{r.track_status, r.n_map, r.map, r.carry_status, r.cur_status, r.corr_p3d, r.corr_p2d, r.corr_point};
}

// the three launches of steps 0-6 on one list, `dev` and `pdev` all device pointers
int launch_frame_track(msf_handle* h, const ft::Map& dmap, const msf_match* d_matches, int32_t cap, const int32_t* d_n_out,
                       int32_t corr_cap, const msfx_track_params& prm, const FrameTrackPlan& p, hipStream_t st) {
  msf::CarryIn in{d_matches, cap, d_n_out, prm.min_matches, corr_cap, {}, p.tcw0};
  std::memcpy(in.tcw0, prm.Tcw0, sizeof in.tcw0);
  HIP_TRY(h, "frame_tracking_carry", msf::frame_tracking_carry(dmap, h->cfg.image_width, h->cfg.image_height, in, p.s,
                                                               carry_out(p.dev), false, st));
  const int32_t pcap = corr_cap > 0 ? corr_cap : 1;
  const msf::PoseLists lists{p.dev.corr_p3d, p.dev.corr_p2d, pcap, p.s.state + 1, 0, p.tcw0, 0, nullptr, 0};
  const msf::PoseParams pp{prm.pose.fx, prm.pose.fy, prm.pose.cx, prm.pose.cy, prm.pose.chi2};
  HIP_TRY(h, "pose_optimize", msf::pose_optimize(1, lists, pp, to_out(p.pdev), st));
  const msf::CutIn cut{p.tcw0, p.pdev.Tcw, p.pdev.n_good, p.pdev.outliers, prm.min_map_matches, d_n_out};
  const msf::CutOut out{p.dev.track_status, p.dev.n_map, p.dev.map, p.dev.Tcw, p.dev.n_good, p.dev.n_kept,
                        p.dev.kept_key, p.dev.kept_point, p.dev.n_removed, p.dev.removed, p.dev.n_matches_map};
  HIP_TRY(h, "frame_tracking_cut", msf::frame_tracking_cut(dmap, cut, p.s, out, st));
  return MSF_OK;
}

const char* device_list_fault(const msf_match* d_matches, int32_t cap, const int32_t* d_n_out, int32_t corr_cap) {
  if (cap < 1 || corr_cap < 0) return "cap < 1 or corr_cap < 0";
  if (!d_matches || !d_n_out) return "a required pointer is NULL (d_matches, d_n_out)";
  return nullptr;
}

}  // namespace

int msfx_frame_tracking_version(void) { return MSFX_FRAME_TRACKING_VERSION; }

int msfx_carry_points_device(msf_handle* h, const msfx_frame_map* map, const msf_match* d_matches, int32_t cap,
                             const int32_t* d_n_out, int32_t corr_cap, msfx_track_result* out, void* stream) {
  return guarded(h, "msfx_carry_points_device", [&]() -> int {
    const std::string who = "msfx_carry_points_device: ";
    if (const char* fault = frame_map_fault(map, out)) return fail(h, MSF_ERR_INVALID_ARG, who + fault);
    if (const char* fault = device_list_fault(d_matches, cap, d_n_out, corr_cap)) return fail(h, MSF_ERR_INVALID_ARG, who + fault);
    CallScope cs{h};
    if (int rc = cs.enter(stream)) return rc;
    FrameTrackPlan p;
    const msf_pose_result no_pose{};
    if (int rc = carve(h, h->d_ftrack, (size_t)1 << 16, "hipMalloc(frame tracking workspace)", [&](msf::Carver& c) {
          frame_track_layout(c, *map, cap, corr_cap, out, *out, &no_pose, no_pose, false, &p);
        }))
      return rc;
    const msf::CarryIn in{d_matches, cap, d_n_out, 0, corr_cap, {}, nullptr};
    HIP_TRY(h, "frame_tracking_carry", msf::frame_tracking_carry(to_frame_map(*map), h->cfg.image_width, h->cfg.image_height, in,
                                                                 p.s, carry_out(p.dev), true, cs.st));
    return cs.finish();
  });
}

int msfx_track_list_device(msf_handle* h, const msfx_frame_map* map, const msf_match* d_matches, int32_t cap,
                           const int32_t* d_n_out, int32_t corr_cap, const msfx_track_params* params,
                           msfx_track_result* out, msf_pose_result* pose, void* stream) {
  return guarded(h, "msfx_track_list_device", [&]() -> int {
    const std::string who = "msfx_track_list_device: ";
    if (const char* fault = frame_map_fault(map, out)) return fail(h, MSF_ERR_INVALID_ARG, who + fault);
    if (const char* fault = track_params_fault(params, pose)) return fail(h, MSF_ERR_INVALID_ARG, who + fault);
    if (const char* fault = device_list_fault(d_matches, cap, d_n_out, corr_cap)) return fail(h, MSF_ERR_INVALID_ARG, who + fault);
    CallScope cs{h};
    if (int rc = cs.enter(stream)) return rc;
    FrameTrackPlan p;
    const msf_pose_result no_pose{};
    const msf_pose_result& pose_given = pose ? *pose : no_pose;
    if (int rc = carve(h, h->d_ftrack, (size_t)1 << 16, "hipMalloc(frame tracking workspace)", [&](msf::Carver& c) {
          frame_track_layout(c, *map, cap, corr_cap, out, *out, &pose_given, pose_given, false, &p);
        }))
      return rc;
    if (int rc = launch_frame_track(h, to_frame_map(*map), d_matches, cap, d_n_out, corr_cap, *params, p, cs.st)) return rc;
    return cs.finish();
  });
}

int msfx_track_frame(msf_handle* h, int32_t query_slot, int32_t train_slot, const msfx_frame_map* map,
                     const msfx_track_params* params, uint32_t flags, int32_t* num_matches, msf_match* out_matches,
                     int32_t cap_per_pair, msfx_track_result* out, msf_pose_result* pose, msfx_device_track* keep) {
  return guarded(h, "msfx_track_frame", [&]() -> int {
    const char* const name = "msfx_track_frame";
    const std::string who = std::string(name) + ": ";
    if (const char* fault = frame_map_fault(map, out)) return fail(h, MSF_ERR_INVALID_ARG, who + fault);
    if (const char* fault = track_params_fault(params, pose)) return fail(h, MSF_ERR_INVALID_ARG, who + fault);
    const bool on_device = flags & MSFX_TRACK_KEEP_ON_DEVICE;
    if (flags & ~MSFX_TRACK_KEEP_ON_DEVICE) return fail(h, MSF_ERR_INVALID_ARG, who + "unknown flag bits");
    if (on_device && (!keep || keep->struct_size != sizeof(msfx_device_track)))
      return fail(h, MSF_ERR_INVALID_ARG, who + "keep is NULL or keep->struct_size is not sizeof(msfx_device_track)");
    if (cap_per_pair < 1 || !num_matches) return fail(h, MSF_ERR_INVALID_ARG, who + "cap_per_pair < 1, or num_matches is NULL");
    if (int rc = one_to_many_args(h, name, query_slot, 1, &train_slot)) return rc;
    const int W = h->cfg.image_width, H = h->cfg.image_height;
    if (const char* fault = ft::map_fault(to_frame_map(*map), W, H)) return fail(h, MSF_ERR_INVALID_ARG, who + fault);
    const int stage_cap = h->stage_cap > 0 ? h->stage_cap : 1;
    const int32_t limit = cap_per_pair < stage_cap ? cap_per_pair : stage_cap;
    if ((long long)map->n_cur + limit >= (1ll << 31)) return fail(h, MSF_ERR_INVALID_ARG, who + "n_cur + cap_per_pair >= 2^31");
    const int32_t corr_cap = map->n_cur + limit;
    CallScope cs{h};
    if (int rc = cs.enter()) return rc;
    hipStream_t st = cs.st;
    FrameTrackPlan p;
    const msf_pose_result no_pose{};
    const msf_pose_result& pose_wanted = pose ? *pose : no_pose;
    if (int rc = carve(h, h->d_ftrack, (size_t)1 << 16, "hipMalloc(frame tracking workspace)", [&](msf::Carver& c) {
          frame_track_layout(c, *map, limit, corr_cap, nullptr, *out, nullptr, pose_wanted, true, &p);
        }))
      return rc;
    Drain drain{st};
    // what the kernels leave alone comes back as 0, as with msf_pose_optimize
    HIP_TRY(h, "hipMemsetAsync", hipMemsetAsync(p.base, 0, p.bytes, st));
    auto up = [&](void* dst, const void* src, size_t bytes) -> int {
      if (!bytes || !src) return MSF_OK;
      HIP_TRY(h, "hipMemcpyAsync(frame map)", hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st));
      return MSF_OK;
    };
    if (int rc = up(p.points, map->points, (size_t)map->n_points * sizeof(msf_map_point))) return rc;
    if (int rc = up(p.observed, map->observed, (size_t)map->n_points)) return rc;
    if (int rc = up(p.ref_key, map->ref_key, (size_t)map->n_ref * sizeof(int32_t))) return rc;
    if (int rc = up(p.ref_point, map->ref_point, (size_t)map->n_ref * sizeof(int32_t))) return rc;
    if (int rc = up(p.cur_key, map->cur_key, (size_t)map->n_cur * sizeof(int32_t))) return rc;
    if (int rc = up(p.cur_point, map->cur_point, (size_t)map->n_cur * sizeof(int32_t))) return rc;
    const ft::Map dmap{map->n_points, map->n_ref, map->n_cur, p.points, p.observed, p.ref_key, p.ref_point, p.cur_key, p.cur_point};
    if (int rc = launch_one_to_many(h, query_slot, 1, &train_slot, st)) return rc;
    if (int rc = launch_frame_track(h, dmap, h->d_out, limit, h->d_n, corr_cap, *params, p, st)) return rc;
    // the copy-back: the summary first -- every scalar of the call in one copy; the counts in it say how much of every
    // array there is to fetch
    int32_t sum[ft::kSummaryWords] = {};
    if (int rc = fetch(h, st, sum, p.s.summary, sizeof sum)) return rc;
    HIP_TRY(h, "hipStreamSynchronize", hipStreamSynchronize(st));
    num_matches[0] = sum[ft::kSumNumMatches];
    const int32_t counts[4] = {sum[ft::kSumStatus], sum[ft::kSumMap], sum[ft::kSumKept], sum[ft::kSumRemoved]};
    bool capacity = false;
    const int w = deliverable(h, num_matches[0], cap_per_pair, &capacity);
    if (num_matches[0] > cap_per_pair) capacity = true;   // the body ran on a clipped list: delivered, and said so
    if (int rc = fetch(h, st, out_matches, h->d_out, (size_t)w * sizeof(msf_match))) return rc;
    out->track_status[0] = counts[0];
    const size_t pcap = corr_cap > 0 ? (size_t)corr_cap : 1;
    const size_t punits[] = {1, msf::kPoseRounds, msf::kPoseIterations};
    if (counts[0] >= 0) {
      const size_t n_map = (size_t)counts[1], n_kept = (size_t)counts[2], n_removed = (size_t)counts[3];
      const bool gated = counts[0] == ft::kFewMatches;
      if (out->n_map) out->n_map[0] = counts[1];
      if (out->n_kept) out->n_kept[0] = counts[2];
      if (out->n_removed) out->n_removed[0] = counts[3];
      if (out->n_good) out->n_good[0] = sum[ft::kSumGood];
      if (out->n_matches_map) out->n_matches_map[0] = sum[ft::kSumMatchesMap];
      if (out->Tcw) std::memcpy(out->Tcw, sum + ft::kSumTcw, 12 * sizeof(float));
      if (int rc = fetch(h, st, out->map, p.dev.map, n_map * sizeof(msfx_frame_point))) return rc;
      if (int rc = fetch(h, st, out->carry_status, p.dev.carry_status, gated ? 0 : (size_t)w)) return rc;
      if (int rc = fetch(h, st, out->cur_status, p.dev.cur_status, (size_t)map->n_cur)) return rc;
      if (int rc = fetch(h, st, out->corr_p3d, p.dev.corr_p3d, n_map * 3 * sizeof(float))) return rc;
      if (int rc = fetch(h, st, out->corr_p2d, p.dev.corr_p2d, n_map * 2 * sizeof(float))) return rc;
      if (int rc = fetch(h, st, out->corr_point, p.dev.corr_point, n_map * sizeof(int32_t))) return rc;
      if (int rc = fetch(h, st, out->kept_key, p.dev.kept_key, n_kept * sizeof(int32_t))) return rc;
      if (int rc = fetch(h, st, out->kept_point, p.dev.kept_point, n_kept * sizeof(int32_t))) return rc;
      if (int rc = fetch(h, st, out->removed, p.dev.removed, n_removed * sizeof(msfx_removed_point))) return rc;
    }
    if (pose) {
      const size_t n_edges = counts[0] == ft::kTracked || counts[0] == ft::kFewMapMatches ? (size_t)counts[1] : 0;
      const msf::Extent all{0, pcap, pcap, n_edges, punits, punits};
      if (int rc = fetch_result(h, st, msf::kPoseArrays, p.pdev, *pose, all)) return rc;
    }
    if (on_device) {
      keep->corr_cap = corr_cap;
      keep->d_track_status = p.dev.track_status;
      keep->d_n_kept = p.dev.n_kept, keep->d_kept_key = p.dev.kept_key, keep->d_kept_point = p.dev.kept_point;
      keep->d_n_map = p.dev.n_map, keep->d_corr_p3d = p.dev.corr_p3d, keep->d_corr_p2d = p.dev.corr_p2d;
      keep->d_corr_point = p.dev.corr_point, keep->d_outliers = p.pdev.outliers, keep->d_Tcw = p.dev.Tcw;
    }
    drain.armed = false;
    if (int rc = cs.finish()) return rc;
    if (capacity && num_matches[0] > cap_per_pair)
      return fail(h, MSF_ERR_CAPACITY, "msfx_track_frame: the list is longer than cap_per_pair; the results are those of its first cap_per_pair matches");
    return capacity ? fail(h, MSF_ERR_CAPACITY, kNoResult) : MSF_OK;
  });
}

}  // extern "C"
