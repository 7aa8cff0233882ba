// What every file of the extern "C" boundary of libmsf.so shares -- msf_abi.cpp and one abi_<family>.cpp per family of
// entry points: the handle, the entry scaffold, the workspace carver, the copy-back, and the few pieces of the matcher
// and of the pose optimiser that more than one family calls.  A family is a workspace member of the handle, and gets a
// file.  The non-template functions declared here are defined once, in msf_abi.cpp.
#ifndef MSF_ABI_CORE_H
#define MSF_ABI_CORE_H

#include "msf_abi.h"

#include <hip/hip_runtime.h>

#include <mutex>
#include <string>
#include <vector>

#include "carve.h"
#include "dev_buf.h"
#include "loftr_pipeline.h"
#include "msf_pose.h"
#include "orb_pipeline.h"
#include "pose_pipeline.h"
#include "result_arrays.h"

namespace msf {
namespace gba {
struct Record;   // gba_solve.h: the handle keeps a pointer to the pinned one, nothing more
}
}  // namespace msf

using msf::DevBuf;   // dev_buf.h: the handle's device blocks go with their members

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

namespace msf {
namespace abi {

// The error text of the calls that have no handle to keep it (msf_create, the weight tools), read by
// msf_last_error(NULL): one object per thread whichever file fails.
extern thread_local std::string g_create_error;

int fail(msf_handle* h, int code, const std::string& msg);
int hip_fail(msf_handle* h, const char* what, hipError_t e);

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
int host_exception(msf_handle* h, const char* where) noexcept;

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
int fetch(msf_handle* h, hipStream_t st, void* dst, const void* src, size_t bytes);

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
// Here the pose optimiser's, which msf_pose.h and msf_frame_tracking.h both launch; the others are with their families.
inline msf::PoseOut to_out(const msf_pose_result& r) {
  return msf::PoseOut{r.n_good, r.Tcw, r.outliers, r.n_edges, r.rounds_run, r.pose_f64, r.round_pose_f64, r.round_n_bad,
                      r.round_iterations, r.it_trials, r.it_lambda_in, r.it_lambda_out, r.it_cost_in, r.it_cost_out,
                      r.it_H, r.it_b, r.it_pose_out};
}

inline msf::PoseParams pose_params(const msf_pose_params& p) {
  return msf::PoseParams{p.fx, p.fy, p.cx, p.cy, p.chi2};
}

// the units of kPoseArrays (result_arrays.h) for one list: the list, its rounds, its iterations
inline constexpr size_t kPoseUnits[] = {1, msf::kPoseRounds, msf::kPoseIterations};

extern const char* const kNoResult;   // the text of MSF_ERR_CAPACITY for a pair without a list (n_out = -1)

template <class... V>
bool aligned16(V... v) {   // pointers and strides alike
  return ((... | (uintptr_t)v) & 15) == 0;
}

// The matcher as the one-vs-many entry points of the other families call it (msf_create_map_points,
// msf_search_local_points, msfx_track_frame); what each does stands with its body in msf_abi.cpp.
int match_slot_pairs(msf_handle* h, int n, const int32_t* d_a, const int32_t* d_b, msf_match* d_out, int cap,
                     int32_t* d_n_out, hipStream_t st, int slot_limit);
int deliverable(const msf_handle* h, int32_t c, int32_t cap, bool* capacity);
int one_to_many_args(msf_handle* h, const char* name, int32_t query_slot, int32_t n, const int32_t* slots);
int launch_one_to_many(msf_handle* h, int32_t query_slot, int32_t n, const int32_t* slots, hipStream_t st);

}  // namespace abi
}  // namespace msf

#endif
