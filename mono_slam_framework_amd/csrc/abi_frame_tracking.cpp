// extern "C" boundary of libmsf.so, frame-to-frame tracking: msfx_carry_points_device, msfx_track_list_device,
// msfx_track_frame (declarations: include/msf_frame_tracking.h; what the files of the boundary share: abi_core.h).
#include "abi_core.h"

#include <cmath>
#include <cstring>

#include "frame_tracking_arrays.h"
#include "frame_tracking_pipeline.h"
#include "msf_frame_tracking.h"

using namespace msf::abi;

extern "C" {

namespace {

namespace ft = msf::ftrack;
namespace tk = msf::tracking;   // the map points are SearchLocalPoints' (tracking_solve.h, through frame_tracking_solve.h)

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
  msf::carve_result(c, msf::kPoseArrays, kPoseUnits, pcap, pose_given, pose_wanted, &p->pdev);
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
  HIP_TRY(h, "pose_optimize", msf::pose_optimize(1, lists, pose_params(prm.pose), to_out(p.pdev), st));
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
      const msf::Extent all{0, pcap, pcap, n_edges, kPoseUnits, kPoseUnits};
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
