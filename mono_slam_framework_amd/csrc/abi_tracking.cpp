// extern "C" boundary of libmsf.so, SearchLocalPoints: msf_frustum*, msf_claim_points_device, msf_search_local_points
// (declarations: include/msf_tracking.h; what the files of the boundary share: abi_core.h).
#include "abi_core.h"

#include <cstring>

#include "msf_tracking.h"
#include "tracking_arrays.h"
#include "tracking_pipeline.h"

using namespace msf::abi;

extern "C" {

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

}  // extern "C"
