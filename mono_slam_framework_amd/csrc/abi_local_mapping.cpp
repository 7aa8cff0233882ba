// extern "C" boundary of libmsf.so, local mapping: msf_new_points*, msf_create_map_points
// (declarations: include/msf_local_mapping.h; what the files of the boundary share: abi_core.h).
#include "abi_core.h"

#include <cmath>

#include "msf_local_mapping.h"
#include "triangulate_pipeline.h"

using namespace msf::abi;

namespace {

msf::NewPointOut to_out(const msf_new_points_result& r) {
  return msf::NewPointOut{r.n_new, r.packed, r.status, r.points, r.hom, r.cos_parallax};
}

msf::NewPointParams new_point_params(const msf_new_points_params* prm) {
  return msf::NewPointParams{prm->max_cos_parallax, prm->chi2};
}

}  // namespace

extern "C" {

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

}  // extern "C"
