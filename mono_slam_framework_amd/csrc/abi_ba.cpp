// extern "C" boundary of libmsf.so, bundle adjustment: msf_bundle_adjust*, msf_global_bundle_adjust*
// (declarations: include/msf_ba.h and include/msf_global_ba.h; what the files of the boundary share: abi_core.h).
#include "abi_core.h"

#include <cmath>

#include "ba_arrays.h"
#include "ba_pipeline.h"
#include "gba_pipeline.h"
#include "msf_ba.h"
#include "msf_global_ba.h"

using namespace msf::abi;

extern "C" {

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

}  // extern "C"
