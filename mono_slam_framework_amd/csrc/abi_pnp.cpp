// extern "C" boundary of libmsf.so, the PnP solver: msf_pnp_ransac*
// (declarations: include/msf_pnp.h; what the files of the boundary share: abi_core.h).
#include "abi_core.h"

#include <cmath>

#include "msf_pnp.h"
#include "pnp_pipeline.h"

using namespace msf::abi;

namespace {

msf::PnpOut to_out(const msf_pnp_result& r) {
  return msf::PnpOut{r.n_records, r.counts, r.iteration, r.n_inliers, r.refined_ok, r.n_refined, r.Tcw_best, r.Tcw_refined,
                     r.inliers_best, r.inliers_refined, r.sets, r.pose_f64, r.cws, r.ut_tail, r.betas, r.rep_errors,
                     r.pca, r.rec_pose_f64, r.rec_cws, r.rec_ut_tail, r.rec_betas, r.rec_rep_errors, r.rec_pca};
}

}  // namespace

extern "C" {

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

}  // extern "C"
