// extern "C" boundary of libmsf.so, pose optimisation: msf_pose_optimize*
// (declarations: include/msf_pose.h; what the files of the boundary share, this family's launch included: abi_core.h).
#include "abi_core.h"

#include <cmath>

#include "msf_pose.h"
#include "pose_pipeline.h"

using namespace msf::abi;

extern "C" {

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
    msf_pose_result dev{};
    PosePlan p;
    if (int rc = carve(h, h->d_pose, (size_t)1 << 16, "hipMalloc(pose workspace)", [&](msf::Carver& c) {
          p.base = c.base;
          p.p3d = c.take<float>(cap * 3);
          p.p2d = c.take<float>(cap * 2);
          p.tcw0 = c.take<float>(12);
          p.mask = mask ? c.take<uint8_t>(cap) : nullptr;
          msf::carve_result(c, msf::kPoseArrays, kPoseUnits, cap, nullptr, *out, &dev);
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
    HIP_TRY(h, "pose_optimize", msf::pose_optimize(1, in, pose_params(*params), to_out(dev), st));
    const msf::Extent all{0, cap, cap, count, kPoseUnits, kPoseUnits};
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
    HIP_TRY(h, "pose_optimize", msf::pose_optimize(n_lists, in, pose_params(*params), to_out(*out), cs.st));
    return cs.finish();
  });
}

}  // extern "C"
