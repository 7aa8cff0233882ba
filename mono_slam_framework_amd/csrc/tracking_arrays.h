// The arrays of msf_frustum_result and msf_claim_result as tables of result_arrays.h, for the host calls of
// include/msf_tracking.h: carve_result() gives them their pieces of the workspace and copy_result() moves them back.  One
// call is one "list"; the units below are the call's own counts.  mono_slam_framework_amd/_lib.py holds the same tables
// (FRUSTUM_ARRAYS, CLAIM_ARRAYS) and tests/test_tracking_arrays_host.py compares the two.  No HIP in here.
#pragma once
#include "msf_tracking.h"
#include "result_arrays.h"

namespace msf {

// unit counts of a frustum call: {1, n_points, n_kf}
enum { kTrPoint = 1, kTrKf = 2, kTrUnits = 3 };
constexpr ResultArray kFrustumArrays[] = {
    MSF_RESULT_ROW(msf_frustum_result, status_word, kPerList, 1, false, true),
    MSF_RESULT_ROW(msf_frustum_result, n_to_match, kTrKf, 1, false, true),
    MSF_RESULT_ROW(msf_frustum_result, status, kTrPoint, 1, false, false),
    MSF_RESULT_ROW(msf_frustum_result, visible, kTrPoint, 1, false, false),
    MSF_RESULT_ROW(msf_frustum_result, owner_kf, kTrPoint, 1, false, false),
    MSF_RESULT_ROW(msf_frustum_result, u, kTrPoint, 1, false, false),
    MSF_RESULT_ROW(msf_frustum_result, v, kTrPoint, 1, false, false),
    MSF_RESULT_ROW(msf_frustum_result, dist, kTrPoint, 1, false, false),
    MSF_RESULT_ROW(msf_frustum_result, view_cos, kTrPoint, 1, false, false),
};
static_assert(covers<msf_frustum_result>(kFrustumArrays), "one row per pointer of msf_frustum_result, in its order");

// unit counts of a claim call: {1, n_kf, corr_cap}; cap = the lists' stride.  `claims` is [n_kf * cap] records packed
// from its start: a per-cap row per key frame as far as its room goes.
enum { kClKf = 1, kClCorr = 2, kClUnits = 3 };
constexpr ResultArray kClaimArrays[] = {
    MSF_RESULT_ROW(msf_claim_result, status_word, kPerList, 1, false, true),
    MSF_RESULT_ROW(msf_claim_result, n_claims, kPerList, 1, false, true),
    MSF_RESULT_ROW(msf_claim_result, n_claimed, kClKf, 1, false, true),
    MSF_RESULT_ROW(msf_claim_result, claims, kClKf, 1, true, false),
    MSF_RESULT_ROW(msf_claim_result, claim_status, kClKf, 1, true, false),
    MSF_RESULT_ROW(msf_claim_result, n_corr, kPerList, 1, false, false),
    MSF_RESULT_ROW(msf_claim_result, corr_p3d, kClCorr, 3, false, false),
    MSF_RESULT_ROW(msf_claim_result, corr_p2d, kClCorr, 2, false, false),
    MSF_RESULT_ROW(msf_claim_result, corr_point, kClCorr, 1, false, false),
};
static_assert(covers<msf_claim_result>(kClaimArrays), "one row per pointer of msf_claim_result, in its order");

}  // namespace msf
