// The arrays of msfx_track_result as a table of result_arrays.h, for the calls of include/msf_frame_tracking.h:
// carve_result() gives them their pieces of the workspace and copy_result() moves them back.  One call is one "list";
// the units below are the call's own counts.  mono_slam_framework_amd/_lib.py holds the same table (TRACK_ARRAYS) and
// tests/test_frame_tracking_arrays_host.py compares the two.  No HIP in here.
#pragma once
#include "msf_frame_tracking.h"
#include "result_arrays.h"

namespace msf {

// unit counts of a call: {1, cap (the match list's), n_cur, corr_cap}.  Every array is needed by a later launch of the
// call or by `keep`, so every row is required: what the caller does not ask for lives in the workspace.
enum { kFtMatch = 1, kFtCur = 2, kFtCorr = 3, kFtUnits = 4 };
constexpr ResultArray kTrackArrays[] = {
    MSF_RESULT_ROW(msfx_track_result, track_status, kPerList, 1, false, true),
    MSF_RESULT_ROW(msfx_track_result, n_map, kPerList, 1, false, true),
    MSF_RESULT_ROW(msfx_track_result, map, kFtCorr, 1, false, true),
    MSF_RESULT_ROW(msfx_track_result, carry_status, kFtMatch, 1, false, true),
    MSF_RESULT_ROW(msfx_track_result, cur_status, kFtCur, 1, false, true),
    MSF_RESULT_ROW(msfx_track_result, corr_p3d, kFtCorr, 3, false, true),
    MSF_RESULT_ROW(msfx_track_result, corr_p2d, kFtCorr, 2, false, true),
    MSF_RESULT_ROW(msfx_track_result, corr_point, kFtCorr, 1, false, true),
    MSF_RESULT_ROW(msfx_track_result, Tcw, kPerList, 12, false, true),
    MSF_RESULT_ROW(msfx_track_result, n_good, kPerList, 1, false, true),
    MSF_RESULT_ROW(msfx_track_result, n_kept, kPerList, 1, false, true),
    MSF_RESULT_ROW(msfx_track_result, kept_key, kFtCorr, 1, false, true),
    MSF_RESULT_ROW(msfx_track_result, kept_point, kFtCorr, 1, false, true),
    MSF_RESULT_ROW(msfx_track_result, n_removed, kPerList, 1, false, true),
    MSF_RESULT_ROW(msfx_track_result, removed, kFtCorr, 1, false, true),
    MSF_RESULT_ROW(msfx_track_result, n_matches_map, kPerList, 1, false, true),
};
static_assert(covers<msfx_track_result>(kTrackArrays), "one row per pointer of msfx_track_result, in its order");

}  // namespace msf
