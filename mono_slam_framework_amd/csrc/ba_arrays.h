// The arrays of msf_ba_result as a table of result_arrays.h, for the one-problem host call: carve_result() gives them
// their pieces of the workspace and copy_result() moves them back.  The row model fits a single problem -- every array
// is [1][rows of its unit] -- with the units below; a batch concatenates problems of different sizes, which the model
// does not express, and the device call takes the caller's pointers as they are.  mono_slam_framework_amd/_lib.py
// holds the same table (BA_ARRAYS) and tests/test_ba_arrays_host.py compares the two.  No HIP in here.
#pragma once
#include "msf_ba.h"
#include "result_arrays.h"

namespace msf {

// unit counts of a bundle-adjustment call: {1, n_cams, n_points, n_edges, 2, 64, 64 * n_cams, 64 * n_points}
enum { kBaCam = 1, kBaPoint = 2, kBaEdge = 3, kBaRound = 4, kBaSlot = 5, kBaSlotCam = 6, kBaSlotPoint = 7, kBaUnits = 8 };
constexpr ResultArray kBaArrays[] = {
    MSF_RESULT_ROW(msf_ba_result, status, kPerList, 1, false, true),
    MSF_RESULT_ROW(msf_ba_result, cam_Tcw, kBaCam, 12, false, false),
    MSF_RESULT_ROW(msf_ba_result, points, kBaPoint, 3, false, false),
    MSF_RESULT_ROW(msf_ba_result, outliers, kBaEdge, 1, false, false),
    MSF_RESULT_ROW(msf_ba_result, cam_pose_f64, kBaCam, 12, false, false),
    MSF_RESULT_ROW(msf_ba_result, points_f64, kBaPoint, 3, false, false),
    MSF_RESULT_ROW(msf_ba_result, round_flags, kBaEdge, 2, false, false),
    MSF_RESULT_ROW(msf_ba_result, round_iterations, kBaRound, 1, false, false),
    MSF_RESULT_ROW(msf_ba_result, it_trials, kBaSlot, 1, false, false),
    MSF_RESULT_ROW(msf_ba_result, it_lambda_in, kBaSlot, 1, false, false),
    MSF_RESULT_ROW(msf_ba_result, it_lambda_out, kBaSlot, 1, false, false),
    MSF_RESULT_ROW(msf_ba_result, it_cost_in, kBaSlot, 1, false, false),
    MSF_RESULT_ROW(msf_ba_result, it_cost_out, kBaSlot, 1, false, false),
    MSF_RESULT_ROW(msf_ba_result, it_cam_in, kBaSlotCam, 7, false, false),
    MSF_RESULT_ROW(msf_ba_result, it_point_in, kBaSlotPoint, 3, false, false),
    MSF_RESULT_ROW(msf_ba_result, it_cam_out, kBaSlotCam, 7, false, false),
    MSF_RESULT_ROW(msf_ba_result, it_point_out, kBaSlotPoint, 3, false, false),
    MSF_RESULT_ROW(msf_ba_result, it_Hcc, kBaSlotCam, 21, false, false),
    MSF_RESULT_ROW(msf_ba_result, it_bc, kBaSlotCam, 6, false, false),
    MSF_RESULT_ROW(msf_ba_result, it_Hpp, kBaSlotPoint, 6, false, false),
    MSF_RESULT_ROW(msf_ba_result, it_bp, kBaSlotPoint, 3, false, false),
};
static_assert(covers<msf_ba_result>(kBaArrays), "one row per pointer of msf_ba_result, in its order");

// the unit counts of one problem
inline void ba_units(size_t n_cams, size_t n_points, size_t n_edges, size_t* units) {
  units[kPerList] = 1, units[kBaCam] = n_cams, units[kBaPoint] = n_points, units[kBaEdge] = n_edges;
  units[kBaRound] = 2, units[kBaSlot] = MSF_BA_SLOTS;
  units[kBaSlotCam] = MSF_BA_SLOTS * n_cams, units[kBaSlotPoint] = MSF_BA_SLOTS * n_points;
}

}  // namespace msf
