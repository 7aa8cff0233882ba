/*
 * msf_global_ba.h -- Optimizer::GlobalBundleAdjustemnt on the device: BundleAdjustment over the whole map, one problem
 * spread over every compute unit.
 *
 * GlobalBundleAdjustemnt (slam_pipeline/src/Optimizer.cc:62-69) is what LoopClosing::RunGlobalBundleAdjustment
 * (LoopClosing.cc:122-127) runs after a loop: BundleAdjustment (:71-215) with every key frame but the first one free.
 * msf_bundle_adjust (msf_ba.h) runs one problem in one workgroup and stops at MSF_BA_MAX_FREE_CAMS = 64 free cameras.
 * The calls here take one problem of up to MSF_GBA_MAX_FREE_CAMS free cameras and run it as a sequence of launches,
 * each over the whole device: the per-edge, per-point and per-camera phases one thread per index, the Schur complement
 * one thread per (row, camera block), the dense Cholesky of S by tiles of msf_global_ba_tile_rows() rows staged in LDS,
 * the tiles of a column spread over the grid.  The host drives the Levenberg-Marquardt loop: after every trial it reads
 * a small record (the costs, the gain's denominators, whether a block or a pivot failed, the stop word) and decides.
 *
 * Same contract as msf_bundle_adjust: the same arguments, msf_ba_params as the schedule (the reference's call is
 * {1, {10, 0}, {0, 0}}; two rounds work too), msf_ba_result with the shapes of one problem ([64], [64][n_cams], ...),
 * the same statuses and refusals.  Arithmetic: csrc/gba_solve.h over csrc/ba_solve.h; every sum in the order ba_solve.h
 * fixes, no fused multiply-add, no matrix instruction, no floating-point atomics, sin / cos of a pose update in plain
 * multiplies and adds.  So the result equals, bit for bit and in every array, what the host build of ba_solve.h gives,
 * and for at most 64 free cameras what msf_bundle_adjust gives.
 *
 * Exported from the same libmsf.so; a header and a version of its own, so that msf_ba.h, MSF_BA_VERSION, the five
 * earlier versions and every earlier symbol list stay what they are.  Plain C; status codes, msf_last_error and
 * threading as in msf_abi.h.  Works on handles of either kind.
 */
#ifndef MSF_GLOBAL_BA_H
#define MSF_GLOBAL_BA_H

#include "msf_ba.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MSF_GLOBAL_BA_VERSION 1
#define MSF_GBA_MAX_FREE_CAMS 1024 /* free cameras of the problem: S is at most 6144 x 6145 f64, about 302 MB */

int msf_global_ba_version(void);

/* the tile edge of the device Cholesky, for tests and tools */
int msf_global_ba_tile_rows(void);

/* One problem, HOST pointers; arguments and results as msf_bundle_adjust.  stop: NULL or a host int32 (pbStopFlag) that
 * another thread may set while the call runs: it is read before every round and at the top of every iteration.
 * MSF_ERR_INVALID_ARG as msf_bundle_adjust; MSF_ERR_CAPACITY for more than MSF_GBA_MAX_FREE_CAMS free cameras.  The
 * workspace is sized by the problem's own free cameras. */
int msf_global_bundle_adjust(msf_handle* h, int32_t n_cams, const float* cam_Tcw, const uint8_t* cam_fixed,
                             int32_t n_points, const float* points, int32_t n_edges, const int32_t* edge_cam,
                             const int32_t* edge_point, const float* edge_obs, const volatile int32_t* stop,
                             const msf_ba_params* params, msf_ba_result* out);

/* The same with the problem and the results in DEVICE memory (out: device pointers, shaped as for one problem of
 * msf_bundle_adjust_device).  max_free_cams (1..MSF_GBA_MAX_FREE_CAMS) bounds the workspace: a problem with more free
 * cameras gets status -1, nothing else is written and the call returns MSF_ERR_CAPACITY; a malformed one (an edge index
 * out of range, edge_point decreasing) gets status -1 and nothing else, and the call returns MSF_OK as
 * msf_bundle_adjust_device does.  A checking launch passes every index and counts the free cameras, and the host reads its
 * verdict, before anything is dereferenced or sized by them; the workspace then takes the size of the counted free
 * cameras.  d_stop: NULL or a device int32; it is read on the device before every round and with every record, so the
 * host sees it once per trial.  The work is enqueued on `stream` (NULL: the handle's), but the host decides every trial:
 * THE CALL RETURNS ONLY WHEN THE PROBLEM IS FINISHED.  It is the one *_device call that is not asynchronous.  The
 * inputs must not overlap the outputs (d_stop alone may be a word the call writes: it is read in stream order); one
 * call in flight per handle (the workspace belongs to the handle). */
int msf_global_bundle_adjust_device(msf_handle* h, int32_t n_cams, const float* d_cam_Tcw, const uint8_t* d_cam_fixed,
                                    int32_t n_points, const float* d_points, int32_t n_edges, const int32_t* d_edge_cam,
                                    const int32_t* d_edge_point, const float* d_edge_obs, int32_t max_free_cams,
                                    const int32_t* d_stop, const msf_ba_params* params, msf_ba_result* out,
                                    void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MSF_GLOBAL_BA_H */
