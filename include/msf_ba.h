/*
 * msf_ba.h -- Optimizer::LocalBundleAdjustment and Optimizer::BundleAdjustment on the device: a Schur-complement
 * Levenberg-Marquardt over key-frame poses and map points, and the vToErase flags.
 *
 * LocalBundleAdjustment (slam_pipeline/src/Optimizer.cc:336-574; LocalMapping::Run calls it after every key frame,
 * LocalMapping.cc:60): 5 iterations with a Huber kernel over the local key frames (free), the key frames that only
 * see the local points (fixed) and the local points, a chi2 / depth classification of every edge, 10 iterations
 * without a kernel over the edges that passed, and the final flags.  BundleAdjustment (:71-215; Tracking.cc:319 on the
 * two-key-frame map, LoopClosing.cc:127): one round of nIterations.  Both are one msf_ba_params schedule of up to two
 * rounds.  Here one workgroup runs one problem and a batch of problems is one launch.  Exported from the same
 * libmsf.so; a header and a version of its own, so that MSF_ABI_VERSION, MSF_INITIALIZER_VERSION,
 * MSF_LOCAL_MAPPING_VERSION, MSF_PNP_VERSION, MSF_POSE_VERSION and the symbol lists of their headers stay what they
 * are.  Plain C; status codes, msf_last_error, threading and streams as in msf_abi.h.  Works on handles of either kind.
 *
 * What stays with the caller: the covisibility walk that collects the problem (:337-384), isBad, what it does with the
 * flags (EraseMapPointMatch / EraseObservation) and with the estimates (SetPose, SetWorldPos, UpdateNormalAndDepth;
 * mTcwGBA / mPosGBA after a loop): csrc/hip_bundle_adjustment.h.
 *
 * Arithmetic: csrc/ba_solve.h, f64 throughout on f32 inputs, shared with a host build that is tested against float64
 * numpy; its header comment restates the parts of g2o it follows and lists the defined divergences.  Every sum is taken
 * in an order fixed by the problem's own arrays: no floating-point atomics, and a problem's result depends neither on
 * the other problems of a call nor on its place in it.
 */
#ifndef MSF_BA_H
#define MSF_BA_H

#include "msf_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MSF_BA_VERSION 1
#define MSF_BA_MAX_FREE_CAMS 64  /* free cameras of one problem: S is at most 384 x 384 */
#define MSF_BA_MAX_ITERATIONS 32 /* per round */
#define MSF_BA_SLOTS 64          /* iteration slots of a problem: slot = round * 32 + iteration */

typedef struct msf_ba_params {
  uint32_t struct_size;  /* sizeof(msf_ba_params) */
  uint32_t reserved;     /* 0 */
  float fx, fy, cx, cy;  /* one set of intrinsics per problem.  Not NaN. */
  int32_t n_rounds;      /* 1 or 2 */
  int32_t iterations[2]; /* each 0..32.  LocalBundleAdjustment: {5, 10}; BundleAdjustment: {nIterations, 0} */
  int32_t robust[2];     /* 0 or 1: a Huber kernel in the round.  LocalBundleAdjustment: {1, 0} */
  double huber_delta2;   /* thHuber2D squared: 5.991 (:105 has 5.99).  > 0, finite */
  double chi2;           /* the classification threshold, 5.991.  Not NaN */
} msf_ba_params;

/* One problem of a device call: its counts and where its cameras, points and edges start in the concatenated arrays.
 * n_cams < 0: no valid problem (status -1).  The ranges of two problems must not overlap. */
typedef struct msf_ba_problem {
  int32_t n_cams, n_points, n_edges;
  int32_t cam0, point0, edge0;
} msf_ba_problem;

/* Every pointer optional except status; a null output is skipped.  msf_bundle_adjust: HOST pointers, one problem;
 * msf_bundle_adjust_device: DEVICE pointers, every per-camera / per-point / per-edge array concatenated at the
 * problems' cam0 / point0 / edge0, a problem's per-iteration block of a per-camera array at 64 * cam0 rows (per-point:
 * 64 * point0) as [64][n_cams] ([64][n_points]), the other per-iteration arrays [n_problems][64], round_iterations
 * [n_problems][2].  For a problem with status -1 nothing else is written.  For every other problem status, cam_Tcw,
 * points, outliers, cam_pose_f64, points_f64, round_iterations and it_trials are written in full; round_flags[.][r]
 * for the rounds r run; the other per-iteration arrays where it_trials is not 0.  msf_bundle_adjust writes every array
 * it is given in full: 0 where the device call would leave it alone. */
typedef struct msf_ba_result {
  uint32_t struct_size; /* sizeof(msf_ba_result) */
  uint32_t reserved;    /* 0 */
  int32_t* status;      /* per problem: -1 (invalid, malformed or more than max_free_cams free cameras) or the rounds run */
  float* cam_Tcw;       /* [cams][12]: cam_pose_f64 rounded to f32, bit for bit; a fixed camera as it came */
  float* points;        /* [points][3]: points_f64 rounded to f32 */
  uint8_t* outliers;    /* [edges]: the vToErase flags (:530-540) */
  double* cam_pose_f64; /* [cams][12]: to_homogeneous_matrix of the kept estimate, R | t; a fixed camera, and every
                           camera when no round ran, as it came */
  double* points_f64;   /* [points][3] */
  uint8_t* round_flags; /* [edges][2]: [0] chi2 > threshold or depth not positive at the estimate round 0 keeps;
                           [1] the final flag after round 1 */
  int32_t* round_iterations; /* [2]: iterations that ran */
  /* per iteration slot, [64]... */
  int32_t* it_trials;    /* trials of the iteration; 0: the iteration was not run */
  double* it_lambda_in;  /* lambda at the first trial */
  double* it_lambda_out; /* lambda after the last */
  double* it_cost_in;    /* sum(rho) over the active edges at the entry estimate */
  double* it_cost_out;   /* at the estimate the iteration keeps */
  double* it_cam_in;     /* [64][cams][7]: the estimates the iteration starts from: quaternion x y z w, t */
  double* it_point_in;   /* [64][points][3] */
  double* it_cam_out;    /* the estimates the iteration keeps */
  double* it_point_out;
  double* it_Hcc;        /* [64][cams][21]: the upper triangle of a camera's block at the entry estimate, row-major,
                            without lambda; 0 for a fixed camera */
  double* it_bc;         /* [64][cams][6] */
  double* it_Hpp;        /* [64][points][6] */
  double* it_bp;         /* [64][points][3] */
} msf_ba_result;

int msf_ba_version(void);

/* One problem, HOST pointers: cam_Tcw [n_cams][12] (rows 0..2 of Tcw, R | t row-major), cam_fixed [n_cams] (non-zero:
 * the camera is fixed), points [n_points][3], edge_cam / edge_point [n_edges] (sorted by point: edge_point is
 * non-decreasing), edge_obs [n_edges][2] (the key points' pixels), stop NULL or a host int32 (pbStopFlag) read when the
 * call starts.  MSF_ERR_INVALID_ARG for a wrong struct_size, a missing required pointer, a negative count, a parameter
 * that is NaN or outside its range, an edge index out of range or edge_point not sorted; MSF_ERR_CAPACITY for more than
 * MSF_BA_MAX_FREE_CAMS free cameras. */
int msf_bundle_adjust(msf_handle* h, int32_t n_cams, const float* cam_Tcw, const uint8_t* cam_fixed, int32_t n_points,
                      const float* points, int32_t n_edges, const int32_t* edge_cam, const int32_t* edge_point,
                      const float* edge_obs, const int32_t* stop, const msf_ba_params* params, msf_ba_result* out);

/* The same for a batch in DEVICE memory: d_problems [n_problems]; the camera, point and edge arrays hold total_cams,
 * total_points and total_edges rows and a problem reads its own ranges; edge indices are local to their problem.
 * max_free_cams (1..MSF_BA_MAX_FREE_CAMS) sizes the per-problem system: a problem with more free cameras gets
 * status -1, and so does a malformed one (an index out of range, edge_point decreasing, a negative count, a range
 * beyond the totals); no bad index is dereferenced.  d_stop: NULL or a device int32 read once before every round and at
 * the top of every iteration.  One kernel launch.  A problem's results equal bit for bit what msf_bundle_adjust returns
 * for it.  The inputs must not overlap the outputs.  Asynchronous on `stream` like the other *_device calls; one
 * stream in flight per handle (the scratch belongs to the handle). */
int msf_bundle_adjust_device(msf_handle* h, int32_t n_problems, const msf_ba_problem* d_problems, const float* d_cam_Tcw,
                             const uint8_t* d_cam_fixed, const float* d_points, const int32_t* d_edge_cam,
                             const int32_t* d_edge_point, const float* d_edge_obs, int64_t total_cams,
                             int64_t total_points, int64_t total_edges, int32_t max_free_cams, const int32_t* d_stop,
                             const msf_ba_params* params, msf_ba_result* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MSF_BA_H */
