/*
 * msf_pose.h -- Optimizer::PoseOptimization on the device: Huber Levenberg-Marquardt rounds and outlier flags.
 *
 * PoseOptimization (slam_pipeline/src/Optimizer.cc:217-334; called by Tracking.cc:402, :463 and :496 on every tracked
 * frame and by :827 once per relocalization candidate, on the output of PnPsolver): a pose-only optimisation over the
 * 3-D / 2-D correspondences of a frame.  Four rounds, each restarting from the entry pose and running g2o's
 * Levenberg-Marquardt for at most 10 iterations over the correspondences the previous round did not flag, rounds 0..2
 * with a Huber kernel; after each round every correspondence is re-flagged by chi2 > 5.991.  Here one wave runs one
 * list, and a batch of lists (the candidates of one Relocalization) is one launch.  Exported from the same libmsf.so;
 * a header and a version of its own, so that MSF_ABI_VERSION, MSF_INITIALIZER_VERSION, MSF_LOCAL_MAPPING_VERSION,
 * MSF_PNP_VERSION and the symbol lists of their headers stay what they are.  Plain C; status codes, msf_last_error,
 * threading and streams as in msf_abi.h.  Works on handles of either kind.
 *
 * What stays with the caller: the gather of the 3-D points (mKeyPointMap, GetWorldPos(), :247-283) and what it does
 * with the flags (SetOutlier, :312-316) and the pose (SetPose, :331): csrc/hip_optimizer.h.
 *
 * Arithmetic: csrc/pose_solve.h, f64 throughout on f32 points, pixels, intrinsics and entry pose, shared with a host
 * build that is tested against float64 numpy; its header comment restates the parts of g2o it follows and lists the
 * defined divergences (every correspondence classified at the kept estimate, a failed solve rejects the trial, a NaN
 * chi2 is no outlier, every loop bounded).
 */
#ifndef MSF_POSE_H
#define MSF_POSE_H

#include "msf_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MSF_POSE_VERSION 1

typedef struct msf_pose_params {
  uint32_t struct_size; /* sizeof(msf_pose_params) */
  uint32_t reserved;    /* 0 */
  float fx, fy, cx, cy; /* FrameBase::fx() ... cy() of the frame */
  float chi2;           /* chi2Mono: 5.991f.  Not NaN. */
} msf_pose_params;

/* Every pointer optional except n_good.  msf_pose_optimize: HOST pointers, n_lists = 1, cap = max(n, 1);
 * msf_pose_optimize_device: DEVICE pointers.  An EDGE is a correspondence inside the list that the mask lets in.
 * For a list without a valid result (d_n < 0) nothing is written except n_good = -1.  For every other list n_good,
 * Tcw, n_edges, rounds_run, pose_f64, round_n_bad, round_iterations and it_trials are written in full; outliers only
 * at the edges; the other per-round arrays for rounds [0, rounds_run) and the other per-iteration arrays where
 * it_trials is not 0.  msf_pose_optimize writes every array it is given in full: 0 where the device call would leave
 * it alone, and an outlier byte outside the mask as the caller had it. */
typedef struct msf_pose_result {
  uint32_t struct_size; /* sizeof(msf_pose_result) */
  uint32_t reserved;    /* 0 */
  int32_t* n_good;      /* [n_lists]: nInitialCorrespondences - nBad of the last round run; 0 with fewer than 3 edges */
  float* Tcw;           /* [n_lists][12]: rows 0..2 of the optimised pose, pose_f64 rounded to f32; with fewer than 3
                           edges Tcw0 as it came */
  uint8_t* outliers;    /* [n_lists][cap]: 1 where the last round run flagged the edge, else 0 */
  int32_t* n_edges;     /* [n_lists]: nInitialCorrespondences */
  int32_t* rounds_run;  /* [n_lists]: 0 (fewer than 3 edges), 1 (fewer than 10) or 4 */
  double* pose_f64;     /* [n_lists][12]: to_homogeneous_matrix of the last round's estimate, R | t */
  /* per round, [n_lists][4]... */
  double* round_pose_f64;    /* [..][12] */
  int32_t* round_n_bad;      /* nBad */
  int32_t* round_iterations; /* iterations of optimize(10) that ran */
  /* per iteration, [n_lists][4][10]... */
  int32_t* it_trials;    /* trials of the iteration; 0: the iteration was not run */
  double* it_lambda_in;  /* lambda at the first trial */
  double* it_lambda_out; /* lambda after the last */
  double* it_cost_in;    /* sum(rho) at the entry estimate */
  double* it_cost_out;   /* at the estimate the iteration keeps */
  double* it_H;          /* [..][21]: the upper triangle of H at the entry estimate, row-major, without lambda */
  double* it_b;          /* [..][6] */
  double* it_pose_out;   /* [..][7]: the estimate the iteration keeps: quaternion x y z w, t */
} msf_pose_result;

int msf_pose_version(void);

/* One list, HOST pointers: p3d [n][3] (GetWorldPos()), p2d [n][2] (the key points' integer pixels as floats), Tcw0 [12]
 * (rows 0..2 of mTcw, R | t row-major), mask [n] or NULL (non-zero: the correspondence is an edge).  n < 3 is no error
 * (n_good = 0).  MSF_ERR_INVALID_ARG for a wrong struct_size, a missing required pointer, a negative length or a NaN
 * chi2. */
int msf_pose_optimize(msf_handle* h, int32_t n, const float* p3d, const float* p2d, const float* Tcw0,
                      const uint8_t* mask, const msf_pose_params* params, msf_pose_result* out);

/* The same for a batch in DEVICE memory: list l is d_p3d + l * cap * 3, d_p2d + l * cap * 2, its length
 * min(d_n[l], cap); d_n[l] < 0 gives n_good[l] = -1.  Its entry pose is the 12 floats at d_Tcw0 + l * Tcw0_stride
 * (a stride in ELEMENTS, >= 0) and its mask the bytes at d_mask + l * mask_stride (a stride in BYTES, >= 0; d_mask NULL:
 * every correspondence is an edge): a caller can point them at Tcw_refined / inliers_refined of an msf_pnp_result
 * (strides max_records * 12 and max_records * cap) without a copy.  The inputs must not overlap the outputs.  One
 * kernel launch.  A list's results do not depend on the other lists of the call or on its row, and equal bit for bit
 * what msf_pose_optimize returns for that list.  n_lists <= 2^31 - 1.  Asynchronous on `stream` like the other
 * *_device calls; one stream in flight per handle. */
int msf_pose_optimize_device(msf_handle* h, int32_t n_lists, const float* d_p3d, const float* d_p2d, int32_t cap,
                             const int32_t* d_n, const float* d_Tcw0, int64_t Tcw0_stride, const uint8_t* d_mask,
                             int64_t mask_stride, const msf_pose_params* params, msf_pose_result* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MSF_POSE_H */
