/*
 * msf_pnp.h -- PnPsolver on the device: EPnP RANSAC, refine and inliers per relocalization candidate.
 *
 * PnPsolver (slam_pipeline/src/PnPsolver.cc, run by Tracking::Relocalization, Tracking.cc:738-864, once per candidate
 * key frame): every RANSAC iteration draws four 3-D / 2-D correspondences, solves P4P by EPnP in double precision,
 * counts the inliers over the list, and whenever a hypothesis reaches the inlier floor runs EPnP again over the
 * inliers of the best hypothesis so far (Refine, :259-300).  Here the iterations of all candidates are independent
 * solves of one launch, and a second launch refines the record-setters.  Exported from the same libmsf.so; a header
 * and a version of its own, so that MSF_ABI_VERSION, MSF_INITIALIZER_VERSION, MSF_LOCAL_MAPPING_VERSION and the symbol
 * lists of their headers stay what they are.  Plain C; status codes, msf_last_error, threading and streams as in
 * msf_abi.h.  Works on handles of either kind.
 *
 * What stays with the caller: the gather of the 3-D points (GetMapPoint2(i), isBad(), GetWorldPos(), :80-112), the
 * adjustment of SetRansacParameters (:130-165, host arithmetic: csrc/hip_pnp_solver.h) and the iterate() bookkeeping
 * over the counts and records this call returns.  (Optimizer::PoseOptimization, which Relocalization runs on this
 * call's Tcw_refined and inliers_refined: include/msf_pose.h.)
 *
 * The call is stateless: it evaluates iterations [0, n_iterations) of every list.  A RECORD is an iteration whose
 * inlier count is at least min_inliers and strictly above every earlier count of its list: exactly the iterations at
 * which the reference replaces mvbBestInliers.  The reference calls Refine() on mvbBestInliers at every iteration that
 * reaches the floor, and its result is a function of the current record alone, so refining the records is exact.
 *
 * Arithmetic: csrc/pnp_solve.h, f64 throughout on f32 points and intrinsics, shared with a host build that is tested
 * against float64 numpy; its header comment lists the defined divergences (rep_errors[N], the singular qr_solve, the
 * pseudo-inverse cut, the basis of a null space of dimension above one, the rank-2 AB').  Because a minimum set gives
 * an 8 x 12 M, the P4P pose depends on the basis the eigen-solver leaves in a 4-dimensional null space: there is no
 * hypothesis-by-hypothesis parity with another SVD, OpenCV's included; everything downstream of the returned basis
 * (ut_tail) is pinned by the tests.
 */
#ifndef MSF_PNP_H
#define MSF_PNP_H

#include "msf_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MSF_PNP_VERSION 1

typedef struct msf_pnp_params {
  uint32_t struct_size; /* sizeof(msf_pnp_params) */
  uint32_t reserved;    /* 0 */
  float fx, fy, cx, cy; /* FrameBase::fx() ... cy() of the current frame */
  float th2;            /* mvMaxError: 5.991 in Relocalization.  Not NaN. */
  int32_t min_inliers;  /* mRansacMinInliers AFTER SetRansacParameters' adjustment; >= 1 */
  int32_t n_iterations; /* iterations [0, n_iterations) of every list; 1 .. 2^20 - 1 */
  int32_t max_records;  /* room per list in the per-record arrays; >= 1 */
  uint64_t seed;        /* of the counter-based draw: (seed, list, iteration, draw) */
} msf_pnp_params;

/* Every pointer optional except n_records.  msf_pnp_ransac: HOST pointers, n_lists = 1, cap = max(n, 1);
 * msf_pnp_ransac_device: DEVICE pointers.  Nothing is written for a list without a valid result except n_records,
 * nothing in a per-record array beyond min(n_records, max_records), nothing in an inlier row beyond the list. */
typedef struct msf_pnp_result {
  uint32_t struct_size; /* sizeof(msf_pnp_result) */
  uint32_t reserved;    /* 0 */
  int32_t* n_records;   /* [n_lists]: the true number of records; -1 for a list without a valid result (d_n < 0, or
                           fewer than 4 correspondences) */
  int32_t* counts;      /* [n_lists][n_iterations]: mnInliersi of every iteration */
  /* per record, [n_lists][max_records]... */
  int32_t* iteration;       /* the iteration that set the record */
  int32_t* n_inliers;       /* its count: mnBestInliers */
  int32_t* refined_ok;      /* Refine()'s return: n_refined > min_inliers, strict */
  int32_t* n_refined;       /* mnRefinedInliers */
  float* Tcw_best;          /* [..][12]: rows 0..2 of mBestTcw, R | t rounded to f32 */
  float* Tcw_refined;       /* [..][12]: rows 0..2 of mRefinedTcw (written whether refined_ok or not) */
  uint8_t* inliers_best;    /* [..][cap]: mvbBestInliers */
  uint8_t* inliers_refined; /* [..][cap]: mvbRefinedInliers */
  /* diagnostics per hypothesis, [n_lists][n_iterations]... */
  int32_t* sets;      /* [..][4]: the minimum sets, written when they were drawn here, so any list can be replayed */
  double* pose_f64;   /* [..][12]: R | t before the rounding */
  double* cws;        /* [..][4][3]: the control points */
  double* ut_tail;    /* [..][4][12]: rows 8..11 of Ut */
  double* betas;      /* [..][3][4]: after Gauss-Newton, per candidate */
  double* rep_errors; /* [..][3] */
  double* pca;        /* [..][3][3]: the unit PCA axes behind cws, by descending eigenvalue, before c0 + k axis */
  /* the same diagnostics of each record's Refine, [n_lists][max_records]... */
  double* rec_pose_f64;
  double* rec_cws;
  double* rec_ut_tail;
  double* rec_betas;
  double* rec_rep_errors;
  double* rec_pca;
} msf_pnp_result;

int msf_pnp_version(void);

/* One list, HOST pointers: p3d [n][3] (mvP3Dw), p2d [n][2] (mvP2D), sets [n_iterations][4] indices into the list or
 * NULL to draw them.  A given set with an index outside [0, n) yields a NaN pose and 0 inliers.  n < 4 is no error
 * (n_records = -1).  MSF_ERR_INVALID_ARG for a wrong struct_size, a missing required pointer, a negative length, a NaN
 * th2 or a parameter outside its range; MSF_ERR_CAPACITY when the list has more than max_records records: the first
 * max_records are complete and n_records holds the true number. */
int msf_pnp_ransac(msf_handle* h, int32_t n, const float* p3d, const float* p2d, const msf_pnp_params* params,
                   const int32_t* sets, msf_pnp_result* out);

/* The same for a batch in DEVICE memory: list l is d_p3d + l * cap * 3, d_p2d + l * cap * 2, its length
 * min(d_n[l], cap); d_n[l] < 0 or a length below 4 gives n_records[l] = -1.  d_sets [n_lists][n_iterations][4] or NULL.
 * Two kernel launches ordered by the stream.  A list's results do not depend on the other lists of the call and equal
 * bit for bit what msf_pnp_ransac returns for that list with the returned sets (the draw is keyed by the list's index
 * in the call).  MSF_ERR_CAPACITY cannot be seen without reading device memory: compare n_records with max_records.
 * n_lists <= 65535 and n_lists * n_iterations <= 2^32 (MSF_ERR_INVALID_ARG beyond).  Asynchronous on `stream` like the other *_device calls; one stream in flight per handle. */
int msf_pnp_ransac_device(msf_handle* h, int32_t n_lists, const float* d_p3d, const float* d_p2d, int32_t cap,
                          const int32_t* d_n, const msf_pnp_params* params, const int32_t* d_sets, msf_pnp_result* out,
                          void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MSF_PNP_H */
