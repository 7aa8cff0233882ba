/*
 * msf_local_mapping.h -- LocalMapping::CreateNewMapPoints on the device: match neighbours, triangulate points.
 *
 * The loop of LocalMapping::CreateNewMapPoints (slam_pipeline/src/LocalMapping.cc:161-282): the current key frame is
 * matched against its covisible neighbours, and every match is triangulated from the two key-frame poses and kept as a
 * new map point when it passes the ray-parallax test, both depth signs and both reprojection errors (:195-265).  Here
 * the per-match body runs as one kernel directly behind the matcher, on the lists as the matcher left them in device
 * memory.  Exported from the same libmsf.so; a header and a version of its own, so that MSF_ABI_VERSION,
 * MSF_INITIALIZER_VERSION and the symbol lists of msf_abi.h / msf_initializer.h stay what they are.  Plain C; status
 * codes, msf_last_error, threading and streams as in msf_abi.h.  Works on handles of either kind.
 *
 * What stays with the caller: the baseline / median-depth gate (:166-174, it needs the map: a neighbour it drops is
 * simply left out of `slots`), and everything behind an accepted point (MapPoint, AddObservation, UpdateNormalAndDepth).
 *
 * Arithmetic (csrc/triangulate_solve.h, shared with a host build that is tested against float64), stage by stage in the
 * reference's order and in the types its expressions have: key points, normalised coordinates, rays and the 4 x 4
 * matrix in f32; cosParallaxRays in f64 on the f32 rays (Mat::dot and cv::norm return double); the null vector by the
 * f32 one-sided Jacobi of msf_initializer.h (within 16 eps s1 / (s3 - s4) of a float64 SVD, defined up to sign -- the
 * division by the fourth entry removes the sign); depths and reprojection errors in f64 on the f32 point.
 *
 * Per-match status: 0 = a new map point, else the stage that rejected it:
 *   1  !(cos > 0)                 (a NaN cosine lands here, as the reference's `else continue`)
 *   2  !(cos < max_cos_parallax)  LocalMapping::mMinParallax, compared with the COSINE exactly as the reference does.
 *                                 SlamParameters sets it to 1.1, so by default this stage rejects nothing: the quirk is
 *                                 kept literal and the value is a parameter.
 *   3  hom[3] == 0 (:224), or a non-finite point.  The second is a defined divergence: the reference's comparisons let
 *      a NaN point through every later check and would store it; here it is rejected, as msf_reconstruct does.
 *   4  z1 <= 0      5  z2 <= 0
 *   6  errX1^2 + errY1^2 > chi2      7  errX2^2 + errY2^2 > chi2      (chi2: 5.991 in the reference)
 * A match is judged exactly as by a float64 SVD of the same matrix unless it lies at one of these thresholds.
 */
#ifndef MSF_LOCAL_MAPPING_H
#define MSF_LOCAL_MAPPING_H

#include "msf_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MSF_LOCAL_MAPPING_VERSION 1

/* A key frame's pose and intrinsics: GetRotation(), GetTranslation(), fx() ... cy().  64 bytes. */
typedef struct msf_view {
  float Rcw[9]; /* row-major */
  float tcw[3];
  float fx, fy, cx, cy;
} msf_view;

/* One accepted match: its index in the list and x3D.  16 bytes. */
typedef struct msf_new_point {
  int32_t match;
  float x, y, z;
} msf_new_point;

typedef struct msf_new_points_params {
  uint32_t struct_size;    /* sizeof(msf_new_points_params) */
  uint32_t reserved;       /* 0 */
  double max_cos_parallax; /* mMinParallax; 1.1 in SlamParameters.  Not NaN. */
  double chi2;             /* 5.991.  Not NaN. */
} msf_new_points_params;

/* Every pointer optional except n_new.  msf_new_points / msf_create_map_points: HOST pointers; msf_new_points_device:
 * DEVICE pointers.  cap = n_matches (msf_new_points) or cap_per_pair. */
typedef struct msf_new_points_result {
  uint32_t struct_size;  /* sizeof(msf_new_points_result) */
  uint32_t reserved;     /* 0 */
  int32_t* n_new;        /* [n_lists]: accepted matches; -1 for a list without a valid result (n_out < 0) */
  msf_new_point* packed; /* [n_lists][cap]: the first n_new records, in match order -- the order in which the
                            reference creates its map points; untouched beyond */
  uint8_t* status;       /* [n_lists][cap]: 0 or the rejecting stage 1..7; untouched beyond the list */
  float* points;         /* [n_lists][cap][3]: x3D, zero where status != 0; untouched beyond the list */
  float* hom;            /* [n_lists][cap][4] diagnostics: the null vector before the division (zero for status 1, 2) */
  double* cos_parallax;  /* [n_lists][cap] diagnostics: cosParallaxRays */
} msf_new_points_result;

int msf_local_mapping_version(void);

/* The loop body of CreateNewMapPoints for one list, HOST pointers: view1 belongs to (x1, y1), view2 to (x2, y2).
 * n_matches == 0 is no error (n_new = 0).  MSF_ERR_INVALID_ARG for a wrong struct_size, a missing required pointer, a
 * negative length, a NaN max_cos_parallax / chi2. */
int msf_new_points(msf_handle* h, int32_t n_matches, const msf_match* matches, const msf_view* view1,
                   const msf_view* view2, const msf_new_points_params* params, msf_new_points_result* out);

/* The same for a batch in DEVICE memory: d_matches / cap_per_pair / d_n_out as msf_match_batch_device or
 * msf_match_slots_device left them (list l: d_matches + l * cap_per_pair, length min(d_n_out[l], cap_per_pair); a
 * negative d_n_out[l] gives n_new[l] = -1 and writes nothing else for that list), d_view1 / d_view2 DEVICE arrays
 * [n_lists].  One kernel launch.  A list's results do not depend on the other lists of the call and equal bit for bit
 * what msf_new_points returns for that list.  n_lists <= 65535.  Asynchronous on `stream` like the other *_device
 * calls; one stream in flight per handle. */
int msf_new_points_device(msf_handle* h, int32_t n_lists, const msf_match* d_matches, int32_t cap_per_pair,
                          const int32_t* d_n_out, const msf_view* d_view1, const msf_view* d_view2,
                          const msf_new_points_params* params, msf_new_points_result* out, void* stream);

/* CreateNewMapPoints' loop in one call, HOST pointers: the launch sequence of msf_match_one_to_many for the stored frame
 * query_slot against slots[0..n), then the new-points kernel on the same stream over the handle's device lists
 * (views[i] belongs to slots[i]), then the copy-back: num_matches [n], the lists (out_matches [n][cap_per_pair], may be
 * NULL) and `out` ([n][cap_per_pair] arrays).  List i is the first min(num_matches[i], cap_per_pair) matches: what
 * out_matches receives is what was triangulated.  Argument checks and MSF_ERR_CAPACITY as msf_match_one_to_many
 * (cap_per_pair >= 1 always: it sizes `out`); a pair without a valid list has n_new = -1.  n == 0 is no error. */
int msf_create_map_points(msf_handle* h, int32_t query_slot, const msf_view* query_view, int32_t n,
                          const int32_t* slots, const msf_view* views, const msf_new_points_params* params,
                          int32_t* num_matches, msf_match* out_matches, int32_t cap_per_pair,
                          msf_new_points_result* out);

#ifdef __cplusplus
}
#endif
#endif /* MSF_LOCAL_MAPPING_H */
