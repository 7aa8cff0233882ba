/*
 * msf_initializer.h -- Initializer::Initialize to the end on the device: pose and map points.
 *
 * The tail of Initializer::Initialize (slam_pipeline/src/Initializer.cc:137-147, 489-934) behind msf_find_models /
 * msf_find_models_device of msf_abi.h: the choice between H and F by RH = SH / (SH + SF) > 0.40, ReconstructH /
 * ReconstructF with DecomposeE, CheckRT with Triangulate for every motion hypothesis, and the two selection rules --
 * what Tracking::MonocularInitialization (slam_pipeline/src/Tracking.cc:251) uses: R21, t21, vP3D, vbTriangulated and
 * the yes / no.  Exported from the same libmsf.so; a header and a version of its own, so that MSF_ABI_VERSION and the
 * symbol list of msf_abi.h stay what they are.  Plain C; status codes, msf_last_error, threading and streams as in
 * msf_abi.h.  Works on handles of either kind.
 *
 * Arithmetic (csrc/reconstruct_solve.h, shared with a host build that is tested against float64): f32 where the reference
 * is CV_32F, in the reference's operation order; cosParallax and acos in f64, as cv::norm / Mat::dot return double.  The
 * 3 x 3 and 4 x 4 SVDs are a one-sided Jacobi in f32: singular values within 16 eps s1 of a float64 SVD, a candidate's
 * (R, t) within 16 eps s1 / gap (gap = min(d1 - d2, d2 - d3) for H, s2 - s3 for E), a triangulated null vector within
 * 16 eps s1 / (s3 - s4).  An SVD is defined up to signs, and a sign choice permutes the hypotheses: candidates compare
 * as a SET with the reference's, the winner by its (R, t), never by its index.  A match is counted exactly as by the
 * reference unless it lies at one of CheckRT's thresholds.  The selection rules are literal, quirks included:
 * ReconstructF needs maxGood >= max(0.9 N, minTriangulated), at most one candidate above 0.7 maxGood and
 * parallax > minParallax for the FIRST candidate that reaches maxGood; ReconstructH takes the first strict maximum and
 * needs nGood >= min(0.9 N, minTriangulated) and parallax >= minParallax.
 */
#ifndef MSF_INITIALIZER_H
#define MSF_INITIALIZER_H

#include "msf_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MSF_INITIALIZER_VERSION 1

/* Initializer(K, sigma) + Initialize(..., minTriangulated, minParallax) */
typedef struct msf_motion_params {
  uint32_t struct_size; /* sizeof(msf_motion_params) */
  uint32_t reserved;    /* 0 */
  float K[9];           /* row-major, CV_32F mK; finite and invertible */
  float sigma;          /* th2 = 4 sigma^2 */
  int32_t min_triangulated;
  float min_parallax;   /* degrees */
} msf_motion_params;

/* Every pointer optional except ok.  msf_reconstruct: HOST pointers of one list; msf_reconstruct_device: DEVICE
 * pointers with a leading [n_lists] dimension. */
typedef struct msf_motion_result {
  uint32_t struct_size;   /* sizeof(msf_motion_result) */
  uint32_t reserved;      /* 0 */
  int32_t* ok;            /* Initialize()'s return value */
  int32_t* model;         /* MSF_MODEL_* that was reconstructed from, -1 if none (a list shorter than 8 or longer than
                             8192, or no kept hypothesis of the chosen model) */
  float* R21;             /* [9] row-major, zeros when !ok */
  float* t21;             /* [3], zeros when !ok */
  float* points;          /* [n_matches or cap_per_pair][3]: vP3D, zero where CheckRT stored nothing */
  uint8_t* triangulated;  /* [n_matches or cap_per_pair]: vbTriangulated, false beyond the list */
  /* diagnostics, for tests and callers that want the losers too */
  int32_t* n_cand;        /* 8 (H), 4 (F), 0 (none; with model = 0: ReconstructH's early return on d1/d2, d2/d3) */
  float* cand_R;          /* [8][9]; zeros beyond n_cand */
  float* cand_t;          /* [8][3] */
  int32_t* cand_good;     /* [8]: CheckRT's nGood */
  float* cand_parallax;   /* [8]: CheckRT's parallax, degrees */
  int32_t* winner;        /* index into the candidates, or -1 */
} msf_motion_result;

int msf_initializer_version(void);

/* ReconstructH (model = MSF_MODEL_HOMOGRAPHY) / ReconstructF (MSF_MODEL_FUNDAMENTAL) alone: one list, HOST pointers;
 * m21 [9] row-major H21 / F21 and inliers [n_matches] (vbMatchesInliers) supplied by the caller.
 * MSF_ERR_INVALID_ARG for a wrong struct_size, a missing required pointer, n_matches > 8192 or < 0, a model other than
 * 0 / 1, a non-finite or singular K.  n_matches < 8 or an all-false inlier list is no error: ok = 0. */
int msf_reconstruct(msf_handle* h, int32_t model, const float* m21, int32_t n_matches, const msf_match* matches,
                    const uint8_t* inliers, const msf_motion_params* params, msf_motion_result* out);

/* The tail of Initialize() for a batch in DEVICE memory: d_matches / cap_per_pair / d_n_out as msf_match_batch_device
 * left them, `found` the msf_ransac_batch that msf_find_models_device filled with the same n_hyp (m21, scores, best and
 * best_inliers of both models are required).  Chooses H or F per list by RH (a NaN ratio: F).  A list's results do not
 * depend on the other lists of the call, and equal bit for bit what msf_reconstruct returns for that list with the chosen
 * model's kept matrix and inliers.  n_lists <= 65535.  Asynchronous on `stream` like the other *_device calls; one
 * stream in flight per handle. */
int msf_reconstruct_device(msf_handle* h, int32_t n_lists, const msf_match* d_matches, int32_t cap_per_pair,
                           const int32_t* d_n_out, int32_t n_hyp, const msf_ransac_batch* found,
                           const msf_motion_params* params, msf_motion_result* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MSF_INITIALIZER_H */
