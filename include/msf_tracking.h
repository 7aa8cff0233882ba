/*
 * msf_tracking.h -- Tracking::SearchLocalPoints on the device: frustum test, gated match, claims.
 *
 * The loop of Tracking::SearchLocalPoints (slam_pipeline/src/Tracking.cc:594-632), which TrackLocalMap runs on every
 * tracked frame: per local key frame Frame::isInFrustum on every map point of the key frame (Frame.cc:48-84),
 * MatchFrames(current, KF) if at least one point is visible, and every matched key point of the current frame that holds
 * no map point takes the map point at the other end (:621-630).  Here the frustum test, the gate and the association
 * run on the device around the matcher, and the correspondences leave in the layout msf_pose_optimize_device reads.
 * Exported from the same libmsf.so; a header and a version of its own, so that MSF_ABI_VERSION, the earlier versions and
 * their symbol lists stay what they are.  Plain C; status codes, msf_last_error, threading and streams as in msf_abi.h.
 * Works on handles of either kind.
 *
 * What stays with the caller: UpdateLocalKeyFrames, the first loop of :576-592 (its result arrives as the "seen" flag
 * and the current frame's map), IncreaseVisible (from `visible`), SetMapPoint (from the claim records), IncreaseFound.
 *
 * The semantics are the order-independent statement of the sequential loop (tests/tracking_ref.py holds the literal
 * restatement and proves the two equal):
 *  1. owner[p] = the smallest flat entry index e with kf_point[e] == p (what mnTrackReferenceForFrame amounts to);
 *     owner_kf[p] = that entry's key frame, -1 if no entry refers to p.
 *  2. status[p], in this order:
 *       9  no entry refers to the point        7  bad (flag bit 0)        8  seen (flag bit 1)
 *       1  PcZ < 0
 *       6  u or v is not finite                (PcZ == +-0 arrives here through invz = inf)
 *       2  u outside [min_x, max_x]            3  v outside [min_y, max_y]
 *       6  dist is not finite                  4  dist > max_distance
 *       6  viewCos is not finite               5  viewCos < viewing_cos_limit
 *       0  visible
 *     Code 6 is a defined divergence: the reference's comparisons let a NaN through as "visible"; here it is rejected,
 *     as msf_new_points rejects a non-finite point.  visible[p] = (status == 0); n_to_match[i] = the number of visible
 *     points with owner_kf == i.
 *  3. Key frame i is matched iff n_to_match[i] > 0; an unmatched key frame reports num_matches[i] = -1 and takes no part
 *     in step 4 (told from a capacity failure by n_to_match[i] == 0).
 *  4. occupied = the set cur_key.  The matched key frames in call order and the first min(n_out, cap) matches of each
 *     in list order: match (i, j) has the ordinal i * cap + j and the pixel keys k1 = y1 * width + x1,
 *     k2 = y2 * width + x2; an end point outside the image has no key (KeyPointMap ignores such points).  It claims k1
 *     iff k1 exists, k1 is not occupied, key frame i has an entry with kf_key == k2 (its kf_point is the claimed point,
 *     whatever its flags: the reference checks nothing there), and no match of smaller ordinal claims the same k1.
 *     claim_status: 0 claimed, 1 k1 outside the image, 2 k1 occupied at entry, 3 no point at k2, 4 lost to an earlier
 *     ordinal.  The records are packed in ordinal order.
 *  5. Correspondences (optional): the n_cur existing entries in key order (p2d = the key's (x, y) as floats, p3d = the
 *     point's pos), then the claims in ordinal order.  n_cur + n_claims > corr_cap: n_corr = -1 and nothing else of
 *     these arrays is written; the claims stay valid.
 *
 * Arithmetic of step 2 (csrc/tracking_solve.h, shared with a host build that is tested against float64), in the types
 * the reference's expressions have: Pc = Rcw P + tcw with f32 products summed left to right, then the f32 add;
 * invz = 1.0f / PcZ, u = fx * PcX * invz + cx and v in f32, left to right; PO = P - Ow in f32;
 * dist = (float)sqrt(sum (double)PO^2) (cv::norm returns a double); viewCos = (float)(sum (double)PO (double)Pn /
 * (double)dist).  The diagnostics u, v, dist, view_cos hold what was computed before the rejecting stage and 0 behind
 * it; a NaN is stored as the quiet NaN 0x7FC00000.
 *
 * A result does not depend on which lane or workgroup handled what (integer min and add only, no floating-point
 * atomics): a call is bit-identical to its replay.
 */
#ifndef MSF_TRACKING_H
#define MSF_TRACKING_H

#include "msf_local_mapping.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MSF_TRACKING_VERSION 1

#define MSF_POINT_BAD 1u  /* MapPoint::isBad() */
#define MSF_POINT_SEEN 2u /* mnLastFrameSeen == the current frame: the points the frame already holds */

/* One map point of the local map.  32 bytes. */
typedef struct msf_map_point {
  float pos[3];       /* GetWorldPos() */
  float normal[3];    /* GetNormal() */
  float max_distance; /* GetDistanceInvariance(): the caller's own 1.2f * mfDistance */
  uint32_t flags;     /* MSF_POINT_BAD | MSF_POINT_SEEN; other bits 0 */
} msf_map_point;

/* One claim: the current frame's pixel key, the point it takes, the key frame and the match that gave it.  16 bytes. */
typedef struct msf_local_claim {
  int32_t key, point, kf, match;
} msf_local_claim;

/* The local map of one call.  HOST pointers for msf_frustum / msf_search_local_points, DEVICE pointers for the
 * *_device calls.  Key frames are a CSR over the point table: key frame i owns the entries [kf_start[i],
 * kf_start[i + 1]), kf_start[0] = 0, kf_start[n_kf] = n_entries; kf_key (the pixel key y * width + x) is strictly
 * increasing inside a key frame and inside the image; kf_point is in [0, n_points).  A point may appear in several key
 * frames, and twice inside one under two keys.  The current frame's own map: cur_key strictly increasing. */
typedef struct msf_local_map {
  uint32_t struct_size; /* sizeof(msf_local_map) */
  uint32_t reserved;    /* 0 */
  int32_t n_points, n_kf, n_entries, n_cur;
  const msf_map_point* points; /* [n_points] */
  const int32_t* kf_start;     /* [n_kf + 1] */
  const int32_t* kf_key;       /* [n_entries] */
  const int32_t* kf_point;     /* [n_entries] */
  const int32_t* cur_key;      /* [n_cur] */
  const int32_t* cur_point;    /* [n_cur] */
} msf_local_map;

typedef struct msf_frustum_params {
  uint32_t struct_size;            /* sizeof(msf_frustum_params) */
  uint32_t reserved;               /* 0 */
  msf_view view;                   /* the current frame: mRcw, mtcw, fx() ... cy() */
  float Ow[3];                     /* GetCameraCenter(): passed, not re-derived */
  float min_x, max_x, min_y, max_y; /* mnMinX ... mnMaxY.  Not NaN. */
  float viewing_cos_limit;         /* 0.5 at the one call site.  Not NaN. */
} msf_frustum_params;

/* Steps 1-2.  Every pointer optional except status_word and (with n_kf > 0) n_to_match. */
typedef struct msf_frustum_result {
  uint32_t struct_size; /* sizeof(msf_frustum_result) */
  uint32_t reserved;    /* 0 */
  int32_t* status_word; /* [1]: 0, or -1 for a malformed local map (then nothing else is written) */
  int32_t* n_to_match;  /* [n_kf] */
  uint8_t* status;      /* [n_points]: the codes above */
  uint8_t* visible;     /* [n_points]: status == 0 */
  int32_t* owner_kf;    /* [n_points] */
  float* u;             /* [n_points] diagnostics */
  float* v;
  float* dist;
  float* view_cos;
} msf_frustum_result;

/* Steps 4-5.  Every pointer optional except status_word, n_claims and (n_kf > 0) n_claimed.  corr_* are written only
 * when n_corr, corr_p3d, corr_p2d and corr_point are all given. */
typedef struct msf_claim_result {
  uint32_t struct_size;    /* sizeof(msf_claim_result) */
  uint32_t reserved;       /* 0 */
  int32_t* status_word;    /* [1]: 0, or -1 for a malformed local map (then nothing else is written) */
  int32_t* n_claims;       /* [1] */
  int32_t* n_claimed;      /* [n_kf]: claims per key frame (0 for an unmatched one) */
  msf_local_claim* claims; /* [n_kf * cap]: the first n_claims records, in ordinal order; untouched beyond */
  uint8_t* claim_status;   /* [n_kf][cap]: per match of a matched key frame's list; untouched beyond the list */
  int32_t* n_corr;         /* [1]: n_cur + n_claims, or -1 if that exceeds corr_cap */
  float* corr_p3d;         /* [corr_cap][3] */
  float* corr_p2d;         /* [corr_cap][2] */
  int32_t* corr_point;     /* [corr_cap] */
} msf_claim_result;

/* msf_search_local_points with MSF_SEARCH_KEEP_ON_DEVICE: the correspondences stay in the handle's workspace, valid
 * until the next call of this family on the handle; msf_pose_optimize_device can follow without a copy (one list,
 * cap = corr_cap, d_n = d_n_corr). */
typedef struct msf_device_corr {
  uint32_t struct_size; /* sizeof(msf_device_corr) */
  int32_t corr_cap;     /* n_cur + n_kf * min(cap_per_pair, the handle's staging capacity): always enough */
  const float* d_corr_p3d;
  const float* d_corr_p2d;
  const int32_t* d_corr_point;
  const int32_t* d_n_corr;
} msf_device_corr;

#define MSF_SEARCH_KEEP_ON_DEVICE 1u

int msf_tracking_version(void);

/* Ordering.  Every call of this family on one handle clears and re-carves the family's one workspace (and may
 * reallocate it when it grows).  The *_device calls are asynchronous on `stream`: the caller orders the calls of this
 * family on a handle -- the next one starts only when the previous one's work has completed or is ordered before it on
 * the same stream -- as with the other *_device calls (one stream in flight per handle).  The pointers of
 * msf_device_corr have the same lifetime: until the next call of this family on the handle. */

/* Steps 1-2 and n_to_match, HOST pointers.  Zero points, key frames or entries are no error.  MSF_ERR_INVALID_ARG,
 * before anything is enqueued, for a wrong struct_size, a missing required pointer, negative counts, kf_start not
 * non-decreasing from 0 to n_entries, a key outside the image or not strictly increasing, a point index out of range,
 * flag bits above 1, a NaN bound. */
int msf_frustum(msf_handle* h, const msf_local_map* map, const msf_frustum_params* params, msf_frustum_result* out);

/* The same with DEVICE pointers in `map` and `out`, asynchronous on `stream`.  The host cannot look at device memory:
 * the kernels check every index before use, and a malformed map writes status_word = -1 and nothing else.  Equals
 * msf_frustum bit for bit. */
int msf_frustum_device(msf_handle* h, const msf_local_map* map, const msf_frustum_params* params,
                       msf_frustum_result* out, void* stream);

/* Steps 4-5 on lists in DEVICE memory as msf_match_slots_device left them: key frame i's list is d_matches +
 * i * cap_per_pair, its length min(d_n_out[i], cap_per_pair); d_matched[i] == 0 (the gate) or d_n_out[i] < 0: no list.
 * n_kf * cap_per_pair < 2^31 (the ordinal has 31 bits).  The first pass takes the minimum ordinal per claimed pixel in
 * one word per pixel of the image, inside the family's workspace and cleared by every call.  DEVICE pointers in `map`
 * and `out`; map->points is read only for the correspondences.  Asynchronous on `stream`. */
int msf_claim_points_device(msf_handle* h, const msf_local_map* map, const msf_match* d_matches, int32_t cap_per_pair,
                            const int32_t* d_n_out, const uint8_t* d_matched, int32_t corr_cap, msf_claim_result* out,
                            void* stream);

/* The loop in one call, HOST pointers: the stored frame query_slot against the stored frames slots[0..map->n_kf),
 * n_kf <= max_batch_pairs.  The uploads, steps 1-2, the gate (written on the device: the train slot of an unmatched
 * key frame becomes -1, which the matcher answers with n_out = -1), the match, steps 4-5 on the handle's lists on the
 * same stream, and the copy-back: num_matches [n_kf], the lists (out_matches [n_kf][cap_per_pair], may be NULL), the
 * frustum arrays and the claims.  corr_* of `claims` need room for n_cur + n_kf * cap_per_pair correspondences;
 * with MSF_SEARCH_KEEP_ON_DEVICE in `flags` they are not copied back and `keep` (required then) receives the device
 * pointers.  Refusals as msf_frustum, and as msf_match_one_to_many for the slots (n_kf > max_batch_pairs, a bad slot,
 * no stored frame), cap_per_pair < 1, unknown flag bits.  MSF_ERR_CAPACITY as msf_match_one_to_many, for matched key
 * frames only. */
int msf_search_local_points(msf_handle* h, int32_t query_slot, const int32_t* slots, const msf_local_map* map,
                            const msf_frustum_params* params, uint32_t flags, int32_t* num_matches,
                            msf_match* out_matches, int32_t cap_per_pair, msf_frustum_result* frustum,
                            msf_claim_result* claims, msf_device_corr* keep);

#ifdef __cplusplus
}
#endif
#endif /* MSF_TRACKING_H */
