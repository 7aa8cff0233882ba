/*
 * msf_frame_tracking.h -- the body of Tracking::TrackWithMotionModel / TrackReferenceKeyFrame on the device: carry the
 * map points over the match list, optimise the pose, cut the outliers.
 *
 * Both functions (slam_pipeline/src/Tracking.cc:434-485 and :380-424) have one body: MatchFrames(current, last or
 * reference) and an early return below mMinLocalMatchCount matches; SetMapPoint(keyPoints1[i], the point at
 * keyPoints2[i]) on the current frame for every match whose second end holds a map point; Optimizer::PoseOptimization;
 * the key points it flagged leave the frame's map and the ones that stay and have observations are counted (>= 10).
 * Here the carry and the cut run on the device around k_pose_optimize, behind the matcher and in front of
 * msf_search_local_points, so that a tracked frame's match list, correspondences and outlier flags never visit the host.
 * Exported from the same libmsf.so; a header and a version of its own.  Plain C; status codes, msf_last_error, threading
 * and streams as in msf_abi.h.  Works on handles of either kind.
 *
 * NAMING RULE, from this header on: the set of msf_-prefixed functions that libmsf.so exports is closed with
 * msf_tracking.h (its test pins that set).  Entry points of every header added after msf_tracking.h carry the prefix
 * msfx_, and so do the macros (MSFX_), the version define and the struct names of such a header.
 *
 * What stays with the caller: UpdateLastFrame, CheckReplacedInLastFrame, the velocity, CreateCurrentMatchImage
 * (msf_render_match_image), mnLastFrameSeen (from `removed` and the kept map), SetPose (from Tcw).
 *
 * The semantics are the order-independent statement of the sequential code (tests/frame_tracking_ref.py holds the
 * literal restatement and proves the two equal).  A pixel key is y * width + x; an end point outside the image has no
 * key (KeyPointMap.cc:37-38, 66-67).
 *  0. The map is checked first: ref_key and cur_key strictly increasing and inside the image, ref_point and cur_point
 *     in [0, n_points).  A malformed map: track_status = -1 and nothing else is written.
 *  1. The gate.  n = d_n_out[0].  n < 0: track_status = -3 and nothing else is written.  n < min_matches:
 *     track_status = 1, nothing is carried: the list counts as empty in steps 2-3 (no carry_status is written), the
 *     optimiser does not run (it is fed d_n = -1), Tcw = Tcw0, n_good = -1, and step 5 runs with no outlier: the kept
 *     map is the entry map and n_removed = 0.  Else the list is the first min(n, cap) matches.
 *     msfx_carry_points_device has no min_matches: only n < 0 stops it.
 *  2. The carry.  Match j has k1 = key(x1, y1), k2 = key(x2, y2).  It is a candidate iff k1 exists and the train frame
 *     has an entry with ref_key == k2 (its ref_point is the carried point, whatever that point is: the reference checks
 *     nothing there).  SetMapPoint overwrites: among the candidates of one k1 the LARGEST j wins, and it wins over an
 *     entry of the current frame at that key.
 *     carry_status[j]: 0 carried, 1 no k1, 3 no point at k2, 4 overwritten by a later match (the numbers of
 *     claim_status in msf_tracking.h; 2 is unused).  cur_status[c]: 0 stays, 1 replaced by a carried point.
 *  3. The frame's map after the carry: n_map records msfx_frame_point {key, point, match, flags} -- match = -1 for an
 *     entry of the frame, flags = 0 here -- in ASCENDING KEY order, the project's canonical order for the iteration of
 *     a std::unordered_map (as in msf_search_local_points).  The correspondences corr_p3d (the point's pos), corr_p2d
 *     (the key's (x, y) as floats) and corr_point follow the same order, in the layout msf_pose_optimize_device reads.
 *     Capacity: n_cur + (the list's length) > min(corr_cap, MSFX_TRACK_MAX_CANDIDATES): track_status = -2 and nothing
 *     else is written.
 *  4. The optimiser: pose_optimize() of msf_pose.h on that one list (cap = corr_cap, no mask) from Tcw0.  The optional
 *     msf_pose_result receives everything msf_pose_optimize returns for the list, bit for bit; for a call that ends
 *     with track_status 1 or negative it receives n_good = -1 alone, as msf_pose_optimize_device says of a list without
 *     a valid result.
 *  5. The cut (:404-421, :465-482).  A record whose outlier byte is set goes to removed [n_removed] as {key, point}
 *     and gets bit 0 of its flags; the others form the kept map kept_key / kept_point [n_kept], keys strictly
 *     increasing: exactly the cur_key / cur_point of an msf_local_map.  n_matches_map = the kept records whose point is
 *     observed (observed == NULL: all of them).
 *  6. track_status = 0 if n_matches_map >= min_map_matches, else 2.  Tcw and n_good are written either way.
 *
 * Only integer sums cross threads (ballots and prefix counts inside one workgroup); no floating-point atomics, no
 * spins, every loop bounded: a call is bit-identical to its replay.
 */
#ifndef MSF_FRAME_TRACKING_H
#define MSF_FRAME_TRACKING_H

#include "msf_pose.h"
#include "msf_tracking.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MSFX_FRAME_TRACKING_VERSION 1

#define MSFX_TRACK_MAX_CANDIDATES 8192 /* n_cur + the list's length, at most: one workgroup sorts them in LDS */
#define MSFX_TRACK_KEEP_ON_DEVICE 1u

/* One record of the current frame's map after the carry.  16 bytes. */
typedef struct msfx_frame_point {
  int32_t key, point, match, flags;
} msfx_frame_point;

/* One record the cut took out of the frame's map.  8 bytes. */
typedef struct msfx_removed_point {
  int32_t key, point;
} msfx_removed_point;

/* The inputs of one call.  HOST pointers for msfx_track_frame, DEVICE pointers for the *_device calls.  Of a point
 * only pos is read, so the table that goes on to msf_search_local_points serves here as it is; `observed` carries
 * Observations() > 0 beside it (NULL: every point is observed).  ref_* is the train frame's mKeyPointMap, cur_* the
 * current frame's own map at entry: empty after TrackWithMotionModel's Clear(), not empty when TrackReferenceKeyFrame
 * runs as the fallback of Tracking.cc:132-134. */
typedef struct msfx_frame_map {
  uint32_t struct_size; /* sizeof(msfx_frame_map) */
  uint32_t reserved;    /* 0 */
  int32_t n_points, n_ref, n_cur, reserved2;
  const msf_map_point* points; /* [n_points] */
  const uint8_t* observed;     /* [n_points] or NULL */
  const int32_t* ref_key;      /* [n_ref] strictly increasing, inside the image */
  const int32_t* ref_point;    /* [n_ref] in [0, n_points) */
  const int32_t* cur_key;      /* [n_cur] strictly increasing, inside the image */
  const int32_t* cur_point;    /* [n_cur] in [0, n_points) */
} msfx_frame_map;

typedef struct msfx_track_params {
  uint32_t struct_size; /* sizeof(msfx_track_params) */
  uint32_t reserved;    /* 0 */
  msf_pose_params pose;
  float Tcw0[12];          /* rows 0..2 of the entry pose, R | t row-major */
  int32_t min_matches;     /* mMinLocalMatchCount: 15 at the call sites */
  int32_t min_map_matches; /* 10 */
} msfx_track_params;

/* Every pointer optional except track_status. */
typedef struct msfx_track_result {
  uint32_t struct_size;        /* sizeof(msfx_track_result) */
  uint32_t reserved;           /* 0 */
  int32_t* track_status;       /* [1]: 0, 1, 2, or -1 / -2 / -3 (then nothing else is written) */
  int32_t* n_map;              /* [1] */
  msfx_frame_point* map;       /* [corr_cap]: the first n_map records, untouched beyond */
  uint8_t* carry_status;       /* [cap]: per match of the list, untouched beyond it */
  uint8_t* cur_status;         /* [n_cur] */
  float* corr_p3d;             /* [corr_cap][3] */
  float* corr_p2d;             /* [corr_cap][2] */
  int32_t* corr_point;         /* [corr_cap] */
  float* Tcw;                  /* [12]        -- from here on: msfx_track_list_device and msfx_track_frame only */
  int32_t* n_good;             /* [1] */
  int32_t* n_kept;             /* [1] */
  int32_t* kept_key;           /* [corr_cap] */
  int32_t* kept_point;         /* [corr_cap] */
  int32_t* n_removed;          /* [1] */
  msfx_removed_point* removed; /* [corr_cap] */
  int32_t* n_matches_map;      /* [1] */
} msfx_track_result;

/* msfx_track_frame with MSFX_TRACK_KEEP_ON_DEVICE: where the kept map, the correspondences and the pose lie in the
 * family's workspace.  Valid across calls of other families (a following msf_search_local_points included), until
 * the next call of THIS family on the handle. */
typedef struct msfx_device_track {
  uint32_t struct_size; /* sizeof(msfx_device_track) */
  int32_t corr_cap;     /* n_cur + min(cap_per_pair, the handle's staging capacity) */
  const int32_t* d_track_status;
  const int32_t* d_n_kept;
  const int32_t* d_kept_key;
  const int32_t* d_kept_point;
  const int32_t* d_n_map;
  const float* d_corr_p3d;
  const float* d_corr_p2d;
  const int32_t* d_corr_point;
  const uint8_t* d_outliers;
  const float* d_Tcw;
} msfx_device_track;

int msfx_frame_tracking_version(void);

/* Ordering.  Every call of this family on one handle re-carves the family's own workspace (not that of
 * msf_tracking.h, not the matcher's lists).  The *_device calls are asynchronous on `stream`; the caller orders the
 * calls of this family on a handle as with the other *_device calls (one stream in flight per handle). */

/* Steps 0, 2, 3 on one list in DEVICE memory as msf_match_slots_device leaves it: d_matches [cap], d_n_out [1].
 * DEVICE pointers in `map` and `out`; the members of `out` behind corr_point are not looked at.  track_status: 0, or
 * -1 / -2 / -3.  One launch.  MSF_ERR_INVALID_ARG for a wrong struct_size, negative counts, a missing required pointer,
 * cap < 1, corr_cap < 0. */
int msfx_carry_points_device(msf_handle* h, const msfx_frame_map* map, const msf_match* d_matches, int32_t cap,
                             const int32_t* d_n_out, int32_t corr_cap, msfx_track_result* out, void* stream);

/* Steps 0-6 on one list in DEVICE memory: three launches (check and carry, k_pose_optimize, cut) and no host decision
 * between them.  DEVICE pointers in `map`, `out` and `pose` (optional; its outliers [corr_cap]).  Also refused: a NaN
 * chi2, negative min_matches / min_map_matches. */
int msfx_track_list_device(msf_handle* h, const msfx_frame_map* map, const msf_match* d_matches, int32_t cap,
                           const int32_t* d_n_out, int32_t corr_cap, const msfx_track_params* params,
                           msfx_track_result* out, msf_pose_result* pose, void* stream);

/* The whole body in one call, HOST pointers: the stored frame query_slot against the stored frame train_slot.  The
 * uploads, the match (the launch sequence of msf_match_one_to_many for one slot), steps 0-6 on the handle's list on the
 * same stream, and one copy-back: num_matches [1], the list (out_matches [cap_per_pair], may be NULL), `out` and
 * `pose` (optional).  The arrays of `out` that are [corr_cap], and pose->outliers, need room for
 * n_cur + cap_per_pair entries.  With MSFX_TRACK_KEEP_ON_DEVICE in `flags`, `keep` (required then) receives the device
 * pointers; the copy-back is the same.  A malformed map is refused with MSF_ERR_INVALID_ARG before anything is
 * enqueued; refusals as msf_match_one_to_many for the slots, cap_per_pair < 1, unknown flag bits.  MSF_ERR_CAPACITY
 * as msf_match_one_to_many (num_matches[0] < 0: no valid list, track_status = -3), and also for num_matches[0] >
 * cap_per_pair or the handle's staging capacity: the body would need the whole list; what is delivered then is the
 * result of its first min(cap_per_pair, staging capacity) matches. */
int msfx_track_frame(msf_handle* h, int32_t query_slot, int32_t train_slot, const msfx_frame_map* map,
                     const msfx_track_params* params, uint32_t flags, int32_t* num_matches, msf_match* out_matches,
                     int32_t cap_per_pair, msfx_track_result* out, msf_pose_result* pose, msfx_device_track* keep);

#ifdef __cplusplus
}
#endif
#endif /* MSF_FRAME_TRACKING_H */
