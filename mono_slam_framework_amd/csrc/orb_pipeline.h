// ORB extract + match on gfx950: host-side launcher interface (implemented in orb_kernels.hip).
//
// Replaces the arithmetic behind the reference's ::FeatureMatcher::MatchFrames
// (src/featurematcher.cpp:10-45): cv::ORB::detectAndCompute x2 + BFMatcher::knnMatch(k=2)
// + ratio test.  Stage names follow SURVEY.md 2.4 (K1..K11).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "dev_buf.h"
#include "msf_abi.h"
#include "orb_plan.h"

namespace msf {

// The level plan, its structs (kernel arguments) and the capacities: orb_plan.h.
constexpr int kOrbStages = 6;

// where level 0 of frame fi of the call lives: fi < n_a ? a + fi*frame_stride : b + (fi-n_a)*frame_stride.
// Two index spaces: the per-call arrays (work rows) are indexed by fi, the per-slot arrays by slot = slot0 + fi.
struct FrameSrc {
  const uint8_t* a;
  const uint8_t* b;
  int n_a;
  int slot0;               // first feature slot written by this call: frame fi's key points go to slot slot0 + fi
  long long frame_stride;
  int row_stride;
};

struct OrbOptions {
  int width = 0, height = 0;
  int max_slots = 0;               // feature slots
  int work_frames = 0;             // frames one extraction may hold (0: max_slots)
  bool blur_half_up = false;       // MSF_FLAG_BLUR_TIE_HALF_UP
  bool blur_sum256 = false;        // MSF_FLAG_BLUR_SUM256
  bool profile = false;            // MSF_FLAG_PROFILE: stage events
  bool dense_fast = false;         // MSF_FLAG_FAST_DENSE
  bool level_size_mul_inv = false; // MSF_FLAG_LEVEL_SIZE_MUL_INV
  int stream_min_frames = 8;       // calls with fewer frames take the dense FAST kernel (MSF_FLAG_FAST_STREAM: 1)
};

class OrbPipeline {
 public:
  OrbPipeline() = default;
  ~OrbPipeline();
  // returns empty string on success
  std::string init(const OrbOptions& o);
  void destroy();                  // the events and the pinned word (the device buffers go with the object); idempotent

  // extract features of n frames into slots [src.slot0, src.slot0 + n)
  hipError_t extract(const FrameSrc& src, int n_frames, hipStream_t st);
  // match slot pairs; d_slot_a/d_slot_b may be null => pair i = (slot_base + i, slot_base + n_pairs + i)
  // slot_limit > 0: slots at or beyond it give n_out = -1 (public entry points: 2 * max_batch_pairs); 0: max_slots()
  hipError_t match(int n_pairs, const int32_t* d_slot_a, const int32_t* d_slot_b, float ratio,
                   msf_match* d_out, int cap_per_pair, int32_t* d_n_out, hipStream_t st, int slot_base = 0,
                   int slot_limit = 0);
  // debug (msf_debug_orb_set_features): n <= kKpCap caller features (HOST pointers) into feature slot `slot`, its count
  // set to n and its status word cleared; enqueued on `st`, the caller waits before kp / desc go away
  hipError_t set_features(int slot, int n, const msf_keypoint* kp, const uint8_t* desc, hipStream_t st);
  // debug (msf_debug_orb_tail): everything behind FAST on candidates the caller supplies.  The pyramid of the n frames
  // is made (k_resize), the lists of (frame, level) -- counts [n][8], cands (lx, ly, score) triples in (frame, level)
  // order, HOST pointers -- are written where a call of n frames keeps them, and launch_tail() runs on them: form 0 the
  // dense form (k_thr_harris with 256 threads scores the kept candidates itself), 1 the streaming form (one wave, then
  // k_harris_flat).  The caller has checked the lists with tail_refusal(); returns with the stream drained.
  hipError_t tail(const FrameSrc& src, int n, const int32_t* counts, const int32_t* cands, int form, hipStream_t st);
  // why tail() may not take these lists (check_tail_lists, orb_plan.h), or empty
  std::string tail_refusal(int n, const int32_t* counts, const int32_t* cands) const;

  const OrbGeometry& geom() const { return g_; }
  int max_slots() const { return max_slots_; }
  int debug_get(int what, int slot, int level, void* host_out, size_t cap, size_t* n_bytes, std::string* err);
  int stage_times(const char** names, float* ms, int cap);
  // true once after the handle switched to per-level walker launches because a unit of an earlier launch gave up waiting
  bool take_degraded_note() { const bool d = degraded_note_; degraded_note_ = false; return d; }
  bool walk_per_level() const { return walk_per_level_; }

 private:
  OrbGeometry g_{};
  OrbPrimLists prim_{};
  HarrisUnits harris_{};
  int max_slots_ = 0;
  int work_frames_ = 0;            // frames one extraction may hold = rows of the per-call arrays (0 at init: max_slots)
  int last_n_ = 0;                 // frames of the last extraction (debug_get maps a slot to its work row)
  bool half_up_ = false, profile_ = false, blur_sum256_ = false;
  int stream_min_frames_ = 8;      // calls with fewer frames take the dense FAST kernel (latency), others the streaming pass
  int force_tau_ = 0;              // > 0: every (frame, level) starts at this FAST score threshold (20 = dense)
  // device storage
  // per CALL (work_frames_ rows, indexed by the frame of the call): pyramid, candidate lists, thresholds, walker state,
  // stage-1 lists
  DevBuf<uint8_t> d_pyr_;
  DevBuf<uint32_t> d_tab_;      // resize tables per level: per group of 4 columns selectors / weights / pair offsets, per row source row | w1 << 16
  bool resize_shared_[kOrbLevels] = {};   // OrbPlan::resize_shared
  DevBuf<uint32_t> d_qstat_;           // [work rows][levels][kQStat]: per (frame, level) the score histogram of the sampled quarter's
                                          // corners, the thresholds and the done counters of the walker launch (see k_walk)
  DevBuf<uint32_t> d_walk_abort_;      // [4] the walker launch's abort word (a unit gave up waiting); zeroed per call
  uint32_t* h_walk_abort_ = nullptr;      // pinned copy of it, written behind every walker launch, read by later calls
  bool degraded_note_ = false;            // the handle has just fallen back to per-level launches (reported once)
  int test_stall_calls_ = 0;
  bool fast_two_part_ = true;             // MSF_ORB_FAST_ONE_PART=1 clears it: no refinement of the first threshold
  int tau_predict_pct_ = 300;             // MSF_ORB_TAU_PREDICT (0 = sample every level)
  bool fused_ = true;                     // MSF_ORB_UNFUSED=1 clears it: k_resize x 7, then one FAST-only walker launch
  bool walk_per_level_ = false;           // MSF_ORB_WALK_PER_LEVEL=1: the fused walker as one launch per level (the
                                          // in-launch waits are then met at once); tests compare it with the one-launch default
  int walk_finish_ = kWalkFinishThr;      // MSF_ORB_WALK_FINISH: finish units inside the one-launch walker (0 off, 1 behind
                                          // the next level's threshold units, 2 behind its sampled quarter; orb_plan.h)
  bool last_finish_ = false;              // the last extraction's walker launch held finish units (MSF_DBG_WALK_FINISHED)
  int test_stall_frame_ = -1;             // MSF_TEST_HOOKS + MSF_ORB_TEST_STALL_FRAME: see k_walk
  int tau2_margin_pct_ = 200;             // MSF_ORB_TAU2_MARGIN_PCT
  bool resize_generic_ = false;           // MSF_ORB_RESIZE_GENERIC: never
  DevBuf<uint32_t> d_cand_cnt_; // [work rows][8]
  DevBuf<uint32_t> d_tau_;      // [2][work rows][8] FAST score threshold used per (frame, level) | first estimate
  DevBuf<uint32_t> d_redo_;     // [1 + work rows * 8] dense-pass queue: count, entries (frame * 8 + level)
  DevBuf<uint32_t> d_redo_hist_;  // [work rows][8][256] dense pass: score histogram of a queued level's maxima (kept zeroed)
  DevBuf<uint32_t> d_redo_thr_;   // [work rows][8] dense pass: the level's retainBest(2N) cut (k_redo_thr)
  DevBuf<uint32_t> d_cand_;     // [work rows][prim_total] + pool (dense calls): key = y << 16 | x
  DevBuf<uint8_t> d_cand_sc_;   // the same shape: FAST score
  DevBuf<uint2> d_cmap_;        // [work rows][8] where the list of (frame, level) lives: (first entry, capacity); reset per call
  DevBuf<uint32_t> d_s1_cnt_;   // [work rows][8]
  DevBuf<uint4> d_s1_;          // [work rows][s1_total] (key, response bits, score, 0)
  // per feature SLOT (max_slots_ rows, indexed by slot = slot0 + frame): what a later match reads
  DevBuf<msf_keypoint> d_kp_;   // [slots][kKpCap]
  DevBuf<uint8_t> d_desc_;      // [slots][kKpCap][32]
  DevBuf<uint32_t> d_kp_cnt_;   // [slots]
  DevBuf<uint32_t> d_status_;   // [slots]
  DevBuf<uint32_t> d_qres_;     // [kSplitMaxPairs][kKpCap] per-query results of the small-batch matcher
  DevBuf<uint32_t> d_done_;     // [kSplitMaxPairs] ticket counters (left at 0)
  int last_match_form_ = 0;     // the last match launch: 0 none yet, 1 k_match_split, 2 k_match (MSF_DBG_ORB_MATCH_FORM)
  uint32_t set_words_[2] = {};  // set_features: the count and the status word while their copies are in flight
  // Stage events (MSF_FLAG_PROFILE).  A RING of event sets: a call records into the next free set and nobody waits, so a
  // caller can enqueue many batches ahead of the device; stage_times() harvests every finished set and returns the SUM
  // of the stage times since the last query (a query after every call sees that call's times, as before).  A set that
  // is needed again before it was queried is harvested first -- it is kEvRing calls old, long finished.
  static constexpr int kEvRing = 32;
  struct EvSet {
    hipEvent_t ev[kOrbStages + 1] = {};
    bool recorded = false, match_only = false;
  };
  EvSet evr_[kEvRing];
  int ev_cur_ = 0;
  hipEvent_t* ev_ = evr_[0].ev;                 // the current set
  float acc_ms_[5] = {};                        // harvested, not yet returned
  int acc_full_ = 0, acc_match_only_ = 0;       // calls behind acc_ms_: with an extraction / slot-pair matches only
  void ev_begin_call();
  void ev_harvest(int i);
  bool ev_ok_ = false, ev_extract_pending_ = false;
  FrameSrc last_src_{};
  bool last_fused_ = false;
  bool last_dense_ = false;        // the last extraction was a dense call (no streaming pass, no dense-pass queue)
  void read_env();                 // the MSF_ORB_* overrides (tests), all in one place
  hipError_t extract_range(const FrameSrc& src, int n, hipStream_t st, hipEvent_t* evs);
  // a call of n frames is dense (k_resize + the tile kernel, lists in the pool) when this is kFastT
  int call_force_tau(int n) const { return (force_tau_ == 0 && n < stream_min_frames_) ? kFastT : force_tau_; }
  void launch_resize(const FrameSrc& src, int n, int l, hipStream_t st);
  // selection and description of n frames whose candidate lists are complete: k_thr_harris (dense_form: 256 threads,
  // scoring what it keeps; else one wave + k_harris_flat), k_select, k_describe; evs as extract_range (3 and 4 recorded)
  // fin: the walker state of this call (its kQFin words name the (frame, level)s already finished inside the walker
  // launch, which the selection kernels skip), or null
  void launch_tail(const FrameSrc& src, int n, bool dense_form, hipStream_t st, hipEvent_t* evs, const uint32_t* fin);
};

}  // namespace msf
