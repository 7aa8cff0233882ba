// LoFTR_teacher (coarse-only, d_model 32, linear attention) on gfx950: host-side launcher interface.
// Replaces Ort::Session::Run + the threshold/decode loop of ::DNNFeatureMatcher::MatchFrames
// (src/dnnfeaturematcher.cpp:44-102).  Implemented in loftr_kernels.hip.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "msf_abi.h"

namespace msf {

class LoftrPipeline {
 public:
  LoftrPipeline() = default;
  ~LoftrPipeline();
  // returns empty string on success; "io: ..." for weight-file problems
  // extra_slots: token slots beyond the 2 * max_pairs caller-visible ones (the handle's transparent frame cache)
  // f32_convs: MSF_FLAG_LOFTR_F32 (no split-bf16 kernels)
  std::string init(const char* weights_path, int max_pairs, bool profile, bool keep_debug, int extra_slots = 0,
                   bool f32_convs = false);
  void destroy();
  hipError_t match(int n_pairs, const uint8_t* d_a, const uint8_t* d_b, long long frame_stride, int row_stride,
                   float threshold, msf_match* d_out, int cap_per_pair, int32_t* d_n_out, hipStream_t st);
  // per-frame token cache: frame -> slot [0, 2*max_pairs), then pairs of slots
  hipError_t extract(int n_frames, const uint8_t* d_frames, long long frame_stride, int row_stride, int first_slot,
                     hipStream_t st);
  // slot_limit > 0: slots at or beyond it give n_out = -1 for the pair (the public entry points pass 2 * max_pairs, so a
  // caller cannot reach the handle's private cache slots); 0: every slot of the pipeline
  hipError_t match_slots(int n_pairs, const int32_t* d_slot_a, const int32_t* d_slot_b, float threshold,
                         msf_match* d_out, int cap_per_pair, int32_t* d_n_out, hipStream_t st, int slot_limit = 0);
  // the matching head alone on caller-supplied post-transformer features (unscaled, [n_pairs][1200][32] each): the same
  // head inputs, kernels and debug copies as match(); not recorded in the stage-timing events (msf_debug_loftr_head)
  hipError_t head_only(int n_pairs, const float* d_f0, const float* d_f1, float threshold, msf_match* d_out,
                       int cap_per_pair, int32_t* d_n_out, hipStream_t st);
  // encoder blocks [first, first + n_blocks) alone (msf_debug_loftr_transformer): d_in0 / d_in1 are the two sequences
  // before block `first`, d_out0 / d_out1 receive them after the range ([n_pairs][1200][32] each); the same kernels and
  // arguments as match() (a layer pair's self-attention blocks share a launch when both are in the range); not timed
  hipError_t transformer_only(int n_pairs, int first, int n_blocks, const float* d_in0, const float* d_in1, float* d_out0,
                              float* d_out1, hipStream_t st);
  // the backbone alone (msf_debug_loftr_backbone): ONE pass of n frames from d_a and, when d_b is not null, n from d_b --
  // the two forms match() and extract() make -- with the kernels a match call of that many images takes on this handle;
  // tokens to d_tok_a / d_tok_b ([n][1200][32] each); with keep_debug the four layer activations of image act_image of
  // the pass (A frames first) are kept for debug_get; n at most backbone_chunk(); not timed
  hipError_t backbone_only(int n, const uint8_t* d_a, const uint8_t* d_b, long long frame_stride, int row_stride,
                           int act_image, float* d_tok_a, float* d_tok_b, hipStream_t st);
  int backbone_chunk() const;   // pairs per backbone pass
  int max_slots() const;
  int debug_get(int what, int slot, int level, void* host_out, size_t cap, size_t* n_bytes, std::string* err);
  int stage_times(const char** names, float* ms, int cap);

  struct Impl;

 private:
  hipError_t transformer_and_head(int n_pairs, float threshold, msf_match* d_out, int cap_per_pair, int32_t* d_n_out,
                                  hipStream_t st);
  // encoder blocks [first, first + n_blocks): block bi updates sequence bi % 2 from itself (bi % 4 < 2) or from the other
  // sequence; the whole range [0, 8) leaves the final features in tok[0] / tok[1], and the split path's blocks 6 and 7
  // also leave the head's inputs (fsc, fsp)
  void transformer(int n_pairs, int first, int n_blocks, hipStream_t st);
  // similarity, dual soft-max, threshold, decode on tok[0] / tok[1] (+ fsc / fsp on the split path)
  void head(int n_pairs, float threshold, msf_match* d_out, int cap_per_pair, int32_t* d_n_out, hipStream_t st);
  Impl* p_ = nullptr;
};

}  // namespace msf
