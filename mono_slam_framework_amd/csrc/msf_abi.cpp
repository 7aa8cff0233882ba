// extern "C" boundary of libmsf.so (declarations + the reference interfaces they replace: include/msf_abi.h).
// Here: the handle's lifetime, the matcher, the frame store and cache, the renderer, the debug hooks and the weight
// tools, and the bodies of what abi_core.h declares.  The geometry families are in abi_<family>.cpp.
#include "abi_core.h"

#include <cstdlib>
#include <cstring>
#include <new>

#include "weights_io.h"

namespace msf {
hipError_t pack_matches(int n, const msf_match* d_in, int cap, const int32_t* d_cnt, msf_match* d_packed,
                        int32_t* d_offsets, hipStream_t st);
hipError_t count_mappoint_matches(int n, const msf_match* d_matches, int cap, const int32_t* d_cnt,
                                  const int32_t* d_map_a, const int32_t* d_map_b, const uint32_t* d_maps, int n_maps,
                                  int map_words, int width, int height, int32_t* d_num_mp, hipStream_t st);
hipError_t render_match_image(const uint8_t* d_f1, const uint8_t* d_f2, int w, int h, long long pitch,
                              const msf_match* d_m, const uint8_t* d_mp1, const uint8_t* d_mp2, int n, uint8_t* d_out,
                              long long out_stride, hipStream_t st);
}

namespace msf {
namespace abi {

thread_local std::string g_create_error;

int fail(msf_handle* h, int code, const std::string& msg) {
  if (h) h->err = msg; else g_create_error = msg;
  return code;
}

int hip_fail(msf_handle* h, const char* what, hipError_t e) {
  return fail(h, MSF_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

int host_exception(msf_handle* h, const char* where) noexcept {
  try {
    fail(h, MSF_ERR_HIP, std::string(where) + ": host exception (out of memory?)");
  } catch (...) {
  }
  return MSF_ERR_HIP;
}

int fetch(msf_handle* h, hipStream_t st, void* dst, const void* src, size_t bytes) {
  if (!dst || !bytes) return MSF_OK;
  HIP_TRY(h, "hipMemcpyAsync", hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st));
  return MSF_OK;
}

const char* const kNoResult = "at least one pair has no valid result (n_out = -1): a fixed-capacity device list "
                              "overflowed, or a unit of the ORB walker launch gave up a bounded wait";

// pairs of slots -> match lists; slot_limit as in the pipelines (0 = every slot, the handle's private ones included)
int match_slot_pairs(msf_handle* h, int n, const int32_t* d_a, const int32_t* d_b, msf_match* d_out, int cap,
                     int32_t* d_n_out, hipStream_t st, int slot_limit) {
  HIP_TRY(h, "match slots",
          h->cfg.kind == MSF_KIND_ORB
              ? h->orb.match(n, d_a, d_b, h->cfg.threshold, d_out, cap, d_n_out, st, 0, slot_limit)
              : h->loftr.match_slots(n, d_a, d_b, h->cfg.threshold, d_out, cap, d_n_out, st, slot_limit));
  return MSF_OK;
}

// What reaches a caller with room for `cap` matches of a pair whose device count is `c`: the staging list keeps
// stage_cap of them.  Sets *capacity when the count is -1 (the pair has no list) or the staging list is shorter than
// what the caller asked for.
int deliverable(const msf_handle* h, int32_t c, int32_t cap, bool* capacity) {
  if (c < 0) {
    *capacity = true;
    return 0;
  }
  const int avail = c < h->stage_cap ? c : h->stage_cap;
  if (avail < c && cap > avail) *capacity = true;
  return avail < cap ? avail : cap;
}

// The front half of the one-vs-many entry points (msf_match_one_to_many, msf_create_map_points), n > 0.
// one_to_many_args: the checks on the slots, with the entry point's name in front of the message.
int one_to_many_args(msf_handle* h, const char* name, int32_t query_slot, int32_t n, const int32_t* slots) {
  const int maxp = h->cfg.max_batch_pairs;
  const std::string who = std::string(name) + ": ";
  if (n > maxp) return fail(h, MSF_ERR_INVALID_ARG, who + "n exceeds max_batch_pairs");
  if (!h->d_store) return fail(h, MSF_ERR_INVALID_ARG, who + "no frame was stored");
  if (query_slot < 0 || query_slot >= 2 * maxp) return fail(h, MSF_ERR_INVALID_ARG, who + "bad query slot");
  for (int i = 0; i < n; i++)
    if (slots[i] < 0 || slots[i] >= 2 * maxp) return fail(h, MSF_ERR_INVALID_ARG, who + "bad slot");
  return MSF_OK;
}

// launch_one_to_many: the slot arrays to the device (h->d_idx: query slot per pair, then train slot per pair), then the
// match of the n pairs into the handle's lists h->d_out [n][stage_cap] and counts h->d_n [n].
int launch_one_to_many(msf_handle* h, int32_t query_slot, int32_t n, const int32_t* slots, hipStream_t st) {
  const int maxp = h->cfg.max_batch_pairs;
  int32_t* d_query = h->d_idx;
  int32_t* d_train = h->d_idx + maxp;
  h->idx_stage.resize((size_t)2 * maxp);
  for (int i = 0; i < n; i++) { h->idx_stage[i] = query_slot; h->idx_stage[maxp + i] = slots[i]; }
  HIP_TRY(h, "hipMemcpyAsync(idx)",
          hipMemcpyAsync(d_query, h->idx_stage.data(), (size_t)2 * maxp * sizeof(int32_t), hipMemcpyHostToDevice, st));
  return match_slot_pairs(h, n, d_query, d_train, h->d_out, h->stage_cap, h->d_n, st, 0);
}

}  // namespace abi
}  // namespace msf

using namespace msf::abi;

namespace {

constexpr int kFrameCacheSlots = 64;   // default capacity of the transparent frame cache (MSF_FRAME_CACHE_SLOTS overrides)
constexpr int kPinMatches = 1024;  // matches fetched together with the count by the single-pair call
constexpr int kStageCap = 4096;  // matches per pair kept by the host-image path (ORB <= n1 <= 2048; LoFTR: see below)
constexpr size_t kRenderRecord = sizeof(msf_match) + 2;   // msf_render_match_image: a match and its two map-point flags

bool image_ok(const msf_handle* h, const msf_image* im) {
  return im && im->data && im->width == h->cfg.image_width && im->height == h->cfg.image_height &&
         im->stride >= h->cfg.image_width;
}

// one host frame into a staging frame (rows h->stage_pitch apart)
int upload_frame(msf_handle* h, uint8_t* dst, const msf_image* im, hipStream_t st) {
  HIP_TRY(h, "hipMemcpy2DAsync", hipMemcpy2DAsync(dst, h->stage_pitch, im->data, im->stride, h->cfg.image_width,
                                                   h->cfg.image_height, hipMemcpyHostToDevice, st));
  return MSF_OK;
}

// per-frame part of n frames (ORB features / LoFTR backbone tokens) into slots slot0 ..
int extract_into_slots(msf_handle* h, const uint8_t* d_frames, int n, long long frame_stride, long long row_stride,
                       int slot0, hipStream_t st) {
  if (h->cfg.kind == MSF_KIND_ORB) {
    msf::FrameSrc src{d_frames, d_frames, n, slot0, frame_stride, (int)row_stride};
    HIP_TRY(h, "orb extract", h->orb.extract(src, n, st));
  } else {
    HIP_TRY(h, "loftr extract", h->loftr.extract(n, d_frames, frame_stride, (int)row_stride, slot0, st));
  }
  return MSF_OK;
}

int run_device(msf_handle* h, int n_pairs, const uint8_t* d_a, const uint8_t* d_b, long long frame_stride,
               long long row_stride, msf_match* d_out, int cap, int32_t* d_n_out, hipStream_t st) {
  if (n_pairs <= 0) return MSF_OK;
  if (n_pairs > h->cfg.max_batch_pairs) return fail(h, MSF_ERR_INVALID_ARG, "n_pairs exceeds max_batch_pairs");
  if (!aligned16(d_a, d_b, frame_stride, row_stride))
    return fail(h, MSF_ERR_INVALID_ARG, "device frames must be 16-byte aligned with strides multiple of 16");
  if (row_stride < h->cfg.image_width) return fail(h, MSF_ERR_INVALID_ARG, "row_stride < image_width");
  if (frame_stride < row_stride * (long long)h->cfg.image_height)
    return fail(h, MSF_ERR_INVALID_ARG, "frame_stride < row_stride * image_height (frames would overlap)");
  if (h->cfg.kind == MSF_KIND_ORB) {
    // the stateless MatchFrames path works in its own feature slots [2P, 4P): slots [0, 2P) are the per-frame cache of
    // msf_extract_device / msf_store_frame, which a MatchFrames call on the same handle must not disturb
    // (KeyFrameMatchDatabase and Tracking share one matcher, src/main.cpp:77-81)
    const int scratch0 = 2 * h->cfg.max_batch_pairs;
    msf::FrameSrc src{d_a, d_b, n_pairs, scratch0, frame_stride, (int)row_stride};
    HIP_TRY(h, "orb extract", h->orb.extract(src, 2 * n_pairs, st));
    if (h->orb.take_degraded_note())    // not an error of THIS call: the text is there for whoever reads msf_last_error
      h->err = "note: a unit of an earlier ORB walker launch gave up a bounded wait (its pairs reported n_out = -1); "
               "this handle now launches the walker one level at a time";
    HIP_TRY(h, "orb match", h->orb.match(n_pairs, nullptr, nullptr, h->cfg.threshold, d_out, cap, d_n_out, st, scratch0));
    return MSF_OK;
  }
  HIP_TRY(h, "loftr match", h->loftr.match(n_pairs, d_a, d_b, frame_stride, (int)row_stride, h->cfg.threshold, d_out,
                                           cap, d_n_out, st));
  return MSF_OK;
}

int ensure_stage(msf_handle* h) {
  if (h->d_stage) return MSF_OK;
  const int W = h->cfg.image_width, H = h->cfg.image_height, maxp = h->cfg.max_batch_pairs;
  h->stage_pitch = (W + 15) & ~15;
  h->stage_frame = (long long)h->stage_pitch * H;
  h->stage_cap = kStageCap;
  HIP_TRY(h, "hipMalloc stage", h->d_stage.reserve((size_t)2 * maxp * h->stage_frame));
  // one leading record in front of the lists: the single-pair call puts its count there, so count + list come back
  // in ONE device-to-host copy into pinned memory (one synchronisation per MatchFrames call instead of two)
  HIP_TRY(h, "hipMalloc out", h->d_out_base.reserve(((size_t)maxp * h->stage_cap + 1) * sizeof(msf_match)));
  h->d_out = h->d_out_base + 1;
  HIP_TRY(h, "hipHostMalloc", hipHostMalloc(&h->h_pin, (size_t)(kPinMatches + 1) * sizeof(msf_match), hipHostMallocDefault));
  HIP_TRY(h, "hipMalloc n", h->d_n.reserve((size_t)maxp * sizeof(int32_t)));
  return MSF_OK;
}

int32_t* single_count(msf_handle* h) { return reinterpret_cast<int32_t*>(h->d_out_base.p); }   // the leading record

int ensure_maps(msf_handle* h) {
  if (h->d_maps) return MSF_OK;
  const int n_maps = 2 * h->cfg.max_batch_pairs;
  const long long n_px = (long long)h->cfg.image_width * h->cfg.image_height;
  h->map_words = (int)((n_px + 31) / 32);
  const size_t bytes = (size_t)n_maps * h->map_words * sizeof(uint32_t);
  HIP_TRY(h, "hipMalloc(map bitmaps)", h->d_maps.reserve(bytes));
  HIP_TRY(h, "hipMemsetAsync", hipMemsetAsync(h->d_maps, 0, bytes, h->stream));
  h->n_maps = n_maps;
  return MSF_OK;
}

// 64-bit content hash of a W x H frame with row stride: four independent multiply-xorshift lanes over 8-byte words
// (one dependent chain would run at a quarter of the speed), folded at the end.
uint64_t hash_image(const msf_image* im) {
  const uint64_t K0 = 0x9E3779B97F4A7C15ull, K1 = 0xC2B2AE3D27D4EB4Full, K2 = 0x165667B19E3779F9ull, K3 = 0xD6E8FEB86659FD93ull;
  uint64_t h0 = K0 ^ (uint64_t)im->width, h1 = K1 ^ (uint64_t)im->height, h2 = K2, h3 = K3;
  const int W = im->width;
  for (int y = 0; y < im->height; y++) {
    const uint8_t* p = im->data + (size_t)y * (size_t)im->stride;
    int x = 0;
    for (; x + 32 <= W; x += 32) {
      uint64_t a, b, c, d;
      std::memcpy(&a, p + x, 8); std::memcpy(&b, p + x + 8, 8); std::memcpy(&c, p + x + 16, 8); std::memcpy(&d, p + x + 24, 8);
      h0 = (h0 ^ a) * K1; h0 ^= h0 >> 29;
      h1 = (h1 ^ b) * K2; h1 ^= h1 >> 31;
      h2 = (h2 ^ c) * K3; h2 ^= h2 >> 30;
      h3 = (h3 ^ d) * K0; h3 ^= h3 >> 28;
    }
    uint64_t tail = 0;
    for (; x < W; x++) tail = (tail << 8) ^ p[x] ^ (tail >> 56);
    h0 = (h0 ^ tail ^ (uint64_t)y) * K2; h0 ^= h0 >> 32;
  }
  uint64_t h = h0 ^ (h1 * K3) ^ (h2 * K0) ^ (h3 * K1);
  h ^= h >> 33; h *= 0xFF51AFD7ED558CCDull; h ^= h >> 33; h *= 0xC4CEB9FE1A85EC53ull; h ^= h >> 33;
  return h;
}

bool same_bytes(const msf_image* im, const std::vector<uint8_t>& bytes) {
  const size_t W = (size_t)im->width;
  for (int y = 0; y < im->height; y++)
    if (std::memcmp(im->data + (size_t)y * (size_t)im->stride, bytes.data() + (size_t)y * W, W) != 0) return false;
  return true;
}

// Slot of `im` in the frame cache, extracting it first if it is not there.  `keep` = an entry that must not be evicted
// (the other frame of the same call), or -1.  `d_stage_frame` = where to upload the frame for an extraction.
int cached_slot(msf_handle* h, const msf_image* im, int keep, uint8_t* d_stage_frame, hipStream_t st, int* entry_out) {
  const int W = h->cfg.image_width, H = h->cfg.image_height;
  const uint64_t hv = hash_image(im) & h->fc_hash_mask;
  int victim = -1;   // an unused entry, else the least recently used one; never `keep`
  for (int i = 0; i < (int)h->fc.size(); i++) {
    msf_handle::CacheEntry& e = h->fc[i];
    if (e.valid && e.hash == hv && same_bytes(im, e.bytes)) {
      e.used = ++h->fc_tick;
      h->fc_hits++;
      *entry_out = i;
      return MSF_OK;
    }
    if (i == keep) continue;
    const uint64_t age = e.valid ? e.used : 0;            // invalid entries first
    if (victim < 0 || age < (h->fc[victim].valid ? h->fc[victim].used : 0)) victim = i;
  }
  if (victim < 0) return fail(h, MSF_ERR_INVALID_ARG, "frame cache has no replaceable entry");
  msf_handle::CacheEntry& e = h->fc[victim];
  e.valid = false;
  e.bytes.resize((size_t)W * H);
  for (int y = 0; y < H; y++) std::memcpy(e.bytes.data() + (size_t)y * W, im->data + (size_t)y * (size_t)im->stride, (size_t)W);
  const msf_image kept{e.bytes.data(), W, H, W};
  if (int rc = upload_frame(h, d_stage_frame, &kept, st)) return rc;
  if (int rc = extract_into_slots(h, d_stage_frame, 1, h->stage_frame, h->stage_pitch, h->fc_slot0 + victim, st)) return rc;
  e.hash = hv;
  e.used = ++h->fc_tick;
  e.valid = true;
  h->fc_misses++;
  *entry_out = victim;
  return MSF_OK;
}

// Lists of the n pairs of one staged call, counts already on the host: pair i to out + i * cap_per_pair (out = NULL:
// the caller wants the counts only).  A pair that sets *capacity does not stop the lists of the others.
int copy_lists_back(msf_handle* h, int n, const int32_t* counts, msf_match* out, int32_t cap_per_pair, bool* capacity) {
  for (int i = 0; i < n; i++) {
    const int w = deliverable(h, counts[i], out ? cap_per_pair : 0, capacity);
    if (w > 0)
      HIP_TRY(h, "hipMemcpy", hipMemcpy(out + (size_t)i * cap_per_pair, h->d_out + (size_t)i * h->stage_cap,
                                        (size_t)w * sizeof(msf_match), hipMemcpyDeviceToHost));
  }
  return MSF_OK;
}

// count (in the record before the list) + list of the single-pair call: one copy, one synchronisation
int fetch_single(msf_handle* h, msf_match* out, int32_t cap_per_pair, int32_t* n_out, hipStream_t st) {
  const int wmax = cap_per_pair < h->stage_cap ? cap_per_pair : h->stage_cap;
  const int wfirst = wmax < kPinMatches ? wmax : kPinMatches;
  HIP_TRY(h, "hipMemcpyAsync", hipMemcpyAsync(h->h_pin, h->d_out_base, (size_t)(1 + wfirst) * sizeof(msf_match),
                                              hipMemcpyDeviceToHost, st));
  HIP_TRY(h, "hipStreamSynchronize", hipStreamSynchronize(st));
  n_out[0] = *reinterpret_cast<const int32_t*>(h->h_pin);
  bool capacity = false;
  const int w = deliverable(h, n_out[0], cap_per_pair, &capacity);
  const int w1 = w < wfirst ? w : wfirst;
  if (w1 > 0) std::memcpy(out, h->h_pin + 1, (size_t)w1 * sizeof(msf_match));
  if (w > w1)   // a list longer than the pinned part: the rest straight from the staging list
    HIP_TRY(h, "hipMemcpy", hipMemcpy(out + w1, h->d_out + w1, (size_t)(w - w1) * sizeof(msf_match), hipMemcpyDeviceToHost));
  return capacity ? fail(h, MSF_ERR_CAPACITY, kNoResult) : MSF_OK;
}

// MatchFrames(a, b) through the frame cache: per frame a hash + byte compare on the host; only frames not seen lately
// are uploaded and extracted; then one slot-pair match.  Same lists as the stateless path (tests/test_frame_cache_gpu.py).
int match_pair_cached(msf_handle* h, const msf_image* a, const msf_image* b, msf_match* out, int32_t cap, int32_t* n_out,
                      hipStream_t st) {
  uint8_t* dA = h->d_stage;
  uint8_t* dB = h->d_stage + (size_t)h->cfg.max_batch_pairs * h->stage_frame;
  int ea = -1, eb = -1;
  if (int rc = cached_slot(h, a, -1, dA, st, &ea)) return rc;
  if (int rc = cached_slot(h, b, ea, dB, st, &eb)) return rc;
  int rc = match_slot_pairs(h, 1, h->d_fc_slots + ea, h->d_fc_slots + eb, h->d_out, h->stage_cap, single_count(h), st, 0);
  if (rc == MSF_OK) rc = fetch_single(h, out, cap, n_out, st);
  if (rc != MSF_OK) {
    // the extractions of this call may not have completed, and a failed (or overflowed) frame must not be served from
    // the cache again: forget both entries
    h->fc[ea].valid = false;
    h->fc[eb].valid = false;
  }
  return rc;
}

}  // namespace

extern "C" {

int msf_abi_version(void) { return MSF_ABI_VERSION; }

void msf_default_config(msf_config* cfg, int kind) {
  if (!cfg) return;
  *cfg = msf_config{};
  cfg->struct_size = sizeof(msf_config);
  cfg->kind = kind;
  cfg->device = 0;
  cfg->threshold = kind == MSF_KIND_LOFTR ? 0.15f : 0.8f;  // dnnfeaturematcher.h:11 / featurematcher.h:9
  cfg->image_width = 640;                                  // dnnfeaturematcher.h:12-13
  cfg->image_height = 480;
  cfg->max_batch_pairs = 1;
  cfg->flags = 0;
  cfg->weights_path = nullptr;
}

int msf_create(const msf_config* cfg, msf_handle** out) {
  return guarded("msf_create", [&]() -> int {
    if (!cfg || !out) return fail(nullptr, MSF_ERR_INVALID_ARG, "msf_create: null argument");
    *out = nullptr;
    if (cfg->struct_size != sizeof(msf_config)) return fail(nullptr, MSF_ERR_INVALID_ARG, "msf_create: struct_size mismatch");
    if (cfg->kind != MSF_KIND_ORB && cfg->kind != MSF_KIND_LOFTR) return fail(nullptr, MSF_ERR_INVALID_ARG, "msf_create: bad kind");
    if (cfg->max_batch_pairs < 1) return fail(nullptr, MSF_ERR_INVALID_ARG, "msf_create: max_batch_pairs < 1");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
      return fail(nullptr, MSF_ERR_HIP, "msf_create: no HIP device (this library has no CPU fallback)");
    if (cfg->device < 0 || cfg->device >= ndev) return fail(nullptr, MSF_ERR_INVALID_ARG, "msf_create: device ordinal out of range");
    HIP_TRY(nullptr, "hipSetDevice", hipSetDevice(cfg->device));
    msf_handle* h = new (std::nothrow) msf_handle();
    if (!h) return fail(nullptr, MSF_ERR_HIP, "out of host memory");
    struct Guard {   // whatever path leaves this function without success (an exception included) frees the handle
      msf_handle* h;
      ~Guard() { if (h) msf_destroy(h); }
    } guard{h};
    h->cfg = *cfg;
    h->cfg.weights_path = nullptr;
    std::string err;
    const bool profile = (cfg->flags & MSF_FLAG_PROFILE) != 0;
    int n_cache = kFrameCacheSlots;
    if (const char* ev = getenv("MSF_FRAME_CACHE_SLOTS")) n_cache = atoi(ev);
    if (cfg->flags & MSF_FLAG_NO_FRAME_CACHE) n_cache = 0;          // the flag wins over the environment
    n_cache = n_cache < 2 ? 0 : n_cache > 4096 ? 4096 : n_cache;   // a pair needs two entries
    if (const char* ev = getenv("MSF_FRAME_CACHE_HASH_BITS")) {    // tests: a few bits make hash collisions the rule
      const int bits = atoi(ev);
      if (bits >= 0 && bits < 64) h->fc_hash_mask = (1ull << bits) - 1ull;
    }
    if (cfg->kind == MSF_KIND_ORB) {
      h->fc_slot0 = 4 * cfg->max_batch_pairs;
      msf::OrbOptions o;
      o.width = cfg->image_width;
      o.height = cfg->image_height;
      o.max_slots = 4 * cfg->max_batch_pairs + n_cache;
      o.work_frames = 2 * cfg->max_batch_pairs;
      o.blur_half_up = (cfg->flags & MSF_FLAG_BLUR_TIE_HALF_UP) != 0;
      o.blur_sum256 = (cfg->flags & MSF_FLAG_BLUR_SUM256) != 0;
      o.profile = profile;
      o.dense_fast = (cfg->flags & MSF_FLAG_FAST_DENSE) != 0;
      o.level_size_mul_inv = (cfg->flags & MSF_FLAG_LEVEL_SIZE_MUL_INV) != 0;
      o.stream_min_frames = (cfg->flags & MSF_FLAG_FAST_STREAM) ? 1 : 8;
      err = h->orb.init(o);
    } else {
      if (cfg->image_width != 640 || cfg->image_height != 480)
        return fail(nullptr, MSF_ERR_UNSUPPORTED, "LoFTR_teacher is a fixed-shape 1x1x480x640 graph (model/LoFTR_teacher.onnx)");
      h->fc_slot0 = 2 * cfg->max_batch_pairs;
      err = h->loftr.init(cfg->weights_path, cfg->max_batch_pairs, profile, (cfg->flags & MSF_FLAG_KEEP_DEBUG) != 0, n_cache,
                          (cfg->flags & MSF_FLAG_LOFTR_F32) != 0);
    }
    if (!err.empty()) {
      const bool io = err.rfind("io:", 0) == 0, arg = err.rfind("arg:", 0) == 0;
      return fail(nullptr, io ? MSF_ERR_IO : arg ? MSF_ERR_INVALID_ARG : MSF_ERR_HIP, err);
    }
    // hipStreamDefault (a "blocking" stream): work on the handle's own stream is ordered against the legacy null stream,
    // which is where a caller that passes stream = NULL (e.g. torch's default stream) has its own work (msf_abi.h)
    HIP_TRY(nullptr, "hipStreamCreate", hipStreamCreateWithFlags(&h->stream, hipStreamDefault));
    if (n_cache > 0) {
      std::vector<int32_t> ids(n_cache);
      for (int i = 0; i < n_cache; i++) ids[i] = h->fc_slot0 + i;
      const size_t bytes = (size_t)n_cache * sizeof(int32_t);
      HIP_TRY(nullptr, "hipMalloc(frame cache slots)", h->d_fc_slots.reserve(bytes));
      HIP_TRY(nullptr, "hipMalloc(frame cache slots)", hipMemcpy(h->d_fc_slots, ids.data(), bytes, hipMemcpyHostToDevice));
      h->fc.resize(n_cache);
    }
    guard.h = nullptr;
    *out = h;
    return MSF_OK;
  });
}

void msf_destroy(msf_handle* h) {
  if (!h) return;
  hipSetDevice(h->cfg.device);
  hipDeviceSynchronize();
  h->orb.destroy();
  h->loftr.destroy();
  if (h->h_pin) hipHostFree(h->h_pin);
  if (h->h_gba_rec) hipHostFree(h->h_gba_rec);
  const hipStream_t stream = h->stream;
  delete h;   // the device buffers go with their DevBuf members, before the stream
  if (stream) hipStreamDestroy(stream);
}

int msf_set_threshold(msf_handle* h, float value) {
  return guarded(h, "msf_set_threshold", [&]() -> int {
    h->cfg.threshold = value;
    return MSF_OK;
  });
}

const char* msf_last_error(const msf_handle* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int msf_match_batch_device(msf_handle* h, int32_t n_pairs, const uint8_t* d_a, const uint8_t* d_b,
                           int64_t frame_stride, int64_t row_stride, msf_match* d_out, int32_t cap_per_pair,
                           int32_t* d_n_out, void* stream) {
  return guarded(h, "msf_match_batch_device", [&]() -> int {
    if (n_pairs < 0 || !d_a || !d_b || !d_out || !d_n_out || cap_per_pair < 1)
      return fail(h, MSF_ERR_INVALID_ARG, "msf_match_batch_device: bad argument");
    CallScope cs{h};
    if (int rc = cs.enter(stream)) return rc;
    if (int rc = run_device(h, n_pairs, d_a, d_b, frame_stride, row_stride, d_out, cap_per_pair, d_n_out, cs.st)) return rc;
    return cs.finish();
  });
}

int msf_match_batch(msf_handle* h, int32_t n_pairs, const msf_image* a, const msf_image* b, msf_match* out,
                    int32_t cap_per_pair, int32_t* n_out) {
  return guarded(h, "msf_match_batch", [&]() -> int {
    if (n_pairs < 0 || !a || !b || !out || !n_out || cap_per_pair < 1)
      return fail(h, MSF_ERR_INVALID_ARG, "msf_match_batch: bad argument");
    CallScope cs{h};
    if (int rc = cs.enter()) return rc;
    for (int i = 0; i < n_pairs; i++)
      if (!image_ok(h, &a[i]) || !image_ok(h, &b[i]))
        return fail(h, MSF_ERR_INVALID_ARG, "msf_match_batch: image size differs from the handle's, or null data");
    if (int rc = ensure_stage(h)) return rc;
    const int maxp = h->cfg.max_batch_pairs;
    hipStream_t st = cs.st;
    uint8_t* dA = h->d_stage;
    uint8_t* dB = h->d_stage + (size_t)maxp * h->stage_frame;
    if (n_pairs == 1) {   // the drop-in call: count in the record before the list, one copy, one synchronisation
      if (!h->fc.empty()) return match_pair_cached(h, &a[0], &b[0], out, cap_per_pair, n_out, st);
      if (int rc = upload_frame(h, dA, &a[0], st)) return rc;
      if (int rc = upload_frame(h, dB, &b[0], st)) return rc;
      if (int rc = run_device(h, 1, dA, dB, h->stage_frame, h->stage_pitch, h->d_out, h->stage_cap, single_count(h), st)) return rc;
      return fetch_single(h, out, cap_per_pair, n_out, st);
    }
    bool capacity = false;
    for (int p0 = 0; p0 < n_pairs; p0 += maxp) {   // chunks of max_batch_pairs: the counts, one wait, then the lists
      const int n = n_pairs - p0 < maxp ? n_pairs - p0 : maxp;
      for (int i = 0; i < n; i++) {
        if (int rc = upload_frame(h, dA + (size_t)i * h->stage_frame, &a[p0 + i], st)) return rc;
        if (int rc = upload_frame(h, dB + (size_t)i * h->stage_frame, &b[p0 + i], st)) return rc;
      }
      if (int rc = run_device(h, n, dA, dB, h->stage_frame, h->stage_pitch, h->d_out, h->stage_cap, h->d_n, st)) return rc;
      HIP_TRY(h, "hipMemcpyAsync", hipMemcpyAsync(n_out + p0, h->d_n, (size_t)n * 4, hipMemcpyDeviceToHost, st));
      HIP_TRY(h, "hipStreamSynchronize", hipStreamSynchronize(st));
      if (int rc = copy_lists_back(h, n, n_out + p0, out + (size_t)p0 * cap_per_pair, cap_per_pair, &capacity)) return rc;
    }
    return capacity ? fail(h, MSF_ERR_CAPACITY, kNoResult) : MSF_OK;
  });
}

int msf_match_pair(msf_handle* h, const msf_image* a, const msf_image* b, msf_match* out, int32_t cap,
                   int32_t* n_out) {
  return msf_match_batch(h, 1, a, b, out, cap, n_out);
}

int msf_extract_device(msf_handle* h, int32_t n_frames, const uint8_t* d_frames, int64_t frame_stride,
                       int64_t row_stride, int32_t first_slot, void* stream) {
  return guarded(h, "msf_extract_device", [&]() -> int {
    // both kinds: the caller's slots are [0, 2P); what lies beyond (scratch of the stateless calls, the transparent
    // frame cache) belongs to the handle
    if (n_frames < 0 || !d_frames || first_slot < 0 || (long long)first_slot + n_frames > 2ll * h->cfg.max_batch_pairs)
      return fail(h, MSF_ERR_INVALID_ARG, "msf_extract_device: slot range outside [0, 2*max_batch_pairs)");
    if (!aligned16(d_frames, frame_stride, row_stride))
      return fail(h, MSF_ERR_INVALID_ARG, "device frames must be 16-byte aligned with strides multiple of 16");
    CallScope cs{h};
    if (int rc = cs.enter(stream)) return rc;
    if (row_stride < h->cfg.image_width ||
        (n_frames > 1 && frame_stride < row_stride * (long long)h->cfg.image_height))   // one frame: its stride is unused
      return fail(h, MSF_ERR_INVALID_ARG, "msf_extract_device: strides smaller than the frame");
    if (int rc = extract_into_slots(h, d_frames, n_frames, frame_stride, row_stride, first_slot, cs.st)) return rc;
    return cs.finish();
  });
}

int msf_match_slots_device(msf_handle* h, int32_t n_pairs, const int32_t* d_slot_a, const int32_t* d_slot_b,
                           msf_match* d_out, int32_t cap_per_pair, int32_t* d_n_out, void* stream) {
  return guarded(h, "msf_match_slots_device", [&]() -> int {
    if (n_pairs < 0 || !d_slot_a || !d_slot_b || !d_out || !d_n_out || cap_per_pair < 1)
      return fail(h, MSF_ERR_INVALID_ARG, "msf_match_slots_device: bad argument");
    CallScope cs{h};
    if (int rc = cs.enter(stream)) return rc;
    if (h->cfg.kind != MSF_KIND_ORB && n_pairs > h->cfg.max_batch_pairs)   // LoFTR works on per-pair token buffers
      return fail(h, MSF_ERR_INVALID_ARG, "n_pairs exceeds max_batch_pairs");
    if (int rc = match_slot_pairs(h, n_pairs, d_slot_a, d_slot_b, d_out, cap_per_pair, d_n_out, cs.st,
                                  2 * h->cfg.max_batch_pairs))   // the caller's slots only
      return rc;
    return cs.finish();
  });
}

int msf_pack_matches_device(msf_handle* h, int32_t n_pairs, const msf_match* d_in, int32_t cap_per_pair,
                            const int32_t* d_n_out, msf_match* d_packed, int32_t* d_offsets, void* stream) {
  return guarded(h, "msf_pack_matches_device", [&]() -> int {
    if (n_pairs < 0 || !d_in || !d_n_out || !d_packed || !d_offsets || cap_per_pair < 1)
      return fail(h, MSF_ERR_INVALID_ARG, "msf_pack_matches_device: bad argument");
    CallScope cs{h};
    if (int rc = cs.enter(stream)) return rc;
    HIP_TRY(h, "pack_matches", msf::pack_matches(n_pairs, d_in, cap_per_pair, d_n_out, d_packed, d_offsets, cs.st));
    return cs.finish();
  });
}

int msf_set_mappoints(msf_handle* h, int32_t map_slot, const int32_t* keys, int32_t n_keys) {
  return guarded(h, "msf_set_mappoints", [&]() -> int {
    const int n_maps = 2 * h->cfg.max_batch_pairs;
    const long long n_px = (long long)h->cfg.image_width * h->cfg.image_height;
    if (map_slot < 0 || map_slot >= n_maps || n_keys < 0 || (n_keys > 0 && !keys))
      return fail(h, MSF_ERR_INVALID_ARG, "msf_set_mappoints: bad argument");
    CallScope cs{h};
    if (int rc = cs.enter()) return rc;
    if (int rc = ensure_maps(h)) return rc;
    h->map_stage.assign(h->map_words, 0u);
    for (int i = 0; i < n_keys; i++) {
      // KeyPointMap::SetMapPoint ignores points outside the image (KeyPointMap.cc:38-39); a key is y*cols + x
      if (keys[i] < 0 || keys[i] >= n_px) continue;
      h->map_stage[keys[i] >> 5] |= 1u << (keys[i] & 31);
    }
    HIP_TRY(h, "hipMemcpyAsync(map bitmap)",
            hipMemcpyAsync(h->d_maps + (size_t)map_slot * h->map_words, h->map_stage.data(),
                           (size_t)h->map_words * sizeof(uint32_t), hipMemcpyHostToDevice, cs.st));
    return cs.finish();
  });
}

int msf_count_mappoint_matches_device(msf_handle* h, int32_t n_pairs, const msf_match* d_matches,
                                      int32_t cap_per_pair, const int32_t* d_n_matches, const int32_t* d_map_a,
                                      const int32_t* d_map_b, int32_t* d_num_mp, void* stream) {
  return guarded(h, "msf_count_mappoint_matches_device", [&]() -> int {
    if (n_pairs < 0 || !d_matches || !d_n_matches || !d_map_a || !d_map_b || !d_num_mp || cap_per_pair < 1)
      return fail(h, MSF_ERR_INVALID_ARG, "msf_count_mappoint_matches_device: bad argument");
    if (!h->d_maps) return fail(h, MSF_ERR_INVALID_ARG, "msf_count_mappoint_matches_device: no map slot was ever set");
    CallScope cs{h};
    if (int rc = cs.enter(stream)) return rc;
    HIP_TRY(h, "count_mappoint_matches",
            msf::count_mappoint_matches(n_pairs, d_matches, cap_per_pair, d_n_matches, d_map_a, d_map_b, h->d_maps, h->n_maps,
                                        h->map_words, h->cfg.image_width, h->cfg.image_height, d_num_mp, cs.st));
    return cs.finish();
  });
}

int msf_store_frame(msf_handle* h, int32_t slot, const msf_image* img) {
  return guarded(h, "msf_store_frame", [&]() -> int {
    const int maxp = h->cfg.max_batch_pairs;
    if (slot < 0 || slot >= 2 * maxp || !image_ok(h, img))
      return fail(h, MSF_ERR_INVALID_ARG, "msf_store_frame: slot outside [0, 2*max_batch_pairs) or image size differs from the handle's");
    CallScope cs{h};
    if (int rc = cs.enter()) return rc;
    if (int rc = ensure_stage(h)) return rc;
    if (!h->d_store) {
      HIP_TRY(h, "hipMalloc(frame store)", h->d_store.reserve((size_t)2 * maxp * h->stage_frame));
      HIP_TRY(h, "hipMalloc(idx)", h->d_idx.reserve((size_t)3 * maxp * sizeof(int32_t)));
    }
    uint8_t* dst = h->d_store + (size_t)slot * h->stage_frame;
    if (int rc = upload_frame(h, dst, img, cs.st)) return rc;
    // features (ORB) / backbone tokens (LoFTR) of the frame are extracted once, here
    if (int rc = extract_into_slots(h, dst, 1, h->stage_frame, h->stage_pitch, slot, cs.st)) return rc;
    return cs.finish();
  });
}

int msf_match_one_to_many(msf_handle* h, int32_t query_slot, int32_t n, const int32_t* slots, int32_t* num_matches,
                          int32_t* num_mp, msf_match* out, int32_t cap_per_pair) {
  return guarded(h, "msf_match_one_to_many", [&]() -> int {
    const char* const name = "msf_match_one_to_many";
    if (n < 0 || (n > 0 && (!slots || !num_matches)) || (out && cap_per_pair < 1))
      return fail(h, MSF_ERR_INVALID_ARG, std::string(name) + ": bad argument");
    if (n == 0) return MSF_OK;
    if (int rc = one_to_many_args(h, name, query_slot, n, slots)) return rc;
    if (num_mp && !h->d_maps) return fail(h, MSF_ERR_INVALID_ARG, "msf_match_one_to_many: no map slot was ever set");
    CallScope cs{h};
    if (int rc = cs.enter()) return rc;
    hipStream_t st = cs.st;
    if (int rc = launch_one_to_many(h, query_slot, n, slots, st)) return rc;
    if (num_mp) {
      const int maxp = h->cfg.max_batch_pairs;
      int32_t* d_num_mp = h->d_idx + 2 * maxp;
      HIP_TRY(h, "count_mappoint_matches",
              msf::count_mappoint_matches(n, h->d_out, h->stage_cap, h->d_n, h->d_idx, h->d_idx + maxp, h->d_maps,
                                          h->n_maps, h->map_words, h->cfg.image_width, h->cfg.image_height, d_num_mp, st));
      HIP_TRY(h, "hipMemcpyAsync", hipMemcpyAsync(num_mp, d_num_mp, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(h, "hipMemcpyAsync", hipMemcpyAsync(num_matches, h->d_n, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    if (int rc = cs.finish()) return rc;
    bool capacity = false;
    if (int rc = copy_lists_back(h, n, num_matches, out, cap_per_pair, &capacity)) return rc;
    return capacity ? fail(h, MSF_ERR_CAPACITY, kNoResult) : MSF_OK;
  });
}


int msf_render_match_image(msf_handle* h, const msf_image* f1, const msf_image* f2, const msf_match* matches,
                           int32_t n_matches, const uint8_t* has_mp1, const uint8_t* has_mp2, uint8_t* out_rgb,
                           int64_t out_stride) {
  return guarded(h, "msf_render_match_image", [&]() -> int {
    const int W = h->cfg.image_width, H = h->cfg.image_height;
    if (!image_ok(h, f1) || !image_ok(h, f2) || n_matches < 0 || (n_matches > 0 && !matches) || !out_rgb || out_stride < 6ll * W)
      return fail(h, MSF_ERR_INVALID_ARG, "msf_render_match_image: bad argument or image size differs from the handle's");
    CallScope cs{h};
    if (int rc = cs.enter()) return rc;
    if (int rc = ensure_stage(h)) return rc;
    hipStream_t st = cs.st;
    // workspace: the two frames use the staging buffers; the RGB image is allocated by the first call, the list + flags
    // buffer grows when a call brings more matches than any before it (no allocation in the steady state)
    uint8_t* dA = h->d_stage;
    uint8_t* dB = h->d_stage + (size_t)h->cfg.max_batch_pairs * h->stage_frame;
    if (!h->d_render) HIP_TRY(h, "hipMalloc(render image)", h->d_render.reserve((size_t)6 * W * H));
    if ((size_t)n_matches * kRenderRecord > h->d_render_m.bytes) {
      HIP_TRY(h, "hipStreamSynchronize", hipStreamSynchronize(st));
      HIP_TRY(h, "hipMalloc(render list)", h->d_render_m.reserve((size_t)n_matches * kRenderRecord, 4096 * kRenderRecord));
    }
    msf_match* d_m = n_matches ? h->d_render_m.p : nullptr;
    uint8_t* d_flags = n_matches ? reinterpret_cast<uint8_t*>(h->d_render_m + h->d_render_m.bytes / kRenderRecord) : nullptr;
    Drain drain{st};
    if (n_matches) {
      HIP_TRY(h, "hipMemcpyAsync", hipMemcpyAsync(d_m, matches, (size_t)n_matches * sizeof(msf_match), hipMemcpyHostToDevice, st));
      HIP_TRY(h, "hipMemsetAsync", hipMemsetAsync(d_flags, 0, (size_t)2 * n_matches, st));
      if (has_mp1) HIP_TRY(h, "hipMemcpyAsync", hipMemcpyAsync(d_flags, has_mp1, n_matches, hipMemcpyHostToDevice, st));
      if (has_mp2) HIP_TRY(h, "hipMemcpyAsync", hipMemcpyAsync(d_flags + n_matches, has_mp2, n_matches, hipMemcpyHostToDevice, st));
    }
    if (int rc = upload_frame(h, dA, f1, st)) return rc;
    if (int rc = upload_frame(h, dB, f2, st)) return rc;
    HIP_TRY(h, "render_match_image",
            msf::render_match_image(dA, dB, W, H, h->stage_pitch, d_m, d_flags, d_flags ? d_flags + n_matches : nullptr,
                                    n_matches, h->d_render, 6ll * W, st));
    HIP_TRY(h, "hipMemcpy2DAsync",
            hipMemcpy2DAsync(out_rgb, out_stride, h->d_render, (size_t)6 * W, (size_t)6 * W, H, hipMemcpyDeviceToHost, st));
    drain.armed = false;
    return cs.finish();   // the one wait of the call
  });
}

int msf_debug_get(msf_handle* h, int32_t what, int32_t slot, int32_t level, void* host_out, size_t cap_bytes,
                  size_t* n_bytes) {
  if (!n_bytes || (!host_out && cap_bytes)) return MSF_ERR_INVALID_ARG;   // refused before the lock, without a text
  return guarded(h, "msf_debug_get", [&]() -> int {
    CallScope cs{h};
    if (int rc = cs.enter()) return rc;
    std::string err;
    const int rc = h->cfg.kind == MSF_KIND_ORB ? h->orb.debug_get(what, slot, level, host_out, cap_bytes, n_bytes, &err)
                                               : h->loftr.debug_get(what, slot, level, host_out, cap_bytes, n_bytes, &err);
    return rc != 0 ? fail(h, rc, err) : MSF_OK;
  });
}

int msf_debug_loftr_head(msf_handle* h, int32_t n_pairs, const float* d_feat0, const float* d_feat1,
                         msf_match* d_out, int32_t cap_per_pair, int32_t* d_n_out, void* stream) {
  return guarded(h, "msf_debug_loftr_head", [&]() -> int {
    if (h->cfg.kind != MSF_KIND_LOFTR) return fail(h, MSF_ERR_INVALID_ARG, "msf_debug_loftr_head: not a LoFTR handle");
    if (n_pairs < 0 || n_pairs > h->cfg.max_batch_pairs || !d_feat0 || !d_feat1 || !d_out || !d_n_out || cap_per_pair < 1)
      return fail(h, MSF_ERR_INVALID_ARG, "msf_debug_loftr_head: bad argument");
    if (!aligned16(d_feat0, d_feat1, d_out) || ((uintptr_t)d_n_out & 3))
      return fail(h, MSF_ERR_INVALID_ARG, "msf_debug_loftr_head: misaligned pointer");
    CallScope cs{h};
    if (int rc = cs.enter(stream)) return rc;
    HIP_TRY(h, "loftr head", h->loftr.head_only(n_pairs, d_feat0, d_feat1, h->cfg.threshold, d_out, cap_per_pair, d_n_out, cs.st));
    return cs.finish();
  });
}

int msf_debug_loftr_transformer(msf_handle* h, int32_t n_pairs, int32_t first_block, int32_t n_blocks,
                                const float* d_in0, const float* d_in1, float* d_out0, float* d_out1, void* stream) {
  return guarded(h, "msf_debug_loftr_transformer", [&]() -> int {
    if (h->cfg.kind != MSF_KIND_LOFTR) return fail(h, MSF_ERR_INVALID_ARG, "msf_debug_loftr_transformer: not a LoFTR handle");
    if (n_pairs < 0 || n_pairs > h->cfg.max_batch_pairs || first_block < 0 || n_blocks < 1 || first_block + n_blocks > 8 ||
        !d_in0 || !d_in1 || !d_out0 || !d_out1)
      return fail(h, MSF_ERR_INVALID_ARG, "msf_debug_loftr_transformer: bad argument");
    if (!aligned16(d_in0, d_in1, d_out0, d_out1))
      return fail(h, MSF_ERR_INVALID_ARG, "msf_debug_loftr_transformer: misaligned pointer");
    CallScope cs{h};
    if (int rc = cs.enter(stream)) return rc;
    HIP_TRY(h, "loftr transformer", h->loftr.transformer_only(n_pairs, first_block, n_blocks, d_in0, d_in1, d_out0, d_out1, cs.st));
    return cs.finish();
  });
}

int msf_debug_loftr_backbone(msf_handle* h, int32_t n, const uint8_t* d_a, const uint8_t* d_b, int64_t frame_stride,
                             int64_t row_stride, int32_t act_image, float* d_tok_a, float* d_tok_b, void* stream) {
  return guarded(h, "msf_debug_loftr_backbone", [&]() -> int {
    if (h->cfg.kind != MSF_KIND_LOFTR) return fail(h, MSF_ERR_INVALID_ARG, "msf_debug_loftr_backbone: not a LoFTR handle");
    const int images = d_b ? 2 * n : n;
    if (n < 0 || n > h->loftr.backbone_chunk() || !d_a || !d_tok_a || (d_b && !d_tok_b) || act_image < 0 ||
        (n > 0 && act_image >= images))
      return fail(h, MSF_ERR_INVALID_ARG, "msf_debug_loftr_backbone: bad argument");
    if (!aligned16(d_a, d_b, frame_stride, row_stride, d_tok_a, d_tok_b))
      return fail(h, MSF_ERR_INVALID_ARG, "msf_debug_loftr_backbone: misaligned pointer");
    if (row_stride < h->cfg.image_width) return fail(h, MSF_ERR_INVALID_ARG, "row_stride < image_width");
    if (frame_stride < row_stride * (long long)h->cfg.image_height)
      return fail(h, MSF_ERR_INVALID_ARG, "frame_stride < row_stride * image_height (frames would overlap)");
    if (n == 0) return MSF_OK;
    CallScope cs{h};
    if (int rc = cs.enter(stream)) return rc;
    HIP_TRY(h, "loftr backbone", h->loftr.backbone_only(n, d_a, d_b, frame_stride, (int)row_stride, act_image, d_tok_a,
                                                        d_tok_b, cs.st));
    return cs.finish();
  });
}

int msf_debug_orb_set_features(msf_handle* h, int32_t slot, int32_t n, const msf_keypoint* kp, const uint8_t* desc) {
  return guarded(h, "msf_debug_orb_set_features", [&]() -> int {
    if (h->cfg.kind != MSF_KIND_ORB) return fail(h, MSF_ERR_INVALID_ARG, "msf_debug_orb_set_features: not an ORB handle");
    if (slot < 0 || slot >= 2 * h->cfg.max_batch_pairs)
      return fail(h, MSF_ERR_INVALID_ARG, "msf_debug_orb_set_features: slot outside [0, 2*max_batch_pairs)");
    if (n < 0 || n > msf::kKpCap) return fail(h, MSF_ERR_INVALID_ARG, "msf_debug_orb_set_features: n outside [0, 2048]");
    if (n > 0 && (!kp || !desc)) return fail(h, MSF_ERR_INVALID_ARG, "msf_debug_orb_set_features: null pointer with n > 0");
    CallScope cs{h};
    if (int rc = cs.enter()) return rc;
    Drain drain{cs.st};   // the copies read the caller's arrays: never return with one in flight
    HIP_TRY(h, "orb set_features", h->orb.set_features(slot, n, kp, desc, cs.st));
    drain.armed = false;
    return cs.finish();
  });
}

int msf_debug_orb_tail(msf_handle* h, int32_t n_frames, const uint8_t* d_frames, int64_t frame_stride, int64_t row_stride,
                       int32_t first_slot, const int32_t* counts, const int32_t* cands, int32_t form) {
  return guarded(h, "msf_debug_orb_tail", [&]() -> int {
    if (h->cfg.kind != MSF_KIND_ORB) return fail(h, MSF_ERR_INVALID_ARG, "msf_debug_orb_tail: not an ORB handle");
    if (n_frames < 1 || !d_frames || !counts || first_slot < 0 ||
        (long long)first_slot + n_frames > 2ll * h->cfg.max_batch_pairs)
      return fail(h, MSF_ERR_INVALID_ARG, "msf_debug_orb_tail: slot range outside [0, 2*max_batch_pairs), or no frames");
    if (form != 0 && form != 1) return fail(h, MSF_ERR_INVALID_ARG, "msf_debug_orb_tail: form is 0 (dense) or 1 (streaming)");
    if (!aligned16(d_frames, frame_stride, row_stride))
      return fail(h, MSF_ERR_INVALID_ARG, "device frames must be 16-byte aligned with strides multiple of 16");
    if (row_stride < h->cfg.image_width ||
        (n_frames > 1 && frame_stride < row_stride * (long long)h->cfg.image_height))
      return fail(h, MSF_ERR_INVALID_ARG, "msf_debug_orb_tail: strides smaller than the frame");
    // the kernels' loads assume what this checks: nothing is enqueued for lists that fail it
    const std::string why = h->orb.tail_refusal(n_frames, counts, cands);
    if (!why.empty()) return fail(h, MSF_ERR_INVALID_ARG, "msf_debug_orb_tail: " + why);
    CallScope cs{h};
    if (int rc = cs.enter()) return rc;
    Drain drain{cs.st};   // the copies read the caller's arrays: never return with one in flight
    msf::FrameSrc src{d_frames, d_frames, n_frames, first_slot, frame_stride, (int)row_stride};
    HIP_TRY(h, "orb tail", h->orb.tail(src, n_frames, counts, cands, form, cs.st));
    drain.armed = false;
    return cs.finish();
  });
}

int msf_stage_times(msf_handle* h, const char** names, float* ms, int32_t cap) {
  if (!names || !ms || cap < 1) return 0;
  const int n = guarded(h, "msf_stage_times", [&]() -> int {
    hipSetDevice(h->cfg.device);
    return h->cfg.kind == MSF_KIND_ORB ? h->orb.stage_times(names, ms, cap) : h->loftr.stage_times(names, ms, cap);
  });
  return n > 0 ? n : 0;   // a number of stages, not a status: nothing to report is 0
}

int msf_frame_cache_stats(msf_handle* h, uint64_t* hits, uint64_t* misses, int32_t* capacity) {
  return guarded(h, "msf_frame_cache_stats", [&]() -> int {   // host state only: the device is not touched
    if (hits) *hits = h->fc_hits;
    if (misses) *misses = h->fc_misses;
    if (capacity) *capacity = (int32_t)h->fc.size();
    return MSF_OK;
  });
}

/* LoFTR weights, on the host (no GPU needed): reads `path` -- the reference's ONNX model or the MSFLTR01 blob -- and
 * reports the number of tensors / floats and a digest of names, shapes and values; equal digests <=> identical weights. */
int msf_weights_info(const char* path, uint64_t* digest, int32_t* n_tensors, int64_t* n_floats) {
  return guarded("msf_weights_info", [&]() -> int {
    if (!path) return fail(nullptr, MSF_ERR_INVALID_ARG, "msf_weights_info: null path");
    // test hook for the no-exceptions guarantee, armed only by the test's environment
    if (std::strcmp(path, "::throw::") == 0 && getenv("MSF_TEST_HOOKS")) throw std::bad_alloc();
    msf::WeightMap w;
    const std::string err = msf::load_weights(path, &w);
    if (!err.empty()) return fail(nullptr, MSF_ERR_IO, err);
    int64_t nf = 0;
    const uint64_t d = msf::weights_digest(w, &nf);
    if (digest) *digest = d;
    if (n_tensors) *n_tensors = (int32_t)w.size();
    if (n_floats) *n_floats = nf;
    return MSF_OK;
  });
}

/* Writes the weights of `src_path` (ONNX model or blob) as an MSFLTR01 blob: a load-time cache, nothing more. */
int msf_convert_weights(const char* src_path, const char* dst_blob_path) {
  return guarded("msf_convert_weights", [&]() -> int {
    if (!src_path || !dst_blob_path) return fail(nullptr, MSF_ERR_INVALID_ARG, "msf_convert_weights: null path");
    msf::WeightMap w;
    std::string err = msf::load_weights(src_path, &w);
    if (err.empty()) err = msf::save_blob(dst_blob_path, w);
    if (!err.empty()) return fail(nullptr, MSF_ERR_IO, err);
    return MSF_OK;
  });
}

}  // extern "C"
