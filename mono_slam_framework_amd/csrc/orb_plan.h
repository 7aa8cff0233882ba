// ORB level plan: everything OrbPipeline::init derives from (width, height, max_slots, options) with integer and float
// arithmetic alone -- level sizes, quotas, list capacities and offsets, the tile and walker-strip grids, the threshold
// sampler's lattice, the 8.8 resize tables and the two checks that decide which kernels a handle may launch.
// Host only, no HIP: builds with plain g++ -std=c++17; tests/cpp/orb_plan_main.cpp runs it under the sanitizers and
// pins it against plans recorded from the code init held before this header (tests/test_orb_plan_host.py).
// Compile with -ffp-contract=off: the level sizes are cvRound of f32 products.
#pragma once

#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

namespace msf {

// Capacities.  A frame whose reference counts exceed one of them comes back with n_out = -1 (MSF_ERR_CAPACITY), in every
// call form and whatever else the call holds; every other frame is exact (tests/orb_capacity.py restates them, and
// tests/test_orb_plan_host.py holds the restatement to the plan's numbers):
//  * kKpCap: final key points of a frame;
//  * per level, min(kS1Cap, full list): key points kept by retainBest(2N) (stage 1);
//  * a dense CALL only (MSF_FLAG_FAST_DENSE, fewer than eight frames): per level, strict FAST maxima at fastThreshold
//    inside the 31-px border > full list (OrbLevelInfo::cand_cap, w h / 8).  A streaming call never lists them all.
constexpr int kOrbLevels = 8;
constexpr int kKpCap = 2048;       // keypoints per frame (cv::ORB nfeatures = 500, + ties)
constexpr int kS1Cap = 8192;       // per level: keypoints kept by retainBest(2N) on the FAST score (+ ties)

constexpr int kEdge = 31;          // edgeThreshold
constexpr int kFastT = 20;         // fastThreshold
constexpr int TW = 128, TH = 32;    // FAST output tile
constexpr int kTileX0 = 16;        // tile grid origin: first output column 31 rounded down to the 16-byte load grid
constexpr int kDiscTasks = 256;    // ICAngles disc: 31 rows x 8 dwords, padded to 4 x 64 tasks (OrbPlan::disc)

constexpr int kWkMaxNx = 17;   // walker strips across a level (4096 px)
constexpr int kWkMaxPx = 244;            // strip pitch <= 244: a group of 4 output px reads two aligned 8-byte pairs <= 8 B apart
constexpr int kWkMaxRows = 240;          // owned rows per strip at most (a strip's emit table lives in four registers per lane)
// Owned rows per strip aimed at.  With the levels as separate launches 80 rows measured best (r03: 48 / 64 / 80 / 96 / 112
// rows 8.19 / 7.97 / 7.83 / 7.88 / 7.96 ms per 720p step: taller strips lengthen every launch's tail).  In the one-launch
// form there is one tail, and what counts is the work a strip repeats -- 8 halo rows, its prologue, its drain:
// 64 / 80 / 112 / 144 / 180 / 240 rows measured 5.47 / 5.24 / 4.97 / 4.86 / 4.78 / 4.79 ms for the stage at 1280 x 720
// (1024 pairs) and 9.92 (80) / 9.45 (112) / 8.80 (144) / 8.62 (240) ms at 640 x 480 (4096 pairs).  Handles for small
// batches keep short strips: their calls are latency-bound chains of (quarter, rest) x 8 levels.
constexpr int kWkRowsTall = 240, kWkRowsShort = 80, kWkTallMinSlots = 4 * 64;
constexpr int kTauSites = 1024;          // sampled runs of 4 px per (frame, level) of the threshold sampler (512 / 2048 / 4096: slower)
// A vector offset no level the walker makes reaches (checked below: such a level is below 1 GB): the buffer range check
// drops a store at it, whatever row offset comes on top.  dxoff | kRzNoStore stays in [1 GB, 2 GB).
constexpr uint32_t kRzNoStore = 0x40000000u;

struct OrbLevelInfo {
  int w, h, pitch;     // level size, row pitch in bytes (multiple of 16)
  int quota;           // nfeaturesPerLevel
  float scale;         // getScale(level)
  int cand_cap;        // FULL capacity of the FAST candidate list of this level (the dense detector: w h / 8)
  int cand_off;        // offset (entries) of this level inside a frame's full-capacity region (dense calls)
  int s1_off;          // offset (entries) of this level inside a slot's stage-1 array
  int tiles_x, tiles_y, tile_base;  // FAST tiling (128 x 32 tiles, dense kernel)
  // column strips of the streaming walker (one wave each) over the WHOLE level: strip (sx, sy) holds the 256-px window
  // starting at x = sx * wk_px and owns rows [sy * wk_rows, (sy + 1) * wk_rows)
  int wk_nx, wk_ny, wk_px, wk_rows, wk_base;   // wk_base: flat index of the level's first strip
  int wk_fused;        // this level (as the DESTINATION of a resize) can be made by the walker of level l - 1
  int tab_yemit;       // offset (entries) of the per-source-row emit table of the resize INTO this level
  int tab_xstrip;      // offset (entries) of the first output group of each walker strip of level l - 1
  int wk_xg[kWkMaxNx + 1];   // the same numbers inside the kernel arguments (a scalar load instead of a dependent memory
                             // round trip in front of the strip's table loads); more strips than kWkMaxNx: not fused
  int tab_off;         // offset (entries) of this level's resize tables
  int samp_sx, samp_sy, samp_rows, samp_cols;   // tau_unit's sample lattice over [31, w-31) x [31, h-31); rows 0 = none
  long long pix_off;   // byte offset of this level inside a slot's pyramid blob (levels >= 1)
};

// per level: capacity of the PRIMARY candidate list (the output-sensitive pass: w h / 64, at least kS1Cap; small levels keep
// their full capacity) and its offset (entries) inside a work row's primary region.  (A struct of its own, passed to the
// one kernel that needs it: inside OrbGeometry or OrbLevelInfo the extra members put the walker's copies into scratch.)
struct OrbPrimLists {
  int cap[kOrbLevels], off[kOrbLevels];
};

struct OrbGeometry {
  int nlevels;
  int w0, h0;
  int total_tiles;
  int total_strips;        // walker strips of all levels
  int max_level_tiles;     // largest tile count of one level
  int cand_total;          // candidate entries of a frame at full capacity (dense calls: one such region per frame in the pool)
  int prim_total;          // candidate entries per work row (primary lists)
  // The candidate arrays are [work rows][prim_total] followed by a POOL of pool_entries entries.  A streaming call lists
  // into the primary lists only: the dense second pass of a (frame, level) counts the scores of its maxima, then lists
  // them all into the level's primary list if they fit, else those at or above the retainBest(2N) cut -- the level's
  // stage 1 (k_fast_redo) --, so no level needs room beyond its own.  A call that is dense altogether (MSF_FLAG_FAST_DENSE, fewer than eight frames)
  // lays its frames' full-capacity regions over the pool (sized for that by plan_orb).
  long long pool_base;     // first pool entry
  unsigned pool_entries;
  int s1_total;            // stage-1 entries per work row
  long long pyr_bytes;     // pyramid blob bytes per work row (levels 1..)
  OrbLevelInfo lv[kOrbLevels];
  int umax[16];
};
// kernel arguments, passed by value: the kernels were tuned with exactly these layouts
static_assert(sizeof(OrbLevelInfo) == 176,"OrbLevelInfo is a kernel argument: members may not be added or moved");
static_assert(sizeof(OrbGeometry) == 1528, "OrbGeometry is a kernel argument: members may not be added or moved");

// units of k_harris_flat: from the quotas only
struct HarrisUnits {
  int base[kOrbLevels + 1];    // first unit of level l; base[nlevels] = units per frame
  int n[kOrbLevels];
};

// ---- the unit order of a walker launch (k_walk): which unit workgroup wg is.  The kernel and the host's grid size both
// come from here; tests/cpp/walk_units_main.cpp holds the order to what the kernel's waits rest on (every unit exactly
// once, every dependency at a lower workgroup index).
// A launch covers levels [l_lo, l_hi] of n_frames frames.  Workgroups b, b + 8, ... share an XCD (observed placement,
// speed only): XCD x takes the frames [x n / 8, (x + 1) n / 8) and walks, level by level, the THRESHOLD units of its
// frames, the sampled quarter of all their strips (strip index a multiple of 4), then the other strips.  With finish
// units (finish = kWalkFinishThr / kWalkFinishQuarter) the FINISH units of level l - 1 stand directly behind the
// threshold units / behind the sampled quarter of level l -- both wait for all strips of level l - 1 -- and those of
// level l_hi behind its last strips.  An XCD with one frame fewer than another leaves its surplus workgroups without a unit.
#if defined(__HIPCC__)
#define MSF_PLAN_HD __host__ __device__
#else
#define MSF_PLAN_HD
#endif
constexpr int kWalkNone = 0, kWalkThreshold = 1, kWalkStrip = 2, kWalkFinish = 3;
constexpr int kWalkFinishOff = 0, kWalkFinishThr = 1, kWalkFinishQuarter = 2;
struct WalkUnit {
  int kind, level, frame, strip;   // frame: index inside the call; strip: kWalkStrip only
};
MSF_PLAN_HD inline WalkUnit walk_unit(const OrbGeometry& g, int l_lo, int l_hi, int n_frames, int finish, unsigned wg) {
  const int xcd = (int)(wg & 7u);
  int r = (int)(wg >> 3);                        // unit of this XCD
  const int nf8 = n_frames >> 3, nrem = n_frames & 7;
  const int nfx = nf8 + (xcd < nrem ? 1 : 0), f0 = xcd * nf8 + (xcd < nrem ? xcd : nrem);
  for (int l = l_lo; l <= l_hi; l++) {
    const int S = g.lv[l].wk_nx * g.lv[l].wk_ny;
    if (r < nfx) return WalkUnit{kWalkThreshold, l, f0 + r, 0};
    r -= nfx;
    if (finish == kWalkFinishThr && l > l_lo) {
      if (r < nfx) return WalkUnit{kWalkFinish, l - 1, f0 + r, 0};
      r -= nfx;
    }
    const int Sq = (S + 3) >> 2, Sr = S - Sq;
    if (r < nfx * Sq) return WalkUnit{kWalkStrip, l, f0 + r / Sq, 4 * (r % Sq)};
    r -= nfx * Sq;
    if (finish == kWalkFinishQuarter && l > l_lo) {
      if (r < nfx) return WalkUnit{kWalkFinish, l - 1, f0 + r, 0};
      r -= nfx;
    }
    if (r < nfx * Sr) {
      const int ip = r % Sr;
      return WalkUnit{kWalkStrip, l, f0 + r / Sr, 4 * (ip / 3) + ip % 3 + 1};
    }
    r -= nfx * Sr;
  }
  if (finish != kWalkFinishOff && r < nfx) return WalkUnit{kWalkFinish, l_hi, f0 + r, 0};
  return WalkUnit{kWalkNone, 0, 0, 0};           // surplus workgroups of an XCD with one frame fewer
}
// workgroups of the launch: per XCD ceil(n / 8) frames x (per level one threshold unit + the level's strips [+ one
// finish unit])
inline long long walk_grid(const OrbGeometry& g, int l_lo, int l_hi, int n_frames, int finish) {
  long long per_frame = 0;
  for (int l = l_lo; l <= l_hi; l++) per_frame += 1 + g.lv[l].wk_nx * g.lv[l].wk_ny + (finish != kWalkFinishOff ? 1 : 0);
  return 8ll * ((n_frames + 7) / 8) * per_frame;
}

struct OrbPlanRequest {
  int width = 0, height = 0;
  int max_slots = 0;
  int work_frames = 0;             // frames one extraction may hold; <= 0 or > max_slots: max_slots
  bool level_size_mul_inv = false; // MSF_FLAG_LEVEL_SIZE_MUL_INV
  bool resize_generic = false;     // no level takes the shared-pair column form (and so none is fused)
  int force_tau = 0;               // kFastT: every call of the handle is dense (every work row has a pool region)
  int stream_min_frames = 8;       // otherwise calls with fewer frames are dense
};

struct OrbPlan {
  OrbGeometry g{};
  OrbPrimLists prim{};
  bool resize_shared[kOrbLevels] = {};   // per level: k_resize may read three pixels' taps from one dword pair
  // resize tables per level: per group of 4 columns selectors / weights / pair offsets, per row source row | w1 << 16
  std::vector<uint32_t> tab;
  // ICAngles disc as 31 rows x 8 dwords of 4 pixels (u = -16 + 4k .. -13 + 4k): per dword the signed byte weights u
  // (0 outside the disc) and the signed byte weights v (the row's, 0 outside the disc), padded to 4 x 64 tasks
  std::vector<uint32_t> disc;
  int work_frames = 0;                   // resolved: rows of the per-call arrays
  HarrisUnits harris{};
};

inline int cv_round_f(float v) { return (int)lrintf(v); }
inline int cv_round_d(double v) { return (int)lrint(v); }

// interpolationLinear<uchar>::getCoeffs (imgproc resize.cpp, INTER_LINEAR_EXACT)
inline void make_table(int src, int dst, uint32_t* tab) {
  const double inv_scale = (double)dst / (double)src;
  const double scale = 1.0 / inv_scale;
  for (int d = 0; d < dst; d++) {
    const double f = scale * ((double)d + 0.5) - 0.5;
    const int i = (int)floor(f);
    if (i >= 0 && src > 1) {
      if (i < src - 1) {
        tab[d] = (uint32_t)i | ((uint32_t)cv_round_d((f - (double)i) * 256.0) << 16);
      } else {
        tab[d] = (uint32_t)(src - 1);   // replicate the last pixel: weight 0 on the (absent) right/bottom tap
      }
    } else {
      tab[d] = 0;                       // replicate the first pixel
    }
  }
}

// returns empty string on success; *out is complete only then
inline std::string plan_orb(const OrbPlanRequest& rq, OrbPlan* out) {
  const int width = rq.width, height = rq.height, max_slots = rq.max_slots, work_frames = rq.work_frames;
  if (width < 64 || height < 64 || width > 8192 || height > 8192) return "arg: ORB image size must be in [64, 8192] x [64, 8192]";
  if (max_slots < 2) return "arg: ORB max_slots < 2";
  *out = OrbPlan();
  // frames one extraction may hold: the pyramid, the candidate and stage-1 lists and the walker's state exist once per
  // frame of a CALL (work rows), only key points and descriptors once per feature slot
  out->work_frames = work_frames <= 0 || work_frames > max_slots ? max_slots : work_frames < 2 ? 2 : work_frames;
  OrbGeometry& g = out->g;
  OrbPrimLists& prim_ = out->prim;
  g.nlevels = kOrbLevels;
  g.w0 = width;
  g.h0 = height;
  // ORB_Impl::detectAndCompute: layer scales and sizes; computeKeyPoints: per-level quotas and umax
  const float scale_factor_f = 1.2f;
  const double scale_factor = (double)scale_factor_f;
  const int nfeatures = 500;
  {
    const float factor = (float)(1.0 / scale_factor);
    float nd = (float)nfeatures * (1 - factor) / (1 - (float)pow((double)factor, (double)g.nlevels));
    int sum = 0;
    for (int l = 0; l < g.nlevels - 1; l++) {
      g.lv[l].quota = cv_round_f(nd);
      sum += g.lv[l].quota;
      nd *= factor;
    }
    g.lv[g.nlevels - 1].quota = nfeatures - sum > 0 ? nfeatures - sum : 0;
  }
  {
    const int half = 15;
    int umax[17] = {0};
    const int vmax = (int)floor(half * sqrt(2.f) / 2 + 1);
    const int vmin = (int)ceil(half * sqrt(2.f) / 2);
    for (int v = 0; v <= vmax; ++v) umax[v] = cv_round_d(sqrt((double)half * half - v * v));
    for (int v = half, v0 = 0; v >= vmin; --v) {
      while (umax[v0] == umax[v0 + 1]) ++v0;
      umax[v] = v0;
      ++v0;
    }
    for (int v = 0; v < 16; v++) g.umax[v] = umax[v];
  }
  long long pix = 0;
  int cand = 0, prim = 0, tiles = 0, strips = 0, tab = 0, s1 = 0;
  g.max_level_tiles = 0;
  for (int l = 0; l < g.nlevels; l++) {
    OrbLevelInfo& L = g.lv[l];
    const float s = (float)pow(scale_factor, (double)l);
    const float inv = 1.0f / s;
    L.scale = s;
    // ORB_Impl::detectAndCompute (OpenCV 3.x / 4.x): Size sz(cvRound(image.cols/scale), cvRound(image.rows/scale));
    // MSF_FLAG_LEVEL_SIZE_MUL_INV selects the 2.4-era cvRound(cols * (1.f / scale)) instead (they differ for a few odd
    // sizes, e.g. width 69 -> 57 vs 58 at level 1; never for 640 / 480 / 1280 / 720 / 1920 / 1080)
    L.w = rq.level_size_mul_inv ? cv_round_f((float)width * inv) : cv_round_f((float)width / s);
    L.h = rq.level_size_mul_inv ? cv_round_f((float)height * inv) : cv_round_f((float)height / s);
    L.pitch = (L.w + 15) & ~15;
    L.pix_off = pix;
    if (l > 0) pix += (long long)L.pitch * L.h;
    // strict 3x3 maxima are at most w*h/4; w*h/8 covers white noise with margin (overflow is flagged, never silent)
    int cap = (int)((long long)L.w * L.h / 8);
    if (cap < 4096) cap = 4096;
    cap = (cap + 15) & ~15;   // score bytes of a level start 16-byte aligned
    L.cand_cap = cap;
    L.cand_off = cand;
    cand += cap;
    // the output-sensitive pass lists the maxima at or above the level's threshold -- about a thousand at 1280 x 720
    // against ~20 000 maxima in all --: the primary list is an eighth of the full one (a list that overflows all the same
    // sends its level to the dense pass, k_fast_check), and at least kS1Cap: the dense pass lists the level's stage 1
    // into it, so every stage 1 that fits kS1Cap fits its primary list
    int pcap = (int)((long long)L.w * L.h / 64);
    if (pcap < kS1Cap) pcap = kS1Cap;
    pcap = (pcap + 15) & ~15;
    // small levels keep their full capacity (little memory, and small levels are the ones that take the dense pass:
    // their thresholds rest on few corners): only lists above 16 K entries are cut
    if (pcap > cap || cap <= 16384) pcap = cap;
    prim_.cap[l] = pcap;
    prim_.off[l] = prim;
    prim += pcap;
    L.s1_off = s1;
    s1 += kS1Cap;
    // FAST tiles cover only the pixels runByImageBorder(31) can keep, [31, w-31) x [31, h-31) (17 % fewer tiles on
    // the 720p pyramid than tiling the whole level); levels without such pixels get no tiles
    L.tiles_x = L.w > 2 * kEdge ? (L.w - kEdge - kTileX0 + TW - 1) / TW : 0;
    L.tiles_y = L.h > 2 * kEdge ? (L.h - 2 * kEdge + TH - 1) / TH : 0;
    if (L.tiles_x == 0 || L.tiles_y == 0) L.tiles_x = L.tiles_y = 0;
    L.tile_base = tiles;
    tiles += L.tiles_x * L.tiles_y;
    // walker strips over the whole level: 256-px windows wk_px apart ((nx - 1) * wk_px + 256 >= w), wk_rows owned rows
    L.wk_nx = L.w > 256 ? (L.w - 256 + kWkMaxPx - 1) / kWkMaxPx + 1 : 1;
    L.wk_px = L.wk_nx > 1 ? (((L.w - 256 + L.wk_nx - 2) / (L.wk_nx - 1)) + 3) & ~3 : kWkMaxPx;
    const int rows_target = max_slots >= kWkTallMinSlots ? kWkRowsTall : kWkRowsShort;
    L.wk_ny = (L.h + rows_target - 1) / rows_target;
    L.wk_rows = (((L.h + L.wk_ny - 1) / L.wk_ny) + 3) & ~3;
    L.wk_ny = (L.h + L.wk_rows - 1) / L.wk_rows;
    L.wk_base = strips;
    strips += L.wk_nx * L.wk_ny;
    L.wk_fused = 0;
    L.tab_yemit = L.tab_xstrip = 0;
    if (L.tiles_x * L.tiles_y > g.max_level_tiles) g.max_level_tiles = L.tiles_x * L.tiles_y;
    // sample lattice of tau_unit: about 4096 pixels of the kept region in runs of 4 (one dword), rows sparser than
    // columns (a sampled pixel touches 7 rows); samp_sx counts dwords and is odd, so that block textures with
    // power-of-two periods are not aliased
    L.samp_sx = L.samp_sy = 1;
    L.samp_rows = L.samp_cols = 0;
    if (L.tiles_x > 0) {
      const int rh = L.h - 2 * kEdge;
      const int n_dw = (L.w - kEdge - ((kEdge + 3) & ~3)) >> 2;          // aligned dwords fully inside [31, w - 31)
      const double s2 = (double)n_dw * rh / (double)kTauSites;          // (dword, row) sites per sampled run
      int sx = (int)(sqrt(s2 > 1.0 ? s2 : 1.0) / 4.0);
      sx = (sx < 1 ? 1 : sx) | 1;
      int sy = (int)(s2 / sx + 0.5);
      sy = sy < 1 ? 1 : sy;
      L.samp_sx = sx;
      L.samp_sy = sy;
      L.samp_rows = (rh + sy - 1) / sy;
      L.samp_cols = n_dw > 0 ? (n_dw + sx - 1) / sx : 0;
      if (L.samp_cols == 0) L.samp_rows = 0;
    }
    L.tab_off = tab;
    if (l > 0) {
      tab += 12 * ((L.w + 3) >> 2) + ((L.h + 3) & ~3);   // 3 x uint4 per group of 4 columns, one dword per row
      L.tab_yemit = tab;                                 // one dword per SOURCE row (level l - 1)
      tab += (g.lv[l - 1].h + 3) & ~3;
      L.tab_xstrip = tab;                                // first output group of each walker strip of level l - 1, + end
      tab += (g.lv[l - 1].wk_nx + 1 + 3) & ~3;
    }
  }
  g.pyr_bytes = (pix + 255) & ~255ll;
  g.cand_total = cand;
  g.prim_total = prim;
  g.s1_total = s1;
  g.total_tiles = tiles;
  g.total_strips = strips;

  std::vector<uint32_t>& htab = out->tab;
  htab.assign(tab > 0 ? tab : 1, 0u);
  for (int l = 1; l < g.nlevels; l++) {
    const OrbLevelInfo& L = g.lv[l];
    const int groups = (L.w + 3) >> 2;
    std::vector<uint32_t> xt(4 * groups);
    make_table(g.lv[l - 1].w, L.w, xt.data());
    for (int x = L.w; x < 4 * groups; x++) xt[x] = xt[L.w - 1];   // pad entries: the last pixel again
    // k_resize<true> reads pixels 4g .. 4g+2 from the dword pair of pixel 4g: needs tap offset (rel. to that pair) <= 6
    bool shared = !rq.resize_generic;
    for (int x = 0; x < 4 * groups; x += 4)
      for (int k = 1; k < 3; k++)
        if ((xt[x + k] & 0xFFFFu) - (xt[x] & 0xFFFCu) > 6u) shared = false;
    out->resize_shared[l] = shared;
    uint32_t* xsel = htab.data() + L.tab_off;
    uint32_t* xwxp = xsel + 4 * groups;
    uint32_t* xoff = xwxp + 4 * groups;
    for (int x = 0; x < 4 * groups; x++) {
      const uint32_t cx = xt[x] & 0xFFFFu, wx1 = xt[x] >> 16;
      const uint32_t base = ((shared && (x & 3) < 3) ? xt[x & ~3] : cx) & 0xFFFCu;   // byte offset of the aligned dword pair
      xoff[x] = base;
      xsel[x] = 0x0c010c00u + (cx - base) * 0x00010001u;   // pair bytes (cx - base, cx - base + 1) -> u16 lanes, zeros between
      xwxp[x] = (256u - wx1) | (wx1 << 16);
    }
    uint32_t* ytab = xoff + 4 * groups;
    make_table(g.lv[l - 1].h, L.h, ytab);
    // ---- tables of the fused form (the walker of level l - 1 makes this level): valid if every source row is the
    // upper tap of at most one output row, the shared-pair column form holds, and every strip's groups fit its window
    const OrbLevelInfo& Ls = g.lv[l - 1];
    bool fused = shared && Ls.wk_rows <= kWkMaxRows && Ls.h < 65536;
    if ((long long)L.pitch * L.h >= (long long)kRzNoStore) fused = false;   // the offset of a dropped store must lie past the level
    uint32_t* yemit = htab.data() + L.tab_yemit;
    uint32_t* xstrip = htab.data() + L.tab_xstrip;
    for (int y = 0; y < L.h; y++) {
      const uint32_t sy = ytab[y] & 0xFFFFu, w1 = ytab[y] >> 16;
      if (sy >= (uint32_t)Ls.h || yemit[sy] != 0u || w1 > 256u) { fused = false; break; }
      yemit[sy] = 0x80000000u | (w1 << 16) | (uint32_t)y;
    }
    // group gq belongs to the last strip whose window starts at or before its first pair
    for (int c = 0; c <= Ls.wk_nx; c++) xstrip[c] = (uint32_t)groups;
    for (int gq = groups - 1; gq >= 0; gq--) {
      const uint32_t b0 = xoff[4 * gq], b3 = xoff[4 * gq + 3];
      int c = (int)(b0 / (uint32_t)Ls.wk_px);
      if (c > Ls.wk_nx - 1) c = Ls.wk_nx - 1;
      const uint32_t xs = (uint32_t)(c * Ls.wk_px);
      // every tap that counts lies inside the 256-px window; the second dword of a pair may stick out of it (it then
      // holds only weight-0 taps: the replicated last pixel) -- the read stays inside the wave's LDS block
      if (b0 < xs || b3 < b0 || b3 + 4u > xs + 256u) fused = false;
      for (int k = 0; k < 4; k++) {
        const uint32_t cx = xt[4 * gq + k] & 0xFFFFu, w1 = xt[4 * gq + k] >> 16;
        if (cx < xs || cx >= xs + 256u || (cx + 1u >= xs + 256u && w1 != 0u)) fused = false;
      }
      for (int cc = 0; cc <= c; cc++) xstrip[cc] = (uint32_t)gq;       // groups are monotone in b0: the last write is the first group
    }
    for (int c = 0; c < Ls.wk_nx; c++)
      if (xstrip[c + 1] < xstrip[c] || xstrip[c + 1] - xstrip[c] > 64u) fused = false;
    if (xstrip[0] != 0u) fused = false;
    if (Ls.wk_nx > kWkMaxNx) fused = false;
    for (int c = 0; c <= kWkMaxNx; c++) g.lv[l].wk_xg[c] = (int)xstrip[c < Ls.wk_nx ? c : Ls.wk_nx];
    g.lv[l].wk_fused = fused ? 1 : 0;
  }
  {
    // candidate arrays: a primary region per work row + the pool.  The pool only serves dense CALLS, whose frames lay
    // their full-capacity regions over it: every row with MSF_FLAG_FAST_DENSE, at most stream_min_frames - 1 frames
    // otherwise.  (The dense second pass of a streaming call lists into the level's primary list: k_fast_redo.)
    const size_t Wk = (size_t)out->work_frames;
    const long long dense_rows = rq.force_tau == kFastT ? (long long)Wk : std::min<long long>((long long)Wk, std::max(rq.stream_min_frames - 1, 0));
    const long long pool_entries_ = std::max<long long>(dense_rows * g.cand_total, 16);
    g.pool_base = (long long)Wk * g.prim_total;
    const long long total = g.pool_base + pool_entries_;
    if (total >= (1ll << 32)) return "ORB candidate arrays exceed 2^32 entries: reduce max_batch_pairs";
    g.pool_entries = (unsigned)pool_entries_;
  }
  {
    std::vector<uint32_t>& disc = out->disc;
    disc.assign(2 * kDiscTasks, 0u);   // padding tasks: zero weights
    for (int v = -15; v <= 15; v++) {
      const int dmax = g.umax[v < 0 ? -v : v];
      for (int k = 0; k < 8; k++) {
        uint32_t wu = 0, w1 = 0;
        for (int b = 0; b < 4; b++) {
          const int u = -16 + 4 * k + b;
          if (u >= -dmax && u <= dmax) {
            wu |= (uint32_t)(uint8_t)(int8_t)u << (8 * b);
            w1 |= (uint32_t)(uint8_t)(int8_t)v << (8 * b);
          }
        }
        disc[2 * ((v + 15) * 8 + k)] = wu;
        disc[2 * ((v + 15) * 8 + k) + 1] = w1;
      }
    }
  }
  {
    HarrisUnits& hw = out->harris;
    int nu = 0;
    for (int l = 0; l < kOrbLevels; l++) {
      hw.base[l] = nu;
      hw.n[l] = l < g.nlevels ? (2 * g.lv[l].quota * 5 / 4 + 63) / 64 : 0;
      if (l < g.nlevels && hw.n[l] < 1) hw.n[l] = 1;
      nu += hw.n[l];
    }
    hw.base[kOrbLevels] = nu;
    for (int l = g.nlevels; l < kOrbLevels; l++) hw.base[l] = nu;
    hw.base[g.nlevels] = nu;
  }
  return "";
}

// msf_debug_orb_tail: the caller's candidate lists -- counts [n][kOrbLevels], cands (lx, ly, score) triples in
// (frame, level) order -- against what the kernels behind FAST take for granted; cap[l] is the capacity of level l's
// list in a call of n frames.  Returns why the lists are refused, or an empty string.
//  * a count may exceed the capacity by kTailCountMargin: k_thr_harris clamps such a count itself and flags the frame
//    (the entries past the capacity are not written anywhere);
//  * every position lies in [kEdge, w - kEdge - 1] x [kEdge, h - kEdge - 1]: harris_at reads 12 aligned bytes around
//    x - 4 .. x + 4 and k_describe 48 around x - 22 .. x + 22 without a bounds check -- FAST never lists a corner
//    outside that rectangle, so the rectangle is the kernels' precondition.
constexpr int kTailCountMargin = 16;
inline std::string check_tail_lists(const OrbGeometry& g, const int* cap, int n, const int32_t* counts,
                                    const int32_t* cands) {
  if (n < 1 || !counts) return "no frames, or null counts";
  size_t at = 0;
  for (int f = 0; f < n; f++)
    for (int l = 0; l < kOrbLevels; l++) {
      const long long c = counts[f * kOrbLevels + l];
      if (c == 0) continue;
      if (l >= g.nlevels || c < 0 || c > (long long)cap[l] + kTailCountMargin) return "count outside [0, capacity + 16]";
      if (!cands) return "null candidates with a count > 0";
      const OrbLevelInfo& L = g.lv[l];
      if (L.w <= 2 * kEdge || L.h <= 2 * kEdge) return "candidates on a level without a key point rectangle";
      for (long long i = 0; i < c; i++, at++) {
        const int32_t x = cands[3 * at], y = cands[3 * at + 1], s = cands[3 * at + 2];
        if (x < kEdge || x > L.w - kEdge - 1 || y < kEdge || y > L.h - kEdge - 1)
          return "position outside [31, w - 32] x [31, h - 32] of its level";
        if (s < 0 || s > 255) return "score outside [0, 255]";
      }
    }
  return "";
}

}  // namespace msf
