// csrc/orb_plan.h in a stand-alone executable (tests/test_orb_plan_host.py), never inside python.
//   orb_plan golden                 the fixed request list below, one line per field group of each plan, to stdout; the
//                                   test compares the lines with tests/golden/orb_plan_digests.txt, recorded from the
//                                   code OrbPipeline::init held before the header existed
//   orb_plan plans W H S M ...      the same lines for the requests (width, height, max_slots, level_size_mul_inv) named
//                                   on the command line (the test holds them to oracle/orb.py and tests/orb_capacity.py)
//   orb_plan sweep K N              (part K of N of) every width 64..8192 at height 64 and every height 64..8192 at width 64, both
//                                   level-size modes, max_slots 2 and 256: the flags, and what the kernels rely on
//                                   re-derived from the tables themselves; failures to stderr and the exit status
//   orb_plan tail_lists W H         check_tail_lists (the host check of msf_debug_orb_tail) on every level of a W x H plan
// Fields are printed, not struct bytes: padding is no part of the contract.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "orb_plan.h"

using namespace msf;

namespace {

int failures = 0;

#define CHECK(cond, ...)                                                   \
  do {                                                                     \
    if (!(cond)) {                                                         \
      if (failures < 50) {                                                 \
        std::fprintf(stderr, "line %d: %s does not hold: ", __LINE__, #cond); \
        std::fprintf(stderr, __VA_ARGS__);                                 \
        std::fprintf(stderr, "\n");                                        \
      }                                                                    \
      failures++;                                                          \
    }                                                                      \
  } while (0)

void print_words(const char* name, const std::vector<uint32_t>& v) {
  uint64_t h = 1469598103934665603ull;   // FNV-1a 64 over the little-endian bytes
  for (uint32_t w : v)
    for (int b = 0; b < 4; b++) { h ^= (w >> (8 * b)) & 0xFFu; h *= 1099511628211ull; }
  std::printf("%s len=%zu fnv=%016llx\n", name, v.size(), (unsigned long long)h);
}

void print_ints(const char* key, const int* v, int n) {
  std::printf(" %s=", key);
  for (int i = 0; i < n; i++) std::printf(i ? ",%d" : "%d", v[i]);
}

void print_plan(const OrbPlanRequest& rq, const std::string& err, const OrbPlan& p) {
  std::printf("req w=%d h=%d max_slots=%d work_frames=%d mul_inv=%d generic=%d force_tau=%d stream_min=%d\n", rq.width,
              rq.height, rq.max_slots, rq.work_frames, (int)rq.level_size_mul_inv, (int)rq.resize_generic, rq.force_tau,
              rq.stream_min_frames);
  if (!err.empty()) {
    std::printf("error %s\n", err.c_str());
    return;
  }
  const OrbGeometry& g = p.g;
  std::printf("geom nlevels=%d w0=%d h0=%d total_tiles=%d total_strips=%d max_level_tiles=%d cand_total=%d prim_total=%d "
              "pool_base=%lld pool_entries=%u s1_total=%d pyr_bytes=%lld work_frames=%d\n",
              g.nlevels, g.w0, g.h0, g.total_tiles, g.total_strips, g.max_level_tiles, g.cand_total, g.prim_total,
              g.pool_base, g.pool_entries, g.s1_total, g.pyr_bytes, p.work_frames);
  for (int l = 0; l < kOrbLevels; l++) {
    const OrbLevelInfo& L = g.lv[l];
    std::printf("lv%d w=%d h=%d pitch=%d quota=%d scale=%a cand_cap=%d cand_off=%d s1_off=%d tiles_x=%d tiles_y=%d "
                "tile_base=%d wk_nx=%d wk_ny=%d wk_px=%d wk_rows=%d wk_base=%d wk_fused=%d tab_yemit=%d tab_xstrip=%d "
                "tab_off=%d samp_sx=%d samp_sy=%d samp_rows=%d samp_cols=%d pix_off=%lld",
                l, L.w, L.h, L.pitch, L.quota, (double)L.scale, L.cand_cap, L.cand_off, L.s1_off, L.tiles_x, L.tiles_y,
                L.tile_base, L.wk_nx, L.wk_ny, L.wk_px, L.wk_rows, L.wk_base, L.wk_fused, L.tab_yemit, L.tab_xstrip,
                L.tab_off, L.samp_sx, L.samp_sy, L.samp_rows, L.samp_cols, L.pix_off);
    print_ints("wk_xg", L.wk_xg, kWkMaxNx + 1);
    std::printf("\n");
  }
  std::printf("prim");
  print_ints("cap", p.prim.cap, kOrbLevels);
  print_ints("off", p.prim.off, kOrbLevels);
  int shared[kOrbLevels];
  for (int l = 0; l < kOrbLevels; l++) shared[l] = p.resize_shared[l] ? 1 : 0;
  std::printf("\nflags");
  print_ints("resize_shared", shared, kOrbLevels);
  print_ints("umax", g.umax, 16);
  std::printf("\nharris");
  print_ints("base", p.harris.base, kOrbLevels + 1);
  print_ints("n", p.harris.n, kOrbLevels);
  std::printf("\n");
  print_words("tab", p.tab);
  print_words("disc", p.disc);
}

OrbPlanRequest request(int w, int h, int max_slots, bool mul_inv = false, int work_frames = 0) {
  OrbPlanRequest rq;
  rq.width = w;
  rq.height = h;
  rq.max_slots = max_slots;
  rq.level_size_mul_inv = mul_inv;
  rq.work_frames = work_frames;
  return rq;
}

// the recorded requests (the golden file holds their plans in this order)
std::vector<OrbPlanRequest> golden_requests() {
  std::vector<OrbPlanRequest> v;
  for (int s : {2, 4160}) {
    v.push_back(request(640, 480, s));
    v.push_back(request(1280, 720, s));
    v.push_back(request(1920, 1080, s));
  }
  v.push_back(request(1280, 720, 2048));                // total_strips 69, total_tiles 626, 19 668 table words
  v.push_back(request(64, 64, 2));                      // levels without tiles
  v.push_back(request(69, 64, 2, false));               // level 1 is 58 wide ...
  v.push_back(request(69, 64, 2, true));                // ... or 57
  v.push_back(request(333, 251, 8));
  v.push_back(request(4096, 2160, 8));
  v.push_back(request(8192, 8192, 2));                  // more than 17 strips: levels 1-4 are not fused
  v.push_back(request(8192, 64, 256));
  v.push_back(request(64, 8192, 256));
  v.push_back(request(640, 480, 4 * 64 + 64, false, 2 * 64));   // a handle of 64 pairs with its frame cache: tall strips
  OrbPlanRequest rq = request(1280, 720, 16);
  rq.resize_generic = true;                             // no shared pairs, so nothing fused
  v.push_back(rq);
  rq = request(1280, 720, 64, false, 32);
  rq.force_tau = kFastT;                                // dense: a pool region per work row
  v.push_back(rq);
  rq = request(1280, 720, 64, false, 32);
  rq.stream_min_frames = 1;                             // streaming only: the pool's 16 entries
  v.push_back(rq);
  rq = request(1280, 720, 64, false, 3);
  v.push_back(rq);                                      // fewer work rows than stream_min_frames - 1
  rq = request(333, 251, 5, true, 1);                   // work_frames 1 -> 2
  v.push_back(rq);
  rq = request(1920, 1080, 16384);
  rq.force_tau = kFastT;                                // 2^32 candidate entries
  v.push_back(rq);
  v.push_back(request(63, 480, 2));                     // the size errors
  v.push_back(request(640, 8193, 2));
  v.push_back(request(640, 480, 1));                    // too few slots
  return v;
}

// ---- what the kernels rely on, from the tables themselves
void check_plan(const OrbPlanRequest& rq, const OrbPlan& p) {
  const OrbGeometry& g = p.g;
  const std::vector<uint32_t>& tab = p.tab;
  char what[96];
  std::snprintf(what, sizeof what, "%d x %d, slots %d, mul_inv %d", rq.width, rq.height, rq.max_slots, (int)rq.level_size_mul_inv);
  // the lists: offsets are the prefix sums of the capacities
  int cand = 0, prim = 0, s1 = 0;
  for (int l = 0; l < kOrbLevels; l++) {
    CHECK(g.lv[l].cand_off == cand && p.prim.off[l] == prim && g.lv[l].s1_off == s1, "%s level %d", what, l);
    CHECK(p.prim.cap[l] <= g.lv[l].cand_cap && (g.lv[l].cand_cap & 15) == 0 && (p.prim.cap[l] & 15) == 0, "%s level %d", what, l);
    cand += g.lv[l].cand_cap;
    prim += p.prim.cap[l];
    s1 += kS1Cap;
  }
  CHECK(g.cand_total == cand && g.prim_total == prim && g.s1_total == s1, "%s totals", what);
  CHECK(g.pool_base == (long long)p.work_frames * g.prim_total, "%s pool", what);
  size_t end = 0;   // the tables: each region behind the one before, all inside tab
  for (int l = 1; l < kOrbLevels; l++) {
    const OrbLevelInfo &L = g.lv[l], &Ls = g.lv[l - 1];
    const int groups = (L.w + 3) >> 2;
    const size_t off[3] = {(size_t)L.tab_off, (size_t)L.tab_yemit, (size_t)L.tab_xstrip};
    const size_t len[3] = {(size_t)(12 * groups + ((L.h + 3) & ~3)), (size_t)((Ls.h + 3) & ~3), (size_t)((Ls.wk_nx + 1 + 3) & ~3)};
    for (int k = 0; k < 3; k++) {
      CHECK(off[k] >= end && off[k] + len[k] <= tab.size(), "%s level %d table %d", what, l, k);
      end = off[k] + len[k];
    }
    if (end > tab.size()) return;
    if (rq.resize_generic) {   // every pixel has a pair of its own: no walker makes this level
      CHECK(!p.resize_shared[l] && L.wk_fused == 0, "%s level %d", what, l);
      continue;
    }
    // the supported sizes keep the shared-pair form, and only the number of strips stands against the fused one
    CHECK(p.resize_shared[l], "%s level %d", what, l);
    CHECK((L.wk_fused != 0) == (Ls.wk_nx <= kWkMaxNx), "%s level %d: fused %d with %d strips", what, l, L.wk_fused, Ls.wk_nx);
    const uint32_t *xsel = tab.data() + L.tab_off, *xwxp = xsel + 4 * groups, *xoff = xwxp + 4 * groups, *ytab = xoff + 4 * groups;
    const uint32_t *yemit = tab.data() + L.tab_yemit, *xstrip = tab.data() + L.tab_xstrip;
    // strips: the first group of each, monotone from 0 to the number of groups, at most 64 apart
    CHECK(xstrip[0] == 0u && xstrip[Ls.wk_nx] == (uint32_t)groups, "%s level %d xstrip ends", what, l);
    for (int c = 0; c < Ls.wk_nx; c++) {
      CHECK(xstrip[c] <= xstrip[c + 1] && xstrip[c + 1] - xstrip[c] <= 64u, "%s level %d strip %d", what, l, c);
      if (xstrip[c] > xstrip[c + 1] || xstrip[c + 1] > (uint32_t)groups) return;
      // every tap of the strip's groups that carries weight lies in the strip's 256-px window and in the source row
      const uint32_t xs = (uint32_t)(c * Ls.wk_px);
      for (uint32_t x = 4 * xstrip[c]; x < 4 * xstrip[c + 1]; x++) {
        const uint32_t cx = xoff[x] + ((xsel[x] - 0x0c010c00u) & 0xFFu), w0 = xwxp[x] & 0xFFFFu, w1 = xwxp[x] >> 16;
        CHECK(w0 + w1 == 256u, "%s level %d column %u", what, l, x);
        CHECK(w0 == 0u || (cx >= xs && cx < xs + 256u && cx < (uint32_t)Ls.w), "%s level %d column %u tap %u", what, l, x, cx);
        CHECK(w1 == 0u || (cx + 1u >= xs && cx + 1u < xs + 256u && cx + 1u < (uint32_t)Ls.w), "%s level %d column %u tap %u + 1", what, l, x, cx);
        CHECK((xoff[x] & 3u) == 0u && xoff[x] >= xs && xoff[x] + 4u <= xs + 256u, "%s level %d column %u pair", what, l, x);
      }
    }
    for (int c = 0; c <= kWkMaxNx; c++)
      CHECK(L.wk_xg[c] == (int)xstrip[c < Ls.wk_nx ? c : Ls.wk_nx], "%s level %d wk_xg %d", what, l, c);
    // rows: every output row is emitted by exactly one source row, with its own weight
    std::vector<uint8_t> seen(L.h, 0);
    int emitted = 0;
    for (int sy = 0; sy < Ls.h; sy++) {
      const uint32_t e = yemit[sy];
      if (e == 0u) continue;
      const uint32_t y = e & 0xFFFFu, w1 = (e >> 16) & 0x7FFFu;
      CHECK((e >> 31) == 1u && y < (uint32_t)L.h && w1 <= 256u, "%s level %d source row %d", what, l, sy);
      if (y >= (uint32_t)L.h) return;
      CHECK(!seen[y] && ytab[y] == ((uint32_t)sy | (w1 << 16)), "%s level %d output row %u", what, l, y);
      CHECK(w1 == 0u || sy + 1 < Ls.h, "%s level %d source row %d + 1", what, l, sy);
      seen[y] = 1;
      emitted++;
    }
    CHECK(emitted == L.h, "%s level %d: %d of %d rows", what, l, emitted, L.h);
    CHECK(Ls.wk_rows <= kWkMaxRows && (long long)L.pitch * L.h < (long long)kRzNoStore, "%s level %d", what, l);
  }
}

// part k of n: the sizes v with v % n == k (the test runs the parts side by side)
int sweep(int k, int n) {
  long plans = 0, unfused_widths = 0;
  int first_unfused = 0;
  for (int axis = 0; axis < 2; axis++)
    for (int v = 64; v <= 8192; v++)
      for (int mul_inv = 0; mul_inv < 2 && v % n == k; mul_inv++)
        for (int slots : {2, 256}) {
          const OrbPlanRequest rq = axis == 0 ? request(v, 64, slots, mul_inv != 0) : request(64, v, slots, mul_inv != 0);
          OrbPlan p;
          const std::string err = plan_orb(rq, &p);
          CHECK(err.empty(), "%d x %d: %s", rq.width, rq.height, err.c_str());
          if (!err.empty()) continue;
          bool fused = true;
          for (int l = 1; l < kOrbLevels; l++) fused = fused && p.g.lv[l].wk_fused != 0;
          // 17 strips reach 16 x 244 + 256 = 4160 px
          CHECK(fused == (rq.width <= 4160), "%d x %d, slots %d, mul_inv %d: fused %d", rq.width, rq.height, slots, mul_inv, (int)fused);
          if (!fused && mul_inv == 0 && slots == 2) {
            if (!unfused_widths) first_unfused = rq.width;
            unfused_widths++;
          }
          check_plan(rq, p);
          plans++;
        }
  std::printf("plans=%ld unfused=%ld first_unfused=%d failures=%d\n", plans, unfused_widths, first_unfused, failures);
  return failures ? 1 : 0;
}

// check_tail_lists (msf_debug_orb_tail's host check) on every level of a w x h plan: the rectangle's corners pass, one
// step outside any edge is refused, and so are levels without a rectangle, counts and scores out of range.  The lists
// are sized exactly, so a read past a list's end is the sanitizer's to report.
int tail_lists(int w, int h) {
  OrbPlan p;
  const std::string err = plan_orb(request(w, h, 4, false), &p);
  CHECK(err.empty(), "%d x %d: %s", w, h, err.c_str());
  if (!err.empty()) return 1;
  const OrbGeometry& g = p.g;
  int cap[kOrbLevels];
  for (int l = 0; l < kOrbLevels; l++) cap[l] = g.lv[l].cand_cap;
  auto one = [&](int l, int x, int y, int s) {
    std::vector<int32_t> counts(2 * kOrbLevels, 0), c = {x, y, s};
    counts[kOrbLevels + l] = 1;                       // the second of two frames
    return check_tail_lists(g, cap, 2, counts.data(), c.data());
  };
  int with_rect = 0;
  for (int l = 0; l < kOrbLevels; l++) {
    const OrbLevelInfo& L = g.lv[l];
    const int x1 = L.w - kEdge - 1, y1 = L.h - kEdge - 1;
    if (x1 < kEdge || y1 < kEdge) {
      CHECK(!one(l, kEdge, kEdge, 50).empty(), "level %d has no rectangle", l);
      continue;
    }
    with_rect++;
    for (int x : {kEdge, x1})
      for (int y : {kEdge, y1}) CHECK(one(l, x, y, 0).empty() && one(l, x, y, 255).empty(), "level %d corner %d %d", l, x, y);
    CHECK(!one(l, kEdge - 1, kEdge, 50).empty() && !one(l, x1 + 1, kEdge, 50).empty(), "level %d x outside", l);
    CHECK(!one(l, kEdge, kEdge - 1, 50).empty() && !one(l, kEdge, y1 + 1, 50).empty(), "level %d y outside", l);
    CHECK(!one(l, -kEdge, kEdge, 50).empty() && !one(l, kEdge, 1 << 20, 50).empty(), "level %d far outside", l);
    CHECK(!one(l, kEdge, kEdge, 256).empty() && !one(l, kEdge, kEdge, -1).empty(), "level %d score", l);
    std::vector<int32_t> counts(kOrbLevels, 0), c;
    counts[l] = cap[l] + kTailCountMargin;
    for (int i = 0; i < counts[l]; i++) { c.push_back(kEdge + i % (x1 - kEdge + 1)); c.push_back(y1); c.push_back(i & 255); }
    CHECK(check_tail_lists(g, cap, 1, counts.data(), c.data()).empty(), "level %d count = capacity + margin", l);
    c[3 * (counts[l] - 1)] = x1 + 1;                  // only the last entry is bad
    CHECK(!check_tail_lists(g, cap, 1, counts.data(), c.data()).empty(), "level %d last entry", l);
    counts[l]++;
    CHECK(!check_tail_lists(g, cap, 1, counts.data(), c.data()).empty(), "level %d count above the margin", l);
    counts[l] = -1;
    CHECK(!check_tail_lists(g, cap, 1, counts.data(), c.data()).empty(), "level %d negative count", l);
    counts[l] = 1;
    CHECK(!check_tail_lists(g, cap, 1, counts.data(), nullptr).empty(), "level %d null candidates", l);
  }
  std::vector<int32_t> none(kOrbLevels, 0);
  CHECK(check_tail_lists(g, cap, 1, none.data(), nullptr).empty(), "%s", "empty lists");
  CHECK(!check_tail_lists(g, cap, 0, none.data(), nullptr).empty() && !check_tail_lists(g, cap, 1, nullptr, nullptr).empty(),
        "%s", "no frames / null counts");
  std::printf("tail_lists %d x %d: levels_with_rectangle=%d failures=%d\n", w, h, with_rect, failures);
  return failures ? 1 : 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 4 && !std::strcmp(argv[1], "sweep") && std::atoi(argv[3]) > 0) return sweep(std::atoi(argv[2]), std::atoi(argv[3]));
  if (argc == 4 && !std::strcmp(argv[1], "tail_lists")) return tail_lists(std::atoi(argv[2]), std::atoi(argv[3]));
  std::vector<OrbPlanRequest> reqs;
  if (argc == 2 && !std::strcmp(argv[1], "golden")) {
    reqs = golden_requests();
  } else if (argc >= 6 && (argc - 2) % 4 == 0 && !std::strcmp(argv[1], "plans")) {
    for (int i = 2; i < argc; i += 4)
      reqs.push_back(request(std::atoi(argv[i]), std::atoi(argv[i + 1]), std::atoi(argv[i + 2]), std::atoi(argv[i + 3]) != 0));
  } else {
    return 2;
  }
  for (const OrbPlanRequest& rq : reqs) {
    OrbPlan p;
    const std::string err = plan_orb(rq, &p);
    print_plan(rq, err, p);
    if (err.empty()) check_plan(rq, p);
  }
  std::fprintf(stderr, "orb_plan: %zu plans, %d failure(s)\n", reqs.size(), failures);
  return failures ? 1 : 0;
}
