// csrc/orb_blur_tiles.h in a stand-alone executable (tests/test_orb_blur_tiles_host.py), never inside python: the patch
// image k_describe keeps in LDS and its row blur as 3 x 3 tiles of a 16 x 16 x 64 integer matrix product, run as the
// header's integer model on heap arrays of exactly the kernel's LDS sizes (so the sanitizers see every index).
//   orb_blur_tiles            both tap sets x (all 0, all 255, 0 | 255 by column, by row, random patches): every
//                             hb[c][r], c < 40, r < 45, against the direct 7-tap sum; what is stored and what is not;
//                             every index of the fetch, the operands, the stores, the moments and the samples.
//                             Failures to stderr and the exit status; one summary line to stdout.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "orb_blur_tiles.h"

using namespace msf::blur_tiles;

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

uint32_t rng_state = 0x9E3779B9u;
uint32_t rng() {   // xorshift32
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 17;
  rng_state ^= rng_state << 5;
  return rng_state;
}

constexpr uint16_t kSentinel = 0xBEEF;   // what hb holds before the model runs; compared exactly where nothing may be stored

// the 45 x 48 pixels of a patch; pixel (r, b) is image pixel (cx - 24 + b, cy - 22 + r)
typedef std::vector<uint8_t> Patch;

Patch make_patch(int kind) {
  Patch p(kRawRows * kRawPitch);
  for (int r = 0; r < kRawRows; r++)
    for (int b = 0; b < kRawPitch; b++) {
      uint8_t v = 0;
      switch (kind) {
        case 0: v = 0; break;
        case 1: v = 255; break;
        case 2: v = (b & 1) ? 255 : 0; break;
        case 3: v = (b & 1) ? 0 : 255; break;
        case 4: v = (r & 1) ? 255 : 0; break;
        case 5: v = (r & 1) ? 0 : 255; break;
        default: v = (uint8_t)(rng() >> 13); break;
      }
      p[r * kRawPitch + b] = v;
    }
  return p;
}

// the kernel's staging: load u of a lane lands at dword raw_dword_of_load(u, lane), as p ^ 0x80; the rest of the image
// is filled with `fill` first (the kernel never writes it)
void stage(const Patch& p, uint8_t fill, uint8_t* raw) {
  std::memset(raw, fill, kRawBytes);
  std::vector<int> written(kRawBytes / 4, 0);
  for (int u = 0; u < kFetchLoads; u++)
    for (int lane = 0; lane < 64; lane++) {
      const int row = 5 * u + fetch_row(lane), dw = fetch_dword(lane), at = raw_dword_of_load(u, lane);
      CHECK(row < kRawRows && dw < kRawPitch / 4, "load %d lane %d fetches row %d dword %d", u, lane, row, dw);
      CHECK(at == row * (kRawPitch / 4) + dw, "load %d lane %d lands at dword %d", u, lane, at);
      CHECK(at >= 0 && at < kRawRows * (kRawPitch / 4), "load %d lane %d lands at dword %d", u, lane, at);
      for (int e = 0; e < 4; e++) raw[4 * at + e] = p[row * kRawPitch + 4 * dw + e] ^ 0x80;
      written[at]++;
    }
  for (int i = 0; i < kRawRows * (kRawPitch / 4); i++) CHECK(written[i] >= 1, "raw dword %d is never written", i);
  for (int i = kRawRows * (kRawPitch / 4); i < kRawBytes / 4; i++) CHECK(written[i] == 0, "raw dword %d is written", i);
}

int patches_checked = 0;

void check_patch(bool sum256, const Patch& p) {
  // twice, with different bytes where the kernel's LDS holds whatever it held: what is stored must not depend on them
  std::vector<uint16_t> hb[2];
  for (int pass = 0; pass < 2; pass++) {
    uint8_t* raw = (uint8_t*)std::malloc(kRawBytes);   // exactly the kernel's array: an index past it is a sanitizer report
    stage(p, pass ? 0x7F : 0x80, raw);
    hb[pass].assign(kHbEntries, kSentinel);
    model_row_blur(sum256, raw, hb[pass].data());
    std::free(raw);
  }
  // (row 45, the pad row the samples read with weight 0, is the blur of raw row 45: it does, and is left out)
  for (int c = 0; c < kHbCols; c++)
    for (int r = 0; r < kHbPitch; r++)
      if (r != kRawRows) CHECK(hb[0][c * kHbPitch + r] == hb[1][c * kHbPitch + r], "hb[%d][%d] depends on raw bytes that are never written", c, r);
  for (int c = 0; c < kHbCols; c++)
    for (int r = 0; r < kHbPitch; r++) {
      const uint16_t got = hb[0][c * kHbPitch + r];
      if (r < kRawRows) {
        uint32_t want = 0;
        for (int j = 0; j < 7; j++) want += (uint32_t)tap(sum256, j) * p[r * kRawPitch + c + 2 + j];
        CHECK(got == want, "sum256=%d hb[%d][%d] = %u, direct sum %u", (int)sum256, c, r, (unsigned)got, (unsigned)want);
      } else if (r >= kHbRows) {
        CHECK(got == kSentinel, "sum256=%d hb[%d][%d] was stored", (int)sum256, c, r);
      }
    }
  patches_checked++;
}

void check_indices() {
  // operands: aligned 16-byte reads inside the raw image; B by its definition
  for (int mt = 0; mt < kTilesM; mt++)
    for (int lane = 0; lane < 64; lane++) {
      const int a = a_byte_offset(mt, lane);
      CHECK(a % 16 == 0 && a >= 0 && a + 16 <= kRawBytes, "A operand of tile %d lane %d at byte %d", mt, lane, a);
      CHECK(a == a_byte_offset(0, lane) + mt * 16 * kRawPitch, "A operand of tile %d lane %d: not lane base + constant", mt, lane);
    }
  for (int s = 0; s < 2; s++)
    for (int nt = 0; nt < kTilesN; nt++)
      for (int lane = 0; lane < 64; lane++)
        for (int d = 0; d < 4; d++) {
          uint32_t want = 0;
          for (int e = 0; e < 4; e++) {
            const int w = b_weight(s != 0, nt, lane, 4 * d + e);
            CHECK(w >= 0 && w < 128, "B weight %d", w);
            want |= (uint32_t)w << (8 * e);
          }
          CHECK(b_dword(s != 0, nt, lane, d) == want, "B register %d of lane %d, column tile %d", d, lane, nt);
        }
  for (int s = 0; s < 2; s++) {
    int sum = 0;
    for (int j = 0; j < 7; j++) sum += tap(s != 0, j);
    CHECK(sum == (s ? 256 : 257) && acc_init(s != 0) == 128 * sum, "tap sum %d", sum);
  }
  // stores: inside hb, aligned to their width, never a row >= 46 or a column >= 40, every (column < 40, row < 46) once
  std::vector<int> stored(kHbEntries, 0);
  for (int mt = 0; mt < kTilesM; mt++)
    for (int nt = 0; nt < kTilesN; nt++)
      for (int lane = 0; lane < 64; lane++) {
        const int n = hb_store_dwords(mt, nt, lane), at = hb_store_byte_offset(mt, nt, lane);
        CHECK(at == hb_store_byte_offset(0, 0, lane) + 2 * (16 * nt * kHbPitch + 16 * mt), "store of tile (%d, %d) lane %d: not lane base + constant", mt, nt, lane);
        if (!n) continue;
        CHECK(at % (4 * n) == 0 && at >= 0 && at + 4 * n <= 2 * kHbEntries, "store of tile (%d, %d) lane %d at byte %d", mt, nt, lane, at);
        CHECK(d_col(nt, lane) < kHbCols && d_row0(mt, lane) + 2 * n <= kHbRows, "store of tile (%d, %d) lane %d: column %d rows %d + %d",
              mt, nt, lane, d_col(nt, lane), d_row0(mt, lane), 2 * n);
        CHECK(at == 2 * (d_col(nt, lane) * kHbPitch + d_row0(mt, lane)), "store of tile (%d, %d) lane %d", mt, nt, lane);
        for (int i = 0; i < 2 * n; i++) stored[at / 2 + i]++;
      }
  for (int c = 0; c < kHbCols; c++)
    for (int r = 0; r < kHbPitch; r++)
      CHECK(stored[c * kHbPitch + r] == (r < kHbRows ? 1 : 0), "hb[%d][%d] is stored %d times", c, r, stored[c * kHbPitch + r]);
  // readers: the moments stay inside the fetched rows; a sample's four dwords stay inside hb, its seven weighted rows
  // are rows < 45 of a column < 40 and the eighth (weight 0) is a stored row
  for (int t = 0; t < 256; t++) CHECK(moment_dword(t) >= 0 && moment_dword(t) < kRawRows * (kRawPitch / 4), "moment task %d reads dword %d", t, moment_dword(t));
  for (int ix = -kSampleReach; ix <= kSampleReach; ix++)
    for (int iy = -kSampleReach; iy <= kSampleReach; iy++) {
      const int at = samp_byte_offset(ix, iy), lo = at & ~3;
      CHECK(lo >= 0 && lo + 16 <= 2 * kHbEntries, "sample (%d, %d) reads bytes %d .. %d", ix, iy, lo, lo + 15);
      const int c = at / 2 / kHbPitch, r = at / 2 % kHbPitch;
      CHECK(c == kSampleReach + ix && c < kHbCols - 1 && r == kSampleReach + iy && r + 6 < kRawRows, "sample (%d, %d): column %d rows %d ..", ix, iy, c, r);
      CHECK(lo / 2 / kHbPitch == c && (lo + 14) / 2 / kHbPitch == c && (lo + 14) / 2 % kHbPitch < kHbRows, "sample (%d, %d) reads past its column's stored rows", ix, iy);
    }
}

}  // namespace

int main() {
  check_indices();
  for (int s = 0; s < 2; s++) {
    for (int kind = 0; kind < 6; kind++) check_patch(s != 0, make_patch(kind));
    for (int i = 0; i < 24; i++) check_patch(s != 0, make_patch(6));
  }
  std::printf("orb_blur_tiles: patches=%d failures=%d\n", patches_checked, failures);
  return failures ? 1 : 0;
}
