// k_describe's patch image in LDS and its 7-tap row blur as nine integer matrix products (v_mfma_i32_16x16x64_i8):
// every index the kernel forms, as host code, plus an integer model of the tiling that tests/cpp/orb_blur_tiles_main.cpp
// holds to the direct sum.  Needs no HIP: the kernel includes it for the constants and the constexpr index functions.
//
//   raw[r][b]    r = 0 .. 44 <-> y = cy - 22 + r,  b = 0 .. 47 <-> x = cx - 24 + b, stored as p ^ 0x80 (= p - 128 as a
//                signed byte), pitch 48 B; rows 45 .. 47 and the 16 B behind them exist but are never written
//   hb[c][r]     = sum_j T[j] * p[r][c + 2 + j],  c = 0 .. 39 <-> x = cx - 19 + c (tap centre), column-major: the rows of
//                a column are consecutive u16, pitch kHbPitch
//
// One product: M = patch row, N = column c, K = raw byte of the row.  A lane's 16 operand bytes are (lane / 16, byte j);
// A and B both give that pair the raw column 16 (lane / 16) + j, so whatever order the hardware sums K in, equal
// (group, byte) pairs meet.  Raw columns 48 .. 63 are the first 16 B of the NEXT row: weight 0.  What is relied on of
// the instruction: A row = lane % 16, B column = lane % 16, D column = lane % 16 and D row = 4 (lane / 16) + register.
#pragma once
#include <stdint.h>

namespace msf {
namespace blur_tiles {

constexpr int kRawPitch = 48;                               // bytes per patch row
constexpr int kRawRows = 45;                                // rows fetched
constexpr int kRawRowsRead = 48;                            // rows the third M tile reads
constexpr int kRawBytes = kRawRowsRead * kRawPitch + 16;    // + the "next row" of row 47
constexpr int kFetchLoads = 9;                              // dword loads per lane: five rows each
constexpr int kFetchLanes = 60;                             // lane -> (row lane / 12 of five, dword lane % 12)
constexpr int kHbCols = 40;                                 // columns stored
constexpr int kHbRows = 46;                                 // rows stored (row 45: pad, read with weight 0)
// u16 per column.  A multiple of 4, so that a lane's four rows are one aligned 8-byte store; 26 dwords put the 16
// columns of such a store on 16 different even banks of the 32 (24 dwords: on 4)
constexpr int kHbPitch = 52;
constexpr int kHbEntries = kHbCols * kHbPitch;
constexpr int kTilesM = 3, kTilesN = 3;

constexpr int tap(bool sum256, int j) {
  const int k = j < 4 ? j : 6 - j;
  return k == 0 ? 18 : k == 1 ? 34 : k == 2 ? (sum256 ? 48 : 49) : (sum256 ? 56 : 55);
}
// the accumulators start at 128 * sum(T): the operand bytes are p - 128
constexpr int acc_init(bool sum256) { return 128 * (sum256 ? 256 : 257); }

// ---- patch fetch: load u of a lane is dword (lane % 12) of row 5 u + lane / 12; lanes 60 .. 63 repeat lane 59
constexpr int fetch_lane(int lane) { return lane < kFetchLanes ? lane : kFetchLanes - 1; }
constexpr int fetch_row(int lane) { return fetch_lane(lane) / 12; }
constexpr int fetch_dword(int lane) { return fetch_lane(lane) % 12; }
constexpr int raw_dword_of_load(int u, int lane) { return 60 * u + fetch_lane(lane); }

// ---- operands
constexpr int raw_col(int group, int byte) { return 16 * group + byte; }
constexpr int a_byte_offset(int mt, int lane) { return (16 * mt + lane % 16) * kRawPitch + 16 * (lane / 16); }
constexpr int b_weight(bool sum256, int nt, int lane, int byte) {
  const int k = raw_col(lane / 16, byte), j = k - (16 * nt + lane % 16) - 2;
  return k < kRawPitch && j >= 0 && j < 7 ? tap(sum256, j) : 0;
}
// register d of a lane's B operand = b_weight of bytes 4 d .. 4 d + 3, as the kernel forms it: the seven taps as the
// bytes of one 64-bit word, shifted by the tap index j0 of the register's first byte (the test holds it to b_weight)
constexpr uint64_t tap_word(bool sum256) {
  return (uint64_t)tap(sum256, 0) | (uint64_t)tap(sum256, 1) << 8 | (uint64_t)tap(sum256, 2) << 16 | (uint64_t)tap(sum256, 3) << 24 |
         (uint64_t)tap(sum256, 4) << 32 | (uint64_t)tap(sum256, 5) << 40 | (uint64_t)tap(sum256, 6) << 48;
}
constexpr uint32_t b_dword(bool sum256, int nt, int lane, int d) {
  const int j0 = 16 * (lane / 16) + 4 * d - (16 * nt + lane % 16) - 2;
  return lane >= 48 || j0 <= -4 || j0 >= 7 ? 0u
         : j0 >= 0 ? (uint32_t)(tap_word(sum256) >> (8 * j0)) : (uint32_t)(tap_word(sum256) << (8 * -j0));
}

// ---- results: register i of a lane is row d_row0 + i of column d_col
constexpr int d_col(int nt, int lane) { return 16 * nt + lane % 16; }
constexpr int d_row0(int mt, int lane) { return 16 * mt + 4 * (lane / 16); }
// dwords (u16 pairs) of its four rows a lane stores: none beyond column 39, rows 44 | 45 only of the last four
constexpr int hb_store_dwords(int mt, int nt, int lane) {
  return d_col(nt, lane) >= kHbCols ? 0 : d_row0(mt, lane) + 4 <= kHbRows ? 2 : d_row0(mt, lane) + 2 <= kHbRows ? 1 : 0;
}
constexpr int hb_store_byte_offset(int mt, int nt, int lane) { return 2 * (d_col(nt, lane) * kHbPitch + d_row0(mt, lane)); }
constexpr uint32_t pack2(uint32_t lo, uint32_t hi) { return (lo & 0xFFFFu) | hi << 16; }   // a stored row is <= 255 * 257

// ---- readers.  Moments: task t (0 .. 255) reads dword 2 + t % 8 of raw row 7 + t / 8 (pixels u = -16 + 4 (t % 8) .. + 3
// of disc row v = t / 8 - 15).  Samples: the seven vertical taps of sample (ix, iy), |ix|, |iy| <= 19, are rows
// 19 + iy .. 25 + iy of column 19 + ix, read as the four dwords from the byte offset below rounded down to 4
constexpr int moment_dword(int t) { return (7 + t / 8) * (kRawPitch / 4) + 2 + t % 8; }
constexpr int kSampleReach = 19;
constexpr int samp_byte_offset(int ix, int iy) { return 2 * ((kSampleReach + ix) * kHbPitch + kSampleReach + iy); }

// ---- the model: what the 64 lanes of a wave do for one patch, one statement per instruction of the kernel.
// raw: kRawBytes (p ^ 0x80; rows >= 45 hold whatever they hold), hb: kHbEntries, untouched where nothing is stored.
inline void model_row_blur(bool sum256, const uint8_t* raw, uint16_t* hb) {
  for (int mt = 0; mt < kTilesM; mt++)
    for (int nt = 0; nt < kTilesN; nt++) {
      int32_t acc[16][16];                                  // [row of the tile][column of the tile]
      for (int i = 0; i < 16; i++)
        for (int n = 0; n < 16; n++) acc[i][n] = acc_init(sum256);
      // the product: row i comes from the lanes with lane % 16 == i, column n likewise; K = (group, byte)
      for (int la = 0; la < 64; la++)
        for (int lb = 0; lb < 64; lb++) {
          if (la / 16 != lb / 16) continue;
          const uint8_t* a = raw + a_byte_offset(mt, la);   // one 16-byte LDS read
          for (int j = 0; j < 16; j++)
            acc[la % 16][lb % 16] += (int32_t)(int8_t)a[j] * (int32_t)(int8_t)(b_dword(sum256, nt, lb, j / 4) >> (8 * (j % 4)));
        }
      for (int lane = 0; lane < 64; lane++) {
        const int n = hb_store_dwords(mt, nt, lane);
        uint16_t* w = hb + hb_store_byte_offset(mt, nt, lane) / 2;
        const int i0 = d_row0(mt, lane) - 16 * mt, c = lane % 16;
        for (int i = 0; i < n; i++) {
          const uint32_t pair = pack2((uint32_t)acc[i0 + 2 * i][c], (uint32_t)acc[i0 + 2 * i + 1][c]);
          w[2 * i] = (uint16_t)pair;                        // little-endian dword
          w[2 * i + 1] = (uint16_t)(pair >> 16);
        }
      }
    }
}

}  // namespace blur_tiles
}  // namespace msf
