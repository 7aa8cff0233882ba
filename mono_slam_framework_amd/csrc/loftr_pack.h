// LoFTR weights -> the operand layouts of the kernels in loftr_kernels.hip.  Host arithmetic only (no HIP include):
// LoftrPipeline::init packs and uploads with it, tests/cpp/loftr_pack_main.cpp checks it in a sanitized CPU build.
//
// Per convolution: d_w (k_conv, f32 MFMA), d_w2 (k_conv RP = 2 / k_block8, row pairs) and at most one split-bf16
// fragment buffer d_wx, whose format conv_format() selects.  Per encoder matrix: the P8 / PD slot orders (pack_linear)
// and, for the four matrices k_attn_update_x multiplies by, their split-bf16 fragments (pack_linear_split).
//
// A split-bf16 buffer is a sequence of fragments of [64 lanes][8] bf16: a lane's 16 bytes are its half of one MFMA
// operand (v_mfma_f32_16x16x32_bf16).  Every value v is stored twice, as hi = bf16(v) and lo = bf16(v - hi).
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

namespace msf {
namespace loftr_pack {

inline uint16_t to_bf16(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  u += 0x7FFFu + ((u >> 16) & 1u);      // round to nearest even (weights are finite)
  return (uint16_t)(u >> 16);
}
inline float from_bf16(uint16_t h) {
  const uint32_t u = (uint32_t)h << 16;
  float f;
  memcpy(&f, &u, 4);
  return f;
}
inline void split(float v, uint16_t* hi, uint16_t* lo) {
  *hi = to_bf16(v);
  *lo = to_bf16(v - from_bf16(*hi));
}

// ------------------------------------------------------------------ the 21 convolutions
// backbone, index = execution order of the graph (and of the weight blob); [20] = outconv
struct ConvShape {
  int cin, cout, ks, stride, hin, win;
  constexpr int hout() const { return (hin + 2 * (ks / 2) - ks) / stride + 1; }
  constexpr int wout() const { return (win + 2 * (ks / 2) - ks) / stride + 1; }
  constexpr size_t weights() const { return (size_t)cout * cin * ks * ks; }
  constexpr size_t at(int co, int ci, int ky, int kx) const { return (((size_t)co * cin + ci) * ks + ky) * ks + kx; }
};
constexpr int kConvs = 21;
constexpr ConvShape kConv[kConvs] = {
    // cin cout ks stride hin win
    {1, 8, 7, 2, 480, 640},   {8, 8, 3, 1, 240, 320},   {8, 8, 3, 1, 240, 320},   {8, 8, 3, 1, 240, 320},
    {8, 8, 3, 1, 240, 320},   {8, 16, 3, 2, 240, 320},  {16, 16, 3, 1, 120, 160}, {8, 16, 1, 2, 240, 320},
    {16, 16, 3, 1, 120, 160}, {16, 16, 3, 1, 120, 160}, {16, 32, 3, 2, 120, 160}, {32, 32, 3, 1, 60, 80},
    {16, 32, 1, 2, 120, 160}, {32, 32, 3, 1, 60, 80},   {32, 32, 3, 1, 60, 80},   {32, 32, 3, 2, 60, 80},
    {32, 32, 3, 1, 30, 40},   {32, 32, 1, 2, 60, 80},   {32, 32, 3, 1, 30, 40},   {32, 32, 3, 1, 30, 40},
    {32, 32, 1, 1, 30, 40}};

// rows of a k_conv weight matrix [k steps padded to whole prefetch groups][4][NPAD] for `ktot` values of k
constexpr int conv_k_rows(int ktot) {
  const int ksteps = (ktot + 3) / 4, grp = ksteps >= 4 ? 4 : ksteps;
  return ((ksteps + grp - 1) / grp) * grp * 4;   // = ConvCfg::NG * G * 4
}

// d_w: [k = (ky * ks + kx) * cin + ci][NPAD], cout padded to a multiple of 16
inline std::vector<float> pack_conv_f32(const ConvShape& c, const std::vector<float>& w) {
  const int npad = ((c.cout + 15) / 16) * 16;
  std::vector<float> wb((size_t)conv_k_rows(c.ks * c.ks * c.cin) * npad, 0.f);
  for (int co = 0; co < c.cout; co++)
    for (int ci = 0; ci < c.cin; ci++)
      for (int ky = 0; ky < c.ks; ky++)
        for (int kx = 0; kx < c.ks; kx++) wb[(size_t)((ky * c.ks + kx) * c.cin + ci) * npad + co] = w[c.at(co, ci, ky, kx)];
  return wb;
}

constexpr bool has_rowpair(const ConvShape& c) { return c.cout == 8 && (c.stride == 1 || c.cin == 1); }

// d_w2, row-packed weights (RP = 2): k = ((kyy * ks + kx) * cin + ci) over ks + stride input rows,
// column = row_sel * 8 + co; output row rs sees input rows stride * rs .. stride * rs + ks - 1
inline std::vector<float> pack_conv_rowpair(const ConvShape& c, const std::vector<float>& w) {
  std::vector<float> w2((size_t)conv_k_rows((c.ks + c.stride) * c.ks * c.cin) * 16, 0.f);
  for (int rs = 0; rs < 2; rs++)
    for (int co = 0; co < 8; co++)
      for (int ci = 0; ci < c.cin; ci++)
        for (int ky = 0; ky < c.ks; ky++)
          for (int kx = 0; kx < c.ks; kx++)
            w2[(size_t)(((ky + c.stride * rs) * c.ks + kx) * c.cin + ci) * 16 + rs * 8 + co] = w[c.at(co, ci, ky, kx)];
  return w2;
}

// ------------------------------------------------------------------ split-bf16 fragments
// [hi | lo] is either the outermost index, [hi | lo][group][tile][lane][8], or sits just above a fragment,
// [group][tile][hi | lo][lane][8]
enum class Planes { Outer, Inner };
struct FragDims {
  int groups, tiles;
  Planes planes;
  constexpr size_t elems() const { return (size_t)2 * groups * tiles * 64 * 8; }
};

// The one fragment writer: value(g, n, lane, j) is element j of lane `lane` of the fragment of group g and tile n.
template <class F>
std::vector<uint16_t> write_fragments(const FragDims& d, F value) {
  std::vector<uint16_t> out(d.elems(), 0);
  const size_t frags = (size_t)d.groups * d.tiles;
  for (int g = 0; g < d.groups; g++)
    for (int n = 0; n < d.tiles; n++) {
      const size_t f = (size_t)g * d.tiles + n;
      const size_t fhi = d.planes == Planes::Outer ? f : 2 * f, flo = d.planes == Planes::Outer ? frags + f : 2 * f + 1;
      for (int l = 0; l < 64; l++)
        for (int j = 0; j < 8; j++) split(value(g, n, l, j), &out[(fhi * 64 + l) * 8 + j], &out[(flo * 64 + l) * 8 + j]);
    }
  return out;
}

enum class ConvFmt { None, Stem8, Block8, Down16, Down16Sc, Block16, Convx2, Convx2Sc, Convx };

// the split-bf16 format of a convolution: exactly one, or None (outconv runs on k_conv only)
constexpr ConvFmt conv_format(int cin, int cout, int ks, int stride) {
  return cin == 1 && ks == 7                               ? ConvFmt::Stem8
         : cout == 8 && cin == 8 && stride == 1            ? ConvFmt::Block8
         : cout == 16 && cin == 8 && stride == 2 && ks == 3 ? ConvFmt::Down16
         : cout == 16 && cin == 8 && stride == 2 && ks == 1 ? ConvFmt::Down16Sc
         : cout == 16 && cin == 16 && stride == 1          ? ConvFmt::Block16
         : cout == 32 && stride == 2 && ks == 3            ? ConvFmt::Convx2
         : cout == 32 && stride == 2 && ks == 1            ? ConvFmt::Convx2Sc
         : cout == 32 && cin == 32 && stride == 1 && ks == 3 ? ConvFmt::Convx
                                                           : ConvFmt::None;
}
constexpr ConvFmt conv_format(const ConvShape& c) { return conv_format(c.cin, c.cout, c.ks, c.stride); }

// fragment counts of each format (the kernels' own constants are asserted equal in loftr_kernels.hip)
constexpr FragDims frag_dims(ConvFmt f, int cin) {
  return f == ConvFmt::Stem8 || f == ConvFmt::Block8 || f == ConvFmt::Down16 ? FragDims{3, 1, Planes::Outer}
         : f == ConvFmt::Down16Sc ? FragDims{1, 1, Planes::Outer}
         : f == ConvFmt::Block16  ? FragDims{5, 1, Planes::Outer}
         : f == ConvFmt::Convx2   ? FragDims{cin == 32 ? 9 : 5, 2, Planes::Inner}
         : f == ConvFmt::Convx2Sc ? FragDims{1, 2, Planes::Inner}
         : f == ConvFmt::Convx    ? FragDims{9, 2, Planes::Inner}
                                  : FragDims{0, 0, Planes::Outer};
}

constexpr size_t frag_elems(ConvFmt f, int cin) { return frag_dims(f, cin).elems(); }

// d_wx of a convolution whose format is not None.  In every format lane l of a 16-cout tile holds cout l & 15 (two rows
// of 8 in the 8-cout kernels) and K block kq = l >> 4; element j is one of 8 input channels (kx in the stem).
inline std::vector<uint16_t> pack_conv_split(const ConvShape& c, const std::vector<float>& w) {
  const ConvFmt f = conv_format(c);
  const FragDims d = frag_dims(f, c.cin);
  const int cin = c.cin;
  auto tap = [&](int co, int ci, int t) { return t < 9 ? w[c.at(co, ci, t / 3, t % 3)] : 0.f; };   // the tenth tap: zero
  switch (f) {
    case ConvFmt::Stem8:
      // k_stem_strip8x stage 0: fragment (hi | lo, row group g): element j = kx of lane (idx = co + 8 rs, kq) is
      // w[co][ky = 4 g + kq - 2 rs][kx] / 255 (0 outside the 7 x 7 window); an output row pair spans image rows s = 0 .. 8
      return write_fragments(d, [&](int g, int, int l, int j) {
        const int co = l & 7, rs = (l >> 3) & 1, ky = 4 * g + (l >> 4) - 2 * rs;
        return (ky >= 0 && ky <= 6 && j <= 6) ? w[c.at(co, 0, ky, j)] * (float)(1.0 / 255.0) : 0.f;
      });
    case ConvFmt::Block8:
      // k_block8x: element j of lane (idx = co + 8 rs, input row s) of fragment kx is w[co][ci = j][ky = s - rs][kx]
      // (0 where output row rs does not see input row s)
      return write_fragments(d, [&](int g, int, int l, int j) {
        const int co = l & 7, rs = (l >> 3) & 1, ky = (l >> 4) - rs;
        return (ky >= 0 && ky <= 2) ? w[c.at(co, j, ky, g)] : 0.f;
      });
    case ConvFmt::Down16:
      // k_down16x stage 1: fragment (hi | lo, ky): element j = ci of lane (cout l & 15, kx = l >> 4) is w[cout][ci][ky][kx]
      // (kx = 3: zero)
      return write_fragments(d, [&](int g, int, int l, int j) { return (l >> 4) < 3 ? w[c.at(l & 15, j, g, l >> 4)] : 0.f; });
    case ConvFmt::Down16Sc:
      // k_down16x shortcut: rides on the ky = 1 fragments, whose kx = 1 block is the pixel (2Y, 2X): other blocks zero
      return write_fragments(d, [&](int, int, int l, int j) { return (l >> 4) == 1 ? w[c.at(l & 15, j, 0, 0)] : 0.f; });
    case ConvFmt::Block16:
      // k_block16x: fragment (hi | lo, g): element j of lane (cout l & 15, kq = l >> 4) is
      // w[cout][ci = 8 (kq & 1) + j][tap 2 g + (kq >> 1)] (0 for the tenth tap)
      return write_fragments(d, [&](int g, int, int l, int j) {
        const int q = l >> 4;
        return tap(l & 15, 8 * (q & 1) + j, 2 * g + (q >> 1));
      });
    case ConvFmt::Convx2:
      // k_convx2<CIN>: fragment (g, cout tile n, hi | lo): lane (cout 16 n + (l & 15), kq = l >> 4), element j:
      //   CIN = 32: w[cout][ci = 8 kq + j][tap g];  CIN = 16: w[cout][ci = 8 (kq & 1) + j][tap 2 g + (kq >> 1)] (tenth tap: 0)
      return write_fragments(d, [&](int g, int n, int l, int j) {
        const int co = 16 * n + (l & 15), q = l >> 4;
        return cin == 32 ? tap(co, 8 * q + j, g) : tap(co, 8 * (q & 1) + j, 2 * g + (q >> 1));
      });
    case ConvFmt::Convx2Sc:
      // k_convx2 shortcut: rides on the centre tap's fragment: CIN = 32: every K block (channel block kq);
      // CIN = 16: the blocks of tap 4 = kq 0, 1 of group 2 (kq 2, 3 hold tap 5: zero)
      return write_fragments(d, [&](int, int n, int l, int j) {
        const int co = 16 * n + (l & 15), q = l >> 4;
        return (cin == 32 || q < 2) ? w[c.at(co, 8 * q + j, 0, 0)] : 0.f;
      });
    case ConvFmt::Convx:
      // k_convx<32>: fragment (tap g, cout tile n, hi | lo): element j of lane (cout 16 n + (l & 15), channel block l >> 4)
      // is w[cout][ci = 8 (l >> 4) + j][ky = g / 3][kx = g % 3]
      return write_fragments(d, [&](int g, int n, int l, int j) { return tap(16 * n + (l & 15), 8 * (l >> 4) + j, g); });
    case ConvFmt::None:
      break;
  }
  return {};
}

// ------------------------------------------------------------------ the encoder's matrices
// slot orders (see the kernel comments at BlockW): P8 (feature 8*kq + s), PD (feature 16*(s/4) + 4*kq + s%4);
// Split: wmlp0's 64 inputs are [x (P8, 8 slots) | merged message (PD, 8 slots)]
enum class SlotOrder { P8, PD, Split };
struct LinearSpec {
  const char* name;
  int in, out;
  SlotOrder order;
  bool split;   // k_attn_update_x multiplies by it: split-bf16 fragments as well
};
constexpr int kLinears = 6;
constexpr LinearSpec kLinear[kLinears] = {{"wq", 32, 32, SlotOrder::P8, true},       {"wk", 32, 32, SlotOrder::P8, false},
                                          {"wv", 32, 32, SlotOrder::P8, false},      {"wmerge", 32, 32, SlotOrder::PD, true},
                                          {"wmlp0", 64, 64, SlotOrder::Split, true}, {"wmlp1", 64, 32, SlotOrder::PD, true}};

// w [in][out] -> [(mtile * slots + slot) * 64 + lane]: lane (column 16 mtile + (lane & 15), kq = lane >> 4)
inline std::vector<float> pack_linear(const std::vector<float>& w, int in, int out, SlotOrder order) {
  const int slots = in / 4, mtiles = out / 16;
  std::vector<float> pk((size_t)in * out);
  for (int mt = 0; mt < mtiles; mt++)
    for (int sl = 0; sl < slots; sl++)
      for (int ln = 0; ln < 64; ln++) {
        const int kq = ln >> 4, p8 = 8 * kq + sl, s2 = order == SlotOrder::Split ? sl & 7 : sl;
        const int pd = 16 * (s2 >> 2) + 4 * kq + (s2 & 3);
        const int feat = order == SlotOrder::P8 ? p8 : order == SlotOrder::PD ? pd : sl < 8 ? p8 : 32 + pd;
        pk[((size_t)mt * slots + sl) * 64 + ln] = w[(size_t)feat * out + 16 * mt + (ln & 15)];
      }
  return pk;
}

constexpr FragDims linear_frag_dims(int in, int out) { return FragDims{out / 16, in / 32, Planes::Inner}; }

// k_attn_update_x: fragment (mtile, K group kg, hi | lo): element j of lane ln is slot 8 kg + j of pack_linear's result
inline std::vector<uint16_t> pack_linear_split(const std::vector<float>& pk, int in, int out) {
  const int slots = in / 4;
  return write_fragments(linear_frag_dims(in, out),
                         [&](int mt, int kg, int ln, int j) { return pk[((size_t)mt * slots + kg * 8 + j) * 64 + ln]; });
}

}  // namespace loftr_pack
}  // namespace msf
