// csrc/loftr_pack.h in a stand-alone sanitized executable (tests/test_loftr_pack_host.py): every operand buffer that
// LoftrPipeline::init uploads is packed from the weights file named on the command line -- 21 d_w, 5 d_w2, 20 d_wx,
// 48 encoder matrices and their 32 split-bf16 twins -- and printed to stdout as "name bytes FNV-1a-64"; the test compares
// those lines with tests/golden/loftr_pack_digests.txt, recorded from the packing loops init had before this header
// existed.  Checks that need no recorded value go to stderr and into the exit status: split() on every weight and on
// edge cases, the non-zero count of every fragment buffer, the format each convolution selects.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>

#include "loftr_pack.h"
#include "weights_io.h"

namespace pk = msf::loftr_pack;

namespace {

int failures = 0;

#define CHECK(cond, ...)                                                   \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::fprintf(stderr, "line %d: %s does not hold: ", __LINE__, #cond); \
      std::fprintf(stderr, __VA_ARGS__);                                   \
      std::fprintf(stderr, "\n");                                          \
      failures++;                                                          \
    }                                                                      \
  } while (0)

int n_buffers[5] = {0, 0, 0, 0, 0};   // d_w, d_w2, d_wx, encoder f32, encoder split

template <class T>
void emit(const std::string& name, const char* kind, int kidx, const std::vector<T>& v) {
  uint64_t h = 1469598103934665603ull;   // FNV-1a 64, as msf::weights_digest
  const uint8_t* b = reinterpret_cast<const uint8_t*>(v.data());
  const size_t bytes = v.size() * sizeof(T);
  for (size_t i = 0; i < bytes; i++) { h ^= b[i]; h *= 1099511628211ull; }
  std::printf("%s.%s %zu %016llx\n", name.c_str(), kind, bytes, (unsigned long long)h);
  n_buffers[kidx]++;
}

float bits_to_float(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }
uint32_t float_to_bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

// round to nearest even without the packer's bit trick: the two bf16 neighbours of a finite v, compared in double
uint16_t bf16_nearest_even(float v) {
  const uint32_t u = float_to_bits(v), down = u & 0xFFFF0000u, up = down + 0x10000u;   // up: away from zero
  const double dd = std::fabs((double)v - (double)bits_to_float(down)), du = std::fabs((double)bits_to_float(up) - (double)v);
  if (dd != du) return (uint16_t)((dd < du ? down : up) >> 16);
  return (uint16_t)((((down >> 16) & 1u) ? up : down) >> 16);
}

// hi is the nearest-even bf16 of v, lo that of v - hi, and hi + lo is v to 2^-16 |v|: each rounding leaves at most half
// a unit of an 8-bit significand, 2^-8 relative, and the second one applies to a remainder of at most 2^-8 |v|
void check_split(float v, const char* what) {
  uint16_t hi, lo;
  pk::split(v, &hi, &lo);
  const float fhi = pk::from_bf16(hi), flo = pk::from_bf16(lo);
  CHECK(hi == bf16_nearest_even(v), "%s: v = %a", what, v);
  CHECK(lo == bf16_nearest_even(v - fhi), "%s: v = %a", what, v);
  CHECK(std::fabs((double)fhi + (double)flo - (double)v) <= std::ldexp(std::fabs((double)v), -16), "%s: v = %a", what, v);
}

size_t nonzero(const std::vector<float>& w) {
  size_t n = 0;
  for (float v : w) n += v != 0.f;
  return n;
}

// non-zero entries of the hi planes: as many as the source has non-zero weights -- none lost, none twice
size_t nonzero_hi(const std::vector<uint16_t>& x, const pk::FragDims& d) {
  size_t n = 0;
  const size_t frags = (size_t)d.groups * d.tiles;
  for (size_t f = 0; f < 2 * frags; f++) {
    const bool hi = d.planes == pk::Planes::Outer ? f < frags : (f & 1) == 0;
    for (size_t e = 0; hi && e < 512; e++) n += (x[f * 512 + e] & 0x7FFFu) != 0;
  }
  return n;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  msf::WeightMap blob;
  const std::string err = msf::load_weights(argv[1], &blob);
  if (!err.empty()) {
    std::fprintf(stderr, "%s\n", err.c_str());
    return 2;
  }

  // split(): every weight of the file, then the edge cases
  size_t n_weights = 0;
  for (const auto& kv : blob)
    for (float v : kv.second.data) {
      check_split(v, kv.first.c_str());
      n_weights++;
    }
  check_split(0.f, "zero");
  check_split(-0.f, "minus zero");
  check_split(bits_to_float(0x00800000u), "smallest normal");
  check_split(bits_to_float(0x3FFFFFFFu), "mantissa all ones");      // hi carries into the exponent: 2.0
  check_split(bits_to_float(0xBFFFFFFFu), "mantissa all ones, negative");
  check_split(bits_to_float(0x3F808000u), "tie, even below");        // 1 + 2^-8: stays at 1.0
  check_split(bits_to_float(0x3F818000u), "tie, even above");        // 1 + 3 * 2^-8: up to 1 + 2^-6
  {
    uint16_t hi, lo;
    pk::split(-0.f, &hi, &lo);
    CHECK(hi == 0x8000u && lo == 0, "minus zero keeps its sign: %04x %04x", hi, lo);
    pk::split(bits_to_float(0x3FFFFFFFu), &hi, &lo);
    CHECK(hi == 0x4000u && lo == 0xB400u, "2 - 2^-23 = 2.0 - 2^-23: %04x %04x", hi, lo);
  }

  // format selection: the kernel that run_backbone launches for each layer reads exactly this format
  using F = pk::ConvFmt;
  const F expect[pk::kConvs] = {F::Stem8,   F::Block8,   F::Block8,  F::Block8, F::Block8, F::Down16,   F::Block16,
                                F::Down16Sc, F::Block16, F::Block16, F::Convx2, F::Convx,  F::Convx2Sc, F::Convx,
                                F::Convx,   F::Convx2,   F::Convx,   F::Convx2Sc, F::Convx, F::Convx,   F::None};
  for (int i = 0; i < pk::kConvs; i++) CHECK(pk::conv_format(pk::kConv[i]) == expect[i], "convolution %d", i);

  for (int i = 0; i < pk::kConvs; i++) {
    const pk::ConvShape& c = pk::kConv[i];
    char nm[32];
    if (i < 20) std::snprintf(nm, sizeof nm, "conv%02d.w", i); else std::snprintf(nm, sizeof nm, "outconv.w");
    const auto it = blob.find(nm);
    if (it == blob.end() || it->second.data.size() != c.weights()) {
      std::fprintf(stderr, "io: weights blob lacks %s\n", nm);
      return 2;
    }
    const std::vector<float>& w = it->second.data;
    const std::vector<float> wb = pk::pack_conv_f32(c, w);
    emit(nm, "d_w", 0, wb);
    CHECK(nonzero(wb) == nonzero(w), "%s d_w", nm);
    if (pk::has_rowpair(c)) {
      const std::vector<float> w2 = pk::pack_conv_rowpair(c, w);
      emit(nm, "d_w2", 1, w2);
      CHECK(nonzero(w2) == 2 * nonzero(w), "%s d_w2: once per output row of the pair", nm);
    }
    if (pk::conv_format(c) != F::None) {
      const pk::FragDims d = pk::frag_dims(pk::conv_format(c), c.cin);
      const std::vector<uint16_t> wx = pk::pack_conv_split(c, w);
      emit(nm, "d_wx", 2, wx);
      CHECK(wx.size() == d.elems(), "%s d_wx: %zu elements", nm, wx.size());
      // the 8-cout formats hold every weight once per output row of the pair (lanes co + 8 rs)
      const size_t copies = c.cout == 8 ? 2 : 1;
      CHECK(nonzero_hi(wx, d) == copies * nonzero(w), "%s d_wx: %zu non-zero hi for %zu weights", nm, nonzero_hi(wx, d),
            nonzero(w));
    }
  }
  for (int b = 0; b < 8; b++)
    for (int k = 0; k < pk::kLinears; k++) {
      const pk::LinearSpec& l = pk::kLinear[k];
      const std::string nm = "blk" + std::to_string(b) + "." + l.name;
      const auto it = blob.find(nm);
      if (it == blob.end() || it->second.data.size() != (size_t)l.in * l.out) {
        std::fprintf(stderr, "io: weights blob lacks %s\n", nm.c_str());
        return 2;
      }
      const std::vector<float> p = pk::pack_linear(it->second.data, l.in, l.out, l.order);
      emit(nm, "p", 3, p);
      CHECK(nonzero(p) == nonzero(it->second.data), "%s", nm.c_str());
      if (l.split) {
        const std::vector<uint16_t> x = pk::pack_linear_split(p, l.in, l.out);
        emit(nm, "x", 4, x);
        CHECK(nonzero_hi(x, pk::linear_frag_dims(l.in, l.out)) == nonzero(it->second.data), "%s split", nm.c_str());
      }
    }
  CHECK(n_buffers[0] == 21 && n_buffers[1] == 5 && n_buffers[2] == 20 && n_buffers[3] == 48 && n_buffers[4] == 32,
        "buffers %d %d %d %d %d", n_buffers[0], n_buffers[1], n_buffers[2], n_buffers[3], n_buffers[4]);
  std::fprintf(stderr, "loftr_pack: %d failure(s), %zu weights split\n", failures, n_weights);
  return failures ? 1 : 0;
}
