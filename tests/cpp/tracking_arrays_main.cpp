// Stand-alone program (its own main; built with -fsanitize=address,undefined by tests/test_tracking_arrays_host.py and
// run as an executable): the tables of msf_frustum_result and msf_claim_result (csrc/tracking_arrays.h) through
// carve_result() and copy_result() of result_arrays.h, as the host entry points of msf_tracking.h use them.  Over calls
// of several sizes (0 included) and the wanted sets none / all / alone / alternating: every piece lies on the 256-byte
// grid, has the documented size and overlaps no other, nothing is carved for what nobody needs, and the copy-back moves
// every byte of a wanted array and nothing else (the caller's arrays are allocated exactly, so a write past one is a
// heap overflow the sanitizer sees).  `--print`: both tables, one row per line, for the comparison with
// _lib.FRUSTUM_ARRAYS / _lib.CLAIM_ARRAYS.  Exit status 0: every case held.
#include <cstdio>
#include <cstring>
#include <vector>

#include "tracking_arrays.h"

using namespace msf;

static int bad = 0;
static void check(bool ok, const char* what, const char* name) {
  if (!ok) std::printf("BAD %s (%s)\n", what, name), bad++;
}

template <class S, size_t N>
static void run(const ResultArray (&table)[N], const size_t* units, size_t cap, int pattern, int alone) {
  std::vector<std::vector<uint8_t>> host(N);
  S out{};
  out.struct_size = sizeof out;
  for (size_t i = 0; i < N; i++) {
    const bool want = pattern == 1 || (pattern == 2 && (int)i == alone) || (pattern == 3 && i % 2 == 0);
    const size_t bytes = array_bytes(table[i], units, cap);
    if (!want || !bytes) continue;
    host[i].assign(bytes, 0xCD);
    set_slot(&out, table[i], host[i].data());
  }
  Carver measure;
  S dev{};
  carve_result(measure, table, units, cap, nullptr, out, &dev);
  std::vector<uint8_t> block(measure.off + 1, 0);
  Carver place{block.data()};
  carve_result(place, table, units, cap, nullptr, out, &dev);
  check(place.off == measure.off, "the two passes disagree", "layout");
  size_t expect = 0;
  for (size_t i = 0; i < N; i++) {
    const ResultArray& a = table[i];
    const size_t bytes = array_bytes(a, units, cap);
    uint8_t* p = slot(dev, a);
    if (!(a.required || slot(out, a))) {
      check(p == nullptr, "a piece nobody needs", a.name);
      continue;
    }
    check(p == block.data() + expect, "piece not where the sizes before it put it", a.name);
    check((size_t)(p - block.data()) % 256 == 0, "piece off the 256-byte grid", a.name);
    expect += (bytes + 255) & ~(size_t)255;
    std::memset(p, (int)(i + 1), bytes);   // what the kernels would write: the sanitizer guards the block's end
  }
  check(expect == measure.off, "the pieces do not add up", "layout");
  const Extent all{0, cap, cap, cap, units, units};
  size_t copies = 0;
  const int rc = copy_result(table, dev, out, all, [&](void* dst, const void* src, size_t bytes) {
    std::memcpy(dst, src, bytes);
    copies++;
    return 0;
  });
  check(rc == 0, "copy_result failed", "copy");
  size_t wanted = 0;
  for (size_t i = 0; i < N; i++) {
    if (host[i].empty()) continue;
    wanted++;
    bool ok = true;
    for (uint8_t b : host[i]) ok = ok && b == (uint8_t)(i + 1);
    check(ok, "the copy-back left bytes of a wanted array", table[i].name);
  }
  check(copies == wanted, "not one copy per wanted array", "copy");
}

template <class S, size_t N>
static void sweep(const ResultArray (&table)[N], const size_t* units, size_t cap) {
  for (int pattern : {0, 1, 3}) run<S>(table, units, cap, pattern, -1);
  for (int alone = 0; alone < (int)N; alone++) run<S>(table, units, cap, 2, alone);
}

int main(int argc, char** argv) {
  if (argc > 1 && std::strcmp(argv[1], "--print") == 0) {
    for (const ResultArray& a : kFrustumArrays)
      std::printf("frustum %s %zu %zu %d %zu %d %d\n", a.name, a.offset, a.elem, a.unit, a.tail, a.per_cap ? 1 : 0, a.required ? 1 : 0);
    for (const ResultArray& a : kClaimArrays)
      std::printf("claim %s %zu %zu %d %zu %d %d\n", a.name, a.offset, a.elem, a.unit, a.tail, a.per_cap ? 1 : 0, a.required ? 1 : 0);
    return 0;
  }
  const size_t sizes[][4] = {{0, 0, 1, 0}, {1, 1, 1, 1}, {65, 3, 7, 30}, {900, 8, 257, 2206}};   // points, key frames, cap, corr_cap
  for (const auto& s : sizes) {
    const size_t f_units[kTrUnits] = {1, s[0], s[1]}, c_units[kClUnits] = {1, s[1], s[3]};
    sweep<msf_frustum_result>(kFrustumArrays, f_units, 1);
    sweep<msf_claim_result>(kClaimArrays, c_units, s[2]);
  }
  std::printf("%d tables x sizes x wanted sets: %s\n", 2, bad ? "BAD" : "ok");
  return bad ? 1 : 0;
}
