// Stand-alone program (its own main; built with -fsanitize=address,undefined by tests/test_ba_arrays_host.py and run
// as an executable): the table of msf_ba_result (csrc/ba_arrays.h) through carve_result() and copy_result() of
// result_arrays.h, as msf_bundle_adjust uses them.  Over problems of several sizes (0 included) and the wanted sets
// none / all / alone / alternating: every piece lies on the 256-byte grid, has the documented size and overlaps no
// other, nothing is carved for what nobody needs, and the copy-back moves every byte of a wanted array and nothing else
// (the caller's arrays are allocated exactly, so a write past one is a heap overflow the sanitizer sees).
// `--print`: the table, one row per line, for the comparison with _lib.BA_ARRAYS.  Exit status 0: every case held.
#include <cstdio>
#include <cstring>
#include <vector>

#include "ba_arrays.h"

using namespace msf;

static int bad = 0;
static void check(bool ok, const char* what, const char* name) {
  if (!ok) std::printf("BAD %s (%s)\n", what, name), bad++;
}

static void run(size_t nc, size_t np, size_t ne, int pattern, int alone) {
  constexpr size_t N = sizeof(kBaArrays) / sizeof(kBaArrays[0]);
  size_t units[kBaUnits];
  ba_units(nc, np, ne, units);
  std::vector<std::vector<uint8_t>> host(N);
  msf_ba_result out{};
  out.struct_size = sizeof out;
  for (size_t i = 0; i < N; i++) {
    const bool want = pattern == 1 || (pattern == 2 && (int)i == alone) || (pattern == 3 && i % 2 == 0);
    const size_t bytes = array_bytes(kBaArrays[i], units, 1);
    if (!want || !bytes) continue;
    host[i].assign(bytes, 0xCD);
    set_slot(&out, kBaArrays[i], host[i].data());
  }
  Carver measure;
  msf_ba_result dev{};
  carve_result(measure, kBaArrays, units, 1, nullptr, out, &dev);
  std::vector<uint8_t> block(measure.off + 1, 0);
  Carver place{block.data()};
  carve_result(place, kBaArrays, units, 1, nullptr, out, &dev);
  check(place.off == measure.off, "the two passes disagree", "layout");
  size_t expect = 0;
  for (size_t i = 0; i < N; i++) {
    const ResultArray& a = kBaArrays[i];
    const size_t bytes = array_bytes(a, units, 1);
    uint8_t* p = slot(dev, a);
    const bool needed = a.required || slot(out, a);
    if (!needed) {
      check(p == nullptr, "a piece nobody needs", a.name);
      continue;
    }
    check(p == block.data() + expect, "piece not where the sizes before it put it", a.name);
    check((size_t)(p - block.data()) % 256 == 0, "piece off the 256-byte grid", a.name);
    expect += (bytes + 255) & ~(size_t)255;
    std::memset(p, (int)(i + 1), bytes);   // what the kernel would write: the sanitizer guards the block's end
  }
  check(expect == measure.off, "the pieces do not add up", "layout");
  const Extent all{0, 1, 1, 1, units, units};
  size_t copies = 0;
  const int rc = copy_result(kBaArrays, dev, out, all, [&](void* dst, const void* src, size_t bytes) {
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
    check(ok, "the copy-back left bytes of a wanted array", kBaArrays[i].name);
  }
  check(copies == wanted, "not one copy per wanted array", "copy");
}

int main(int argc, char** argv) {
  if (argc > 1 && std::strcmp(argv[1], "--print") == 0) {
    for (const ResultArray& a : kBaArrays)
      std::printf("ba %s %zu %zu %d %zu %d %d\n", a.name, a.offset, a.elem, a.unit, a.tail, a.per_cap ? 1 : 0, a.required ? 1 : 0);
    return 0;
  }
  constexpr int N = (int)(sizeof(kBaArrays) / sizeof(kBaArrays[0]));
  const size_t sizes[][3] = {{0, 0, 0}, {1, 1, 1}, {2, 40, 80}, {8, 63, 255}, {66, 5, 0}};
  for (const auto& s : sizes) {
    for (int pattern : {0, 1, 3}) run(s[0], s[1], s[2], pattern, -1);
    for (int alone = 0; alone < N; alone++) run(s[0], s[1], s[2], 2, alone);
  }
  std::printf("%d tables x sizes x wanted sets: %s\n", 1, bad ? "BAD" : "ok");
  return bad ? 1 : 0;
}
