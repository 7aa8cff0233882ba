// Stand-alone program (its own main; built with -fsanitize=address,undefined by tests/test_frame_tracking_arrays_host.py
// and run as an executable): the table of msfx_track_result (csrc/frame_tracking_arrays.h) through carve_result() and
// copy_result() of result_arrays.h, as the entry points of msf_frame_tracking.h use them.  Over calls of several sizes
// (0 included), the wanted sets none / all / alone / alternating, and both forms of the carve -- the host call's (every
// array gets a piece: each is read by a later launch or by `keep`) and the device call's (the caller's pointer where
// there is one): every piece lies on the 256-byte grid, has the documented size and overlaps no other, and the copy-back
// moves every byte of a wanted array and nothing else.  `--print`: the table, one row per line, for the comparison with
// _lib.TRACK_ARRAYS.  Exit status 0: every case held.
#include <cstdio>
#include <cstring>
#include <vector>

#include "frame_tracking_arrays.h"

using namespace msf;

static int bad = 0;
static void check(bool ok, const char* what, const char* name) {
  if (!ok) std::printf("BAD %s (%s)\n", what, name), bad++;
}

template <size_t N>
static void run(const ResultArray (&table)[N], const size_t* units, int pattern, int alone, bool device_form) {
  std::vector<std::vector<uint8_t>> host(N);
  msfx_track_result out{};
  out.struct_size = sizeof out;
  for (size_t i = 0; i < N; i++) {
    const bool want = pattern == 1 || (pattern == 2 && (int)i == alone) || (pattern == 3 && i % 2 == 0);
    const size_t bytes = array_bytes(table[i], units, 1);
    if (!want || !bytes) continue;
    host[i].assign(bytes, 0xCD);
    set_slot(&out, table[i], host[i].data());
  }
  Carver measure;
  msfx_track_result dev{};
  carve_result(measure, table, units, 1, device_form ? &out : nullptr, out, &dev);
  std::vector<uint8_t> block(measure.off + 1, 0);
  Carver place{block.data()};
  carve_result(place, table, units, 1, device_form ? &out : nullptr, out, &dev);
  check(place.off == measure.off, "the two passes disagree", "layout");
  size_t expect = 0;
  for (size_t i = 0; i < N; i++) {
    const ResultArray& a = table[i];
    const size_t bytes = array_bytes(a, units, 1);
    uint8_t* p = slot(dev, a);
    check(a.required, "every array of this family is required", a.name);
    if (device_form && slot(out, a)) {
      check(p == slot(out, a), "the caller's array was not used", a.name);
      continue;
    }
    check(p == block.data() + expect, "piece not where the sizes before it put it", a.name);
    check((size_t)(p - block.data()) % 256 == 0, "piece off the 256-byte grid", a.name);
    expect += (bytes + 255) & ~(size_t)255;
    std::memset(p, (int)(i + 1), bytes);   // what the kernels would write: the sanitizer guards the block's end
  }
  check(expect == measure.off, "the pieces do not add up", "layout");
  if (device_form) return;
  const Extent all{0, 1, 1, 1, units, units};
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

int main(int argc, char** argv) {
  if (argc > 1 && std::strcmp(argv[1], "--print") == 0) {
    for (const ResultArray& a : kTrackArrays)
      std::printf("track %s %zu %zu %d %zu %d %d\n", a.name, a.offset, a.elem, a.unit, a.tail, a.per_cap ? 1 : 0, a.required ? 1 : 0);
    return 0;
  }
  constexpr int N = (int)(sizeof kTrackArrays / sizeof kTrackArrays[0]);
  const size_t sizes[][3] = {{1, 0, 0}, {1, 0, 1}, {7, 3, 10}, {330, 150, 480}, {4096, 0, 4096}};   // cap, n_cur, corr_cap
  for (const auto& s : sizes) {
    const size_t units[kFtUnits] = {1, s[0], s[1], s[2]};
    for (bool device_form : {false, true}) {
      for (int pattern : {0, 1, 3}) run(kTrackArrays, units, pattern, -1, device_form);
      for (int alone = 0; alone < N; alone++) run(kTrackArrays, units, 2, alone, device_form);
    }
  }
  std::printf("1 table x sizes x wanted sets x 2 forms: %s\n", bad ? "BAD" : "ok");
  return bad ? 1 : 0;
}
