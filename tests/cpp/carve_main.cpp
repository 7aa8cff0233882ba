// csrc/carve.h in a stand-alone sanitized executable (tests/test_carve_host.py): one layout with pieces of 0, 1, 255,
// 256 and 257 bytes, a given pointer, a piece under a false condition and two typed pieces.  The measuring pass sizes a
// malloc block of exactly that many bytes; every piece of the placing pass is then written in full, so ASan sees an
// overrun of the block, and the checks below see pieces that overlap, are out of order or leave the 256-byte grid.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "carve.h"

namespace {

struct Pair16 {
  double a, b;
};
static_assert(sizeof(Pair16) == 16, "a 16-byte struct");

struct Plan {
  uint8_t* b0 = nullptr, *b1 = nullptr, *b255 = nullptr, *b256 = nullptr, *b257 = nullptr;
  float* given = nullptr;
  int32_t* absent = nullptr;
  double* d = nullptr;
  Pair16* s = nullptr;
  size_t after_b0 = 0, after_given = 0, after_absent = 0;   // the offset after the pieces that must take no room
};

constexpr size_t kDoubles = 33, kStructs = 17;   // 264 and 272 bytes: each rounds up to 512

void layout(msf::Carver& c, float* user, bool wanted, Plan* p) {
  p->b0 = c.take<uint8_t>(0);
  p->after_b0 = c.off;
  p->b1 = c.take<uint8_t>(1);
  p->b255 = c.take<uint8_t>(255);
  p->given = c.take(user, 1000);
  p->after_given = c.off;
  p->b256 = c.take<uint8_t>(256);
  p->absent = wanted ? c.take<int32_t>(100) : nullptr;
  p->after_absent = c.off;
  p->b257 = c.take<uint8_t>(257);
  p->d = c.take<double>(kDoubles);
  p->s = c.take<Pair16>(kStructs);
}

int failures = 0;

#define CHECK(cond)                                               \
  do {                                                            \
    if (!(cond)) {                                                \
      std::printf("line %d: %s does not hold\n", __LINE__, #cond); \
      failures++;                                                 \
    }                                                             \
  } while (0)

}  // namespace

int main() {
  float user[4] = {1.0f, 2.0f, 3.0f, 4.0f};

  msf::Carver measure;
  Plan m;
  layout(measure, user, false, &m);
  CHECK(measure.base == nullptr);
  CHECK(m.given == user);
  CHECK(m.after_b0 == 0);                      // the zero-byte piece
  CHECK(m.after_given == 512);                 // 1 and 255 bytes before it, nothing for the given pointer
  CHECK(m.after_absent == 768);                // 256 bytes after it, nothing for the piece that is not wanted
  CHECK(measure.off == 768 + 512 + 512 + 512); // 257 bytes, 33 doubles and 17 structs round up to 512 each

  const size_t total = measure.off;
  uint8_t* block = static_cast<uint8_t*>(std::malloc(total));
  if (!block) return 2;
  msf::Carver place{block};
  Plan p;
  layout(place, user, false, &p);
  CHECK(place.off == total);                   // the two passes end at the same offset
  CHECK(p.after_b0 == m.after_b0 && p.after_given == m.after_given && p.after_absent == m.after_absent);
  CHECK(p.given == user);                      // unchanged, and still the caller's values after the writes below
  CHECK(p.absent == nullptr);

  // every piece written in full
  std::memset(p.b1, 0x11, 1);
  std::memset(p.b255, 0x22, 255);
  std::memset(p.b256, 0x33, 256);
  std::memset(p.b257, 0x44, 257);
  for (size_t i = 0; i < kDoubles; i++) p.d[i] = (double)i;
  for (size_t i = 0; i < kStructs; i++) p.s[i] = Pair16{(double)i, -(double)i};
  CHECK(user[0] == 1.0f && user[3] == 4.0f);

  // on the 256-byte grid, in order and disjoint: each piece starts where the one before it ends, rounded up
  struct Piece {
    const void* at;
    size_t bytes;
  };
  const Piece pieces[] = {{p.b1, 1}, {p.b255, 255}, {p.b256, 256}, {p.b257, 257}, {p.d, kDoubles * sizeof(double)},
                          {p.s, kStructs * sizeof(Pair16)}};
  size_t expect = 0;
  for (const Piece& q : pieces) {
    const size_t at = (size_t)(static_cast<const uint8_t*>(q.at) - block);
    CHECK(at % 256 == 0);
    CHECK(at == expect);
    CHECK(at + q.bytes <= total);
    expect = at + ((q.bytes + 255) & ~(size_t)255);
  }
  CHECK(expect == total);
  CHECK(p.b0 == block);                        // the zero-byte piece sits where the next one starts

  // the writes did not run into one another
  CHECK(p.b1[0] == 0x11 && p.b255[0] == 0x22 && p.b255[254] == 0x22 && p.b256[255] == 0x33 && p.b257[256] == 0x44);
  CHECK(p.d[kDoubles - 1] == (double)(kDoubles - 1) && p.s[0].a == 0.0 && p.s[kStructs - 1].b == -(double)(kStructs - 1));

  // the same layout with the condition true and no given pointer: both pieces now take room, in both passes alike
  msf::Carver measure2;
  Plan m2;
  layout(measure2, nullptr, true, &m2);
  CHECK(measure2.off == total + 4096 + 512);   // 1000 floats = 4000 bytes -> 4096; 100 int32 = 400 bytes -> 512
  uint8_t* block2 = static_cast<uint8_t*>(std::malloc(measure2.off));
  if (!block2) return 2;
  msf::Carver place2{block2};
  Plan p2;
  layout(place2, nullptr, true, &p2);
  CHECK(place2.off == measure2.off);
  CHECK((uint8_t*)p2.given == block2 + 512 && (uint8_t*)p2.absent == block2 + 512 + 4096 + 256);
  for (size_t i = 0; i < 1000; i++) p2.given[i] = 1.0f;
  for (size_t i = 0; i < 100; i++) p2.absent[i] = -1;
  std::memset(p2.b256, 0x33, 256);
  std::memset(p2.b257, 0x44, 257);
  for (size_t i = 0; i < kStructs; i++) p2.s[i] = Pair16{1.0, 2.0};
  CHECK(p2.given[999] == 1.0f && p2.b256[0] == 0x33 && p2.absent[0] == -1 && p2.absent[99] == -1 && p2.b257[0] == 0x44);
  CHECK((uint8_t*)(p2.s + kStructs) <= block2 + measure2.off);

  std::free(block2);
  std::free(block);
  std::printf("carve: %d failure(s), %zu and %zu bytes\n", failures, total, measure2.off);
  return failures ? 1 : 0;
}
