// csrc/result_arrays.h in a stand-alone sanitized executable (tests/test_result_arrays_host.py).  For each of the four
// tables, over lists {1, 3}, cap {1, 5}, the smallest unit counts and the wanted sets none / all / each array alone /
// alternating: carve_result() is measured on a null base, placed in a malloc block of exactly that many bytes and every
// piece written in full, so ASan sees a piece the measuring pass did not count; copy_result() then runs with memcpy into
// host arrays malloc'd at exactly their documented size and filled with a canary, so ASan sees an overrun and the checks
// see a byte that moved beyond the extent asked for.  `--print` lists the tables for the comparison with _lib.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "result_arrays.h"

namespace {

int failures = 0;

#define CHECK(cond)                                                              \
  do {                                                                           \
    if (!(cond)) {                                                               \
      if (failures < 40) std::printf("line %d (%s): %s does not hold\n", __LINE__, g_case, #cond); \
      failures++;                                                                \
    }                                                                            \
  } while (0)

char g_case[160] = "";
constexpr uint8_t kCanary = 0xEE;
uint8_t g_marker[64];   // addresses that stand for "the caller has an array here"

size_t round256(size_t b) { return (b + 255) & ~(size_t)255; }

// the documented size, worked out here from the row alone
size_t documented_bytes(const msf::ResultArray& a, size_t lists, const size_t* units, size_t cap) {
  return lists * (a.unit == 0 ? 1 : units[a.unit]) * a.tail * (a.per_cap ? cap : 1) * a.elem;
}

uint8_t device_byte(size_t array, size_t at) { return (uint8_t)((array * 31 + at * 7 + 1) & 0x7F); }   // never the canary

// which arrays of a table of N rows the caller asks for: none, all, one alone, every other one
struct Wanted {
  enum Kind { kNone, kAll, kOne, kEven, kOdd } kind;
  size_t one;
  bool has(size_t i) const {
    return kind == kAll || (kind == kOne && i == one) || (kind == kEven && i % 2 == 0) || (kind == kOdd && i % 2 == 1);
  }
};

std::vector<Wanted> wanted_sets(size_t n) {
  std::vector<Wanted> w = {{Wanted::kNone, 0}, {Wanted::kAll, 0}, {Wanted::kEven, 0}, {Wanted::kOdd, 0}};
  for (size_t i = 0; i < n; i++) w.push_back({Wanted::kOne, i});
  return w;
}

template <class S, size_t N>
void check_carve(const msf::ResultArray (&table)[N], const size_t* units, size_t cap, const Wanted& want) {
  const size_t lists = units[0];
  S wanted{};
  for (size_t i = 0; i < N; i++)
    if (want.has(i)) msf::set_slot(&wanted, table[i], g_marker + i);

  // the host call: a piece iff required or wanted
  msf::Carver measure;
  S none{};
  msf::carve_result(measure, table, units, cap, nullptr, wanted, &none);
  const size_t total = measure.off;
  CHECK(total > 0);   // every table has a required array
  uint8_t* block = static_cast<uint8_t*>(std::malloc(total));
  if (!block) std::exit(2);
  msf::Carver place{block};
  S dev{};
  msf::carve_result(place, table, units, cap, nullptr, wanted, &dev);
  CHECK(place.off == total);
  size_t expect = 0;
  for (size_t i = 0; i < N; i++) {
    uint8_t* p = msf::slot(dev, table[i]);
    const size_t bytes = documented_bytes(table[i], lists, units, cap);
    CHECK(msf::array_bytes(table[i], units, cap) == bytes);
    if (!(table[i].required || want.has(i))) {
      CHECK(p == nullptr);
      continue;
    }
    CHECK(p != nullptr);
    if (!p) continue;
    const size_t at = (size_t)(p - block);
    CHECK(at % 256 == 0);
    CHECK(at == expect);   // in order, disjoint, and exactly `bytes` rounded up to the grid apart
    CHECK(at + bytes <= total);
    std::memset(p, (int)(i + 1), bytes);   // in full: ASan sees a piece that the measuring pass did not count
    expect = at + round256(bytes);
  }
  CHECK(expect == total);
  for (size_t i = 0; i < N; i++)
    if (uint8_t* p = msf::slot(dev, table[i])) {
      const size_t bytes = documented_bytes(table[i], lists, units, cap);
      CHECK(p[0] == (uint8_t)(i + 1) && p[bytes - 1] == (uint8_t)(i + 1));   // the writes did not run into one another
    }
  std::free(block);

  // the device call: `wanted` now stands for the caller's device arrays
  msf::Carver measure2;
  msf::carve_result(measure2, table, units, cap, &wanted, wanted, &none);
  size_t room = 0;
  for (size_t i = 0; i < N; i++)
    if (table[i].required && !want.has(i)) room += round256(documented_bytes(table[i], lists, units, cap));
  CHECK(measure2.off == room);   // only what is required and missing takes room
  uint8_t* block2 = static_cast<uint8_t*>(std::malloc(room ? room : 1));
  if (!block2) std::exit(2);
  msf::Carver place2{block2};
  S dev2{};
  msf::carve_result(place2, table, units, cap, &wanted, wanted, &dev2);
  CHECK(place2.off == room);
  for (size_t i = 0; i < N; i++) {
    uint8_t* p = msf::slot(dev2, table[i]);
    if (want.has(i)) {
      CHECK(p == g_marker + i);   // the caller's pointer, untouched
    } else if (table[i].required) {
      CHECK(p >= block2 && p + documented_bytes(table[i], lists, units, cap) <= block2 + room);
      if (p) std::memset(p, 0x55, documented_bytes(table[i], lists, units, cap));
    } else {
      CHECK(p == nullptr);
    }
  }
  std::free(block2);
}

// One copy_result() of list `list` out of units[0]: n entries of every per-cap row, rows[k] rows of unit k.
template <class S, size_t N>
void check_copy(const msf::ResultArray (&table)[N], const size_t* units, size_t dcap, size_t hcap, size_t n,
                const size_t* rows, size_t list, const Wanted& want) {
  const size_t lists = units[0];
  S dev{}, out{};
  std::vector<uint8_t*> d(N, nullptr), h(N, nullptr);
  for (size_t i = 0; i < N; i++) {
    const size_t db = documented_bytes(table[i], lists, units, dcap), hb = documented_bytes(table[i], lists, units, hcap);
    d[i] = static_cast<uint8_t*>(std::malloc(db));
    if (!d[i]) std::exit(2);
    for (size_t b = 0; b < db; b++) d[i][b] = device_byte(i, b);
    msf::set_slot(&dev, table[i], d[i]);
    if (!want.has(i)) continue;
    h[i] = static_cast<uint8_t*>(std::malloc(hb));   // exactly the documented size
    if (!h[i]) std::exit(2);
    std::memset(h[i], kCanary, hb);
    msf::set_slot(&out, table[i], h[i]);
  }
  size_t copies = 0;
  const msf::Extent e{list, dcap, hcap, n, units, rows};
  const int rc = msf::copy_result(table, dev, out, e, [&](void* dst, const void* src, size_t bytes) {
    CHECK(bytes > 0);
    std::memcpy(dst, src, bytes);
    copies++;
    return 0;
  });
  CHECK(rc == 0);
  size_t most = 0;   // copies when no run of rows can be merged
  for (size_t i = 0; i < N; i++) {
    if (!h[i]) continue;
    const msf::ResultArray& a = table[i];
    const size_t per = a.unit == 0 ? 1 : units[a.unit], el = a.tail * a.elem;
    const size_t drow = el * (a.per_cap ? dcap : 1), hrow = el * (a.per_cap ? hcap : 1), w = el * (a.per_cap ? n : 1);
    const size_t hb = documented_bytes(a, lists, units, hcap);
    if (w) most += a.per_cap && !(n == dcap && n == hcap) ? rows[a.unit] : (rows[a.unit] ? 1 : 0);
    for (size_t b = 0; b < hb; b++) {
      const size_t row = b / hrow, in_row = b % hrow;
      const bool moved = row / per == list && row % per < rows[a.unit] && in_row < w;
      const uint8_t expect = moved ? device_byte(i, row * drow + in_row) : kCanary;
      if (h[i][b] != expect) {
        CHECK(h[i][b] == expect);
        break;
      }
    }
  }
  CHECK(copies == most);   // full rows and rows that do not run along the list: one copy per array
  for (size_t i = 0; i < N; i++) {
    std::free(d[i]);
    std::free(h[i]);
  }
}

template <class S, size_t N>
void run_table(const char* name, const msf::ResultArray (&table)[N], size_t n_units, size_t u1, size_t u2) {
  const std::vector<Wanted> sets = wanted_sets(N);
  for (size_t lists : {(size_t)1, (size_t)3})
    for (size_t cap : {(size_t)1, (size_t)5}) {
      const size_t units[3] = {lists, u1, u2};
      for (size_t s = 0; s < sets.size(); s++) {
        std::snprintf(g_case, sizeof g_case, "%s lists %zu cap %zu units %zu %zu wanted %d/%zu", name, lists, cap, u1, u2,
                      (int)sets[s].kind, sets[s].one);
        check_carve<S>(table, units, cap, sets[s]);
      }
      // copy-back of the last list: full rows, short rows, another stride on the device, no records, an empty list
      const size_t full[3] = {1, u1, u2}, no_rows[3] = {1, n_units > 1 ? u1 : 0, 0}, fewer[3] = {1, u1, u2 - (u2 > 1)};
      for (const Wanted& want : {Wanted{Wanted::kAll, 0}, Wanted{Wanted::kEven, 0}, Wanted{Wanted::kOdd, 0}}) {
        std::snprintf(g_case, sizeof g_case, "%s copy lists %zu cap %zu units %zu %zu wanted %d", name, lists, cap, u1, u2,
                      (int)want.kind);
        check_copy<S>(table, units, cap, cap, cap, full, lists - 1, want);
        check_copy<S>(table, units, cap, cap, cap - 1, full, lists - 1, want);       // n < cap (n = 0 when cap = 1)
        check_copy<S>(table, units, cap + 2, cap, cap, full, lists - 1, want);       // dcap != hcap, the host rows full
        check_copy<S>(table, units, cap + 2, cap, cap / 2, fewer, 0, want);          // dcap != hcap, short rows
        check_copy<S>(table, units, cap, cap + 3, cap, full, lists / 2, want);       // the host rows wider
        check_copy<S>(table, units, cap, cap, cap, no_rows, lists - 1, want);        // zero records
        check_copy<S>(table, units, cap, cap, 0, full, 0, want);                     // n = 0
      }
    }
}

template <size_t N>
void print_table(const char* name, const msf::ResultArray (&table)[N]) {
  for (const msf::ResultArray& a : table)
    std::printf("%s %s %zu %zu %d %zu %d %d\n", name, a.name, a.offset, a.elem, a.unit, a.tail, (int)a.per_cap,
                (int)a.required);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc > 1 && std::strcmp(argv[1], "--print") == 0) {   // table, name, offset, elem, unit, tail, per_cap, required
    print_table("pnp", msf::kPnpArrays);
    print_table("pose", msf::kPoseArrays);
    print_table("motion", msf::kMotionArrays);
    print_table("new_points", msf::kNewPointsArrays);
    return 0;
  }
  for (size_t its : {(size_t)1, (size_t)3})
    for (size_t recs : {(size_t)1, (size_t)2}) run_table<msf_pnp_result>("pnp", msf::kPnpArrays, 3, its, recs);
  run_table<msf_pose_result>("pose", msf::kPoseArrays, 3, msf::kPoseRounds, msf::kPoseIterations);
  run_table<msf_motion_result>("motion", msf::kMotionArrays, 1, 0, 0);
  run_table<msf_new_points_result>("new_points", msf::kNewPointsArrays, 1, 0, 0);
  std::printf("result_arrays: %d failure(s)\n", failures);
  return failures ? 1 : 0;
}
