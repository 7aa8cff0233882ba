// csrc/hip_device_block.h in a stand-alone sanitized executable (tests/test_device_block_host.py), against the host
// stand-in for the HIP runtime API of tests/cpp/hip_host: "device" memory is malloc memory of exactly the size asked
// for, so a piece the measuring pass did not count, or a copy past either block, is an overrun that AddressSanitizer
// reports, and a block that is not freed is a leak that LeakSanitizer reports.  One layout of mixed types with pieces
// of 0, 1, 255, 256 and 257 bytes among the inputs and the outputs.
#include <cstdio>
#include <cstring>
#include <vector>

#include "hip_device_block.h"

namespace {

struct Pair16 {
  double a, b;
};

struct View {
  uint8_t* in1;     // 1 byte; the first piece: the base of its side
  double* in_d;     // 33 doubles = 264 bytes -> 512
  uint8_t* in0;     // 0 bytes: no room
  uint8_t* in255;
  size_t inputs_end;
  uint8_t* out256;
  int32_t* out_i;   // 100 int32 = 400 bytes -> 512
  uint8_t* out0;    // 0 bytes: no room
  uint8_t* out257;  // -> 512
  Pair16* out_s;    // 17 x 16 = 272 bytes -> 512
};

constexpr size_t kDoubles = 33, kInts = 100, kStructs = 17;
constexpr size_t kInputs = 256 + 512 + 0 + 256, kTotal = kInputs + 256 + 512 + 0 + 512 + 512;

View layout(msf::Carver& c) {
  View v;
  v.in1 = c.take<uint8_t>(1);
  v.in_d = c.take<double>(kDoubles);
  v.in0 = c.take<uint8_t>(0);
  v.in255 = c.take<uint8_t>(255);
  v.inputs_end = c.off;
  v.out256 = c.take<uint8_t>(256);
  v.out_i = c.take<int32_t>(kInts);
  v.out0 = c.take<uint8_t>(0);
  v.out257 = c.take<uint8_t>(257);
  v.out_s = c.take<Pair16>(kStructs);
  return v;
}

struct Nothing {
  size_t inputs_end;
};

Nothing empty_layout(msf::Carver& c) { return Nothing{c.off}; }

int failures = 0;

#define CHECK(cond)                                               \
  do {                                                            \
    if (!(cond)) {                                                \
      std::printf("line %d: %s does not hold\n", __LINE__, #cond); \
      failures++;                                                 \
    }                                                             \
  } while (0)

hip_host::State& hip() { return hip_host::state(); }

// the `at`-th call of `kind` from now on fails (0: none does)
void arm(int kind, int at) {
  hip() = hip_host::State{hip().live, {0, 0, 0, 0}, kind, at};
}

size_t offset_of(const void* p, const View& v) { return (size_t)(static_cast<const uint8_t*>(p) - v.in1); }

void fill_inputs(const View& v) {
  v.in1[0] = 0x11;
  for (size_t i = 0; i < kDoubles; i++) v.in_d[i] = 0.5 + (double)i;
  std::memset(v.in255, 0x22, 255);
}

// what the test's "kernel" leaves in the outputs of the device side, every piece in full
void write_outputs(const View& v) {
  std::memset(v.out256, 0x33, 256);
  for (size_t i = 0; i < kInts; i++) v.out_i[i] = -(int32_t)i - 1;
  std::memset(v.out257, 0x44, 257);
  for (size_t i = 0; i < kStructs; i++) v.out_s[i] = Pair16{(double)i, -(double)i};
}

bool outputs_hold_the_pattern(const View& v) {
  bool ok = true;
  for (size_t i = 0; i < 256; i++) ok = ok && v.out256[i] == 0x33;
  for (size_t i = 0; i < kInts; i++) ok = ok && v.out_i[i] == -(int32_t)i - 1;
  for (size_t i = 0; i < 257; i++) ok = ok && v.out257[i] == 0x44;
  for (size_t i = 0; i < kStructs; i++) ok = ok && v.out_s[i].a == (double)i && v.out_s[i].b == -(double)i;
  return ok;
}

void the_layout_and_the_two_copies() {
  msf::Carver measure;
  layout(measure);
  CHECK(measure.off == kTotal);
  {
    msf::DeviceBlock block;
    View dev, host;
    CHECK(block.place(layout, &dev, &host));
    CHECK(hip().live == 1);
    CHECK(block.bytes() == measure.off);   // the total is what the carver measures for the same layout
    CHECK(dev.in1 != host.in1 && dev.inputs_end == kInputs && host.inputs_end == kInputs);

    // the same member is the same offset on the two sides, on the 256-byte grid, in order; 0 bytes take no room
    const void* d[] = {dev.in1, dev.in_d, dev.in0, dev.in255, dev.out256, dev.out_i, dev.out0, dev.out257, dev.out_s};
    const void* h[] = {host.in1, host.in_d, host.in0, host.in255, host.out256, host.out_i, host.out0, host.out257, host.out_s};
    const size_t bytes[] = {1, kDoubles * 8, 0, 255, 256, kInts * 4, 0, 257, kStructs * 16};
    size_t expect = 0;
    for (int k = 0; k < 9; k++) {
      CHECK(offset_of(d[k], dev) == offset_of(h[k], host));
      CHECK(offset_of(h[k], host) % 256 == 0);
      CHECK(offset_of(h[k], host) == expect);
      expect += (bytes[k] + 255) & ~(size_t)255;
    }
    CHECK(expect == kTotal);
    CHECK(host.in0 == host.in255 && host.out0 == host.out257);

    // both blocks arrive zeroed, the device's although its memory did not
    for (size_t i = 0; i < kTotal; i++) CHECK(dev.in1[i] == 0 && host.in1[i] == 0);

    // upload: the device holds the host inputs and zeros elsewhere
    fill_inputs(host);
    std::memset(host.out256, 0x7f, 256);   // an output on the host side: must not travel
    CHECK(block.upload());
    CHECK(std::memcmp(dev.in1, host.in1, kInputs) == 0);
    CHECK(dev.in1[0] == 0x11 && dev.in_d[kDoubles - 1] == 0.5 + (double)(kDoubles - 1) && dev.in255[254] == 0x22);
    for (size_t i = kInputs; i < kTotal; i++) CHECK(dev.in1[i] == 0);

    // the "kernel", then download: the host outputs hold the pattern, the host inputs are as they were
    const std::vector<uint8_t> inputs_before(host.in1, host.in1 + kInputs);
    write_outputs(dev);
    std::memset(dev.in255, 0x55, 255);     // an input on the device side: must not travel back
    CHECK(block.download());
    CHECK(outputs_hold_the_pattern(host));
    CHECK(std::memcmp(host.in1, inputs_before.data(), kInputs) == 0);
    CHECK(std::memcmp(host.in1 + kInputs, dev.in1 + kInputs, kTotal - kInputs) == 0);

    // placing again on the same object frees the first block and starts from zeros
    CHECK(block.place(layout, &dev, &host));
    CHECK(hip().live == 1);
    for (size_t i = 0; i < kTotal; i++) CHECK(dev.in1[i] == 0 && host.in1[i] == 0);
    write_outputs(dev);
    CHECK(block.upload() && block.download() && outputs_hold_the_pattern(host));
  }
  CHECK(hip().live == 0);
}

void a_layout_of_nothing() {
  {
    msf::DeviceBlock block;
    Nothing dev, host;
    CHECK(block.place(empty_layout, &dev, &host));
    CHECK(hip().live == 1 && block.bytes() == 0 && host.inputs_end == 0);   // 256 bytes are allocated all the same
    CHECK(block.upload() && block.download());
  }
  CHECK(hip().live == 0);
}

void every_call_failing_in_turn() {
  for (int kind = 0; kind < hip_host::kCalls; kind++) {
    {
      msf::DeviceBlock block;
      View dev, host;
      arm(kind, 1);
      const bool placed = block.place(layout, &dev, &host);
      CHECK(placed == (kind != hip_host::kMalloc && kind != hip_host::kMemset));
      if (!placed) {
        CHECK(hip().live == 0);                       // nothing is held after a failed place
        CHECK(!block.upload() && !block.download());   // and nothing is copied
        CHECK(block.place(layout, &dev, &host));      // the object can be placed again
        CHECK(hip().live == 1);
      }
      fill_inputs(host);
      const bool up = block.upload();
      CHECK(up == (kind != hip_host::kUpload));
      write_outputs(dev);
      const bool down = block.download();
      CHECK(down == (kind != hip_host::kDownload));
      CHECK(hip().live == 1);                         // a failed copy leaves the block to the destructor
      if (down) CHECK(outputs_hold_the_pattern(host));
    }
    CHECK(hip().live == 0);
  }
  // the second place of one object failing: the first block is gone, none is held
  {
    msf::DeviceBlock block;
    View dev, host;
    arm(hip_host::kMalloc, 2);
    CHECK(block.place(layout, &dev, &host) && hip().live == 1);
    CHECK(!block.place(layout, &dev, &host) && hip().live == 0);
  }
  CHECK(hip().live == 0);
  arm(-1, 0);
}

}  // namespace

int main() {
  the_layout_and_the_two_copies();
  a_layout_of_nothing();
  every_call_failing_in_turn();
  std::printf("device block: %d failure(s), %zu bytes, %zu of them inputs\n", failures, kTotal, kInputs);
  return failures ? 1 : 0;
}
