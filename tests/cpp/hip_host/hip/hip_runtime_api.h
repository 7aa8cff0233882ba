// Host stand-in for the four HIP runtime calls of csrc/hip_device_block.h, for tests/cpp/device_block_main.cpp only:
// "device" memory is malloc memory.  It counts the live blocks and can make the k-th call of one kind fail.  In a
// directory of its own: on the include path of the adapter-syntax tests it would shadow the real header.
#pragma once
#include <cstdlib>
#include <cstring>

typedef int hipError_t;
enum { hipSuccess = 0, hipErrorOutOfMemory = 2, hipErrorUnknown = 999 };
enum hipMemcpyKind { hipMemcpyHostToDevice = 1, hipMemcpyDeviceToHost = 2 };

namespace hip_host {
enum Call { kMalloc, kMemset, kUpload, kDownload, kCalls };
struct State {
  int live = 0;                    // blocks allocated and not yet freed
  int calls[kCalls] = {0, 0, 0, 0};
  int fail_kind = -1, fail_at = 0;   // the fail_at-th call (from 1) of kind fail_kind returns an error
};
inline State& state() {
  static State s;
  return s;
}
inline bool fails(Call kind) {
  State& s = state();
  return ++s.calls[kind] == s.fail_at && s.fail_kind == kind;
}
}  // namespace hip_host

inline hipError_t hipMalloc(void** p, size_t bytes) {
  if (hip_host::fails(hip_host::kMalloc)) return hipErrorOutOfMemory;
  *p = std::malloc(bytes);
  if (!*p) return hipErrorOutOfMemory;
  std::memset(*p, 0xA5, bytes);   // device memory arrives with anything in it
  hip_host::state().live++;
  return hipSuccess;
}

inline hipError_t hipFree(void* p) {
  if (p) hip_host::state().live--;
  std::free(p);
  return hipSuccess;
}

inline hipError_t hipMemset(void* p, int value, size_t bytes) {
  if (hip_host::fails(hip_host::kMemset)) return hipErrorUnknown;
  std::memset(p, value, bytes);
  return hipSuccess;
}

inline hipError_t hipMemcpy(void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
  if (hip_host::fails(kind == hipMemcpyHostToDevice ? hip_host::kUpload : hip_host::kDownload)) return hipErrorUnknown;
  if (bytes) std::memcpy(dst, src, bytes);
  return hipSuccess;
}
