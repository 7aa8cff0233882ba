// Owning device allocation: a pointer and its size in bytes; reads as the pointer, freed with its owner.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>

namespace msf {

template <class T>
struct DevBuf {
  T* p = nullptr;
  size_t bytes = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  operator T*() const { return p; }
  void release() {
    if (p) hipFree(p);   // waits for the device: no earlier call still uses the block
    p = nullptr;
    bytes = 0;
  }
  // Drops the old block, then allocates max(want, floor) bytes; empty after a failure.
  hipError_t reserve(size_t want, size_t floor = 0) {
    release();
    const size_t n = want > floor ? want : floor;
    const hipError_t e = hipMalloc(&p, n);
    if (e != hipSuccess) p = nullptr; else bytes = n;
    return e;
  }
};

}  // namespace msf
