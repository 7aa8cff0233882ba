// Workspace carver: typed pieces of one block, each rounded up to 256 bytes.  A layout is one function of a Carver&
// that fills a plan struct; it runs once on a null base to measure and once on the block to place, so the offsets and
// the pointers cannot disagree.  No HIP in here: any C++17 compiler takes it (tests/cpp/carve_main.cpp).
#pragma once
#include <cstddef>
#include <cstdint>

namespace msf {

struct Carver {
  uint8_t* base = nullptr;   // null: the measuring pass -- only `off` advances, the pointers handed out are not used
  size_t off = 0;            // bytes handed out so far

  // `count` elements of T.  A piece of zero bytes takes no room.
  template <class T>
  T* take(size_t count) {
    const size_t at = off;
    off += (count * sizeof(T) + 255) & ~(size_t)255;
    return base ? reinterpret_cast<T*>(base + at) : nullptr;
  }

  // The caller's array where it gave one -- unchanged, no room taken -- else a piece.
  template <class T>
  T* take(T* given, size_t count) {
    return given ? given : take<T>(count);
  }
};

}  // namespace msf
