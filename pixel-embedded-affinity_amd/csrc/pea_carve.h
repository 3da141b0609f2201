// pea_carve.h -- the layout of a workspace block, stated once (plain C++, no HIP): saturating arithmetic on byte counts and a cursor that
// hands out the blocks one after the other.  A family writes ONE function over a Carver; with a null base it is the family's
// *_workspace_bytes, with the workspace it fills the launch entry's pointers -- the size and the pointers cannot disagree.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace pea {

// a * b and a + b, UINT64_MAX where they do not fit
inline uint64_t mul_sat(uint64_t a, uint64_t b) {
  uint64_t r;
  return __builtin_mul_overflow(a, b, &r) ? UINT64_MAX : r;
}
inline uint64_t add_sat(uint64_t a, uint64_t b) {
  uint64_t r;
  return __builtin_add_overflow(a, b, &r) ? UINT64_MAX : r;
}
// x rounded up to a multiple of `a` (a power of two), saturating; al8: of 8
inline uint64_t al_sat(uint64_t x, uint64_t a) { return x > UINT64_MAX - (a - 1) ? UINT64_MAX : (x + a - 1) & ~(a - 1); }
inline uint64_t al8(uint64_t x) { return al_sat(x, 8); }

struct Carver {
  char* base;        // may be null: sizes only
  uint64_t off = 0;  // UINT64_MAX once anything saturated
  explicit Carver(void* b) : base((char*)b) {}
  // the next block: `count` elements of T, its bytes rounded up to `align`; nullptr for a null base (or past a saturated offset)
  template <typename T>
  T* take(uint64_t count, uint64_t align = 8) {
    const uint64_t at = off;
    off = add_sat(at, al_sat(mul_sat(count, sizeof(T)), align));
    return base && off != UINT64_MAX ? (T*)(base + at) : nullptr;
  }
  // the total; SIZE_MAX where it does not fit
  size_t bytes() const { return off >= (uint64_t)SIZE_MAX ? SIZE_MAX : (size_t)off; }
};

}  // namespace pea
