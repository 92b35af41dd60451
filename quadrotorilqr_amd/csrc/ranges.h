// ranges.h -- the two questions every call on the caller's own arrays asks of their addresses before anything is launched: do two byte
// ranges overlap, and does every array start on a 16-byte boundary.  Used by the rules of the seven *_launch.h and by the shift's
// (host/caller_arrays.h); the records those calls share are call_parts.h's.  Host code only; compiles under g++ (the tests' harnesses).
#pragma once

#include <cstddef>
#include <cstdint>
#include <initializer_list>

namespace qilqr {

// [a, a + na) and [b, b + nb) share a byte (a null pointer is no range)
inline bool ranges_overlap(const void *a, size_t na, const void *b, size_t nb) {
  const char *x = (const char *)a, *y = (const char *)b;
  return x && y && x < y + nb && y < x + na;
}

// one of the pointers lies off a 16-byte boundary (a null pointer lies on one)
inline bool off_16_bytes(std::initializer_list<const void *> ps) {
  uintptr_t bits = 0;
  for (const void *p : ps) bits |= (uintptr_t)p;
  return (bits & 15) != 0;
}

}  // namespace qilqr
