// rtg_stage.h — where the parts of a one-shot call lie in its one device
// allocation (one_shot, rtg_entry.h).  A pure function of the sizes: no HIP
// header, so tests/stage_layout.cpp checks it on the CPU.
#pragma once

#include <stddef.h>

namespace rtg {

// Every non-empty part starts on a multiple of this: what a hipMalloc of its
// own would give it, and more than any kernel asks (16 for the 32-byte
// records, 8 for the matte masks).
constexpr size_t kStageAlign = 256;
// The offset of an empty part: it has no place (and a null device pointer).
constexpr size_t kStageAbsent = ~(size_t)0;

// offsets[i] of part i of bytes[i] bytes, in list order; returns the total,
// the end of the last non-empty part (0: nothing to allocate).  No overflow
// test: the callers' checks bound a part by 2^32 - 1 records or 2^48 pixels of
// at most 32 bytes, under 2^53 bytes, and a call has fewer than 16 parts, so
// the sums with their padding stay under 2^58.
inline size_t stage_layout(const size_t* bytes, size_t count, size_t* offsets) {
  size_t end = 0;
  for (size_t i = 0; i < count; ++i) {
    if (!bytes[i]) {
      offsets[i] = kStageAbsent;
      continue;
    }
    offsets[i] = (end + kStageAlign - 1) & ~(kStageAlign - 1);
    end = offsets[i] + bytes[i];
  }
  return end;
}

}  // namespace rtg
