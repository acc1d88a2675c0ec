// host_copies.h -- the device-free side of the handle's derived row copies (squared norms, bf16, int8 groups, u8, u6, u42
// planes): which rows one copy covers, what each mutation does to that coverage, and whether its allocations may stay.  The
// copies themselves -- buffers, quantiser launches, validity flags -- are described once each in host_index.h (DERIVED_COPIES).
// Included by wdbx_hip.hip and, on its own, by tests/host_harness/copies_harness.cpp (plain g++ in the CPU suite,
// tests/test_copies_host.py).  No HIP, no kernel types in here.
#pragma once

#include <algorithm>
#include <cstdint>

struct RowRange {
  uint64_t first = 0, end = 0;  // rows [first, end)
  bool empty() const { return first >= end; }
};

// One copy holds rows [0, rows) of the stored rows; rows behind that are picked up lazily by the next search that reads it.
struct CopyCoverage {
  uint64_t rows = 0;
  uint64_t no_room_cap = ~0ull;  // the capacity at which the copy's allocation was last refused
  uint32_t granule = 1;          // rows whose images depend on each other (64: an int8 group's scale is that of all its rows)
  bool remembers = true;         // false: a refusal is not remembered, every call tries again (the bf16 copy)

  // the part of the overwritten rows [first, end) the copy holds: what a write has to refresh in place (empty: nothing)
  RowRange overlap(uint64_t first, uint64_t end) const {
    const uint64_t e = std::min(end, rows);
    return first < e ? RowRange{first, e} : RowRange{};
  }
  // a compaction moved every row from first_moved on: the copy stays valid below it, in whole granules
  void cut(uint64_t first_moved) { rows = std::min(rows, first_moved / granule * granule); }
  void reset() { rows = 0; }
  void extended_to(uint64_t n) { rows = n; }
  bool covers(uint64_t n) const { return rows >= n; }
  bool refused_at(uint64_t cap) const { return remembers && no_room_cap == cap; }
  void refuse_at(uint64_t cap) {
    if (remembers) no_room_cap = cap;
  }
};

// May a copy's allocations stay?  SHADOW_KEPT: the shape is the same and every part is large enough.  Else SHADOW_FRESH:
// release the parts, restart the coverage at 0 and allocate anew -- unless that was refused at this very capacity before
// (refused_here = CopyCoverage::refused_at): SHADOW_NO_ROOM (= 0), the caller stays on its other paths.
enum { SHADOW_NO_ROOM = 0, SHADOW_KEPT = 1, SHADOW_FRESH = 2 };
static inline int copy_room_decision(bool shape_changed, bool part_too_small, bool refused_here) {
  if (!shape_changed && !part_too_small) return SHADOW_KEPT;
  return refused_here ? SHADOW_NO_ROOM : SHADOW_FRESH;
}
