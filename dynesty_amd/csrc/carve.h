// Internal: the walk over a layout.  A layout is THE list of one scratch user's arrays -- element type, element count,
// wanted or not --, written once as a function of a Carver and walked twice: first without a base for the total, then
// with the block for the addresses (arena_carve of ctx.h, device_carve of merge_dev.h).  The layouts themselves live in
// merge_plan.h (the combiner) and stage_plan.h (the host-pointer entry points).  Plain C++17: no HIP include.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace dh_carve {

// One array of a walk, for the host test.
struct Slot {
  const char* name;
  size_t off, bytes;  // bytes == 0: not wanted -- no room, a null pointer
  bool null;
};

// Hands out consecutive 256-byte aligned arrays of a block; without a base it only adds up.
struct Carver {
  char* base = nullptr;
  size_t off = 0;
  Slot* log = nullptr;  // where the host test has the walk written down
  int nlog = 0;
  template <class T>
  void operator()(T*& p, const char* name, size_t count, bool wanted = true) {
    p = nullptr;
    const size_t bytes = wanted ? count * sizeof(T) : 0;
    if (wanted && base) p = (T*)(base + off);
    if (log) log[nlog++] = Slot{name, off, bytes, p == nullptr};
    off += (bytes + 255) & ~(size_t)255;
  }
};

}  // namespace dh_carve
