// mpc_image_probe.h -- the one probe loop of the open-addressing maps keyed by line address: image accounting's
// (mpc_image.hip) and rewrite accounting's (mpc_rewrite.hip).  Device code only; the maps' layout and the hash are in
// mpc_image.h.
#pragma once
#include "mpc_kernel_common.h"
#include "mpc_image.h"

// the slot of `key` in an open-addressing map: found, or claimed (then *claimed).  ~0 when `max_tries` slots in a row
// were taken by other keys, or when a long probe finds *stop set (looked at every 64 slots; null: never).
__device__ __forceinline__ u64 image_slot(u64 *keys, u64 mask, u64 hash_mask, u64 key, u64 max_tries, const u64 *stop, bool *claimed)
{
  u64 slot = mpc_image_mix(key) & hash_mask & mask;
  for (u64 tries = 0; tries < max_tries; tries++, slot = (slot + 1ull) & mask) {
    if (stop && (tries & 63ull) == 63ull && __hip_atomic_load(stop, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0ull) break;
    u64 cur = __hip_atomic_load(&keys[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == kMpcImageEmpty) {
      cur = atomicCAS(&keys[slot], kMpcImageEmpty, key);
      if (cur == kMpcImageEmpty) {
        *claimed = true;
        return slot;
      }
    }
    if (cur == key) return slot;
  }
  return kMpcImageEmpty;
}
