// mpc_classes.h -- the accounting pass that breaks per-line sizes down by a per-line class byte (mpc_classes.hip): a
// GROUP BY over the 2-byte sizes the evaluator kernels wrote, next to the size histograms of mpc_sizes.h.
//
// Input: n class bytes (or none: every line is class 0) and m device arrays of n uint16 sizes, one per member, as
// MpcSizesArgs has them.
//
//   per member i with table[i] != null   T = table[i] + class * MPC_CLASS_ROW:
//                                        T[0] += 1, T[1] += size (unclipped), T[1 + sectors(size)] += 1 per line
//   with best != null                    the same with b = min_i size_i over all m members (the participation and tie
//                                        rules of the best-of: the caller passes the set; a tie does not change b)
//
//   sectors(size) = min(max(1, ceil(size / (8 * sector_bytes))), S),  S = ceil(L / sector_bytes) <= MPC_CLASS_MAX_SECTORS
//
// which is mpc_size_sectors' formula.  Columns 2 + S .. MPC_CLASS_ROW - 1 of a row stay 0.
//
// The class of line k is classes[k] (uint8), or with class_bias == 1 the byte is a member's int8 `selected` value and
// the class is selected + 1: 0 = uncompressed (-1), k + 1 = cluster k.
//
// All accumulators are plain uint64 sums (device-scope atomic adds), so shards and ranks add.
#pragma once
#include <stdint.h>

#include "mpc_sizes.h"

#define MPC_CLASS_COUNT 256
#ifndef MPC_CLASS_ROW
#define MPC_CLASS_ROW 10
#endif
#define MPC_CLASS_MAX_SECTORS 8                  /* MPC_CLASS_ROW - 2 */
#define MPC_CLASS_TABLE_LEN (MPC_CLASS_COUNT * MPC_CLASS_ROW)

struct MpcClassArgs {
  const uint16_t *sizes[MPC_SIZES_MAX];          // [m] device (or device-visible) arrays of n sizes
  unsigned long long *table[MPC_SIZES_MAX];      // [m] per member [MPC_CLASS_TABLE_LEN], null: no table for this member
  unsigned long long *best;                      // [MPC_CLASS_TABLE_LEN], null: no table of the per-line minimum (else over all m members, m >= 2)
  const uint8_t *classes;                        // [n] device (or device-visible) class bytes, null: class 0 for every line
  int class_bias;                                // 0: uint8 classes; 1: int8 `selected` values, class = value + 1
  int m;                                         // 1 .. MPC_SIZES_MAX
  unsigned sector_bits;                          // 8 * sector_bytes, > 0
  unsigned max_sectors;                          // S, 1 .. MPC_CLASS_MAX_SECTORS
};
