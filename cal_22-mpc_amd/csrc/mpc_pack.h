// mpc_pack.h -- the accounting pass that sums per-line sizes over blocks of N consecutive lines and rounds each block
// up to whole sectors once (mpc_pack.hip), next to the size histograms of mpc_sizes.h and the class tables of
// mpc_classes.h.  It reads only what the evaluators wrote: 2 bytes per line and member.
//
// Input: m device arrays of n uint16 sizes, one per member (as MpcSizesArgs has them); the launch's first line is line
// `pos` of its block (0 <= pos < N).  Block j of the launch is lines [j N - pos, (j + 1) N - pos) cut to [0, n).
//
//   block 0, when pos > 0            begins with *carry_in[i], the payload of the lines of that block in earlier launches
//   the last block, when it is open  ((pos + n) % N != 0): its payload so far goes to *carry_out[i]; nothing else is counted
//   every other block is closed      T = table[i]: T[0] += payload, T[sectors(payload + header_bits)] += 1
//   with best != null                the same with b = min_i size_i per line over all m members and best_header_bits
//
//   sectors(bits) = min(max(1, ceil(bits / sector_bits)), max_sectors)
//
// carry_in[i] and carry_out[i] are different words (the caller double-buffers them): the lane that closes block 0 and
// the one that leaves the last block open do not wait for each other.  Launches of one table that touch a carry must
// not overlap; the caller chains them.
//
// The device table is uint64 [MPC_PACK_DEV_LEN]: [0] the payload bits of the closed blocks, [k] the closed blocks that
// occupy k sectors, k = 1 .. max_sectors.  The number of closed blocks and of their sectors follow from the
// histogram.  All plain uint64 sums (device-scope atomic adds), so shards add.
//
// A block's bits are summed in 32 bits: N <= MPC_PACK_MAX_BLOCK_LINES keeps 4095 N + 65535 + 3 N below 2^32 (no
// evaluator writes a size above 4095 bits, mpc_sizes.h; 3: the tag bits of a best-of of 8).
#pragma once
#include <stdint.h>

#include "mpc_sizes.h"

#define MPC_PACK_MAX_SECTORS 1024
#define MPC_PACK_DEV_LEN (1 + MPC_PACK_MAX_SECTORS)
#define MPC_PACK_MAX_BLOCK_LINES (1ull << 19)
#define MPC_PACK_LANE_MAX 32u                    /* N up to here: a lane owns whole blocks                       */
#define MPC_PACK_WAVE_MAX 511u                   /* ... up to here: a wave strides a block; above: a workgroup   */

struct MpcPackArgs {
  const uint16_t *sizes[MPC_SIZES_MAX];          // [m] device (or device-visible) arrays of n sizes
  unsigned long long *table[MPC_SIZES_MAX];      // [m] per member [MPC_PACK_DEV_LEN], null: no table for this member
  const uint32_t *carry_in[MPC_SIZES_MAX];       // [m] read when pos > 0 (null with a null table)
  uint32_t *carry_out[MPC_SIZES_MAX];            // [m] written when the launch ends inside a block
  unsigned long long *best;                      // [MPC_PACK_DEV_LEN], null: no table of the per-line minimum (else over all m members, m >= 2)
  const uint32_t *best_carry_in;
  uint32_t *best_carry_out;
  unsigned long long block_lines;                // N, 1 .. MPC_PACK_MAX_BLOCK_LINES
  unsigned long long pos;                        // < N
  int m;                                         // 1 .. MPC_SIZES_MAX
  unsigned sector_bits;                          // 8 * sector_bytes, > 0
  unsigned max_sectors;                          // S_B, 1 .. MPC_PACK_MAX_SECTORS
  unsigned header_bits, best_header_bits;
};
