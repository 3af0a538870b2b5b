// mpc_sizes.h -- the accounting pass over per-line sizes (mpc_sizes.hip): a histogram of the sizes per member and,
// for a set of members, the per-line minimum ("best-of").
//
// Input: m device arrays of n uint16 sizes, one per member, as the evaluator kernels wrote them for the same n lines.
//
//   per member i with hist[i] != null   hist[i][min(size, MPC_SIZE_BINS - 1)] += 1 per line
//   with best != null                   b = min_i size_i, winner = the first i (member order) with size_i == b:
//                                       best[min(b, MPC_SIZE_BINS - 1)] += 1, best[MPC_SIZES_WINS + winner] += 1,
//                                       best[MPC_SIZES_BITS] += b (the unclipped size; no tag bits, the host adds them)
//
// Bin MPC_SIZE_BINS - 1 also takes every larger size.  No evaluator reaches it for lines of up to 256 bytes:
//
//   VPC       id bits + 8 L                               <= 2048 + 32 at L = 256 (and every size < hist_bins of its own histogram)
//   BDI       8 L + 4                                     2052 at L = 256
//   FPC       35 bits per 32-bit word (3 prefix + 32)     2240 at L = 256, the largest of all
//   BPC       first word <= 33, 33 planes of <= 32 bits   1089 at any L <= 128; 217 bits at L = 8, more than 8 L: bins are NOT sized by 8 L
//   SC2       33 bits per word                            2112 at L = 256
//   Pattern   smallest scan + 4, at most 8 L + 4          2052 at L = 256
//   C-Pack    34 bits per word (2 prefix + 32)            2176 at L = 256; more than 8 L, like BPC
//
// All accumulators are plain uint64 sums (device-scope atomic adds), so shards and ranks add.
#pragma once
#include <stdint.h>

#ifndef MPC_SIZE_BINS
#define MPC_SIZE_BINS 4096
#endif
#define MPC_SIZES_MAX 8                          /* arrays one launch takes (8 histograms + the best-of one = 144 KiB of LDS) */
#define MPC_SIZES_WINS MPC_SIZE_BINS             /* best[]: [MPC_SIZE_BINS] histogram | [MPC_SIZES_MAX] wins | [1] bits */
#define MPC_SIZES_BITS (MPC_SIZE_BINS + MPC_SIZES_MAX)
#define MPC_SIZES_BEST_LEN (MPC_SIZES_BITS + 1)

struct MpcSizesArgs {
  const uint16_t *sizes[MPC_SIZES_MAX];          // [m] device (or device-visible) arrays of n sizes
  unsigned long long *hist[MPC_SIZES_MAX];       // [m] per member [MPC_SIZE_BINS], null: no histogram for this member
  unsigned long long *best;                      // [MPC_SIZES_BEST_LEN], null: no best-of (else over all m members, m >= 2)
  int m;                                         // 1 .. MPC_SIZES_MAX
};
