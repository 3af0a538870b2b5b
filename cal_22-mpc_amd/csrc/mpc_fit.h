// mpc_fit.h -- constants of the two Fit analyses (mpc_create_fit_pairs, mpc_create_fit_residues), shared by the kernels
// (mpc_fit.hip) and the host side (mpc_capi.hip).  Plain C: the tests read MPC_FIT_SPILL_LINES from this file.
//
// bitlen8(v): 0 for v = 0, else the position of the highest set bit of v plus 1 (1..8).  Every residue is a uint8
// difference mod 256, as ResidueModule.cpp:34 has it: -1 is 255 and costs 8.
//
// Device raw statistics (uint64 sums; lanes of a wave are neighbours in both):
//   pairs:    [0] lines, then [1 + (i * 8 + (k - 1)) * L + j] = lines with bitlen8((line[i] - line[j]) & 255) == k, k = 1..8.
//             Bin 0 is not counted: it is lines minus the eight others (derive_stats).
//   residues: [0] lines, then [1 + v * L + i] = lines with (line[i] - line[base[i]]) & 255 == v.
#pragma once
#include <stdint.h>

/* Pair kernel: a lane counts a pair's bins 1..8 in eight 7-bit fields of one 64-bit register pair and adds them into the
   workgroup's uint32 table in LDS after this many increments at the latest, before a field can wrap (127 = 2^7 - 1).  A
   wave's unit of work is this many consecutive lines per counter. */
#define MPC_FIT_SPILL_LINES 127
#define MPC_FIT_PAIR_BINS 8        /* counted bins (k = 1..8) */
#define MPC_FIT_PAIR_THREADS 256
#define MPC_FIT_RES_THREADS 1024
/* A launch takes at most this many lines: a workgroup's uint32 LDS counters then stay below 2^32 whatever the grid. */
#define MPC_FIT_LAUNCH_LINES (1ull << 31)

static inline uint64_t mpc_fit_pairs_raw_len(unsigned L) { return 1ull + (uint64_t)MPC_FIT_PAIR_BINS * L * L; }
static inline uint64_t mpc_fit_pairs_stats_len(unsigned L) { return 3ull + 9ull * L * L; }
static inline uint64_t mpc_fit_residues_raw_len(unsigned L) { return 1ull + 256ull * L; }
static inline uint64_t mpc_fit_residues_stats_len(unsigned L) { return 3ull + 256ull * L; }
