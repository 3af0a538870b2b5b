// mpc_pattern.h -- what the host side (mpc_capi.hip: launch_pattern, pattern_status) and the gfx950 kernels of the
// Pattern analyser (mpc_pattern.hip, launchers in mpc_launch.h; reference src/compressor/Pattern.{h,cpp}, LRU.h) share: the raw statistics layout and the
// control block of the distinct-line set.
#pragma once

#include <stdint.h>

/* The reference's LRU holds CACHESIZE = 2^24 - 1 lines before it evicts (LRU.h).  Below that "existed before" means
 * "an equal line came earlier"; eviction is not modelled: the handle accepts this many distinct lines and no more. */
#define MPC_PATTERN_CAPACITY ((1u << 24) - 1u)
/* Open-addressing table: 2^25 slots (load <= 1/2 at the capacity), a 64-bit tag and the whole line per slot:
 * (8 + L) * 2^25 bytes of device memory per handle -- 0.5 GiB for 8-byte lines, 2.25 GiB for 64, 8.25 GiB for 256. */
#define MPC_PATTERN_SLOT_BITS 25

/* Device-side raw statistics (uint64 each, plain sums):
 *   [0] lines  [1] sum of returned sizes  [2] all-zero lines  [3] all-word-same lines (zero lines included)
 *   [4] lines that existed before  [5] lines of no pattern (NotDefined)
 *   [6,12) ImplicitCounts (bytes)  [12,18) ExplicitCounts (bytes)  [18] lines that joined the set
 *   [19, 275)  byte counts of the ordinary lines (neither all-zero nor all-word-same)
 *   [275, 531) per byte value, how often it is one of the four bytes of the word of a NON-ZERO all-word-same line
 *              (such a line holds each of them L/4 times; a zero line holds L zero bytes)                        */
enum {
  MPC_PAT_LINES = 0, MPC_PAT_SIZES, MPC_PAT_ZERO, MPC_PAT_SAME, MPC_PAT_EXISTED, MPC_PAT_UNDEF,
  MPC_PAT_IMPLICIT = 6, MPC_PAT_EXPLICIT = 12, MPC_PAT_JOINED = 18, MPC_PAT_HIST = 19, MPC_PAT_SAME_HIST = 275,
  MPC_PATTERN_RAW_LEN = 531
};

/* Control block of the set (device memory, uint64 each) */
enum {
  MPC_PSET_DISTINCT = 0,   /* lines in the set since creation (kept by mpc_stats_reset)                            */
  MPC_PSET_OVERFLOW,       /* != 0: a line beyond the capacity arrived; the handle is finished                     */
  MPC_PSET_PENDING_A,      /* entries of pending list A (claim pass -> compare pass)                               */
  MPC_PSET_PENDING_B,      /* entries of pending list B (compare pass -> tail)                                     */
  MPC_PSET_WORDS = 8
};

/* Lines of one launch of the set passes (the pending lists hold one 8-byte entry per line) */
#define MPC_PATTERN_CHUNK (1u << 22)

struct MpcPatternSet {
  unsigned long long *tags;    /* [2^MPC_PATTERN_SLOT_BITS]  0 = empty                                              */
  unsigned long long *store;   /* [2^MPC_PATTERN_SLOT_BITS][L / 8]  the line of a claimed slot                      */
  unsigned long long *ctl;     /* [MPC_PSET_WORDS]                                                                */
  uint2 *pend_a, *pend_b;      /* [MPC_PATTERN_CHUNK] each: (line index in the launch, slot)                       */
  unsigned long long tag_mask; /* product: all ones.  Test library: MPC_TEST_PATTERN_TAG_BITS low bits, so that
                                  unequal lines collide on the tag (the slot index is cut the same way)            */
};
