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

/* ---- the evicting set (mpc_pattern_evict.hip; mpc_create_pattern_evicting) -------------------------------------------
 * The reference's cache under exist / put is a FIFO over insertions.  Every insertion gets a stamp, the number of
 * insertions before it, and an entry is live while stamp >= insertions - capacity: the stamp is the only liveness
 * test and nothing is ever deleted.  Two generations of the open-addressing table; a slot holds the tag, the stamp of the
 * line's latest insertion (MPC_ESET_NO_STAMP: never inserted), the line's first position in the launch that last touched
 * it, and the line.  Every line a launch touches gets an entry in the newer table (a line found only in the older one
 * brings its stamp along).  At a launch boundary where the insertions since the newer table became the newer one reach
 * the capacity, every entry of the older one is dead: it is cleared and becomes the newer one.  The newer table then
 * holds at most C live lines brought along plus C - 1 + (lines of a launch) insertions; it has the smallest power of two
 * of slots that is >= 1.5 x that, so its load stays below 2/3. */
#define MPC_ESET_NO_STAMP (~0ull)
enum {
  MPC_ESET_INSERTIONS = 0, /* insertions up to the end of the last launch (same word as MPC_PSET_DISTINCT)                */
  MPC_ESET_OVERFLOW = 1,   /* != 0: a probe went round a whole table (unreachable by the sizing above)                   */
  MPC_ESET_PENDING_A = 2, MPC_ESET_PENDING_B = 3,
  MPC_ESET_I0,             /* insertions at the start of the current launch                                            */
  MPC_ESET_I_ROT,          /* insertions when the newer table became the newer one                                     */
  MPC_ESET_NEWER,          /* which of the two tables is the newer one                                                 */
  MPC_ESET_ROTATE,         /* != 0: this launch recycles the older table (decided on the device)                       */
  MPC_ESET_SEQ,            /* launches so far                                                                          */
  MPC_ESET_N_GONE,         /* this launch: first occurrences of gone lines                                             */
  MPC_ESET_N_RISK,         /* this launch: occurrences of at-risk lines                                                */
  /* test library only (-DMPC_TESTING=1; mpc_test_evict_counters): sums over the launches since creation; the product's
   * kernels never touch these words */
  MPC_ESET_T_ROTATIONS,    /* launches that recycled the older table                                                   */
  MPC_ESET_T_GONE,         /* first occurrences of gone lines                                                          */
  MPC_ESET_T_RISK,         /* occurrences of at-risk lines                                                             */
  MPC_ESET_T_RISK_MISS,    /* ... that missed                                                                          */
  MPC_ESET_T_LIST_B,       /* entries put on list B: by the compare pass and, round after round, by the tail            */
  MPC_ESET_WORDS = 16
};

struct MpcEvictTable {
  unsigned long long *tags;    /* [slots]  0 = empty                                                                */
  unsigned long long *stamps;  /* [slots]                                                                           */
  unsigned long long *first;   /* [slots]  (2^40 - 1 - launch number) << 24 | first position: later launches win an atomicMin */
  unsigned long long *store;   /* [slots][L / 8]                                                                    */
};

struct MpcEvictSet {
  MpcEvictTable tab[2];
  unsigned long long *ctl;     /* [MPC_ESET_WORDS]                                                                  */
  uint2 *pend_a, *pend_b;      /* [launch_max] each                                                                 */
  uint32_t *ent;               /* [launch_max]  the slot (newer table) of every line of the launch                  */
  uint32_t *gone_before;       /* [launch_max]  A(p): first occurrences of gone lines before p                      */
  uint32_t *risk_before;       /* [launch_max]  at-risk occurrences before p                                        */
  uint32_t *risk;              /* [launch_max]  the positions of the at-risk occurrences, ascending                 */
  uint32_t *risk_missed;       /* [launch_max + 1]  misses among the first k at-risk occurrences                    */
  uint8_t *kind;               /* [launch_max]  MPC_ELINE_*                                                         */
  uint2 *block_sums;           /* [ceil(launch_max / 256)]  per 256 lines (gone firsts, at-risk), then their offsets */
  unsigned long long tag_mask; /* as MpcPatternSet's                                                                */
  unsigned long long capacity; /* C, 1 .. MPC_PATTERN_CAPACITY                                                      */
  uint32_t slot_mask;          /* slots - 1                                                                         */
  uint32_t launch_max;         /* min(C, MPC_PATTERN_CHUNK)                                                         */
};
enum { MPC_ELINE_HIT = 0, MPC_ELINE_GONE_FIRST = 1, MPC_ELINE_RISK = 2, MPC_ELINE_RISK_MISS = 3 };
