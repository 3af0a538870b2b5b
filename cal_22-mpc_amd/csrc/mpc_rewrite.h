// mpc_rewrite.h -- the accounting pass that follows, per distinct line address, the SEQUENCE of sizes evaluated there
// (mpc_rewrite.hip), next to the histograms of mpc_sizes.h, the class tables of mpc_classes.h, the pack tables of
// mpc_pack.h and the image of mpc_image.h.  It reads what the evaluators wrote, 2 bytes per line, and 8 bytes of address
// per line.  Unlike the image it depends on order, inside a launch and between launches.
//
// The map is image accounting's (mpc_image.h: keys[slots], kMpcImageEmpty a free slot, the hash mpc_image_mix, linear
// chains that wrap, slots a power of two >= 2 x capacity, the probe loop of mpc_image_probe.h), its value one word:
//     latest : 16 | peak : 16 | count : 32      (count saturates at 2^32 - 1)
// 16 bytes per slot, 32 bytes per line of capacity.
//
// A launch is cut into sub-batches of at most MPC_REWRITE_BATCH lines.  Per sub-batch, on one stream:
//   keys    key_i = addr_i / L and i; lines, bits and misaligned summed in registers -> wave -> LDS -> one add per workgroup
//   sort    a stable rocprim::radix_sort_pairs of (key, i): equal keys stay in position order
//   in-run  a lane per sorted element: an element whose left neighbour has its key adds trans[c(prev)][c(own)] and
//           equal_bits into the workgroup's matrix in LDS (flushed once, non-zero entries only), and every element writes
//           (size << 48) | (1 << 24) | j for the reduction
//   runs    one rocprim::reduce_by_key with (max, +, min) over those words: per run its largest size, its length and
//           its first element (lengths and positions are below 2^24: MPC_REWRITE_BATCH is 2^22) -- no lane walks a run
//   apply   a lane per run: probes or claims the key's slot, reads the old value, counts first[c(first)] for a new key
//           or trans[c(old latest)][c(first)] and equal_bits for a known one, writes latest = the run's last, the peak
//           and the count, counts claims.  A key has one writer per sub-batch, so the value needs no atomic.
// Sub-batches of one handle are ordered by the stream or by the event the host chains them with; no lane ever waits for
// another lane or workgroup.
//
// What an overflowing trace may cost is bounded as the image's is: a probe gives up after capacity + 1 slots, reads the
// overflow flag every 64 slots, every wave of the apply kernel reads it first and leaves when it is set; a workgroup adds
// its claims once and the add that passes the capacity sets the flag.
//
// dev is uint64 [MPC_REWRITE_DEV_LEN]: the counters, first[32], trans[32][32], then the table of a get's pass (one kernel
// over the slots: three histograms in LDS and four sums).
//
// Scratch of a sub-batch, allocated at enable and freed by mpc_destroy (mpc_rewrite_scratch_bytes): per line of
// MPC_REWRITE_BATCH 8 + 8 bytes of keys (in, sorted), 4 + 4 of indices, 8 of reduction words, 8 + 8 of run keys and run
// aggregates = 48 bytes, 192 MiB, and rocPRIM's temporary storage for the sort and the reduction (the larger of the two).
#pragma once
#include <stddef.h>
#include <stdint.h>

#define MPC_REWRITE_BATCH (4ull << 20)   /* lines of a sub-batch: the accounting piece size; at most 2^22 */
#define MPC_REWRITE_MAX_CLASSES 32
#define MPC_REWRITE_CTL_LINES 0          /* lines evaluated with an address                 */
#define MPC_REWRITE_CTL_BITS 1           /* sum of their sizes                              */
#define MPC_REWRITE_CTL_KEYS 2           /* claims: distinct keys D                         */
#define MPC_REWRITE_CTL_MISALIGNED 3     /* lines whose address was no multiple of L        */
#define MPC_REWRITE_CTL_OVERFLOW 4       /* non-zero: more keys than the capacity           */
#define MPC_REWRITE_CTL_EQUAL 5          /* rewrites with exactly the size before           */
#define MPC_REWRITE_CTL_LEN 8
#define MPC_REWRITE_DEV_FIRST MPC_REWRITE_CTL_LEN                                   /* [c - 1]                           */
#define MPC_REWRITE_DEV_TRANS (MPC_REWRITE_DEV_FIRST + MPC_REWRITE_MAX_CLASSES)     /* [(c_old - 1) * 32 + (c_new - 1)]  */
#define MPC_REWRITE_DEV_OUT (MPC_REWRITE_DEV_TRANS + MPC_REWRITE_MAX_CLASSES * MPC_REWRITE_MAX_CLASSES)
#define MPC_REWRITE_OUT_LATEST_CLASSES 0 /* sum over keys of c(latest)                      */
#define MPC_REWRITE_OUT_PEAK_CLASSES 1
#define MPC_REWRITE_OUT_LATEST_BITS 2
#define MPC_REWRITE_OUT_PEAK_BITS 3
#define MPC_REWRITE_OUT_HIST_LATEST 4    /* [c - 1] keys whose latest class is c            */
#define MPC_REWRITE_OUT_HIST_PEAK (MPC_REWRITE_OUT_HIST_LATEST + 32)
#define MPC_REWRITE_OUT_HIST_COUNT (MPC_REWRITE_OUT_HIST_PEAK + 32)                 /* [b] keys with floor(log2(count)) == b */
#define MPC_REWRITE_OUT_LEN (MPC_REWRITE_OUT_HIST_COUNT + 32)
#define MPC_REWRITE_DEV_LEN (MPC_REWRITE_DEV_OUT + MPC_REWRITE_OUT_LEN)

// the scratch of a sub-batch: pointers into one allocation (mpc_rewrite_scratch_carve)
struct MpcRewriteScratch {
  unsigned long long *keys_in, *keys_out;  // [lines]
  unsigned *idx_in, *idx_out;              // [lines]
  unsigned long long *words;               // [lines] (size << 48) | (1 << 24) | j of the sorted elements
  unsigned long long *run_keys, *run_agg;  // [lines] per run: its key; (max size << 48) | (length << 24) | first element
  unsigned long long *runs;                // [1] the number of runs
  void *temp;                              // rocPRIM's temporary storage
  size_t temp_bytes;
  unsigned long long lines;                // the sub-batch's most lines
};

// the map of one handle
struct MpcRewriteMap {
  unsigned long long *keys, *vals;         // [slot_mask + 1]
  unsigned long long *dev;                 // [MPC_REWRITE_DEV_LEN]
  unsigned long long slot_mask;            // slots - 1
  unsigned long long hash_mask;            // all ones; the test library may keep only a few low bits of the hash
  unsigned long long capacity;             // <= slots / 2
  unsigned granule_bits;                   // 8 g
  unsigned classes;                        // G = ceil(L / g), 1 .. 32
};
