/*
 * mpc_hip_rewrite.h -- rewrite accounting of libmpc_hip.so: how the size of a line changes when its address is
 * evaluated again.  Included by mpc_hip.h (include that).
 *
 * Image accounting (mpc_hip_image.h) keeps, per line address, the size of the latest line: a static picture of the
 * memory at the end of the trace.  A design that stores compressed lines in place has to know whether a line that is
 * written again still fits where the old one was.  Rewrite accounting follows, per distinct line address, the sequence
 * of sizes in trace order and reports the transition matrix between size classes, growth, shrink and first-touch
 * counts, and per address the latest size, the peak size and the number of observations (csrc/mpc_rewrite.hip: per
 * sub-batch of at most 4 Mi lines a stable sort by key, the transitions inside runs of one key, and one lane per run
 * that applies the run to a device hash map; the passes of one handle are chained in the order of its calls).
 *
 * A handle with rewrite accounting on numbers the lines it evaluates from 0, in the order of its calls, through every
 * ingestion path and as a member of a group (the position of pack and image accounting).  A line at position p with
 * address a and size s bits has key k = a / L (floor, L the line size); an address that is no multiple of L counts
 * under that key and as misaligned.  With granule_bytes g and G = ceil(L / g) the class of a size is
 *     c(s) = min(max(1, ceil(s / (8 g))), G)              (sizes above 8 L -- BPC and C-Pack are uncapped -- clamp to G)
 * Let the observations at a key, in ascending p, have sizes s_1 .. s_m; every addressed line is an observation, read or
 * write.  Then first[c(s_1)] += 1; for j >= 2, trans[c(s_{j-1})][c(s_j)] += 1 and equal_bits += (s_j == s_{j-1}); and
 * the key's state is latest = s_m, peak = max s_j, count = m.  The count saturates at 2^32 - 1 (not tested: it would
 * take 2^32 lines at one address).  Every entry of the table is an integer that does not depend on how the device
 * schedules its threads.
 *
 * The accounting is OFF until it is switched on; while it is off nothing is allocated or launched for it, and not one
 * number of any existing call changes.
 *
 * Out of scope: observations restricted to writes, and reads and writes kept apart; a best-of member for groups;
 * merging the maps of shards; eviction at the capacity; addresses for .npy and .txt traces; -a SC2, -a PATTERN and
 * -a CPACK in the command line.
 */
#ifndef MPC_HIP_REWRITE_H
#define MPC_HIP_REWRITE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* A rewrite table is uint64 [MPC_REWRITE_TABLE_LEN]:
 *   [0] lines  [1] sum of sizes  [2] distinct keys D  [3] misaligned
 *   [4] rewrites (= [0] - [2] = sum of trans)  [5] grows (c_new > c_old)  [6] shrinks  [7] equal_bits
 *   [8] sum over keys of c(latest)  [9] sum over keys of c(peak)  [10] sum of latest bits  [11] sum of peak bits
 *   [12] granule_bytes  [13] capacity  [14] G  [15] 0
 *   [16 + c - 1] first[c]     [48 + c - 1] keys whose latest class is c     [80 + c - 1] keys whose peak class is c
 *   [112 + b] keys with floor(log2(count)) == b, b = 0 .. 31
 *   [144 + (c_old - 1) * 32 + (c_new - 1)] trans
 * Derived on the host: overflow_rate = [5] / [4], image_granule_ratio = [2] G / [8], peak_granule_ratio = [2] G / [9],
 * traffic_ratio = [0] 8 L / [1].                                                                                     */
#define MPC_REWRITE_MAX_CLASSES 32
#define MPC_REWRITE_TABLE_LEN (144 + MPC_REWRITE_MAX_CLASSES * MPC_REWRITE_MAX_CLASSES)
#define MPC_REWRITE_MAX_CAPACITY (1ull << 28)

/* Idempotent for the same two values.  MPC_E_INVAL with a message for granule_bytes == 0, granule_bytes > L, G > 32,
 * capacity_lines == 0 or above MPC_REWRITE_MAX_CAPACITY, for values other than those already in use, and for a Fit
 * handle.  granule_bytes may be smaller than a sector.  Device memory, allocated here and freed by mpc_destroy: the map,
 * 16 bytes per slot, slots = the smallest power of two >= 2 x capacity_lines (and >= 2; capacity 2^24: 512 MiB), and the
 * scratch of a sub-batch of 4 Mi lines: 48 bytes per line (192 MiB) and rocPRIM's temporary storage for its sort.
 *
 * A handle takes addresses when image OR rewrite accounting is on (the addressed calls and the .log path of
 * mpc_hip_image.h), and refuses lines without addresses when either is on; both may be on at once, each with its own map.
 *
 * A line with a new key that arrives when D == capacity_lines finishes the handle exactly as image accounting does: the
 * call that brought it, or the next synchronising one, returns MPC_E_INVAL with a message naming the capacity, the handle
 * then refuses lines and mpc_rewrite_stats_get reports the same error.  Work past the overflow is bounded.            */
int mpc_rewrite_stats_enable(mpc_handle *h, uint64_t capacity_lines, unsigned granule_bytes);
/* Needs no device: the refusals of mpc_rewrite_stats_enable that depend on the values and the line size alone.
 * MPC_OK, or MPC_E_INVAL with the message in mpc_last_error(NULL).                                                  */
int mpc_rewrite_check_values(unsigned line_size, uint64_t capacity_lines, unsigned granule_bytes);
/* n == MPC_REWRITE_TABLE_LEN.  Waits like mpc_stats_get.  MPC_E_INVAL when accounting is not on.  NOT destructive: get,
 * feed more lines, get again.  mpc_stats_reset clears the map, the position and the table with the statistics.      */
int mpc_rewrite_stats_get(mpc_handle *h, uint64_t *table, size_t n);

/* ---- groups ----
 * Switches the accounting on for every member with the same values; a member's map is its handle's.  Every member must
 * be fresh, just reset, or already on with the same values and at the same line.  A group call finds its members at one
 * common line; if one of them was fed alone in between, the call returns MPC_E_INVAL with a message that says so (pack
 * accounting's refusal).  A chunk's keys are sorted once and applied to each member's map.                          */
int mpc_group_rewrite_stats_enable(mpc_group *g, uint64_t capacity_lines, unsigned granule_bytes);
int mpc_group_rewrite_stats_get(mpc_group *g, int member, uint64_t *table, size_t n);

#ifdef __cplusplus
}
#endif
#endif /* MPC_HIP_REWRITE_H */
