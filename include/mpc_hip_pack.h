/*
 * mpc_hip_pack.h -- pack accounting of libmpc_hip.so: the sectors that blocks of N consecutive lines occupy when their
 * compressed lines are packed together and the block is rounded up to whole sectors once.  Included by mpc_hip.h
 * (include that).
 *
 * The sector accounting of mpc_hip_sizes.h and mpc_hip_classes.h rounds every line on its own.  A 32-byte line is one
 * 32-byte sector whatever it compresses to, so at the granule of GPGPU-Sim traces every compressor's sector ratio is
 * 1.0.  Real designs pack the compressed lines of a larger unit -- the sectors of a 128- or 256-byte block, the lines
 * of a 4 KiB page -- and round once.  This is the accounting for that: a sum over consecutive lines of the 2-byte
 * sizes the evaluators already wrote (csrc/mpc_pack.hip), on the device, next to the other two.
 *
 * A handle with pack accounting on numbers the lines it evaluates from 0, in the order of its calls, through every
 * ingestion path and as a member of a group, from the moment accounting is switched on or last reset.  Block b is
 * lines [b N, (b + 1) N): the notion of mpc_create_cpack_blocks.  When a block's last line has been evaluated the block
 * is closed:
 *     payload = sum of size_bits of its lines (unclipped)      bits = payload + header_bits
 *     sectors = min(max(1, ceil(bits / (8 sector_bytes))), S_B),     S_B = ceil(N line_size / sector_bytes)
 * A block may begin in one call and end in a much later one.  The lines behind the last closed block are the open
 * block; it is reported apart and never enters the histogram.
 *
 * The accounting is OFF until it is switched on; while it is off nothing is allocated or launched for it, and not one
 * number of any existing call changes.
 */
#ifndef MPC_HIP_PACK_H
#define MPC_HIP_PACK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* A pack table is uint64 [MPC_PACK_TABLE_LEN]:
 *   [0] closed blocks   [1] sum of their payload bits   [2] sum of their sectors
 *   [3] lines of the open block (0 .. N - 1)   [4] their payload bits
 *   [5] N   [6] sector_bytes   [7] header_bits
 *   [8 + k - 1] closed blocks that occupy k sectors, k = 1 .. S_B; the rest 0                                       */
#define MPC_PACK_MAX_SECTORS 1024
#define MPC_PACK_TABLE_LEN (8 + MPC_PACK_MAX_SECTORS)
#define MPC_PACK_MAX_BLOCK_LINES (1ull << 19)

/* Idempotent for the same three values.  MPC_E_INVAL with a message for block_lines == 0 or above
 * MPC_PACK_MAX_BLOCK_LINES (a block's bits are summed in 32 bits), sector_bytes == 0 or above block_lines x line_size,
 * S_B above MPC_PACK_MAX_SECTORS, header_bits above 65535, values other than those already in use, and a Fit handle.
 * block_lines == 1 with header_bits == 0 counts what mpc_size_sectors makes of the handle's histogram.  The device
 * table (8 KiB) and the open block's carry are freed by mpc_destroy.  A VPC handle with pack accounting on produces its
 * sizes on the device like every other; mpc_compress_batch_device without a size_bits_out array is cut into pieces of
 * 4 Mi lines over the scratch array that the other two accountings use, and blocks run across those seams.          */
int mpc_pack_stats_enable(mpc_handle *h, uint64_t block_lines, unsigned sector_bytes, unsigned header_bits);
/* Needs no device: the refusals of mpc_pack_stats_enable that depend on the three values and the line size alone.
 * MPC_OK, or MPC_E_INVAL with the message in mpc_last_error(NULL).                                                  */
int mpc_pack_check_values(unsigned line_size, uint64_t block_lines, unsigned sector_bytes, unsigned header_bits);
/* n == MPC_PACK_TABLE_LEN.  Waits like mpc_stats_get.  MPC_E_INVAL when accounting is not on.  The device table plus
 * what mpc_pack_stats_merge added.  mpc_stats_reset clears the table, the open block and the position with the
 * statistics.                                                                                                       */
int mpc_pack_stats_get(mpc_handle *h, uint64_t *table, size_t n);
/* Adds [0] .. [2] and the histogram of another handle's table (a shard's) and takes over its open block: the next
 * line this handle evaluates continues it.  MPC_E_INVAL if [5] .. [7] differ or if both sides have open lines:
 * shards are cut at multiples of N, so only the last one has a tail.                                                */
int mpc_pack_stats_merge(mpc_handle *h, const uint64_t *table, size_t n);
/* Needs no device.  The open block of k > 0 lines of a table, closed as a short block: *tail_cap = ceil(k line_size /
 * sector_bytes), *tail_sectors by the formula above with that cap, header bits included.  Both 0 for k == 0.         */
int mpc_pack_sectors_of_tail(const uint64_t *table, size_t n, unsigned line_size, uint64_t *tail_sectors, uint64_t *tail_cap);

/* ---- groups ----
 * Switches the accounting on for every member with the same values.  Every member must be fresh, just reset, or
 * already on with the same values and at the same line.  If the group's best-of is on at that moment, one more table,
 * owned by the group, is kept for the per-line minimum over the members that take part in the best-of (its
 * participation and tie rules), counted with header_bits + N tag_bits, tag_bits = ceil(log2(participants)); the
 * members must then be at the start of a block.  mpc_group_best_reset clears that table.
 * A group call finds its members at one common line.  If one of them was fed alone in between, the call returns
 * MPC_E_INVAL with a message that says so; misaligned blocks are never counted.                                     */
int mpc_group_pack_stats_enable(mpc_group *g, uint64_t block_lines, unsigned sector_bytes, unsigned header_bits);
/* member: an index into the group, or MPC_PACK_BEST for the table of the per-line minimum (MPC_E_INVAL if the best-of
 * was off when the group's accounting was switched on).  n == MPC_PACK_TABLE_LEN.  Waits like mpc_group_sync.       */
#define MPC_PACK_BEST (-1)
int mpc_group_pack_stats_get(mpc_group *g, int member, uint64_t *table, size_t n);

#ifdef __cplusplus
}
#endif
#endif /* MPC_HIP_PACK_H */
