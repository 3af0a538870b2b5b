/*
 * mpc_hip_image.h -- image accounting of libmpc_hip.so: what the MEMORY that a trace touches compresses to, by line
 * address.  Included by mpc_hip.h (include that).
 *
 * The size histogram, the class tables and the pack tables account a trace's traffic: every request counts, a hot line
 * as often as it is requested, and a block of N consecutive requests is not a block of memory.  Image accounting takes
 * a 64-bit address per line and keeps, for every distinct line address, the size of the LATEST line evaluated there
 * (csrc/mpc_image.hip: a device hash map updated behind every evaluator launch).  A get reports what that image
 * occupies when address-aligned blocks of N lines are packed and rounded up to whole sectors once.
 *
 * A handle with image accounting on numbers the lines it evaluates from 0, in the order of its calls, through every
 * ingestion path and as a member of a group, from the moment accounting is switched on or last reset (the position of
 * pack accounting).  A line at position p with address a and size s bits has key k = a / L (floor, L the line size);
 * an address that is no multiple of L still counts under that key and is counted as misaligned.  The image maps each
 * key to the size of the line with the largest p among the lines of that key.  Block b holds the keys [b N, (b + 1) N);
 * it is touched when at least one of them is in the image.  A touched block with T keys in the image and payload = the
 * sum of their latest sizes occupies
 *     cap     = ceil(T L / sector_bytes)                  (a short block, as mpc_pack_sectors_of_tail closes one)
 *     sectors = min(max(1, ceil((payload + header_bits) / (8 sector_bytes))), cap)
 * Every entry of the table is an integer that does not depend on how the device schedules its threads.
 *
 * The accounting is OFF until it is switched on; while it is off nothing is allocated or launched for it, and not one
 * number of any existing call changes.
 *
 * Out of scope: a best-of image for groups; merging the images of shards (one handle covers one trace on one GPU, as
 * SC2 and Pattern do); eviction at the capacity; addresses for .npy and .txt traces.
 */
#ifndef MPC_HIP_IMAGE_H
#define MPC_HIP_IMAGE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* An image table is uint64 [MPC_IMAGE_TABLE_LEN]:
 *   [0] lines evaluated with an address       [1] sum of their sizes (the traffic)
 *   [2] distinct keys D                       [3] sum of the latest sizes
 *   [4] touched blocks                        [5] sum of their sectors        [6] sum of their caps
 *   [7] lines whose address was not a multiple of L
 *   [8] N  [9] sector_bytes  [10] header_bits  [11] capacity        [12..15] 0
 *   [16 + k - 1] touched blocks that occupy k sectors, k = 1 .. S_B = ceil(N L / sector_bytes) <= 1024; the rest 0
 * Derived on the host: traffic_ratio = [0] 8 L / [1], image_ratio = [2] 8 L / [3], image_sector_ratio = [6] / [5].   */
#define MPC_IMAGE_MAX_SECTORS 1024
#define MPC_IMAGE_TABLE_LEN (16 + MPC_IMAGE_MAX_SECTORS)
#define MPC_IMAGE_MAX_CAPACITY (1ull << 28)

/* Idempotent for the same four values.  MPC_E_INVAL with a message for what mpc_pack_check_values refuses for
 * (block_lines, sector_bytes, header_bits), for capacity_lines == 0 or above MPC_IMAGE_MAX_CAPACITY, for values other
 * than those already in use, and for a Fit handle.  Device memory: 16 bytes per slot, slots = the smallest power of two
 * >= 2 x capacity_lines (and >= 2), allocated here and freed by mpc_destroy (capacity 2^24: 512 MiB); a get allocates,
 * for its own duration, a block map of 16 bytes per slot of the smallest power of two >= 2 D.
 * A VPC handle with image accounting on produces its sizes on the device like every other; mpc_compress_batch_device_
 * addressed without a size_bits_out array is cut into pieces of 4 Mi lines over the scratch array that the other three
 * accountings use, and positions and addresses run across those seams.
 *
 * A line with a new key that arrives when D == capacity_lines finishes the handle: the call that brought it, or the next
 * synchronising one, returns MPC_E_INVAL with a message, the handle then refuses lines and mpc_image_stats_get reports
 * the same error (the behaviour of mpc_create_pattern's capacity).  Which keys entered before that is unspecified.
 * The device stops probing and claiming once it has seen the capacity exceeded, so a trace far beyond the capacity
 * costs no more than one within it.                                                                                 */
int mpc_image_stats_enable(mpc_handle *h, uint64_t capacity_lines, uint64_t block_lines, unsigned sector_bytes, unsigned header_bits);
/* Needs no device: the refusals of mpc_image_stats_enable that depend on the values and the line size alone.
 * MPC_OK, or MPC_E_INVAL with the message in mpc_last_error(NULL).                                                  */
int mpc_image_check_values(unsigned line_size, uint64_t capacity_lines, uint64_t block_lines, unsigned sector_bytes, unsigned header_bits);
/* n == MPC_IMAGE_TABLE_LEN.  Waits like mpc_stats_get.  MPC_E_INVAL when accounting is not on.  NOT destructive: get,
 * feed more lines, get again.  mpc_stats_reset clears the image, the position and the table with the statistics.    */
int mpc_image_stats_get(mpc_handle *h, uint64_t *table, size_t n);

/* mpc_compress_batch / mpc_compress_batch_device with one address per line (addresses: host memory; d_addresses:
 * device memory, 8-byte aligned, read on hip_stream behind the evaluator).  MPC_E_INVAL on a handle without image
 * accounting.  On a handle WITH image accounting on, every call that brings no addresses -- mpc_compress_batch,
 * mpc_compress_batch_device, their classed twins, mpc_compress_npy -- is MPC_E_INVAL with a message: a silent hole in
 * the image is worse than a refusal.  mpc_compress_gpgpusim_log on such a handle takes each evaluated record's
 * mem_addr (the u64 at byte 30 of the record's header); class fields of the same log keep working next to it.  With
 * class accounting on too, addressed lines count in class 0.                                                        */
int mpc_compress_batch_addressed(mpc_handle *h, const uint8_t *lines, uint64_t n, const uint64_t *addresses, uint16_t *size_bits_out,
                                 int8_t *selected_out);
int mpc_compress_batch_device_addressed(mpc_handle *h, const void *d_lines, uint64_t n, const uint64_t *d_addresses, uint16_t *d_size_bits_out,
                                        int8_t *d_selected_out, void *hip_stream);

/* Pure host code: the hash whose low bits give a key's first slot, slot0 = mpc_image_hash(key) & (slots - 1) with
 * slots the smallest power of two >= 2 x capacity_lines and at least 2; the chain is linear and wraps.  (The test
 * library, -DMPC_TESTING=1, keeps only the low k bits of the hash in a handle switched on under
 * MPC_TEST_IMAGE_HASH_BITS=k; this function is the same in both.)                                                   */
uint64_t mpc_image_hash(uint64_t key);

/* ---- groups ----
 * Switches the accounting on for every member with the same values; a member's image is its handle's.  Every member
 * must be fresh, just reset, or already on with the same values and at the same line.  A group call finds its members
 * at one common line; if one of them was fed alone in between, the call returns MPC_E_INVAL with a message that says
 * so (pack accounting's refusal).  The addressed group calls need the group's accounting on and deliver the addresses
 * to all members, as mpc_group_compress_gpgpusim_log does with each record's mem_addr.                              */
int mpc_group_image_stats_enable(mpc_group *g, uint64_t capacity_lines, uint64_t block_lines, unsigned sector_bytes, unsigned header_bits);
int mpc_group_image_stats_get(mpc_group *g, int member, uint64_t *table, size_t n);
int mpc_group_compress_batch_addressed(mpc_group *g, const uint8_t *lines, uint64_t n, const uint64_t *addresses, uint16_t *const *size_bits_out,
                                       int8_t *const *selected_out);
int mpc_group_compress_batch_device_addressed(mpc_group *g, const void *d_lines, uint64_t n, const uint64_t *d_addresses,
                                              uint16_t *const *d_size_bits_out, int8_t *const *d_selected_out, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* MPC_HIP_IMAGE_H */
