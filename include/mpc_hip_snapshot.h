/*
 * mpc_hip_snapshot.h -- snapshots of libmpc_hip.so: the memory image of a trace rebuilt as DATA, and evaluated at any
 * line size.  Included by mpc_hip.h (include that).
 *
 * Image accounting (mpc_hip_image.h) keeps, per distinct line address, the SIZE of the latest line evaluated there.  A
 * snapshot keeps the BYTES: for every distinct unit address the bytes of the latest unit added there.  It then writes
 * out address-aligned lines of L = k x U bytes assembled from those units, in ascending address order, as an ordinary
 * device-resident array of lines with addresses, which goes through mpc_compress_batch_device(_addressed) into any
 * handle or group with every accounting the library has.  That is how a GPGPU-Sim .log trace, which delivers 32-byte
 * requests, is evaluated at the 64-, 128- or 256-byte lines of the memory it touched.
 *
 * Semantics (all integers, no dependence on how the device schedules its threads).  A snapshot has a unit size U in
 * {32, 64, 128} bytes and a capacity in units.  Units are numbered from 0 in the order they are added, across calls.  A
 * unit at position p with address a has key a / U (floor); an address that is no multiple of U counts under that key
 * and is counted as misaligned.  The snapshot maps each key to the U bytes of the unit with the largest p among the
 * units of that key.  For a line size L = k U, k in {1, 2, 4, 8}, L <= 256: the line key is key / k, the line address
 * (key / k) L, unit key % k sits at byte offset (key % k) U.  A line is touched when at least one of its units is
 * present and complete when all k are; bit j of its presence mask is set when unit j is present.  partial = skip emits
 * the complete lines only, partial = zero every touched line with its missing units as zero bytes; emitted lines are in
 * ascending line-key order, so emitted line i, i = 0 .. n_out - 1, is a pure function of what was added.
 *
 * A new key that arrives when the snapshot holds `capacity` units finishes the snapshot: that add (mpc_snapshot_add,
 * mpc_snapshot_add_gpgpusim_log) or the next synchronising call (after mpc_snapshot_add_device) returns MPC_E_INVAL with
 * a message, later adds, plans, writes and evaluations are refused; mpc_snapshot_reset empties and revives it.
 *
 * Device memory: 16 + U bytes per slot, slots = the smallest power of two >= 2 x capacity (and >= 2), allocated at
 * creation: 1.5 GiB at U = 32 and a capacity of 2^24 units, 4.5 GiB at U = 128.  A plan holds, until the next add or
 * reset, 12 bytes per distinct unit (the sorted keys and their slots) and 4 bytes per emitted line, and takes some 30
 * bytes per distinct unit more while it runs.  mpc_snapshot_evaluate and mpc_snapshot_read_lines own a scratch buffer of
 * L + 9 bytes per line of a piece of at most 4 Mi lines.
 *
 * One snapshot is used from one thread at a time.  The mpc_snapshot_add_device calls of one snapshot are ordered by the
 * caller: on one stream, or with events between them (their launches share a scratch array and the table's payload).
 *
 * Out of scope: reads and writes kept apart, a snapshot "as of" an earlier position, eviction at the capacity, .npy and
 * .txt traces (they carry no addresses), merging the snapshots of shards.
 */
#ifndef MPC_HIP_SNAPSHOT_H
#define MPC_HIP_SNAPSHOT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mpc_snapshot mpc_snapshot;

#define MPC_SNAPSHOT_MAX_CAPACITY (1ull << 28)
#define MPC_SNAPSHOT_MAX_LINE 256
#define MPC_SNAPSHOT_PARTIAL_SKIP 0   /* emit complete lines only                               */
#define MPC_SNAPSHOT_PARTIAL_ZERO 1   /* emit every touched line, missing units as zero bytes   */
#define MPC_SNAPSHOT_TABLE_LEN 8      /* the length of a stats and of a plan vector             */

/* Needs no device: MPC_OK, or MPC_E_INVAL with the message in mpc_snapshot_last_error(NULL) for a unit_bytes other than
 * 32, 64 or 128, a capacity_units of 0 or above MPC_SNAPSHOT_MAX_CAPACITY, a line_size that is no k x unit_bytes with k
 * in {1, 2, 4, 8}, and a line_size above 256.  line_size == 0 checks the first two alone (what a create needs).      */
int mpc_snapshot_check_values(unsigned unit_bytes, uint64_t capacity_units, unsigned line_size);
/* device < 0 selects the current HIP device.  MPC_E_NODEVICE without one, MPC_E_NOMEM when the table does not fit.  */
int mpc_snapshot_create(unsigned unit_bytes, uint64_t capacity_units, int device, mpc_snapshot **out);
void mpc_snapshot_destroy(mpc_snapshot *s);
/* Empties the snapshot: no units, position 0, not finished.  Waits for the device.                                  */
int mpc_snapshot_reset(mpc_snapshot *s);
/* Last error text of this snapshot (or of the last failed create / check_values if s == NULL).                      */
const char *mpc_snapshot_last_error(const mpc_snapshot *s);

/* n units of unit_bytes bytes with one address each, in HOST memory; staged in chunks; returns when they are in.    */
int mpc_snapshot_add(mpc_snapshot *s, const uint8_t *units, uint64_t n, const uint64_t *addresses);
/* The same from DEVICE memory (units 16-byte aligned, addresses 8-byte aligned), asynchronous on hip_stream.        */
int mpc_snapshot_add_device(mpc_snapshot *s, const void *d_units, uint64_t n, const uint64_t *d_addresses, void *hip_stream);
/* Every evaluated record of a GPGPU-Sim .log (GLOBAL_ACC_R / GLOBAL_ACC_W: mpc_compress_gpgpusim_log's filter) adds its
 * payload at its mem_addr, in file order.  MPC_E_INVAL for a log whose line size is not unit_bytes and for one that
 * mixes request sizes among its evaluated records.  units_added may be NULL.                                        */
int mpc_snapshot_add_gpgpusim_log(mpc_snapshot *s, const char *log_path, uint64_t *units_added);

/* t[8]: [0] units added  [1] distinct units D  [2] misaligned units  [3] capacity  [4] unit_bytes  [5..7] 0.  Waits.  */
int mpc_snapshot_stats(mpc_snapshot *s, uint64_t *t);
/* p[8]: [0] touched lines  [1] complete lines  [2] partial lines  [3] units present in partial lines  [4] missing
 * units  [5] n_out, the emitted lines  [6..7] 0.  k [1] + [3] == D, [3] + [4] == k [2], [5] == [1] (skip) or [0] (zero).
 * Waits.  The sorted keys behind a plan are kept until the next add or reset.                                       */
int mpc_snapshot_plan(mpc_snapshot *s, unsigned line_size, int partial, uint64_t *p);

/* Emitted lines [first, first + n) of (line_size, partial) into caller-owned DEVICE memory, on hip_stream:
 * d_lines_out n x line_size bytes (16-byte aligned), d_addresses_out n uint64 or NULL, d_presence_out n bytes or NULL
 * (the presence mask: a ready class array for the *_classed calls).  first + n > n_out is MPC_E_INVAL.  Plans first
 * (and waits) unless the plan of the same (line_size, partial) is still current.                                    */
int mpc_snapshot_write_lines(mpc_snapshot *s, unsigned line_size, int partial, uint64_t first, uint64_t n, void *d_lines_out,
                             uint64_t *d_addresses_out, uint8_t *d_presence_out, void *hip_stream);
/* The same into HOST memory (through the snapshot's scratch buffer, in pieces); returns when the lines are there.   */
int mpc_snapshot_read_lines(mpc_snapshot *s, unsigned line_size, int partial, uint64_t first, uint64_t n, uint8_t *lines_out,
                            uint64_t *addresses_out, uint8_t *presence_out);

/* Materialises the emitted lines in pieces of at most 4 Mi lines into the snapshot's scratch buffer and feeds each piece
 * to the handle (group) through the device batch call: with the lines' addresses when the handle (group) has image
 * accounting on, with the presence masks as classes when by_presence != 0 and the handle (group) has class accounting on
 * (a group whose classes come from a member refuses by_presence).  Then synchronises (mpc_sync / mpc_group_sync).  The
 * handle's line size must be line_size, its device the snapshot's.  A failure of the handle or group is reported in its
 * own mpc_last_error / mpc_group_last_error and in the snapshot's.  The lines fed are the plan's n_out.             */
int mpc_snapshot_evaluate(mpc_snapshot *s, mpc_handle *h, unsigned line_size, int partial, int by_presence);
int mpc_snapshot_evaluate_group(mpc_snapshot *s, mpc_group *g, unsigned line_size, int partial, int by_presence);

#ifdef __cplusplus
}
#endif
#endif /* MPC_HIP_SNAPSHOT_H */
