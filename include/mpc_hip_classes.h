/*
 * mpc_hip_classes.h -- per-class accounting of libmpc_hip.so: an evaluator's lines, compressed bits and sector counts
 * broken down by a per-line class byte.  Included by mpc_hip.h (include that).
 *
 * A run reports one ratio per compressor for the whole trace.  What do the reads compress to, and the writes?  What
 * does each kernel of the application compress to?  Of the lines that VPC's module k wins, what do BDI or C-Pack make?
 * All three are one operation: a class byte per line goes in, and the lines, the compressed bits and the sectors are
 * summed per class -- a GROUP BY over the 2-byte sizes the evaluators already wrote (csrc/mpc_classes.hip), on the
 * device, next to the size histograms of mpc_hip_sizes.h.  The reference has nothing like it.
 *
 * The accounting is OFF until it is switched on for a handle or a group; while it is off nothing is allocated or
 * launched for it, and not one number of any existing call changes.  The accumulators are plain uint64 sums: shards
 * add (mpc_class_stats_merge).
 */
#ifndef MPC_HIP_CLASSES_H
#define MPC_HIP_CLASSES_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* A class table is uint64 [256][MPC_CLASS_ROW], row c for the lines of class c:
 *   [0] lines   [1] sum of the sizes in bits, unclipped   [1 + k] lines that occupy k sectors, k = 1 .. S   the rest 0
 * with S = ceil(line_size / sector_bytes) <= 8 and, per line of `bits` bits, mpc_size_sectors' formula:
 * min(max(1, ceil(bits / (8 * sector_bytes))), S).  A Pattern line counts with the value its per-line output has.   */
#define MPC_CLASS_COUNT 256
#define MPC_CLASS_ROW 10
#define MPC_CLASS_TABLE_LEN (MPC_CLASS_COUNT * MPC_CLASS_ROW)

/* Counts the lines the handle evaluates from now on, through every ingestion path and as a member of a group;
 * idempotent for the same sector_bytes.  MPC_E_INVAL with a message for sector_bytes == 0 or above the line size,
 * for more than 8 sectors a line, for another sector_bytes than the handle already counts with, and for a Fit handle
 * (an analysis has no per-line sizes).  The device table (20 KiB) is freed by mpc_destroy.  Like the size histogram,
 * mpc_compress_batch_device on a handle with accounting on and no size_bits_out array of the caller's evaluates a batch
 * of more than 4 Mi lines as consecutive pieces of 4 Mi lines over ONE scratch array that both accountings share.  */
int mpc_class_stats_enable(mpc_handle *h, unsigned sector_bytes);
/* n == MPC_CLASS_TABLE_LEN.  Waits like mpc_stats_get.  MPC_E_INVAL when accounting is not on.  The device table plus
 * what mpc_class_stats_merge added.  mpc_stats_reset clears both with the statistics.                               */
int mpc_class_stats_get(mpc_handle *h, uint64_t *table, size_t n);
/* += a table of another handle (a shard); n == MPC_CLASS_TABLE_LEN.                                                 */
int mpc_class_stats_merge(mpc_handle *h, const uint64_t *table, size_t n);
/* The sector_bytes accounting was switched on with.  MPC_E_INVAL when it is not on.                                 */
int mpc_class_sector_bytes(const mpc_handle *h, unsigned *sector_bytes);

/* mpc_compress_batch / mpc_compress_batch_device with one class byte per line: `classes` is n_lines uint8 in HOST
 * memory, `d_classes` n_lines uint8 in DEVICE memory (any alignment; only these n_lines bytes are read).  NULL counts
 * every line in class 0, which is also what every un-classed call does on a handle with accounting on.  A classed call
 * on a handle without accounting is MPC_E_INVAL.  Sizes and selected are those of the un-classed call.             */
int mpc_compress_batch_classed(mpc_handle *h, const uint8_t *lines, uint64_t n_lines, const uint8_t *classes,
                               uint16_t *size_bits_out, int8_t *selected_out);
int mpc_compress_batch_device_classed(mpc_handle *h, const void *d_lines, uint64_t n_lines, const uint8_t *d_classes,
                                      uint16_t *d_size_bits_out, int8_t *d_selected_out, void *hip_stream);

/* Classes from the records of a GPGPU-Sim .log (mpc_compress_gpgpusim_log): which field of the 62-byte record header
 * is the class of the record's line.  The stager fills a pinned class buffer per staging slot beside the lines (it
 * and its device twin exist only once accounting is on and a field is chosen).                                    */
#define MPC_CLASS_LOG_NONE   0   /* the default: class 0                                      */
#define MPC_CLASS_LOG_KERNEL 1   /* record byte 0, the kernel id                              */
#define MPC_CLASS_LOG_RW     2   /* req_type 0 (GLOBAL_ACC_R) -> class 0, 4 (GLOBAL_ACC_W) -> class 1 */
#define MPC_CLASS_LOG_MFTYPE 3   /* record byte 1, mf_type                                    */
int mpc_class_log_field(mpc_handle *h, int field);

/* ---- groups ----
 * Switches the accounting on for every member (mpc_class_stats_enable on each: a member's table is its handle's) and,
 * when the group's best-of is on -- now or later --, keeps one more table for the per-line minimum over the members
 * that take part in the best-of, under its participation and tie rules.  Idempotent for the same sector_bytes.     */
int mpc_group_class_stats_enable(mpc_group *g, unsigned sector_bytes);
/* member: an index into the group, or MPC_CLASS_BEST for the best-of's table (MPC_E_INVAL while the best-of is off;
 * mpc_group_best_reset clears it).  n == MPC_CLASS_TABLE_LEN.  Waits like mpc_group_sync.                          */
#define MPC_CLASS_BEST (-1)
int mpc_group_class_stats_get(mpc_group *g, int member, uint64_t *table, size_t n);
/* mpc_group_compress_batch / mpc_group_compress_batch_device with one class byte per line, as above.  MPC_E_INVAL
 * when the group's accounting is off, and for a class array while the classes come from a member.                 */
int mpc_group_compress_batch_classed(mpc_group *g, const uint8_t *lines, uint64_t n_lines, const uint8_t *classes,
                                     uint16_t *const *size_bits_out, int8_t *const *selected_out);
int mpc_group_compress_batch_device_classed(mpc_group *g, const void *d_lines, uint64_t n_lines, const uint8_t *d_classes,
                                            uint16_t *const *d_size_bits_out, int8_t *const *d_selected_out, void *hip_stream);
int mpc_group_class_log_field(mpc_group *g, int field);
/* The class of a line is member i's `selected` + 1, through every ingestion path: for a VPC member 0 = uncompressed
 * and k + 1 = module k's cluster, for a BDI member the state + 1.  Member i's `selected` is then produced on the
 * device whether or not the caller asked for it, and its kernel runs before the accounting launch on the same stream.
 * It takes precedence over a .log field.  MPC_E_INVAL for a member without `selected` (FPC, BPC, C-Pack: theirs is
 * always 0) and when the group's accounting is off.  member == -1 switches it off again.                           */
int mpc_group_class_from_member(mpc_group *g, int member);

#ifdef __cplusplus
}
#endif
#endif /* MPC_HIP_CLASSES_H */
