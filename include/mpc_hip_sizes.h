/*
 * mpc_hip_sizes.h -- size accounting of libmpc_hip.so: per-evaluator histograms of the per-line compressed sizes, the
 * per-line best-of of a group, and the 32-byte-sector view of such a histogram.  Included by mpc_hip.h (include that).
 *
 * The reference reports one number per compressor, sum of original bits / sum of compressed bits, and a size histogram
 * for VPC only (VPCResult::PrintDetail, VPC.h; the PrintDetail of BDI, FPC, BPC, SC2 and Pattern is empty).  A memory
 * system moves lines in sectors (ACCESS_GRAN 32 / REQ_SIZE 32 in the reference), so what it gains is decided by the
 * distribution of the sizes, not by their sum.  The accounting here is OFF until it is switched on for a handle or a
 * group; while it is off nothing is allocated or launched for it.  Switched on, one more kernel per chunk reads the
 * 2-byte sizes the evaluators wrote (csrc/mpc_sizes.hip).  The accumulators are plain uint64 sums: shards add.
 */
#ifndef MPC_HIP_SIZES_H
#define MPC_HIP_SIZES_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bins of a size histogram: bin s counts lines of s bits, the last bin also every larger size.  No evaluator reaches
 * the last bin for lines of up to 256 bytes: the largest size is FPC's 35 bits per word, 2240 bits at 256 bytes (BDI
 * and Pattern 8 L + 4, SC2 33 bits per word, VPC 8 L + id bits, BPC at most 1089 bits at any line size -- and 217 bits
 * for an 8-byte line, more than 8 L).                                                                              */
#define MPC_SIZE_BINS 4096

/* Counts the lines the handle evaluates from now on, through every ingestion path and as a member of a group;
 * idempotent.  BDI, FPC, BPC, SC2 and Pattern handles get a device accumulator of MPC_SIZE_BINS uint64 (freed by
 * mpc_destroy); a Pattern line counts with the value its per-line output has, the smallest scan + 4 bits.  A VPC
 * handle allocates nothing: its histogram is the sum over the clusters of the histogram in its statistics.
 * mpc_compress_batch_device on a handle with accounting on and no size_bits_out array of the caller's evaluates a
 * batch of more than 4 Mi lines as consecutive pieces of 4 Mi lines on the caller's stream (8 MiB of scratch per
 * handle), which is what smaller calls by the caller would do.                                                     */
int mpc_size_hist_enable(mpc_handle *h);
/* n == MPC_SIZE_BINS.  Waits like mpc_stats_get.  MPC_E_INVAL when accounting is not on.  mpc_stats_reset clears the
 * histogram with the statistics; mpc_stats_merge / mpc_stats_set do not reach it.                                  */
int mpc_size_hist_get(mpc_handle *h, uint64_t *bins, size_t n);

/* Best-of for a group: per line the smallest size over the members that take part -- every member but Pattern ones
 * (an analyser: its CompressedSize stays 0) -- with the first such member, in member order, as the winner of a tie.
 * Counts lines the group evaluates from now on; idempotent.  MPC_E_INVAL with a message when fewer than 2 or more
 * than 8 members take part.  The accumulator is freed by mpc_group_destroy.                                        */
int mpc_group_best_enable(mpc_group *g);
/* bins[n], n == MPC_SIZE_BINS: histogram of the best size WITHOUT tag bits.  wins[n_members], n_members == the group's:
 * lines won per member, 0 for a member outside the set.  *best_bits: sum of the best sizes.  *lines: lines counted.
 * A hybrid that picks the best member per line also stores which: ceil(log2(members taking part)) tag bits per line,
 * a multiplication the caller does.  Waits like mpc_group_sync.  Any output pointer may be NULL.                   */
int mpc_group_best_get(mpc_group *g, uint64_t *bins, size_t n, uint64_t *wins, size_t n_members, uint64_t *best_bits,
                       uint64_t *lines);
int mpc_group_best_reset(mpc_group *g);

/* Needs no device: the sectors of `sector_bytes` bytes that lines of `line_size` bytes with this histogram occupy.
 * Per line of `bits` bits: min(max(1, ceil(bits / (8 * sector_bytes))), ceil(line_size / sector_bytes)) -- a line
 * takes at least one sector and never more than the uncompressed line.  n == MPC_SIZE_BINS.
 * classes[c - 1] = lines that occupy c sectors, n_classes == ceil(line_size / sector_bytes); *total_sectors their sum
 * weighted by c; *ratio = lines * n_classes / total sectors (0 for no lines).  classes, total_sectors and ratio may
 * each be NULL.  MPC_E_INVAL for sector_bytes == 0 or > line_size, or a wrong n or n_classes.                      */
int mpc_size_sectors(const uint64_t *bins, size_t n, unsigned line_size, unsigned sector_bytes,
                     uint64_t *classes, size_t n_classes, uint64_t *total_sectors, double *ratio);

#ifdef __cplusplus
}
#endif
#endif /* MPC_HIP_SIZES_H */
