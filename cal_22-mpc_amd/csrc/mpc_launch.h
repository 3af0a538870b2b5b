// mpc_launch.h -- every host-callable launcher of the kernel translation units, declared once.
//
// The launchers have C linkage, so a declaration that drifted from its definition would still link and then misbehave.
// This header is therefore included by the callers (mpc_capi.hip, mpc_jit.h) AND by the units that define the
// launchers (mpc_kernels.hip, mpc_baselines.hip, mpc_sc2.hip, mpc_pattern.hip, mpc_pattern_evict.hip, mpc_cpack.hip, mpc_cpack_blocks.hip, mpc_fit.hip, mpc_sizes.hip, mpc_classes.hip, mpc_pack.hip, mpc_image.hip, mpc_rewrite.hip, the host section of mpc_vpc_lane.hip):
// the compiler sees declaration and definition together and refuses a mismatch.  Host code only -- the run-time
// compiled source of mpc_jit.h (-DMPC_LANE_JIT) never sees it, and it is not one of the files that key the code
// object cache.
//
// The parameter blocks are only named here (their definitions: mpc_device.h, mpc_sc2.h, mpc_pattern.h, mpc_sizes.h, mpc_classes.h, mpc_pack.h, mpc_image.h, mpc_rewrite.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

struct MpcVpcParams;
struct MpcBaselinesArgs;
struct MpcSc2Table;
struct MpcPatternSet;
struct MpcEvictSet;
struct MpcSizesArgs;
struct MpcClassArgs;
struct MpcPackArgs;
struct MpcImageArgs;
struct MpcImageGetArgs;
struct MpcRewriteScratch;
struct MpcRewriteMap;

extern "C" {
// mpc_kernels.hip
size_t mpc_vpc_generic_smem(const MpcVpcParams *P);
hipError_t mpc_launch_vpc_generic(const void *d_lines, unsigned long long n_lines, const MpcVpcParams *P, uint16_t *d_sizes, int8_t *d_sel,
                                  unsigned long long *d_stats, int grid, hipStream_t stream);
hipError_t mpc_launch_bdi(const void *d_lines, unsigned long long n_lines, int L, uint16_t *d_sizes, int8_t *d_sel, unsigned long long *d_stats,
                          int grid, hipStream_t stream);
hipError_t mpc_launch_fpc(const void *d_lines, unsigned long long n_lines, int L, uint16_t *d_sizes, int8_t *d_sel, unsigned long long *d_stats,
                          int grid, hipStream_t stream);
hipError_t mpc_launch_bpc(const void *d_lines, unsigned long long n_lines, int L, uint16_t *d_sizes, int8_t *d_sel, unsigned long long *d_stats,
                          int grid, hipStream_t stream);
hipError_t mpc_launch_synth(void *d_out, unsigned long long n_lines, unsigned L, int kind, unsigned long long first_line, unsigned long long seed,
                            const uint32_t *d_sine, hipStream_t stream);
hipError_t mpc_launch_read_probe(const void *d_buf, unsigned long long bytes, uint32_t *d_sink, int grid, hipStream_t stream);

// mpc_baselines.hip
hipError_t mpc_launch_baselines(const void *d_lines, unsigned long long n_lines, int L, const MpcBaselinesArgs *A, int grid, hipStream_t stream);

// mpc_vpc_lane.hip (the dispatcher unit, and one unit per line size)
int mpc_vpc_lane_unrolled(const MpcVpcParams *P);
size_t mpc_vpc_lane_ring_plan(const MpcVpcParams *P, unsigned *ring_cfg, int *wpb);
size_t mpc_vpc_lane_smem(const MpcVpcParams *P);
hipError_t mpc_launch_vpc_lane(const void *d_lines, unsigned long long n_lines, const MpcVpcParams *P, uint16_t *d_sizes, int8_t *d_sel,
                               unsigned long long *d_stats, int grid, hipStream_t stream);
hipError_t mpc_launch_vpc_lane_w8(const void *d_lines, unsigned long long n_lines, const MpcVpcParams *P, uint16_t *d_sizes, int8_t *d_sel,
                                  unsigned long long *d_stats, int grid, hipStream_t stream);
hipError_t mpc_launch_vpc_lane_w16(const void *d_lines, unsigned long long n_lines, const MpcVpcParams *P, uint16_t *d_sizes, int8_t *d_sel,
                                   unsigned long long *d_stats, int grid, hipStream_t stream);
hipError_t mpc_launch_vpc_lane_w32(const void *d_lines, unsigned long long n_lines, const MpcVpcParams *P, uint16_t *d_sizes, int8_t *d_sel,
                                   unsigned long long *d_stats, int grid, hipStream_t stream);
hipError_t mpc_launch_vpc_lane_jit(hipFunction_t fn_stats, hipFunction_t fn_lines, const void *d_lines, unsigned long long n_lines,
                                   const MpcVpcParams *P, uint16_t *d_sizes, int8_t *d_sel, unsigned long long *d_stats, int grid,
                                   hipStream_t stream);

// mpc_sc2.hip
hipError_t mpc_launch_sc2_count(const void *d_lines, unsigned long long n_lines, int L, unsigned long long *d_tab, unsigned long long mask,
                                uint16_t *d_sizes, int8_t *d_sel, unsigned long long *d_stats, hipStream_t stream);
hipError_t mpc_launch_sc2_hist(const unsigned long long *d_tab, unsigned long long n_slots, unsigned long long prefix, int shift, uint32_t *d_hist,
                               int grid, hipStream_t stream);
hipError_t mpc_launch_sc2_collect(const unsigned long long *d_tab, unsigned long long n_slots, unsigned long long threshold,
                                  unsigned long long *d_out, uint32_t *d_count, int grid, hipStream_t stream);
hipError_t mpc_launch_sc2_size(const void *d_lines, unsigned long long n_lines, int L, const MpcSc2Table *T, uint16_t *d_sizes, int8_t *d_sel,
                               unsigned long long *d_stats, int grid, hipStream_t stream);

// mpc_pattern.hip
hipError_t mpc_launch_pattern(const void *d_lines, unsigned long long n_lines, int L, uint16_t *d_sizes, int8_t *d_sel,
                              unsigned long long *d_stats, int grid, hipStream_t stream);
hipError_t mpc_launch_pattern_set(const void *d_lines, uint32_t n_lines, int L, const MpcPatternSet *S, unsigned long long *d_stats,
                                  int compare_grid, hipStream_t stream);

// mpc_pattern_evict.hip
hipError_t mpc_launch_pattern_evict(const void *d_lines, uint32_t n_lines, int L, const MpcEvictSet *S, unsigned long long *d_stats,
                                    int compare_grid, int clear_grid, hipStream_t stream);

// mpc_cpack.hip
hipError_t mpc_launch_cpack(const void *d_lines, unsigned long long n_lines, int L, uint16_t *d_sizes, int8_t *d_sel, unsigned long long *d_stats,
                            int grid, hipStream_t stream);

// mpc_cpack_blocks.hip: n_lines lines that begin `pos` lines into a block of block_lines lines (pos < block_lines).  The open
// block's dictionary (MPC_CPACK_STATE_WORDS words) is read from d_state when pos > 0 and written to d_state_out, another array, when
// the launch ends inside a block: launches of one handle must not overlap.  One lane
// per block: the grid is sized for ceil((pos + n_lines) / block_lines) work items of MPC_CPACK_BLOCK_THREADS lanes a workgroup.
#define MPC_CPACK_BLOCK_THREADS 64
#define MPC_CPACK_STATE_WORDS 32      /* 16 entries in ring order, the front, padding */
hipError_t mpc_launch_cpack_blocks(const void *d_lines, unsigned long long n_lines, int L, unsigned long long block_lines, unsigned long long pos,
                                   uint16_t *d_sizes, int8_t *d_sel, unsigned long long *d_stats, const uint32_t *d_state, uint32_t *d_state_out,
                                   int grid, hipStream_t stream);

// mpc_fit.hip: the two Fit analyses (layouts: mpc_fit.h).  `grid` bounds the workgroups of a launch: num_cus x the
// *_wg_per_cu of the line size.  d_base: the residue analysis's base table, L bytes on the device, every entry < L.
int mpc_fit_pairs_wg_per_cu(int L);
hipError_t mpc_launch_fit_pairs(const void *d_lines, unsigned long long n_lines, int L, unsigned long long *d_stats, int grid, hipStream_t stream);
int mpc_fit_residues_wg_per_cu(int L);
hipError_t mpc_launch_fit_residues(const void *d_lines, unsigned long long n_lines, int L, const uint8_t *d_base, unsigned long long *d_stats,
                                   int grid, hipStream_t stream);

// mpc_sizes.hip
int mpc_sizes_wg_per_cu(const MpcSizesArgs *A);
hipError_t mpc_launch_sizes(const MpcSizesArgs *A, unsigned long long n_lines, int grid, hipStream_t stream);

// mpc_classes.hip: the per-class tables of the sizes of n_lines lines (mpc_classes.h); cut into launches as mpc_launch_sizes is
int mpc_classes_wg_per_cu(const MpcClassArgs *A);
hipError_t mpc_launch_classes(const MpcClassArgs *A, unsigned long long n_lines, int grid, hipStream_t stream);

// mpc_pack.hip: the sector histograms of blocks of N lines over the sizes of n_lines lines (mpc_pack.h); one launch, never cut.
// `grid` bounds the workgroups; the launcher sizes them down to the blocks.  The name of the kernel form a block size takes.
const char *mpc_pack_form_name(unsigned long long block_lines);
hipError_t mpc_launch_pack(const MpcPackArgs *A, unsigned long long n_lines, int grid, hipStream_t stream);

// mpc_image.hip: the latest size per line address of n_lines lines into the image's hash map (mpc_image.h); one launch, never cut.
// The get pass: the image's live slots into the block map, then the touched blocks into the sector histogram (two launches).
// `grid` bounds the workgroups; the launchers size them down to the work.
hipError_t mpc_launch_image_update(const MpcImageArgs *A, unsigned long long n_lines, int grid, hipStream_t stream);
hipError_t mpc_launch_image_get(const MpcImageGetArgs *A, int grid, hipStream_t stream);

// mpc_rewrite.hip: the scratch of a sub-batch of at most `lines` lines (its bytes; its arrays carved out of one allocation),
// and the passes of a sub-batch of n_lines <= S->lines (mpc_rewrite.h): keys (keys == 0: only the sums of a further member
// of a group into its dev), the sort, and the sorted sub-batch applied to one map with its handle's sizes (three launches
// and a keyed reduction).  The get pass: one launch over the slots.  `grid` bounds the workgroups.
hipError_t mpc_rewrite_scratch_bytes(unsigned long long lines, size_t *bytes);
hipError_t mpc_rewrite_scratch_carve(void *base, unsigned long long lines, MpcRewriteScratch *S);
hipError_t mpc_launch_rewrite_keys(const MpcRewriteScratch *S, const uint64_t *addrs, const uint16_t *sizes, unsigned long long n_lines, unsigned line_size,
                                   unsigned long long *dev, int keys, int grid, hipStream_t stream);
hipError_t mpc_launch_rewrite_sort(const MpcRewriteScratch *S, unsigned long long n_lines, hipStream_t stream);
hipError_t mpc_launch_rewrite_apply(const MpcRewriteScratch *S, const MpcRewriteMap *M, const uint16_t *sizes, unsigned long long n_lines, hipStream_t stream);
hipError_t mpc_launch_rewrite_get(const MpcRewriteMap *M, int grid, hipStream_t stream);
}
