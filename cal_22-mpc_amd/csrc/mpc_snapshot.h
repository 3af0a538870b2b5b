// mpc_snapshot.h -- a snapshot of the memory that a trace touched (mpc_snapshot.hip, include/mpc_hip_snapshot.h): per
// distinct unit address the BYTES of the latest unit added there, where image accounting (mpc_image.h) keeps a size.
//
// The table is image accounting's open-addressing map with a payload: keys[slots] (kMpcImageEmpty: a free slot),
// stamp[slots] and payload[slots x U], slots a power of two >= 2 x capacity -- 16 + U bytes per slot.  A key's first slot
// is mpc_image_mix(key) & hash_mask & slot_mask, the chain is linear and wraps, slots are claimed with a 64-bit
// compare-and-swap and never freed.  A unit at position p does atomicMax(stamp[slot], p + 1) in the stamp kernel; the copy
// kernel, behind the kernel boundary, copies the unit whose p + 1 the stamp holds: one unit per key and launch, so no two
// lanes write the same bytes, and launches are ordered by their stream.  unit_slot[] carries the slot from the first
// kernel to the second (kMpcSnapNoSlot: a unit that a later one of the same wave overrides, or a failed probe).
//
// ctl is uint64 [MPC_SNAP_CTL_LEN]: the claims (distinct keys D, which only grows: a new key beyond the capacity is
// D > capacity once a launch is complete), the misaligned units and the overflow flag, all as mpc_image.h's.
//
// Plan and write: the live (key, slot) pairs are gathered, sorted by key (rocPRIM), and kept until the next add.  For a
// line size L = k U the mark kernel finds every unit that begins a line (key / k differs from its left neighbour's),
// counts touched and complete lines and the units of partial ones, and flags the lines that are emitted; an exclusive
// scan of the flags numbers them, the heads kernel writes heads[j] = the sorted index of emitted line j's first unit.
// The gather kernel writes emitted lines [first, first + n): 16 bytes per lane, from the payload or zero.
#pragma once
#include <stdint.h>

#include "mpc_image.h"

#define MPC_SNAP_MAX_CAPACITY (1ull << 28)
#define MPC_SNAP_MAX_LINE 256
#define MPC_SNAP_CTL_KEYS 0          /* claims: distinct keys D                         */
#define MPC_SNAP_CTL_MISALIGNED 1    /* units whose address was no multiple of U        */
#define MPC_SNAP_CTL_OVERFLOW 2      /* non-zero: more keys than the capacity           */
#define MPC_SNAP_CTL_LEN 8
#define MPC_SNAP_PLAN_TOUCHED 0      /* the mark kernel's sums                          */
#define MPC_SNAP_PLAN_COMPLETE 1
#define MPC_SNAP_PLAN_PARTIAL_UNITS 2
#define MPC_SNAP_PLAN_LEN 4
#define kMpcSnapNoSlot 0xffffffffu

struct MpcSnapAddArgs {
  const uint8_t *units;                // [n x U] device-visible, 16-byte aligned
  const uint64_t *addrs;               // [n]
  unsigned long long *keys, *stamp;    // [slot_mask + 1]
  uint8_t *payload;                    // [(slot_mask + 1) x U]
  uint32_t *unit_slot;                 // [n] scratch: kernel 1 writes it, kernel 2 reads it
  unsigned long long *ctl;             // [MPC_SNAP_CTL_LEN]
  unsigned long long slot_mask, hash_mask, pos, capacity;
  unsigned long long flush_claims;     // (set by the launcher) as MpcImageArgs'
  unsigned unit_bytes;                 // 32, 64 or 128
  int unit_shift;                      // unit_bytes == 1 << unit_shift
};

struct MpcSnapLinesArgs {
  const unsigned long long *skeys;     // [D] the live keys, ascending
  const uint32_t *sslot;               // [D] their slots
  unsigned long long D;
  uint32_t *flags;                     // [D] mark: 1 where an emitted line begins
  const uint32_t *index;               // [D] the exclusive scan of flags
  uint32_t *heads;                     // [n_out]
  unsigned long long *plan;            // [MPC_SNAP_PLAN_LEN], zero before the mark kernel
  const uint8_t *payload;
  unsigned unit_bytes, k;              // L = k x unit_bytes, k in {1, 2, 4, 8}
  int zero_fill;                       // partial = zero: every touched line is emitted
  // the gather kernel: emitted lines [first, first + n)
  unsigned long long first, n;
  uint8_t *lines_out;                  // [n x L], 16-byte aligned
  uint64_t *addrs_out;                 // [n] or null
  uint8_t *presence_out;               // [n] or null
};

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
extern "C" {
// `grid`: the most workgroups a launch may have; each launcher sizes it down to its work.  All kernels stride.
hipError_t mpc_launch_snapshot_add(const MpcSnapAddArgs *A, unsigned long long n, int grid, hipStream_t stream);
hipError_t mpc_launch_snapshot_compact(const unsigned long long *keys, unsigned long long slots, unsigned long long *okeys, uint32_t *oslot,
                                       unsigned long long cap, unsigned long long *counter, int grid, hipStream_t stream);
hipError_t mpc_launch_snapshot_mark(const MpcSnapLinesArgs *A, int grid, hipStream_t stream);
hipError_t mpc_launch_snapshot_heads(const MpcSnapLinesArgs *A, int grid, hipStream_t stream);
hipError_t mpc_launch_snapshot_gather(const MpcSnapLinesArgs *A, int grid, hipStream_t stream);
}

// What mpc_snapshot_evaluate (mpc_capi.hip) needs of a snapshot: the plan of (line_size, partial) and pieces of the
// emitted lines in the snapshot's scratch buffer, written on the snapshot's stream.  MPC_OK or an MPC_E_* code with the
// message in mpc_snapshot_last_error(s).
struct mpc_snapshot;
int mpc_snapshot_piece_lines();      // the most lines of a piece (4 Mi)
int mpc_snapshot_piece(mpc_snapshot *s, unsigned line_size, int partial, unsigned long long first, unsigned long long n, const void **d_lines,
                       const uint64_t **d_addrs, const uint8_t **d_presence, void **stream);
int mpc_snapshot_device_of(const mpc_snapshot *s);
int mpc_snapshot_fail(mpc_snapshot *s, int code, const char *msg);
#endif
