// mpc_image.h -- the accounting pass that keeps, per distinct line address, the size of the latest line evaluated there
// (mpc_image.hip), next to the size histograms of mpc_sizes.h, the class tables of mpc_classes.h and the pack tables of
// mpc_pack.h.  It reads what the evaluators wrote, 2 bytes per line, and 8 bytes of address per line.
//
// The image is an open-addressing table in device memory: keys[slots] (kMpcImageEmpty: a free slot; no key is all ones,
// a key is address / line_size with line_size >= 4) and vals[slots], slots a power of two >= 2 x capacity.  A key's
// first slot is mpc_image_mix(key) & hash_mask & slot_mask, the chain is linear and wraps.  Slots are claimed with a
// 64-bit compare-and-swap and never freed, so a key has one slot whatever the order of arrival.  A line at position p
// with size s does atomicMax(vals[slot], (p << 16) | s): the latest line wins however the device schedules its lanes
// (2^48 positions cannot be reached, no evaluator writes a size above 65535).
//
// ctl is uint64 [MPC_IMAGE_CTL_LEN]: plain sums (device-scope atomic adds), the claims among them -- the distinct keys
// D, which only grows, so "a new key arrived when D was the capacity" is D > capacity once a launch is complete, which
// the host reads -- and the overflow flag.  The flag is set by the add of claims that takes D past the capacity and by
// a probe that met capacity + 1 taken slots in a row (more keys than the capacity); a wave that reads it set leaves.
// A probe loop of the update is bounded by capacity + 1, one of the get by the block map's slots.
//
// The get pass (two kernels, run only on a get): one over the slots sums the latest sizes and adds each live slot's
// (1 << MPC_IMAGE_COUNT_SHIFT) + size into a second map of the same kind keyed by block = key / N; one over that map
// closes every touched block: T = count, cap = ceil(T L / sector_bytes), sectors = min(max(1, ceil((payload +
// header_bits) / sector_bits)), cap), into an LDS histogram flushed as pack_account_kernel's.  N <= 2^19 keeps the
// count (< 2^20) and the payload (< 2^19 x 2^16) apart in one 64-bit word.
#pragma once
#include <stdint.h>

#define MPC_IMAGE_MAX_SECTORS 1024
#define MPC_IMAGE_MAX_CAPACITY (1ull << 28)
#define MPC_IMAGE_CTL_LINES 0        /* lines evaluated with an address                 */
#define MPC_IMAGE_CTL_BITS 1         /* sum of their sizes                              */
#define MPC_IMAGE_CTL_KEYS 2         /* claims: distinct keys D                         */
#define MPC_IMAGE_CTL_MISALIGNED 3   /* lines whose address was no multiple of L        */
#define MPC_IMAGE_CTL_OVERFLOW 4     /* non-zero: more keys than the capacity           */
#define MPC_IMAGE_CTL_LEN 8
#define MPC_IMAGE_COUNT_SHIFT 40
#define MPC_IMAGE_OUT_LATEST 0       /* sum of the latest sizes                         */
#define MPC_IMAGE_OUT_CAPS 1         /* sum of the touched blocks' caps                 */
#define MPC_IMAGE_OUT_FULL 2         /* non-zero: the block map was full (its sizing excludes that) */
#define MPC_IMAGE_OUT_HIST 4         /* [k - 1]: touched blocks that occupy k sectors   */
#define MPC_IMAGE_OUT_LEN (MPC_IMAGE_OUT_HIST + MPC_IMAGE_MAX_SECTORS)

#define kMpcImageEmpty 0xffffffffffffffffull

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MPC_IMAGE_HD __host__ __device__
#else
#define MPC_IMAGE_HD
#endif

// the hash behind mpc_image_hash (include/mpc_hip_image.h): the 64-bit finaliser of MurmurHash3, a bijection
MPC_IMAGE_HD static inline unsigned long long mpc_image_mix(unsigned long long k)
{
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33;
  k *= 0xc4ceb9fe1a85ec53ull;
  k ^= k >> 33;
  return k;
}

struct MpcImageArgs {
  const uint64_t *addrs;               // [n] device-visible line addresses
  const uint16_t *sizes;               // [n] device (or device-visible) sizes of the same lines
  unsigned long long *keys, *vals;     // [slot_mask + 1]
  unsigned long long *ctl;             // [MPC_IMAGE_CTL_LEN]
  unsigned long long slot_mask;        // slots - 1
  unsigned long long hash_mask;        // all ones; the test library may keep only a few low bits of the hash
  unsigned long long pos;              // the position of the launch's first line
  unsigned long long capacity;         // <= slots / 2
  unsigned long long flush_claims;     // (set by the launcher) a wave adds its claims to ctl once it holds this many
  unsigned line_size;
  int line_shift;                      // line_size == 1 << line_shift, or -1
};

struct MpcImageGetArgs {
  const unsigned long long *keys, *vals;   // the image, [slots]
  unsigned long long slots;
  unsigned long long *bkeys, *bvals;       // the block map, [bmask + 1]; keys all ones, values 0 before the pass
  unsigned long long bmask;
  unsigned long long hash_mask;
  unsigned long long block_lines;          // N
  unsigned long long *out;                 // [MPC_IMAGE_OUT_LEN], zero before the pass
  unsigned line_size, sector_bytes, header_bits;
  unsigned max_sectors;                    // S_B = ceil(N L / sector_bytes), 1 .. MPC_IMAGE_MAX_SECTORS
};
