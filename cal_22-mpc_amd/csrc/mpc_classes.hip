// mpc_classes.hip -- gfx950 kernel of the per-class accounting pass (mpc_classes.h): lines, compressed bits and sector
// counts summed per class byte.  It runs on the stream of the evaluators' launches, directly behind them (and behind
// the size histograms' pass when that is on too), and reads only what they wrote: 2 bytes per line and member, plus
// one class byte per line.
//
// Persistent and grid-stride, the loads of mpc_sizes.hip: a lane takes a chunk of 8 consecutive lines, one 16-byte
// load per member and one 8-byte load of the classes (the last, partial chunk and arrays that are not aligned take
// 2-byte and 1-byte loads, every one bounds-checked).  A wave therefore holds 512 consecutive lines.
//
// A workgroup keeps, per accumulator (a member's table, or the per-line minimum's), [256][kLdsRow] uint32 in LDS:
// the bits and the S sector counts of a class.  The lines of a class are the sum of its sector counts -- every line
// occupies exactly one number of sectors -- so that column is not kept in LDS; the flush forms it.
//
// Real class arrays are long runs of one value (a kernel id rises through a trace; an .npy is class 0 throughout),
// and 64 lanes adding to one LDS address serialise.  Three tiers, cheapest first:
//   * the wave's 512 lines share a class (a ballot of "my 8 class bytes equal the first lane's"): the lanes sum in
//     registers, the wave reduces with DPP shuffles and issues ONE LDS add per column, from 1 + S lanes;
//   * else a lane whose own 8 lines share a class adds its register sums once per column it touched;
//   * else a lane adds line by line.
// No lane waits for another lane, workgroup or kernel; the only barriers are the workgroup's around an LDS flush.
//
// The LDS sums are 32-bit.  The largest is a class's bits: no evaluator writes a size above 4095 bits (mpc_sizes.h:
// the largest is 2240), so it cannot wrap while a workgroup has added fewer than 2^32 / 4095 = 1 048 832 lines.  A
// workgroup takes 256 x 8 = 2048 lines per iteration of its loop and flushes to the uint64 device tables (vector
// atomics, non-zero entries only) every kFlushIters = 512 iterations = 2^20 lines, and at its end.
#include "mpc_kernel_common.h"
#include "mpc_classes.h"
#include "mpc_launch.h"

constexpr int kClassThreads = 256;
constexpr int kLdsRow = 1 + MPC_CLASS_MAX_SECTORS;       // bits, then lines that occupy 1 .. 8 sectors
constexpr int kLdsTable = MPC_CLASS_COUNT * kLdsRow;     // 9 KiB per accumulator; the odd row length spreads the rows over the banks
constexpr u64 kItersPerWg = 8;                           // the launcher sizes the grid for at least this many iterations a workgroup
constexpr u32 kFlushIters = 512;                         // x 2048 lines = 2^20 lines; 4095 x 2^20 < 2^32
static_assert(4095ull * (u64)kFlushIters * kClassThreads * 8ull < (1ull << 32), "a class's bits must fit the 32-bit LDS sum between two flushes");
static_assert(kClassThreads == MPC_CLASS_COUNT, "the flush gives every class one thread");

struct ClassSlots {
  int table[MPC_SIZES_MAX];   // LDS accumulator of member i (-1: none)
  int best;                   // ... of the per-line minimum (-1: none)
};

// what a lane (or, reduced, a wave) has summed for one accumulator: bits, and the sector counts as 16-bit fields
// (sectors 1..4 in lo, 5..8 in hi; a wave holds 512 lines, so no field wraps)
struct ClassAcc {
  u32 bits;
  u64 lo, hi;
};

__device__ __forceinline__ void acc_line(ClassAcc &a, u32 size, u32 sector_bits, u32 max_sectors)
{
  // min(max(1, ceil(size / sector_bits)), S) - 1 without a division: one more sector per multiple of sector_bits exceeded
  u32 s = 0;
#pragma unroll
  for (u32 k = 1; k < MPC_CLASS_MAX_SECTORS; k++) s += (k < max_sectors && size > k * sector_bits) ? 1u : 0u;
  const u64 one = 1ull << (16u * (s & 3u));
  a.bits += size;
  a.lo += s < 4u ? one : 0ull;
  a.hi += s < 4u ? 0ull : one;
}

__device__ __forceinline__ u32 acc_field(const ClassAcc &a, int k)      // k = 0: bits, 1..8: lines in k sectors
{
  return k == 0 ? a.bits : (u32)((k <= 4 ? a.lo >> (16 * (k - 1)) : a.hi >> (16 * (k - 5))) & 0xffffull);
}

// one lane adds its sums to the row of `cls`
__device__ __forceinline__ void lane_add(u32 *tab, u32 cls, const ClassAcc &a)
{
  if ((a.lo | a.hi) == 0ull) return;
  u32 *row = tab + cls * kLdsRow;
  if (a.bits) atomicAdd(&row[0], a.bits);
#pragma unroll
  for (int k = 1; k <= MPC_CLASS_MAX_SECTORS; k++) {
    const u32 v = acc_field(a, k);
    if (v) atomicAdd(&row[k], v);
  }
}

// the whole wave adds its lanes' sums to the row of `cls` (wave-uniform): one LDS add per column
__device__ __forceinline__ void wave_add(u32 *tab, u32 cls, ClassAcc a, int lane)
{
  for (int o = 32; o > 0; o >>= 1) {
    a.bits += __shfl_xor(a.bits, o);
    a.lo += __shfl_xor(a.lo, o);
    a.hi += __shfl_xor(a.hi, o);
  }
  const u32 v = lane < kLdsRow ? acc_field(a, lane) : 0u;
  if (v) atomicAdd(&tab[cls * kLdsRow + (u32)lane], v);
}

// sizes 8c .. 8c+7 of one member, two per dword; `vec`: the array is 16-byte aligned
__device__ __forceinline__ uint4 class_sizes_load8(const uint16_t *__restrict__ p, u64 c, u64 n, bool vec)
{
  const u64 first = c * 8ull;
  if (vec && first + 8ull <= n) return *reinterpret_cast<const uint4 *>(p + first);
  u32 w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int j = 0; j < 8; j++)
    if (first + (u64)j < n) w[j >> 1] |= (u32)p[first + (u64)j] << (16 * (j & 1));
  return make_uint4(w[0], w[1], w[2], w[3]);
}

// class bytes 8c .. 8c+7, byte j in bits 8j; the bytes behind the last line repeat the chunk's first byte, so that
// "all 8 equal" holds for a partial chunk of one class.  `vec`: the array is 8-byte aligned.  p == null: class 0.
__device__ __forceinline__ u64 classes_load8(const uint8_t *__restrict__ p, u64 c, u64 n, bool vec, u32 bias)
{
  if (!p) return 0ull;
  const u64 first = c * 8ull;
  u64 v;
  if (vec && first + 8ull <= n) {
    v = *reinterpret_cast<const u64 *>(p + first);
  } else {
    const u64 b0 = (u64)p[first];        // (the caller has checked first < n)
    v = 0ull;
#pragma unroll
    for (int j = 0; j < 8; j++) v |= (first + (u64)j < n ? (u64)p[first + (u64)j] : b0) << (8 * j);
  }
  if (bias) v = (u64)badd((u32)v, 0x01010101u) | ((u64)badd((u32)(v >> 32), 0x01010101u) << 32);   // selected + 1 per byte
  return v;
}

// a workgroup's LDS sums -> the uint64 device tables, thread t the row of class t; the rows are cleared for the next round
template <int M>
__device__ __forceinline__ void class_flush(const MpcClassArgs &A, const ClassSlots &S, u32 *s_tab, int tid)
{
#pragma unroll
  for (int i = 0; i <= M; i++) {
    const int slot = i < M ? S.table[i] : S.best;
    if (slot < 0) continue;
    u64 *g = (i < M ? A.table[i] : A.best) + (u64)tid * MPC_CLASS_ROW;
    u32 *row = s_tab + slot * kLdsTable + tid * kLdsRow;
    u64 lines = 0ull;
#pragma unroll
    for (int k = 1; k <= MPC_CLASS_MAX_SECTORS; k++) {
      const u32 v = row[k];
      lines += v;
      if (v) {
        atomicAdd(&g[1 + k], (u64)v);
        row[k] = 0u;
      }
    }
    if (lines) atomicAdd(&g[0], lines);
    if (row[0]) {
      atomicAdd(&g[1], (u64)row[0]);
      row[0] = 0u;
    }
  }
}

template <int M>
__global__ void __launch_bounds__(kClassThreads)
classes_account_kernel(MpcClassArgs A, ClassSlots S, int n_acc, u64 n, int vec, int cvec)
{
  extern __shared__ u32 s_tab[];            // [n_acc][kLdsTable]
  for (int i = threadIdx.x; i < n_acc * kLdsTable; i += kClassThreads) s_tab[i] = 0u;
  __syncthreads();

  const int lane = threadIdx.x & 63;
  const bool best = S.best >= 0;
  const u64 n_chunks = (n + 7ull) / 8ull;
  const u64 stride = (u64)gridDim.x * kClassThreads;
  const u32 sector_bits = A.sector_bits, max_sectors = A.max_sectors;
  u32 since = 0u;
  // the loop is uniform over the workgroup (the flush inside it has barriers), so a wave may run an iteration without a chunk
  for (u64 base = (u64)blockIdx.x * kClassThreads; base < n_chunks; base += stride) {
    const u64 c = base + (u64)threadIdx.x;
    const u64 first = c * 8ull;
    const int cnt = first >= n ? 0 : (n - first < 8ull ? (int)(n - first) : 8);
    if (__ballot(cnt != 0) != 0ull) {        // (wave-uniform; chunks are consecutive, so the wave's first lane has one)
      uint4 q[M];
#pragma unroll
      for (int i = 0; i < M; i++) q[i] = cnt ? class_sizes_load8(A.sizes[i], c, n, vec != 0) : make_uint4(0u, 0u, 0u, 0u);
      const u64 c8 = cnt ? classes_load8(A.classes, c, n, cvec != 0, (u32)A.class_bias) : 0ull;
      const u32 lead = (u32)__builtin_amdgcn_readfirstlane((int)(u32)(c8 & 0xffull));
      const bool wave_uniform = __ballot(cnt != 0 && c8 != (u64)lead * 0x0101010101010101ull) == 0ull;
      const bool lane_uniform = c8 == (c8 & 0xffull) * 0x0101010101010101ull;
      ClassAcc acc[M + 1];
#pragma unroll
      for (int i = 0; i <= M; i++) acc[i] = ClassAcc{0u, 0ull, 0ull};
#pragma unroll
      for (int j = 0; j < 8; j++) {
        if (j < cnt) {
          u32 b = 0xffffffffu;
#pragma unroll
          for (int i = 0; i < M; i++) {
            const u32 w = (j >> 1) == 0 ? q[i].x : (j >> 1) == 1 ? q[i].y : (j >> 1) == 2 ? q[i].z : q[i].w;
            const u32 v = (j & 1) ? (w >> 16) : (w & 0xffffu);
            if (S.table[i] >= 0) acc_line(acc[i], v, sector_bits, max_sectors);
            b = min(b, v);
          }
          if (best) acc_line(acc[M], b, sector_bits, max_sectors);
        }
        // mixed wave: a lane of one class adds once, behind its last line; every other lane line by line
        if (!wave_uniform && (!lane_uniform || j == 7)) {
          const u32 cls = (u32)(c8 >> (8 * j)) & 0xffu;
#pragma unroll
          for (int i = 0; i <= M; i++) {
            const int slot = i < M ? S.table[i] : S.best;
            if (slot < 0) continue;
            lane_add(s_tab + slot * kLdsTable, cls, acc[i]);
            acc[i] = ClassAcc{0u, 0ull, 0ull};
          }
        }
      }
      if (wave_uniform) {
#pragma unroll
        for (int i = 0; i <= M; i++) {
          const int slot = i < M ? S.table[i] : S.best;
          if (slot >= 0) wave_add(s_tab + slot * kLdsTable, lead, acc[i], lane);
        }
      }
    }
    if (++since == kFlushIters && base + stride < n_chunks) {
      __syncthreads();
      class_flush<M>(A, S, s_tab, threadIdx.x);
      __syncthreads();
      since = 0u;
    }
  }
  __syncthreads();
  class_flush<M>(A, S, s_tab, threadIdx.x);
}

namespace {

int class_slots(const MpcClassArgs *A, ClassSlots *S)
{
  int n_acc = 0;
  for (int i = 0; i < MPC_SIZES_MAX; i++) S->table[i] = (i < A->m && A->table[i]) ? n_acc++ : -1;
  S->best = A->best ? n_acc++ : -1;
  return n_acc;
}

template <int M>
hipError_t classes_launch(const MpcClassArgs &A, const ClassSlots &S, int n_acc, u64 n, int vec, int cvec, int grid, hipStream_t stream)
{
  const size_t smem = (size_t)n_acc * kLdsTable * sizeof(u32);
  if (smem > (64u << 10))   // more than the default LDS allowance
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&classes_account_kernel<M>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
  hipLaunchKernelGGL(classes_account_kernel<M>, dim3(grid), dim3(kClassThreads), smem, stream, A, S, n_acc, n, vec, cvec);
  return hipGetLastError();
}

}  // namespace

// workgroups of the pass that fit a CU beside each other (their LDS tables), at most 8
extern "C" int mpc_classes_wg_per_cu(const MpcClassArgs *A)
{
  ClassSlots S;
  const int n_acc = class_slots(A, &S);
  if (n_acc == 0) return 0;
  const int fit = (160 * 1024) / (n_acc * kLdsTable * (int)sizeof(u32) + 128);
  return fit > 8 ? 8 : fit;
}

extern "C" hipError_t mpc_launch_classes(const MpcClassArgs *A, u64 n_lines, int grid, hipStream_t stream)
{
  if (A->m < 1 || A->m > MPC_SIZES_MAX || (A->best && A->m < 2) || A->sector_bits == 0 || A->max_sectors < 1 ||
      A->max_sectors > MPC_CLASS_MAX_SECTORS || (A->class_bias != 0 && A->class_bias != 1))
    return hipErrorInvalidValue;
  ClassSlots S;
  const int n_acc = class_slots(A, &S);
  if (n_acc == 0 || n_lines == 0) return hipSuccess;
  int vec = 1;
  for (int i = 0; i < A->m; i++) vec &= (reinterpret_cast<uintptr_t>(A->sizes[i]) & 15u) == 0 ? 1 : 0;
  const int cvec = (reinterpret_cast<uintptr_t>(A->classes) & 7u) == 0 ? 1 : 0;
  const u64 kMaxLines = mpc_launch_cap(1ull << 31);     // per launch, as mpc_launch_sizes cuts (a piece's first line keeps both alignments)
  for (u64 at = 0; at < n_lines; at += kMaxLines) {
    const u64 take = n_lines - at < kMaxLines ? n_lines - at : kMaxLines;
    MpcClassArgs P = *A;
    for (int i = 0; i < A->m; i++) P.sizes[i] = A->sizes[i] + at;
    if (A->classes) P.classes = A->classes + at;
    mpc_count_launch();
    // a workgroup that has work for kItersPerWg iterations takes them: its LDS set-up and its flush -- up to 2560 device
    // atomics, which for a trace of one class all land on the same ten words -- are then paid once per 16 Ki lines
    const u64 chunks = (take + 7) / 8;
    const u64 need = (chunks + kClassThreads * kItersPerWg - 1) / (kClassThreads * kItersPerWg);
    const int g = (int)(need < (u64)(grid < 1 ? 1 : grid) ? need : (u64)(grid < 1 ? 1 : grid));
    hipError_t e;
    switch (A->m) {
    case 1: e = classes_launch<1>(P, S, n_acc, take, vec, cvec, g, stream); break;
    case 2: e = classes_launch<2>(P, S, n_acc, take, vec, cvec, g, stream); break;
    case 3: e = classes_launch<3>(P, S, n_acc, take, vec, cvec, g, stream); break;
    case 4: e = classes_launch<4>(P, S, n_acc, take, vec, cvec, g, stream); break;
    case 5: e = classes_launch<5>(P, S, n_acc, take, vec, cvec, g, stream); break;
    case 6: e = classes_launch<6>(P, S, n_acc, take, vec, cvec, g, stream); break;
    case 7: e = classes_launch<7>(P, S, n_acc, take, vec, cvec, g, stream); break;
    default: e = classes_launch<8>(P, S, n_acc, take, vec, cvec, g, stream); break;
    }
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}
