// mpc_pack.hip -- gfx950 kernel of the pack accounting pass (mpc_pack.h): the sizes of N consecutive lines summed per
// block, the block rounded up to whole sectors once, a histogram of the closed blocks over their sector counts.  It
// runs on the stream of the evaluators' launches, directly behind them (and behind the other two accounting passes
// when they are on too), and reads only what they wrote: 2 bytes per line and member.
//
// Three forms, chosen by N alone (pack_form); all of them persistent and grid-stride over the blocks of the launch,
// all of them with 2-byte loads that are bounds-checked by construction (a block's lines are cut to [0, n)):
//   * lane       N <= 32: a lane owns a whole block, neighbouring lanes neighbouring blocks.  A wave therefore walks
//                64 N consecutive sizes, at most 4 KiB, and every 128-byte line it touches it uses whole.
//   * wave       N <= 511: the 64 lanes of a wave stride one block (lane l reads sizes l, l + 64, ...: 128 consecutive
//                bytes a load) and reduce with DPP shuffles; lane 0 closes the block.
//   * workgroup  larger N: the 256 lanes of a workgroup stride one block, the waves reduce, their first lanes add to an
//                LDS word per accumulator and thread 0 closes the block.  No lane walks a long block alone.
//
// A workgroup keeps, per accumulator (a member's table, or the per-line minimum's), a histogram of max_sectors uint32
// in LDS and flushes the non-zero entries with device-scope uint64 atomic adds at its end.  Blocks of a trace are
// often alike (all of one sector count): in the lane form a wave whose blocks all occupy the same number of sectors
// adds once, from one lane, instead of serialising 64 adds on one LDS word.  The payload is summed in registers
// (uint64), reduced over the wave, then over the workgroup in LDS, and added to the device table once per workgroup.
// What a workgroup sends to the device tables -- one payload and at most max_sectors counts per accumulator -- lands on
// the same few words for every workgroup of a trace whose blocks are alike, and the memory side serialises those adds:
// the caller sizes the grid for kPackRounds rounds of the loop a workgroup, which divides them.
//
// Carries: the thread that owns block 0 adds *carry_in when the launch begins inside a block; the thread that owns the
// last block writes *carry_out instead of closing it when the launch ends inside one.  They are different words, so the
// two threads -- the same one when nothing closes -- need no order between them.
#include "mpc_kernel_common.h"
#include "mpc_pack.h"
#include "mpc_launch.h"

constexpr int kPackThreads = 256;
constexpr int kPackWaves = kPackThreads / 64;

enum PackForm { kPackLane = 0, kPackWave = 1, kPackGroup = 2 };

// what the kernel needs beside MpcPackArgs, worked out once on the host
struct PackGeom {
  u64 n;            // lines of the launch
  u64 nb;           // blocks the launch touches: ceil((pos + n) / N)
  int tail_open;    // the last of them stays open
  int shift;        // sector_bits == 1 << shift, or -1
};

__device__ __forceinline__ u32 pack_sectors(u32 bits, const MpcPackArgs &A, int shift)
{
  // min(max(1, ceil(bits / sector_bits)), S_B); (bits - 1) / sector_bits + 1 cannot wrap
  const u32 s = bits == 0u ? 1u : (shift >= 0 ? ((bits - 1u) >> shift) : (bits - 1u) / A.sector_bits) + 1u;
  return s < A.max_sectors ? s : A.max_sectors;
}

// lines [lo, hi) of block j within the launch
__device__ __forceinline__ void pack_range(const MpcPackArgs &A, const PackGeom &G, u64 j, u64 &lo, u64 &hi)
{
  lo = j == 0ull ? 0ull : j * A.block_lines - A.pos;
  const u64 end = (j + 1ull) * A.block_lines - A.pos;
  hi = end < G.n ? end : G.n;
}

// One thread has block j's sum of accumulator i (i == M: the minimum's): carry in, carry out, or close it into the LDS
// histogram.  `pay` collects the closed payload.  FORM kPackLane: called by every lane of the wave (`have`: this lane
// has a block), so that a wave of like blocks adds once; else by the one thread that holds the sum.
template <int FORM>
__device__ __forceinline__ void pack_close(const MpcPackArgs &A, const PackGeom &G, const u32 *carry_in, u32 *carry_out, u32 header, u32 *s_hist,
                                           u64 j, u32 sum, bool have, u64 &pay)
{
  if (have && j == 0ull && A.pos != 0ull) sum += *carry_in;
  const bool open = have && G.tail_open && j == G.nb - 1ull;
  if (open) *carry_out = sum;
  const bool closes = have && !open;
  const u32 s = pack_sectors(sum + header, A, G.shift) - 1u;
  if (closes) pay += sum;
  if (FORM == kPackLane) {
    const u64 mask = __ballot(closes);
    if (mask == 0ull) return;
    const int first = __ffsll((long long)mask) - 1;
    const u32 lead = (u32)__shfl((int)s, first);
    if (__ballot(closes && s != lead) == 0ull) {
      if ((int)(threadIdx.x & 63) == first) atomicAdd(&s_hist[lead], (u32)__popcll(mask));
    } else if (closes) {
      atomicAdd(&s_hist[s], 1u);
    }
  } else if (closes) {
    atomicAdd(&s_hist[s], 1u);
  }
}

template <int M, int FORM>
__global__ void __launch_bounds__(kPackThreads)
pack_account_kernel(MpcPackArgs A, PackGeom G)
{
  extern __shared__ u64 s_pay[];            // [M + 1] payloads, then [M + 1][max_sectors] histograms, then [M + 1] the workgroup form's sums
  u32 *s_mem = reinterpret_cast<u32 *>(s_pay + (M + 1));
  const u32 S = A.max_sectors;
  u32 *s_team = s_mem + (M + 1) * S;
  for (u32 i = threadIdx.x; i < (M + 1) * S + (M + 1); i += kPackThreads) s_mem[i] = 0u;
  if (threadIdx.x <= M) s_pay[threadIdx.x] = 0ull;
  __syncthreads();

  const int lane = threadIdx.x & 63;
  const bool best = A.best != nullptr;
  u64 pay[M + 1];
#pragma unroll
  for (int i = 0; i <= M; i++) pay[i] = 0ull;

  // the sums of lines lo + first, lo + first + step, ... < hi, per member and of the per-line minimum
  auto walk = [&](u64 lo, u64 hi, u32 first, u32 step, u32 (&sum)[M + 1]) {
#pragma unroll
    for (int i = 0; i <= M; i++) sum[i] = 0u;
    for (u64 k = lo + first; k < hi; k += step) {
      u32 b = 0xffffffffu;
#pragma unroll
      for (int i = 0; i < M; i++) {
        const u32 v = A.sizes[i][k];
        sum[i] += v;
        b = min(b, v);
      }
      sum[M] += b;
    }
  };
  auto close_all = [&](u64 j, const u32 (&sum)[M + 1], bool have) {
#pragma unroll
    for (int i = 0; i < M; i++)
      if (A.table[i]) pack_close<FORM>(A, G, A.carry_in[i], A.carry_out[i], A.header_bits, s_mem + i * S, j, sum[i], have, pay[i]);
    if (best) pack_close<FORM>(A, G, A.best_carry_in, A.best_carry_out, A.best_header_bits, s_mem + M * S, j, sum[M], have, pay[M]);
  };

  if (FORM == kPackLane) {
    // (uniform over the wave: pack_close ballots)
    for (u64 base = (u64)blockIdx.x * kPackThreads; base < G.nb; base += (u64)gridDim.x * kPackThreads) {
      const u64 j = base + threadIdx.x;
      const bool have = j < G.nb;
      u64 lo = 0ull, hi = 0ull;
      if (have) pack_range(A, G, j, lo, hi);
      u32 sum[M + 1];
      walk(lo, hi, 0u, 1u, sum);
      close_all(j, sum, have);
    }
  } else if (FORM == kPackWave) {
    for (u64 j = (u64)blockIdx.x * kPackWaves + (threadIdx.x >> 6); j < G.nb; j += (u64)gridDim.x * kPackWaves) {
      u64 lo, hi;
      pack_range(A, G, j, lo, hi);
      u32 sum[M + 1];
      walk(lo, hi, (u32)lane, 64u, sum);
#pragma unroll
      for (int i = 0; i <= M; i++)
        for (int o = 32; o > 0; o >>= 1) sum[i] += __shfl_xor(sum[i], o);
      close_all(j, sum, lane == 0);
    }
  } else {
    // (uniform over the workgroup: the barriers)
    for (u64 j = blockIdx.x; j < G.nb; j += gridDim.x) {
      u64 lo, hi;
      pack_range(A, G, j, lo, hi);
      u32 sum[M + 1];
      walk(lo, hi, threadIdx.x, (u32)kPackThreads, sum);
#pragma unroll
      for (int i = 0; i <= M; i++) {
        for (int o = 32; o > 0; o >>= 1) sum[i] += __shfl_xor(sum[i], o);
        if (lane == 0 && sum[i]) atomicAdd(&s_team[i], sum[i]);
      }
      __syncthreads();
      if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i <= M; i++) {
          sum[i] = s_team[i];
          s_team[i] = 0u;
        }
      }
      close_all(j, sum, threadIdx.x == 0);
      __syncthreads();
    }
  }

  // the payload: over the wave, then over the workgroup
#pragma unroll
  for (int i = 0; i <= M; i++) {
    u64 p = pay[i];
    for (int o = 32; o > 0; o >>= 1) p += __shfl_xor(p, o);
    if (lane == 0 && p) atomicAdd(&s_pay[i], p);
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i <= M; i++) {
    u64 *g = i < M ? A.table[i] : A.best;
    if (!g) continue;
    if (threadIdx.x == 0 && s_pay[i]) atomicAdd(&g[0], s_pay[i]);
    for (u32 k = threadIdx.x; k < S; k += kPackThreads) {
      const u32 v = s_mem[i * S + k];
      if (v) atomicAdd(&g[1 + k], (u64)v);
    }
  }
}

namespace {

int pack_form(u64 N) { return N <= MPC_PACK_LANE_MAX ? kPackLane : N <= MPC_PACK_WAVE_MAX ? kPackWave : kPackGroup; }

// blocks a workgroup takes per round of its loop, and the rounds the launcher gives a workgroup that has the work for them
u64 pack_blocks_per_wg(int form) { return form == kPackLane ? (u64)kPackThreads : form == kPackWave ? (u64)kPackWaves : 1ull; }
constexpr u64 kPackRounds = 4;

template <int M>
hipError_t pack_launch(const MpcPackArgs &A, const PackGeom &G, int form, int grid, hipStream_t stream)
{
  const size_t smem = (M + 1) * sizeof(u64) + ((size_t)(M + 1) * A.max_sectors + (M + 1)) * sizeof(u32);      // at most 36 KiB
  switch (form) {
  case kPackLane: hipLaunchKernelGGL((pack_account_kernel<M, kPackLane>), dim3(grid), dim3(kPackThreads), smem, stream, A, G); break;
  case kPackWave: hipLaunchKernelGGL((pack_account_kernel<M, kPackWave>), dim3(grid), dim3(kPackThreads), smem, stream, A, G); break;
  default: hipLaunchKernelGGL((pack_account_kernel<M, kPackGroup>), dim3(grid), dim3(kPackThreads), smem, stream, A, G); break;
  }
  return hipGetLastError();
}

}  // namespace

extern "C" const char *mpc_pack_form_name(unsigned long long block_lines)
{
  static const char *const names[] = {"a lane per block", "a wave per block", "a workgroup per block"};
  return names[pack_form(block_lines)];
}

// `grid`: the most workgroups the launch may have (the caller's CUs x workgroups per CU); it is sized down to the blocks
extern "C" hipError_t mpc_launch_pack(const MpcPackArgs *A, u64 n_lines, int grid, hipStream_t stream)
{
  if (A->m < 1 || A->m > MPC_SIZES_MAX || (A->best && A->m < 2) || A->sector_bits == 0 || A->max_sectors < 1 ||
      A->max_sectors > MPC_PACK_MAX_SECTORS || A->block_lines < 1 || A->block_lines > MPC_PACK_MAX_BLOCK_LINES || A->pos >= A->block_lines)
    return hipErrorInvalidValue;
  bool any = A->best != nullptr;
  for (int i = 0; i < A->m; i++) {
    if (!A->sizes[i]) return hipErrorInvalidValue;
    if (A->table[i] && (!A->carry_in[i] || !A->carry_out[i] || A->carry_in[i] == A->carry_out[i])) return hipErrorInvalidValue;
    any = any || A->table[i] != nullptr;
  }
  if (A->best && (!A->best_carry_in || !A->best_carry_out || A->best_carry_in == A->best_carry_out)) return hipErrorInvalidValue;
  if (!any || n_lines == 0) return hipSuccess;
  PackGeom G;
  G.n = n_lines;
  G.nb = (A->pos + n_lines + A->block_lines - 1) / A->block_lines;
  G.tail_open = (A->pos + n_lines) % A->block_lines != 0 ? 1 : 0;
  G.shift = -1;
  for (int b = 0; b < 32; b++)
    if (A->sector_bits == (1u << b)) G.shift = b;
  const int form = pack_form(A->block_lines);
  const u64 per = pack_blocks_per_wg(form) * kPackRounds;
  const u64 need = (G.nb + per - 1) / per;
  const u64 cap = (u64)(grid < 1 ? 1 : grid);
  const int g = (int)(need < cap ? need : cap);      // (lines and blocks are 64-bit in the kernel: a launch is never cut)
  switch (A->m) {
  case 1: return pack_launch<1>(*A, G, form, g, stream);
  case 2: return pack_launch<2>(*A, G, form, g, stream);
  case 3: return pack_launch<3>(*A, G, form, g, stream);
  case 4: return pack_launch<4>(*A, G, form, g, stream);
  case 5: return pack_launch<5>(*A, G, form, g, stream);
  case 6: return pack_launch<6>(*A, G, form, g, stream);
  case 7: return pack_launch<7>(*A, G, form, g, stream);
  default: return pack_launch<8>(*A, G, form, g, stream);
  }
}
