// mpc_fit.hip -- the two Fit analyses (mpc_create_fit_pairs, mpc_create_fit_residues): what fit.py needs to fit a
// DiffBase module's BaseIndexTable and DiffTable to a trace.  Layouts and constants: mpc_fit.h.  Neither kernel has a
// per-line result and neither keeps state across lines: all counters are integer sums.
#include "mpc_kernel_common.h"
#include "mpc_fit.h"
#include "mpc_launch.h"

// ---------------------------------------------------------------------------
// Pair table: for every byte pair (i, j) of a line the bit length of (line[i] - line[j]) & 255.
//
// Lanes own pairs, not lines.  Lane j of a wave holds byte j of the wave's current line; byte i reaches every lane as a
// wave-uniform value (v_readlane_b32 into an SGPR), so a pair costs no memory access.  Per pair: with X2 = 2 x_j (per
// line) and XI2 = 2 x_i + 1 (scalar), d = (XI2 - X2) & 0x1ff = 2 ((x_i - x_j) & 255) + 1 is never zero and one bit
// longer than the residue; 210 - 7 clz(d) = 7 (k - 1) is the position of bin k's 7-bit field in the pair's 64-bit
// counter, and for k = 0 it is -7 = 57 mod 64, inside the eight unused top bits, which overflow off the top.
// Two instructions to d, v_ffbh, a multiply-add, a 64-bit shift and a 64-bit add.
//
// A wave's unit of work is a chunk of MPC_FIT_SPILL_LINES consecutive lines per counter; behind it the wave adds its
// fields into the workgroup's uint32 table in LDS ([row][bin][j]: the lanes of a ds_add are neighbours) and starts from
// zero, so no field passes 127.  The workgroup flushes the table with one uint64 atomic per non-zero entry at its end.
//   L = 64:  64 rows x 1 byte per lane = 64 counters (128 VGPRs); a wave takes one line per step.
//   L = 128: 16384 pairs do not fit a wave.  A workgroup takes a quarter of the rows (32 rows x 2 bytes per lane = 64
//            counters) and every line; the four quarters are workgroups b, b + 1, b + 2, b + 3.
//   L = 32:  32 rows x 1 byte per lane; lanes 0-31 take the even lines of the chunk and lanes 32-63 the odd ones, so a
//            step is two lines: both rows' bytes are packed into one scalar and a lane shifts its own down.
// The table is 128 KiB (32 KiB at L = 32): one workgroup of four waves per CU, one wave per SIMD.  The next step's
// bytes are loaded before the current step's pairs are counted.
// ---------------------------------------------------------------------------
template <int L> struct FitPairGeom {
  static constexpr int NI = L == 64 ? 64 : 32;      // rows a workgroup counts
  static constexpr int NJ = L == 128 ? 2 : 1;       // bytes of a line per lane
  static constexpr int LPW = L == 32 ? 2 : 1;       // lines per wave step
  static constexpr int PARTS = L == 128 ? 4 : 1;    // workgroups that share a line's rows
  static constexpr u32 TABLE = (u32)NI * MPC_FIT_PAIR_BINS * L;   // uint32 entries in LDS
};

template <int L>
__global__ void __launch_bounds__(MPC_FIT_PAIR_THREADS)
fit_pairs_kernel(const uint8_t *__restrict__ lines, u64 n_lines, u64 *g)
{
  using G = FitPairGeom<L>;
  constexpr int NI = G::NI, NJ = G::NJ, LPW = G::LPW, PARTS = G::PARTS;
  constexpr int WAVES = MPC_FIT_PAIR_THREADS / 64;
  extern __shared__ u32 s_fit[];      // [NI][8][L]
  for (u32 e = threadIdx.x; e < G::TABLE; e += MPC_FIT_PAIR_THREADS) s_fit[e] = 0;
  __syncthreads();
  const u32 lane = threadIdx.x & 63u;
  const u32 wave = (u32)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const u32 part = PARTS > 1 ? blockIdx.x % (u32)PARTS : 0u;      // rows [part NI, part NI + NI)
  const u64 group = blockIdx.x / (u32)PARTS, groups = gridDim.x / (u32)PARTS;      // (the grid is a multiple of PARTS)
  const u32 half = LPW == 2 ? lane >> 5 : 0u;                     // L = 32: which line of the step
  const u32 sh16 = half * 16u;
  constexpr u64 CHUNK = (u64)MPC_FIT_SPILL_LINES * LPW;
  const u64 n_chunks = (n_lines + CHUNK - 1) / CHUNK;
  for (u64 c = group * WAVES + wave; c < n_chunks; c += groups * WAVES) {
    const u64 first = c * CHUNK;
    const u32 cnt = (u32)(n_lines - first < CHUNK ? n_lines - first : CHUNK);      // lines of this chunk
    const u32 steps = (cnt + LPW - 1) / LPW;
    const uint8_t *p = lines + first * (u64)L + lane;      // L = 32: lane = 32 half + j, the step's two lines are 64 bytes
    u64 acc[NI][NJ];
#pragma unroll
    for (int ii = 0; ii < NI; ii++)
#pragma unroll
      for (int n = 0; n < NJ; n++) acc[ii][n] = 0;
    u32 nx[NJ];
    {
      const bool live = half < cnt;       // (cnt >= 1)
#pragma unroll
      for (int n = 0; n < NJ; n++) nx[n] = live ? (u32)p[64 * n] : 0u;
    }
    for (u32 t = 0; t < steps; t++) {
      const bool active = t * LPW + half < cnt;
      u32 x[NJ];
#pragma unroll
      for (int n = 0; n < NJ; n++) x[n] = nx[n];
      if (t + 1 < steps) {      // the next step's bytes
        const bool live = (t + 1) * LPW + half < cnt;
        const uint8_t *q = p + (u64)(t + 1) * (LPW * L);
#pragma unroll
        for (int n = 0; n < NJ; n++) nx[n] = live ? (u32)q[64 * n] : 0u;
      }
      const u64 one = active ? 1ull : 0ull;
      u32 x2[NJ];
#pragma unroll
      for (int n = 0; n < NJ; n++) x2[n] = x[n] << 1;
      // the register that holds this workgroup's rows, and the lane of row 0 in it
      const u32 rows = (L == 128 && part >= 2u) ? x[NJ - 1] : x[0];
      const u32 row0 = L == 128 ? (part & 1u) * 32u : 0u;
#pragma unroll
      for (int ii = 0; ii < NI; ii++) {
        u32 xi2;
        if (LPW == 2) {
          const u32 a = (u32)__builtin_amdgcn_readlane((int)rows, ii), b = (u32)__builtin_amdgcn_readlane((int)rows, 32 + ii);
          xi2 = (((a << 1) | 1u) | (((b << 1) | 1u) << 16)) >> sh16;      // (bits 9.. are masked below)
        } else {
          xi2 = ((u32)__builtin_amdgcn_readlane((int)rows, (int)(row0 + (u32)ii)) << 1) | 1u;
        }
#pragma unroll
        for (int n = 0; n < NJ; n++) {
          const u32 d = (xi2 - x2[n]) & 0x1ffu;
          const u32 sh = 210u - 7u * (u32)__builtin_clz(d);
          acc[ii][n] += one << (sh & 63u);
        }
      }
    }
    // the chunk's fields into the workgroup's table
#pragma unroll
    for (int ii = 0; ii < NI; ii++)
#pragma unroll
      for (int n = 0; n < NJ; n++) {
        const u32 j = LPW == 2 ? (lane & 31u) : lane + 64u * (u32)n;
#pragma unroll
        for (int b = 0; b < MPC_FIT_PAIR_BINS; b++)
          atomicAdd(&s_fit[(u32)(ii * MPC_FIT_PAIR_BINS + b) * (u32)L + j], (u32)(acc[ii][n] >> (7 * b)) & 127u);
      }
  }
  __syncthreads();
  u64 *out = g + 1 + (u64)part * G::TABLE;
  for (u32 e = threadIdx.x; e < G::TABLE; e += MPC_FIT_PAIR_THREADS) {
    const u32 v = s_fit[e];
    if (v) atomicAdd(&out[e], (u64)v);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&g[0], n_lines);
}

// ---------------------------------------------------------------------------
// Residue histogram for a base table: one lane per byte, grid-stride over the bytes of the launch with a stride that is
// a multiple of L, so a lane keeps its column i and the distance to its base byte.  Two byte loads (the second hits the
// line the first fetched), one ds_add into the workgroup's [256][L] uint32 histogram (lanes are neighbours for equal
// residues), flushed with uint64 atomics at the end.  32, 64 or 128 KiB of LDS.
// ---------------------------------------------------------------------------
template <int L>
__global__ void __launch_bounds__(MPC_FIT_RES_THREADS)
fit_residues_kernel(const uint8_t *__restrict__ lines, u64 n_lines, const uint8_t *__restrict__ base, u64 *g)
{
  static_assert(MPC_FIT_RES_THREADS % L == 0, "a lane keeps its column");
  constexpr u32 TABLE = 256u * L;
  extern __shared__ u32 s_fit[];      // [256][L]
  for (u32 e = threadIdx.x; e < TABLE; e += MPC_FIT_RES_THREADS) s_fit[e] = 0;
  __syncthreads();
  const u32 i = threadIdx.x % (u32)L;
  const long long off = (long long)base[i] - (long long)i;      // base[i] < L: the base byte is in the same line
  const u64 total = n_lines * (u64)L, stride = (u64)gridDim.x * MPC_FIT_RES_THREADS;
  u64 at = (u64)blockIdx.x * MPC_FIT_RES_THREADS + threadIdx.x;
  for (; at < total && total - at > 3 * stride; at += 4 * stride) {
    u32 r[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const uint8_t *q = lines + at + (u64)k * stride;
      r[k] = ((u32)q[0] - (u32)q[off]) & 255u;
    }
#pragma unroll
    for (int k = 0; k < 4; k++) atomicAdd(&s_fit[r[k] * (u32)L + i], 1u);
  }
  for (; at < total; at += stride) {
    const uint8_t *q = lines + at;
    atomicAdd(&s_fit[(((u32)q[0] - (u32)q[off]) & 255u) * (u32)L + i], 1u);
  }
  __syncthreads();
  for (u32 e = threadIdx.x; e < TABLE; e += MPC_FIT_RES_THREADS) {
    const u32 v = s_fit[e];
    if (v) atomicAdd(&g[1 + e], (u64)v);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&g[0], n_lines);
}

// ---------------------------------------------------------------------------
// launchers.  A launch takes at most MPC_FIT_LAUNCH_LINES lines (a workgroup's uint32 LDS counters); `grid` is the
// caller's bound on the workgroups that are resident at once.
// ---------------------------------------------------------------------------
template <int L>
static hipError_t launch_pairs(const uint8_t *lines, u64 n_lines, u64 *d_stats, int grid, hipStream_t stream)
{
  using G = FitPairGeom<L>;
  const size_t smem = (size_t)G::TABLE * sizeof(u32);
  if (smem > (64u << 10))
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&fit_pairs_kernel<L>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
  const u64 cap = mpc_launch_cap(MPC_FIT_LAUNCH_LINES);
  for (u64 at = 0; at < n_lines; at += cap) {
    const u64 take = n_lines - at < cap ? n_lines - at : cap;
    const u64 chunks = (take + (u64)MPC_FIT_SPILL_LINES * G::LPW - 1) / ((u64)MPC_FIT_SPILL_LINES * G::LPW);
    const u64 need = (chunks + 3) / 4;      // four waves a workgroup
    u64 groups = (u64)(grid > G::PARTS ? grid / G::PARTS : 1);
    if (groups > need) groups = need;
    mpc_count_launch();
    hipLaunchKernelGGL(fit_pairs_kernel<L>, dim3((unsigned)(groups * G::PARTS)), dim3(MPC_FIT_PAIR_THREADS), smem, stream, lines + at * (u64)L, take,
                       d_stats);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

extern "C" int mpc_fit_pairs_wg_per_cu(int L) { return L == 32 ? 4 : 1; }

extern "C" hipError_t mpc_launch_fit_pairs(const void *d_lines, u64 n_lines, int L, u64 *d_stats, int grid, hipStream_t stream)
{
  const uint8_t *l = static_cast<const uint8_t *>(d_lines);
  if (L == 32) return launch_pairs<32>(l, n_lines, d_stats, grid, stream);
  if (L == 64) return launch_pairs<64>(l, n_lines, d_stats, grid, stream);
  if (L == 128) return launch_pairs<128>(l, n_lines, d_stats, grid, stream);
  return hipErrorInvalidValue;
}

template <int L>
static hipError_t launch_residues(const uint8_t *lines, u64 n_lines, const uint8_t *d_base, u64 *d_stats, int grid, hipStream_t stream)
{
  const size_t smem = 256u * (size_t)L * sizeof(u32);
  if (smem > (64u << 10))
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&fit_residues_kernel<L>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
  const u64 cap = mpc_launch_cap(MPC_FIT_LAUNCH_LINES);
  for (u64 at = 0; at < n_lines; at += cap) {
    const u64 take = n_lines - at < cap ? n_lines - at : cap;
    const u64 need = (take * (u64)L + 4ull * MPC_FIT_RES_THREADS - 1) / (4ull * MPC_FIT_RES_THREADS);      // four bytes a lane
    const u64 blocks = need < (u64)grid ? need : (u64)(grid > 0 ? grid : 1);
    mpc_count_launch();
    hipLaunchKernelGGL(fit_residues_kernel<L>, dim3((unsigned)blocks), dim3(MPC_FIT_RES_THREADS), smem, stream, lines + at * (u64)L, take, d_base,
                       d_stats);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

extern "C" int mpc_fit_residues_wg_per_cu(int L) { return L == 32 ? 2 : 1; }

extern "C" hipError_t mpc_launch_fit_residues(const void *d_lines, u64 n_lines, int L, const uint8_t *d_base, u64 *d_stats, int grid,
                                              hipStream_t stream)
{
  const uint8_t *l = static_cast<const uint8_t *>(d_lines);
  if (L == 32) return launch_residues<32>(l, n_lines, d_base, d_stats, grid, stream);
  if (L == 64) return launch_residues<64>(l, n_lines, d_base, d_stats, grid, stream);
  if (L == 128) return launch_residues<128>(l, n_lines, d_base, d_stats, grid, stream);
  return hipErrorInvalidValue;
}
