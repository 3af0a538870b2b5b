// mpc_cpack.hip -- C-Pack with a per-line dictionary (mpc_create_cpack, MPC_CPACK_DICT_PER_LINE): cpack_kernel for
// 32-, 64- and 128-byte lines, cpack_any_kernel for every other line size, and their launcher.  What a line costs
// (cpack_line), the feed and the per-lane accumulator (CpackAcc) are mpc_baselines.h's.  A translation unit of its own,
// like the group's kernel: the kernels of mpc_kernels.hip keep the register allocation they were measured with.
#include "mpc_baselines.h"
#include "mpc_launch.h"

// One lane per line, the line in registers; counts per lane, per-workgroup counts in LDS, one atomic per non-zero
// word at the end (as fpc_kernel).  The lines stream through the one-stage ring of bdi_kernel (ring_feed): measured
// against the staged loads of fpc_kernel / bpc_kernel on one box, ms per 16 GiB, 32-byte random 3.06 -> 2.83, 64-byte
// random 3.76 -> 3.54, mixed 3.66 -> 3.47, all-zero 3.48 -> 3.31, 128-byte pointers 5.70 -> 5.60.
template <int NW>   // words per line: 8, 16 or 32
__global__ void __launch_bounds__(256)
cpack_kernel(const uint4 *__restrict__ lines, u64 n_lines, uint16_t *__restrict__ sizes_out,
             int8_t *__restrict__ sel_out, u64 *gstats)
{
  __shared__ u64 s_counts[MPC_CPACK_RAW_LEN];
  __shared__ __attribute__((aligned(1024))) uint4 s_ring[4 * 64 * (NW / 4)];
  if (threadIdx.x < MPC_CPACK_RAW_LEN) s_counts[threadIdx.x] = 0;
  __syncthreads();
  CpackAcc acc;
  u32 uniform = 0;      // (ring_feed carries a wave-uniform word of its caller's through the group code; none here)
  ring_feed<NW>(lines, n_lines, s_ring, threadIdx.x & 63u, uni(threadIdx.x >> 6), uniform, [&](const u32 (&w)[NW], u64 line, bool active) __attribute__((always_inline)) {
    if (!active) return;
    CpackCounts n = {0, 0, 0, 0, 0};      // this line's counts
    const u32 size = cpack_line<NW>(w, n);
    put_line(sizes_out, sel_out, line, size, 0);
    acc.add(n, size, NW, s_counts);
  });
  acc.flush(s_counts);
  __syncthreads();
  if (threadIdx.x < MPC_CPACK_RAW_LEN && s_counts[threadIdx.x]) atomicAdd(&gstats[threadIdx.x], s_counts[threadIdx.x]);
}

// ---------------------------------------------------------------------------
// Any other line size (a multiple of 4 from 4 to 256 bytes; lines start on a 4-byte boundary): one lane per line and
// the FIFO as CPACK.cpp has it, a ring of 16 words per lane in LDS (entry e of lane t at e * 128 + t: no bank
// conflicts), scanned from the front.  Exact and slow, like baseline_generic_kernel.
// ---------------------------------------------------------------------------
constexpr int kCpackAnyThreads = 128;

__global__ void __launch_bounds__(kCpackAnyThreads)
cpack_any_kernel(const u32 *__restrict__ words, u64 n_lines, int W, uint16_t *__restrict__ sizes_out,
                 int8_t *__restrict__ sel_out, u64 *gstats)
{
  __shared__ u64 s_counts[MPC_CPACK_RAW_LEN];
  __shared__ u32 s_dict[16][kCpackAnyThreads];
  if (threadIdx.x < MPC_CPACK_RAW_LEN) s_counts[threadIdx.x] = 0;
  __syncthreads();
  // bits per pattern in CPACKPattern order (CPACK.h:18-26; m_PatternLength is indexed otherwise), one byte each
  constexpr u64 kBits = 2ull | (12ull << 8) | (6ull << 16) | (16ull << 24) | (24ull << 32) | (34ull << 40);
  for (u64 line = (u64)blockIdx.x * kCpackAnyThreads + threadIdx.x; line < n_lines; line += (u64)gridDim.x * kCpackAnyThreads) {
    const u32 *src = words + line * (u64)W;
    for (int e = 0; e < 16; e++) s_dict[e][threadIdx.x] = 0;
    u32 front = 0, size = 0;
    for (int i = 0; i < W; i++) {
      const u32 v = src[i];
      int pat = 5;
      if ((v & 0xffffffu) == 0u) {
        pat = v == 0u ? 0 : 1;
      } else {
        for (u32 e = 0; e < 16u; e++) {
          const u32 x = s_dict[(front + e) & 15u][threadIdx.x] ^ v;
          if ((x & 0xffffu) != 0u) continue;
          pat = (x & 0xff0000u) ? 4 : (x ? 3 : 2);
          break;
        }
        if (pat == 5) {                                  // pushed at the back, the front entry leaves
          s_dict[front][threadIdx.x] = v;
          front = (front + 1u) & 15u;
        }
      }
      size += (u32)(kBits >> (8 * pat)) & 0xffu;
      atomicAdd(&s_counts[pat], 1ull);
    }
    atomicAdd(&s_counts[6], (u64)size);
    put_line(sizes_out, sel_out, line, size, 0);
  }
  __syncthreads();
  if (threadIdx.x < MPC_CPACK_RAW_LEN && s_counts[threadIdx.x]) atomicAdd(&gstats[threadIdx.x], s_counts[threadIdx.x]);
}

extern "C" hipError_t mpc_launch_cpack(const void *d_lines, u64 n_lines, int L, uint16_t *d_sizes, int8_t *d_sel, u64 *d_stats,
                                       int grid, hipStream_t stream)
{
  if (L < 4 || L > MPC_MAX_LINE || L % 4 != 0) return hipErrorInvalidValue;
  const uint4 *l = static_cast<const uint4 *>(d_lines);
  if (L == 32) hipLaunchKernelGGL(cpack_kernel<8>, dim3(grid), dim3(256), 0, stream, l, n_lines, d_sizes, d_sel, d_stats);
  else if (L == 64) hipLaunchKernelGGL(cpack_kernel<16>, dim3(grid), dim3(256), 0, stream, l, n_lines, d_sizes, d_sel, d_stats);
  else if (L == 128) hipLaunchKernelGGL(cpack_kernel<32>, dim3(grid), dim3(256), 0, stream, l, n_lines, d_sizes, d_sel, d_stats);
  else
    hipLaunchKernelGGL(cpack_any_kernel, dim3(grid), dim3(kCpackAnyThreads), 0, stream, static_cast<const u32 *>(d_lines), n_lines, L / 4,
                       d_sizes, d_sel, d_stats);
  return hipGetLastError();
}
