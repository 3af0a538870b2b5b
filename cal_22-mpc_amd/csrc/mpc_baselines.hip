// mpc_baselines.hip -- baselines_kernel, the kernel of a group of handles (mpc_capi.hip) whose members are BDI, FPC
// and BPC, and its launcher.  A translation unit of its own, apart from the kernels of a single handle
// (mpc_kernels.hip): compiled in one unit with them, fpc_kernel<32> and bpc_kernel<32> came out with one more VGPR
// each.  What a line costs, the two feeds and the per-lane accumulators are mpc_baselines.h's, the
// same code as theirs.
#include "mpc_baselines.h"
#include "mpc_launch.h"

// ---------------------------------------------------------------------------
// BDI, FPC and BPC in one pass: the three map a line the same way -- one lane per
// line, the line in registers -- and each has little arithmetic behind the load, so the line is loaded once and every
// member of the launch (MASK: bit 0 BDI, bit 1 FPC, bit 2 BPC; at least two) is evaluated on the same registers.
// How the lines reach the lanes was picked by measurement (ms per 16 GiB with all three members): at
// 32 and 64 bytes the one-stage ring of bdi_kernel (random 7.13 against 7.61, mixed 7.33 against 7.96), at 128 bytes
// the transposed coalesced non-temporal loads of fpc_kernel / bpc_kernel (pointers 7.33 against 8.18).  BDI as in
// bdi_kernel: at 32 and 64 bytes, exact scans that only a few lines of a group need are queued and run later, 64
// queued lines at a time (without that the sine trace took 11.8 ms, more than the three solo launches together);
// which scans run for the whole wave is a routing choice, a line's result does not depend on it.
// Each member's per-line outputs and raw statistics are its
// own and laid out as its own kernel's: per-workgroup counts in LDS, one atomic per non-zero word at the end.
// ---------------------------------------------------------------------------
template <int NW, int MASK>   // words per line: 8, 16 or 32
__global__ void __launch_bounds__(256)
baselines_kernel(const uint4 *__restrict__ lines, u64 n_lines, MpcBaselinesArgs A)
{
  constexpr bool BDI = (MASK & 1) != 0, FPC = (MASK & 2) != 0, BPC = (MASK & 4) != 0;
  constexpr bool RING = NW <= 16;            // how the lines reach the lanes: see above
  constexpr bool DEFER = BDI && NW <= 16;    // BDI scans that few lines of a group need are queued, as in bdi_kernel
  __shared__ u32 s_queue[DEFER ? 4 : 1][DEFER ? kBdiQueue : 1];
  __shared__ u64 s_bdi[MPC_BDI_RAW_LEN], s_fpc[MPC_FPC_RAW_LEN], s_bpc[MPC_BPC_RAW_LEN];
  __shared__ __attribute__((aligned(1024))) uint4 s_stage[4][64 * (NW / 4)];
  if (threadIdx.x < MPC_BDI_RAW_LEN) {
    s_bdi[threadIdx.x] = 0;
    if (threadIdx.x < MPC_FPC_RAW_LEN) s_fpc[threadIdx.x] = s_bpc[threadIdx.x] = 0;
  }
  __syncthreads();
  const u32 lane = threadIdx.x & 63u;
  const u32 wave = uni(threadIdx.x >> 6);
  // (test library: the BDI member's route counters sit behind its raw statistics, as for bdi_kernel)
  BdiLane bdi = {A.bdi.sizes, A.bdi.sel, s_bdi, s_queue[DEFER ? wave : 0u], (MPC_TESTING && BDI) ? A.bdi.raw + MPC_BDI_RAW_LEN : nullptr};
  const bool can_defer = n_lines <= kBdiDeferMaxLines;      // queue entries are 32-bit line indices
  FpcAcc fpc;
  BpcAcc bpc;
  // every member on one line held in w (every lane stays in: bdi_line votes across the wave)
  auto evaluate = [&](const u32 (&w)[NW], u64 line, bool active) __attribute__((always_inline)) {
    if (FPC && active) {
      FpcCounts n = {0, 0, 0, 0, 0, 0, 0, 0};
      const u32 size = fpc_line<NW>(w, n);
      put_line(A.fpc.sizes, A.fpc.sel, line, size, 0);
      fpc.add(n, size, NW, s_fpc);
    }
    if (BPC && active) {
      const u32 length = bpc_line<NW>(w, bpc.even, bpc.odd);
      put_line(A.bpc.sizes, A.bpc.sel, line, length, 0);
      bpc.add(length, s_bpc);
    }
    if (BDI) bdi.group<NW, DEFER>(lines, lane, w, line, active, can_defer);
  };
  if constexpr (RING) ring_feed<NW>(lines, n_lines, s_stage[0], lane, wave, bdi.qn, evaluate);
  else staged_feed<NW>(lines, n_lines, s_stage[wave], lane, evaluate);
  if (DEFER) bdi.drain<NW>(lines, lane);
  if (BDI) bdi.flush();
  if (FPC) fpc.flush(s_fpc);
  if (BPC) bpc.flush(s_bpc);
  __syncthreads();
  if (BDI && threadIdx.x < MPC_BDI_RAW_LEN && s_bdi[threadIdx.x]) atomicAdd(&A.bdi.raw[threadIdx.x], s_bdi[threadIdx.x]);
  if (FPC && threadIdx.x < MPC_FPC_RAW_LEN && s_fpc[threadIdx.x]) atomicAdd(&A.fpc.raw[threadIdx.x], s_fpc[threadIdx.x]);
  if (BPC && threadIdx.x < MPC_BPC_RAW_LEN && s_bpc[threadIdx.x]) atomicAdd(&A.bpc.raw[threadIdx.x], s_bpc[threadIdx.x]);
}

// The group's launch for BDI / FPC / BPC members (raw != NULL) of 32-, 64- or 128-byte lines, at least two of them.
template <int NW>
static void launch_baselines(int mask, int grid, hipStream_t stream, const uint4 *l, u64 n_lines, const MpcBaselinesArgs &A)
{
  switch (mask) {
  case 3: hipLaunchKernelGGL((baselines_kernel<NW, 3>), dim3(grid), dim3(256), 0, stream, l, n_lines, A); break;
  case 5: hipLaunchKernelGGL((baselines_kernel<NW, 5>), dim3(grid), dim3(256), 0, stream, l, n_lines, A); break;
  case 6: hipLaunchKernelGGL((baselines_kernel<NW, 6>), dim3(grid), dim3(256), 0, stream, l, n_lines, A); break;
  default: hipLaunchKernelGGL((baselines_kernel<NW, 7>), dim3(grid), dim3(256), 0, stream, l, n_lines, A); break;
  }
}

extern "C" hipError_t mpc_launch_baselines(const void *d_lines, u64 n_lines, int L, const MpcBaselinesArgs *A, int grid, hipStream_t stream)
{
  const int mask = (A->bdi.raw ? 1 : 0) | (A->fpc.raw ? 2 : 0) | (A->bpc.raw ? 4 : 0);
  if ((mask & (mask - 1)) == 0 || (L != 32 && L != 64 && L != 128)) return hipErrorInvalidValue;   // fewer than two members
  const uint4 *l = static_cast<const uint4 *>(d_lines);
  if (L == 32) launch_baselines<8>(mask, grid, stream, l, n_lines, *A);
  else if (L == 64) launch_baselines<16>(mask, grid, stream, l, n_lines, *A);
  else launch_baselines<32>(mask, grid, stream, l, n_lines, *A);
  return hipGetLastError();
}
