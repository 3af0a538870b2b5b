// mpc_cpack_blocks.hip -- C-Pack with a dictionary shared by blocks of N lines (mpc_create_cpack_blocks): cpack_block_kernel
// and its launcher.  A translation unit of its own: the kernels of mpc_cpack.hip keep the register allocation they were
// measured with.  The nested counts and the per-lane accumulator (cpack_count, CpackAcc) are mpc_baselines.h's.
#include "mpc_baselines.h"
#include "mpc_launch.h"

// ---------------------------------------------------------------------------
// One lane per block, consecutive lanes of a wave on consecutive blocks; a lane walks the words of its lines in trace
// order.  A launch of n lines that begins `pos` lines into a block (pos < N) has ceil((pos + n) / N) blocks: block 0 is
// the open one (N - pos lines at most; its dictionary comes from `state` when pos > 0), block j > 0 begins at line
// j N - pos with 16 zero entries, and the lane of the last block leaves its dictionary in `state_out` when the launch
// ends inside it (another array than `state`: the first and the last lane of a launch run in no order).  A state is the
// 16 entries in ring order, then the front.
//
// The FIFO is a ring of 16 words per lane in LDS (entry e of lane t at e * 64 + t: no bank conflicts) with the front in
// a register.  The scan needs no order: pushed entries that are still in the FIFO have pairwise different keys (a word is
// pushed only when no entry has its key), the zero entries are all equal, and a key-0 word is pushed only when no zero
// entry is left -- every entry that matches a word's key is the same word, so all 16 are read from fixed addresses and
// whichever matches decides (what "the first from the front" comes to in CPACK.cpp:40-84).
//
// The lines reach the lanes through per-lane loads: 4-byte loads up to the first 16-byte boundary and after the last,
// 16-byte loads between, four of them (64 bytes) in flight ahead of the words they feed.  Line, word and byte offsets
// are 64-bit (a batch may pass 2^32 bytes, a block 2^32 lines).  Counts per lane in registers (CpackAcc), per-workgroup
// counts in LDS, one atomic per non-zero word per workgroup at the end, as cpack_kernel.
// ---------------------------------------------------------------------------
constexpr int kCpackBlockThreads = MPC_CPACK_BLOCK_THREADS;

struct CpackBlockLane {
  u32 (*dict)[kCpackBlockThreads];
  u32 front, W, wi;
  u64 line;
  CpackCounts n;
  CpackAcc acc;
  uint16_t *sizes_out;
  int8_t *sel_out;
  u64 *s_counts;

  __device__ __forceinline__ void word(u32 v)
  {
    const u32 t = threadIdx.x;
    const bool zzz = (v & 0xffffffu) == 0u;
    u32 m = ~v;                                          // (no entry with this key: the XOR below has a key part)
    if (!zzz) {
#pragma unroll
      for (int e = 0; e < 16; e++) {
        const u32 ent = dict[e][t];
        m = ((ent ^ v) & 0xffffu) == 0u ? ent : m;
      }
    }
    const u32 y = m ^ v;
    const bool hit = !zzz && (y & 0xffffu) == 0u;
    cpack_count(v, zzz, hit, y >> 16, n);
    if (!zzz && !hit) {                                  // pushed at the back, the front entry leaves
      dict[front][t] = v;
      front = (front + 1u) & 15u;
    }
    if (++wi == W) {                                     // the line is complete
      const u32 size = 34u * W - 22u * n.a - 10u * n.b - 10u * n.c - 8u * n.d - 10u * n.e;
      put_line(sizes_out, sel_out, line, size, 0);
      acc.add(n, size, W, s_counts);
      n = CpackCounts{0, 0, 0, 0, 0};
      wi = 0;
      line++;
    }
  }
  __device__ __forceinline__ void quad(const uint4 &q) { word(q.x); word(q.y); word(q.z); word(q.w); }
};

__global__ void __launch_bounds__(kCpackBlockThreads)
cpack_block_kernel(const u32 *__restrict__ words, u64 n_lines, u32 W, u64 N, u64 pos, u64 n_blocks, uint16_t *__restrict__ sizes_out,
                   int8_t *__restrict__ sel_out, u64 *gstats, const u32 *__restrict__ state, u32 *__restrict__ state_out)
{
  __shared__ u64 s_counts[MPC_CPACK_RAW_LEN];
  __shared__ u32 s_dict[16][kCpackBlockThreads];
  if (threadIdx.x < MPC_CPACK_RAW_LEN) s_counts[threadIdx.x] = 0;
  __syncthreads();
  const u32 t = threadIdx.x;
  CpackBlockLane lane;
  lane.dict = s_dict;
  lane.W = W;
  lane.sizes_out = sizes_out;
  lane.sel_out = sel_out;
  lane.s_counts = s_counts;
  lane.n = CpackCounts{0, 0, 0, 0, 0};
  for (u64 j = (u64)blockIdx.x * kCpackBlockThreads + t; j < n_blocks; j += (u64)gridDim.x * kCpackBlockThreads) {
    const u64 first = j ? j * N - pos : 0ull;
    const u64 stop = (j + 1ull) * N - pos;
    const u64 end = stop < n_lines ? stop : n_lines;
    const bool resume = j == 0ull && pos != 0ull;        // the open block: its dictionary as the launch before left it
#pragma unroll
    for (int e = 0; e < 16; e++) s_dict[e][t] = resume ? state[e] : 0u;
    lane.front = resume ? state[16] & 15u : 0u;
    lane.wi = 0;
    lane.line = first;
    const u32 *p = words + first * (u64)W;
    const u32 *const pend = words + end * (u64)W;
    while (p < pend && ((uintptr_t)p & 15u)) lane.word(*p++);
    if ((u64)(pend - p) >= 16ull) {
      const uint4 *q = reinterpret_cast<const uint4 *>(p);
      uint4 a0 = q[0], a1 = q[1], a2 = q[2], a3 = q[3];
      p += 16;
      while ((u64)(pend - p) >= 16ull) {                 // the next 64 bytes are on their way while these are walked
        q = reinterpret_cast<const uint4 *>(p);
        const uint4 b0 = q[0], b1 = q[1], b2 = q[2], b3 = q[3];
        p += 16;
        lane.quad(a0); lane.quad(a1); lane.quad(a2); lane.quad(a3);
        a0 = b0; a1 = b1; a2 = b2; a3 = b3;
      }
      lane.quad(a0); lane.quad(a1); lane.quad(a2); lane.quad(a3);
    }
    for (; (u64)(pend - p) >= 4ull; p += 4) lane.quad(*reinterpret_cast<const uint4 *>(p));
    while (p < pend) lane.word(*p++);
    if (j == n_blocks - 1ull && stop > n_lines) {        // the launch ends inside this block
#pragma unroll
      for (int e = 0; e < 16; e++) state_out[e] = s_dict[e][t];
      state_out[16] = lane.front;
    }
  }
  lane.acc.flush(s_counts);
  __syncthreads();
  if (threadIdx.x < MPC_CPACK_RAW_LEN && s_counts[threadIdx.x]) atomicAdd(&gstats[threadIdx.x], s_counts[threadIdx.x]);
}

extern "C" hipError_t mpc_launch_cpack_blocks(const void *d_lines, u64 n_lines, int L, u64 block_lines, u64 pos, uint16_t *d_sizes, int8_t *d_sel,
                                              u64 *d_stats, const uint32_t *d_state, uint32_t *d_state_out, int grid, hipStream_t stream)
{
  if (L < 4 || L > MPC_MAX_LINE || L % 4 != 0 || block_lines == 0 || pos >= block_lines || !d_state || !d_state_out || d_state == d_state_out) return hipErrorInvalidValue;
  if (n_lines == 0) return hipSuccess;
  const u64 n_blocks = (pos + n_lines + block_lines - 1ull) / block_lines;
  hipLaunchKernelGGL(cpack_block_kernel, dim3(grid), dim3(kCpackBlockThreads), 0, stream, static_cast<const u32 *>(d_lines), n_lines, (u32)(L / 4),
                     block_lines, pos, n_blocks, d_sizes, d_sel, d_stats, d_state, d_state_out);
  return hipGetLastError();
}
