// mpc_image.hip -- gfx950 kernels of the image accounting pass (mpc_image.h): a keyed last-writer-wins update into a
// device hash map behind the evaluators' launches, and the two kernels of a get that close the image into blocks.
//
// Update: persistent, grid-stride over the lines of the launch, a lane per line: 8 bytes of address and 2 bytes of size
// in, one 64-bit compare-and-swap where a key is new, one 64-bit atomic max per line that goes to memory.  A lane whose
// right neighbour in the wave holds the same key stays off the table: the neighbour's line is later, its stamp larger,
// so a run of one address costs one atomic per wave and run instead of 64 on one word.  The three sums (lines, bits,
// misaligned) are kept in registers, reduced over the wave, then over the workgroup in LDS, and added once per workgroup
// (as mpc_pack.hip's payload); the claims are counted per wave and added in lots (below): a count of distinct keys that
// every round of every wave bumped was 2^20 adds to one word for a piece of distinct lines, which the memory side serialises.  What remains are 8-byte device-scope
// atomics to random 64-byte segments; their rate is what the pass costs.
//
// What an overflowing trace may cost is bounded three ways.  A probe gives up after capacity + 1 slots: a run of more
// than `capacity` taken slots means more than `capacity` keys, which is the overflow itself, so the bound is exact and a
// probe never walks a table that filled up.  A wave adds its claims to the device's count whenever `flush_claims` of them
// have gathered (the launcher sizes that so that all waves together hold back at most a quarter of the capacity), and the
// add that passes the capacity sets the overflow flag: the table stays well below full at the capacities where a long
// probe would hurt.  And every wave reads the flag in every 16th round of its loop, the first one included, and leaves
// behind that round when it is set, in this launch and in every later one; a probe that has grown long reads it every 64
// slots and gives up when it is set, so the rounds between two looks stay short too.
//
// All indices are masked with the table's slot mask; lines are read only below n.
#include "mpc_kernel_common.h"
#include "mpc_image.h"
#include "mpc_image_probe.h"      // image_slot: the probe loop, shared with mpc_rewrite.hip
#include "mpc_launch.h"

constexpr int kImageThreads = 256;

__global__ void __launch_bounds__(kImageThreads)
image_update_kernel(MpcImageArgs A, u64 n)
{
  __shared__ u64 s_sum[4];
  if (threadIdx.x < 4) s_sum[threadIdx.x] = 0ull;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  u64 bits = 0ull, lines = 0ull, mis = 0ull;
  u64 claims = 0ull;                             // of the wave, not yet added to the device's count (the same in every lane)
  u32 round = 0u;
  const u64 max_tries = A.capacity < A.slot_mask ? A.capacity + 1ull : A.slot_mask + 1ull;
  // (uniform over the wave: the shuffles, the ballot, the way out)
  for (u64 base = (u64)blockIdx.x * kImageThreads; base < n; base += (u64)gridDim.x * kImageThreads) {
    // (every 16th round: all waves of the device read this one word, and such reads are served one at a time, some 3 ns
    // each -- read in every round they added half to the time of a pass.  Read at the top, looked at at the bottom.)
    u64 over = 0ull;
    if ((round++ & 15u) == 0u) over = __hip_atomic_load(&A.ctl[MPC_IMAGE_CTL_OVERFLOW], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const u64 i = base + threadIdx.x;
    const bool have = i < n;
    u64 key = kMpcImageEmpty;
    u32 size = 0u;
    if (have) {
      const u64 a = A.addrs[i];
      size = A.sizes[i];
      key = A.line_shift >= 0 ? a >> A.line_shift : a / A.line_size;
      mis += a != key * A.line_size ? 1ull : 0ull;
      lines += 1ull;
      bits += size;
    }
    const u64 next = (u64)__shfl_down((long long)key, 1);
    bool claimed = false;
    if (have && (lane == 63 || next != key)) {
      const u64 slot = image_slot(A.keys, A.slot_mask, A.hash_mask, key, max_tries, &A.ctl[MPC_IMAGE_CTL_OVERFLOW], &claimed);
      if (slot == kMpcImageEmpty) atomicOr(&A.ctl[MPC_IMAGE_CTL_OVERFLOW], 1ull);
      else atomicMax(&A.vals[slot], ((A.pos + i) << 16) | (u64)size);
    }
    claims += (u64)__popcll(__ballot(claimed));
    if (claims >= A.flush_claims) {
      if (lane == 0 && atomicAdd(&A.ctl[MPC_IMAGE_CTL_KEYS], claims) + claims > A.capacity) atomicOr(&A.ctl[MPC_IMAGE_CTL_OVERFLOW], 1ull);
      claims = 0ull;
    }
    if (__any(over != 0ull)) break;              // the handle is finished: what the table holds no longer counts
  }
  for (int o = 32; o > 0; o >>= 1) {
    bits += __shfl_xor(bits, o);
    lines += __shfl_xor(lines, o);
    mis += __shfl_xor(mis, o);
  }
  if (lane == 0) {
    if (lines) atomicAdd(&s_sum[0], lines);
    if (bits) atomicAdd(&s_sum[1], bits);
    if (mis) atomicAdd(&s_sum[2], mis);
    if (claims) atomicAdd(&s_sum[3], claims);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    if (s_sum[0]) atomicAdd(&A.ctl[MPC_IMAGE_CTL_LINES], s_sum[0]);
    if (s_sum[1]) atomicAdd(&A.ctl[MPC_IMAGE_CTL_BITS], s_sum[1]);
    if (s_sum[2]) atomicAdd(&A.ctl[MPC_IMAGE_CTL_MISALIGNED], s_sum[2]);
    if (s_sum[3] && atomicAdd(&A.ctl[MPC_IMAGE_CTL_KEYS], s_sum[3]) + s_sum[3] > A.capacity) atomicOr(&A.ctl[MPC_IMAGE_CTL_OVERFLOW], 1ull);
  }
}

// get, first kernel: the live slots of the image into the block map, and the sum of the latest sizes
__global__ void __launch_bounds__(kImageThreads)
image_blocks_kernel(MpcImageGetArgs A)
{
  __shared__ u64 s_latest;
  if (threadIdx.x == 0) s_latest = 0ull;
  __syncthreads();
  u64 latest = 0ull;
  for (u64 i = (u64)blockIdx.x * kImageThreads + threadIdx.x; i < A.slots; i += (u64)gridDim.x * kImageThreads) {
    const u64 key = A.keys[i];
    if (key == kMpcImageEmpty) continue;
    const u64 size = A.vals[i] & 0xffffull;
    latest += size;
    bool claimed = false;
    const u64 slot = image_slot(A.bkeys, A.bmask, A.hash_mask, key / A.block_lines, A.bmask + 1ull, nullptr, &claimed);
    if (slot == kMpcImageEmpty) {
      atomicOr(&A.out[MPC_IMAGE_OUT_FULL], 1ull);
      continue;
    }
    atomicAdd(&A.bvals[slot], (1ull << MPC_IMAGE_COUNT_SHIFT) + size);
  }
  for (int o = 32; o > 0; o >>= 1) latest += __shfl_xor(latest, o);
  if ((threadIdx.x & 63) == 0 && latest) atomicAdd(&s_latest, latest);
  __syncthreads();
  if (threadIdx.x == 0 && s_latest) atomicAdd(&A.out[MPC_IMAGE_OUT_LATEST], s_latest);
}

// get, second kernel: every touched block closed into the workgroup's LDS histogram
__global__ void __launch_bounds__(kImageThreads)
image_close_kernel(MpcImageGetArgs A)
{
  __shared__ u32 s_hist[MPC_IMAGE_MAX_SECTORS];
  __shared__ u64 s_caps;
  const u32 S = A.max_sectors;
  for (u32 k = threadIdx.x; k < S; k += kImageThreads) s_hist[k] = 0u;
  if (threadIdx.x == 0) s_caps = 0ull;
  __syncthreads();
  const u64 sector_bits = 8ull * A.sector_bytes;
  u64 caps = 0ull;
  for (u64 i = (u64)blockIdx.x * kImageThreads + threadIdx.x; i <= A.bmask; i += (u64)gridDim.x * kImageThreads) {
    if (A.bkeys[i] == kMpcImageEmpty) continue;
    const u64 v = A.bvals[i];
    const u64 T = v >> MPC_IMAGE_COUNT_SHIFT, payload = v & ((1ull << MPC_IMAGE_COUNT_SHIFT) - 1ull);
    const u64 cap = (T * A.line_size + A.sector_bytes - 1ull) / A.sector_bytes;     // 1 .. S: T is 1 .. N
    u64 s = (payload + A.header_bits + sector_bits - 1ull) / sector_bits;
    s = s < 1ull ? 1ull : s;
    s = s < cap ? s : cap;
    s = s < (u64)S ? s : (u64)S;                                                    // (cap <= S; keeps the LDS index in range whatever the map holds)
    caps += cap;
    atomicAdd(&s_hist[s - 1ull], 1u);
  }
  for (int o = 32; o > 0; o >>= 1) caps += __shfl_xor(caps, o);
  if ((threadIdx.x & 63) == 0 && caps) atomicAdd(&s_caps, caps);
  __syncthreads();
  if (threadIdx.x == 0 && s_caps) atomicAdd(&A.out[MPC_IMAGE_OUT_CAPS], s_caps);
  for (u32 k = threadIdx.x; k < S; k += kImageThreads) {
    const u32 v = s_hist[k];
    if (v) atomicAdd(&A.out[MPC_IMAGE_OUT_HIST + k], (u64)v);
  }
}

namespace {
bool pow2(u64 v) { return v && !(v & (v - 1ull)); }
int grid_of(u64 work, int grid)
{
  const u64 need = (work + kImageThreads - 1) / kImageThreads;
  const u64 cap = (u64)(grid < 1 ? 1 : grid);
  return (int)(need < cap ? need : cap);
}
}  // namespace

// `grid`: the most workgroups the launch may have; it is sized down to the lines (lines are 64-bit in the kernel: a launch is never cut)
extern "C" hipError_t mpc_launch_image_update(const MpcImageArgs *A, u64 n_lines, int grid, hipStream_t stream)
{
  if (!A->addrs || !A->sizes || !A->keys || !A->vals || !A->ctl || !pow2(A->slot_mask + 1ull) || A->slot_mask + 1ull < 2ull || A->capacity == 0 ||
      A->capacity > (A->slot_mask + 1ull) / 2ull || A->line_size == 0 || (A->line_shift >= 0 && A->line_size != (1u << A->line_shift)))
    return hipErrorInvalidValue;
  if (n_lines == 0) return hipSuccess;
  const int g = grid_of(n_lines, grid);
  MpcImageArgs B = *A;
  // all waves of the launch together hold back at most capacity / 4 claims (and the up to 63 of a round that passes the mark)
  const u64 share = A->capacity / (4ull * (u64)g * (kImageThreads / 64));
  B.flush_claims = share < 1ull ? 1ull : share > 1024ull ? 1024ull : share;
  hipLaunchKernelGGL(image_update_kernel, dim3(g), dim3(kImageThreads), 0, stream, B, n_lines);
  return hipGetLastError();
}

extern "C" hipError_t mpc_launch_image_get(const MpcImageGetArgs *A, int grid, hipStream_t stream)
{
  if (!A->keys || !A->vals || !A->bkeys || !A->bvals || !A->out || !pow2(A->slots) || !pow2(A->bmask + 1ull) || A->block_lines == 0 ||
      A->block_lines > (1ull << 19) || A->line_size == 0 || A->sector_bytes == 0 || A->max_sectors < 1 || A->max_sectors > MPC_IMAGE_MAX_SECTORS)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(image_blocks_kernel, dim3(grid_of(A->slots, grid)), dim3(kImageThreads), 0, stream, *A);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(image_close_kernel, dim3(grid_of(A->bmask + 1ull, grid)), dim3(kImageThreads), 0, stream, *A);
  return hipGetLastError();
}
