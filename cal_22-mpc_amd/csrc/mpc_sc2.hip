// mpc_sc2.hip -- gfx950 kernels of SC2 (reference src/compressor/SC2.cpp), a Huffman code over the line's 32-bit
// words whose table is built once, after a warm-up sample:
//
//   sc2_count_kernel    warm-up lines: exact frequencies of their words in a device hash table
//   sc2_hist_kernel /   selection of the 1024 largest (count, symbol) pairs (a radix select over the 64-bit slots)
//   sc2_collect_kernel
//   sc2_size_kernel     every later line: per-word code length from the table in LDS (the hot path)
//
// Hash table (global memory).  One uint64 slot per distinct word: count << 32 | word.  A slot is empty while its
// count is 0, so every 32-bit key, 0 and 0xFFFFFFFF included, is a valid word.  Counts are summed into the high half
// with a 64-bit atomic add (the key in the low half never changes once a slot is claimed by compare-and-swap).  The
// C ABI sizes it to the next power of two >= 2 S W slots (S warm-up lines of W words: at most S W distinct words, so
// the load stays <= 1/2 and linear probing always ends) and bounds S W <= 2^28 (a table of at most 4 GiB; every
// count < 2^32).  The slot value orders exactly as the reference's (freq, symbol) key (huffman::cmp), so the kept set
// is the 1024 largest nonzero slots.
//
// Warm-up traces are zero-heavy: a workgroup first aggregates its 4096 words in an LDS table of 8192 slots, so an
// all-zero sample sends one atomic per workgroup, not one per word, to the zero word's slot.
#include "mpc_kernel_common.h"
#include "mpc_sc2.h"
#include "mpc_launch.h"

constexpr int kCountThreads = 256;
constexpr int kCountWords = 4096;             // words per workgroup
constexpr int kCountSlots = 2 * kCountWords;  // LDS slots (64 KiB)

__device__ __forceinline__ void sc2_lds_add(u64 *s, u32 k, u64 c)
{
  u32 i = mpc_sc2_hash(k, 0u) & (kCountSlots - 1);
  for (int probe = 0; probe < kCountSlots; probe++) {
    u64 v = s[i];
    if (v == 0ull) {
      v = atomicCAS(&s[i], 0ull, (c << 32) | k);
      if (v == 0ull) return;
    }
    if ((u32)v == k) {
      atomicAdd(&s[i], c << 32);
      return;
    }
    i = (i + 1) & (kCountSlots - 1);
  }
}

__device__ __forceinline__ void sc2_global_add(u64 *tab, u64 mask, u32 k, u64 c)
{
  u64 i = (u64)mpc_sc2_hash(k, 0x5C2u) & mask;
  for (u64 probe = 0; probe <= mask; probe++) {
    u64 v = __hip_atomic_load(&tab[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (v == 0ull) {
      v = atomicCAS(&tab[i], 0ull, (c << 32) | k);
      if (v == 0ull) return;
    }
    if ((u32)v == k) {
      atomicAdd(&tab[i], c << 32);
      return;
    }
    i = (i + 1) & mask;
  }
}

// n_lines warm-up lines of W words (4-byte aligned): count their words, write their sizes (W x 33 bits against the
// empty table, SC2.cpp:316-330) and selected = 0, add their bits to the raw statistics
__global__ void __launch_bounds__(kCountThreads)
sc2_count_kernel(const u32 *__restrict__ words, u64 n_lines, int W, u64 *tab, u64 mask, uint16_t *__restrict__ sizes_out,
                 int8_t *__restrict__ sel_out, u64 *gstats)
{
  __shared__ u64 s_slot[kCountSlots];
  for (int i = threadIdx.x; i < kCountSlots; i += kCountThreads) s_slot[i] = 0ull;
  __syncthreads();
  const u64 n_words = n_lines * (u64)W;
  const u64 w0 = (u64)blockIdx.x * kCountWords;
#pragma unroll 4
  for (int j = 0; j < kCountWords / kCountThreads; j++) {
    const u64 idx = w0 + (u64)j * kCountThreads + threadIdx.x;
    if (idx < n_words) sc2_lds_add(s_slot, words[idx], 1ull);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kCountSlots; i += kCountThreads) {
    const u64 v = s_slot[i];
    if (v) sc2_global_add(tab, mask, (u32)v, v >> 32);
  }
  const u64 gid = (u64)blockIdx.x * kCountThreads + threadIdx.x, gsz = (u64)gridDim.x * kCountThreads;
  for (u64 line = gid; line < n_lines; line += gsz) {
    if (sizes_out) sizes_out[line] = (uint16_t)(MPC_SC2_MISS_BITS * W);
    if (sel_out) sel_out[line] = 0;
  }
  if (gid == 0) atomicAdd(&gstats[0], n_lines * (u64)W * MPC_SC2_MISS_BITS);
}

// radix select: histogram of the 8-bit digit at `shift` over the nonzero slots whose bits above it equal `prefix`
__global__ void __launch_bounds__(256)
sc2_hist_kernel(const u64 *__restrict__ tab, u64 n_slots, u64 prefix, int shift, u32 *hist)
{
  __shared__ u32 s_h[256];
  s_h[threadIdx.x] = 0;
  __syncthreads();
  for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < n_slots; i += (u64)gridDim.x * 256) {
    const u64 v = tab[i];
    if (v != 0ull && (shift >= 56 || (v >> (shift + 8)) == prefix)) atomicAdd(&s_h[(v >> shift) & 255u], 1u);
  }
  __syncthreads();
  if (s_h[threadIdx.x]) atomicAdd(&hist[threadIdx.x], s_h[threadIdx.x]);
}

// every nonzero slot >= threshold (at most MPC_SC2_ENTRIES of them by construction; bounds-checked anyway)
__global__ void __launch_bounds__(256)
sc2_collect_kernel(const u64 *__restrict__ tab, u64 n_slots, u64 threshold, u64 *out, u32 *count)
{
  for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < n_slots; i += (u64)gridDim.x * 256) {
    const u64 v = tab[i];
    if (v != 0ull && v >= threshold) {
      const u32 at = atomicAdd(count, 1u);
      if (at < MPC_SC2_ENTRIES) out[at] = v;
    }
  }
}

// ---------------------------------------------------------------------------
// Sizing (SC2.cpp:316-330): per word the code length when the word is in the table, else 33 bits.  Persistent and
// grid-stride: a workgroup copies the bucket image into LDS once.  Each lane reads 16 B (4 words) of the trace, so
// LPL = L/16 consecutive lanes hold one line and sum their sizes with cross-lane adds; the first of them writes the
// line's size.  Statistics: per lane in registers, one atomic per workgroup and raw word at the end.
// ---------------------------------------------------------------------------
__device__ __forceinline__ u32 sc2_probe(uint4 b, u32 k, bool &hit)
{
  const u32 c = b.w >> 30;
  hit = true;
  if (c > 0u && b.x == k) return b.w & 1023u;
  if (c > 1u && b.y == k) return (b.w >> 10) & 1023u;
  if (c > 2u && b.z == k) return (b.w >> 20) & 1023u;
  hit = false;
  return MPC_SC2_MISS_BITS;
}

__device__ __forceinline__ u32 sc2_word_bits(const uint4 *s_tab, const MpcSc2Table &T, u32 k, u32 &found)
{
  const uint4 b = s_tab[mpc_sc2_hash(k, T.seed1) & T.mask];
  bool hit;
  u32 len = sc2_probe(b, k, hit);
  if (!hit && (b.w >> 30) == 3u) len = sc2_probe(s_tab[mpc_sc2_hash(k, T.seed2) & T.mask], k, hit);   // first bucket full
  found += hit ? 1u : 0u;
  return len;
}

__device__ __forceinline__ void sc2_load_table(uint4 *s_tab, const MpcSc2Table &T)
{
  const uint4 *g = static_cast<const uint4 *>(T.buckets);
  for (u32 i = threadIdx.x; i <= T.mask; i += blockDim.x) s_tab[i] = g[i];
  __syncthreads();
}

__device__ __forceinline__ void sc2_flush(u64 bits, u64 found, u64 *s_red, u64 *gstats)
{
  for (int o = 32; o > 0; o >>= 1) {
    bits += __shfl_xor(bits, o);
    found += __shfl_xor(found, o);
  }
  const int wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    s_red[2 * wave] = bits;
    s_red[2 * wave + 1] = found;
  }
  __syncthreads();
  if (threadIdx.x < MPC_SC2_RAW_LEN) {
    u64 t = 0;
    for (int w = 0; w < waves; w++) t += s_red[2 * w + threadIdx.x];
    if (t) atomicAdd(&gstats[threadIdx.x], t);
  }
}

constexpr int kSizeThreads = 256;
constexpr int kSizeUnroll = 4;     // 16-B loads in flight per lane

template <int LPL>   // lanes per line = L / 16
__global__ void __launch_bounds__(kSizeThreads)
sc2_size_kernel(const uint4 *__restrict__ lines, u64 n_lines, MpcSc2Table T, uint16_t *__restrict__ sizes_out,
                int8_t *__restrict__ sel_out, u64 *gstats)
{
  extern __shared__ uint4 s_tab[];
  __shared__ u64 s_red[2 * (kSizeThreads / 64)];
  sc2_load_table(s_tab, T);
  const u64 n_chunks = n_lines * LPL;
  const u64 step = (u64)gridDim.x * kSizeThreads * kSizeUnroll;
  u64 bits = 0, found = 0;
  const bool leader = (threadIdx.x & (LPL - 1)) == 0;
  for (u64 base = (u64)blockIdx.x * kSizeThreads * kSizeUnroll; base < n_chunks; base += step) {
    uint4 q[kSizeUnroll];
#pragma unroll
    for (int u = 0; u < kSizeUnroll; u++) {
      const u64 c = base + (u64)u * kSizeThreads + threadIdx.x;
      q[u] = c < n_chunks ? lines[c] : make_uint4(0u, 0u, 0u, 0u);
    }
#pragma unroll
    for (int u = 0; u < kSizeUnroll; u++) {
      const u64 c = base + (u64)u * kSizeThreads + threadIdx.x;
      const bool in = c < n_chunks;
      u32 f = 0;
      u32 s = sc2_word_bits(s_tab, T, q[u].x, f) + sc2_word_bits(s_tab, T, q[u].y, f) +
              sc2_word_bits(s_tab, T, q[u].z, f) + sc2_word_bits(s_tab, T, q[u].w, f);
      if (!in) { s = 0; f = 0; }
      bits += s;
      found += f;
#pragma unroll
      for (int o = 1; o < LPL; o <<= 1) s += __shfl_xor(s, o);      // the line's lanes are aligned groups of LPL
      if (in && leader) {
        const u64 line = c / LPL;
        if (sizes_out) sizes_out[line] = (uint16_t)s;
        if (sel_out) sel_out[line] = 1;
      }
    }
  }
  sc2_flush(bits, found, s_red, gstats);
}

// line sizes that are not a multiple of 16 bytes: one lane per line, 4-byte loads
__global__ void __launch_bounds__(kSizeThreads)
sc2_size_any_kernel(const u32 *__restrict__ words, u64 n_lines, int W, MpcSc2Table T, uint16_t *__restrict__ sizes_out,
                    int8_t *__restrict__ sel_out, u64 *gstats)
{
  extern __shared__ uint4 s_tab[];
  __shared__ u64 s_red[2 * (kSizeThreads / 64)];
  sc2_load_table(s_tab, T);
  u64 bits = 0, found = 0;
  for (u64 line = (u64)blockIdx.x * kSizeThreads + threadIdx.x; line < n_lines; line += (u64)gridDim.x * kSizeThreads) {
    u32 s = 0, f = 0;
    for (int i = 0; i < W; i++) s += sc2_word_bits(s_tab, T, words[line * (u64)W + (u64)i], f);
    bits += s;
    found += f;
    if (sizes_out) sizes_out[line] = (uint16_t)s;
    if (sel_out) sel_out[line] = 1;
  }
  sc2_flush(bits, found, s_red, gstats);
}

extern "C" hipError_t mpc_launch_sc2_count(const void *d_lines, u64 n_lines, int L, u64 *d_tab, u64 mask, uint16_t *d_sizes,
                                           int8_t *d_sel, u64 *d_stats, hipStream_t stream)
{
  const int W = L / 4;
  const u64 blocks = (n_lines * (u64)W + kCountWords - 1) / kCountWords;
  if (blocks == 0) return hipSuccess;
  hipLaunchKernelGGL(sc2_count_kernel, dim3((unsigned)blocks), dim3(kCountThreads), 0, stream, static_cast<const u32 *>(d_lines),
                     n_lines, W, d_tab, mask, d_sizes, d_sel, d_stats);
  return hipGetLastError();
}

extern "C" hipError_t mpc_launch_sc2_hist(const u64 *d_tab, u64 n_slots, u64 prefix, int shift, u32 *d_hist, int grid,
                                          hipStream_t stream)
{
  hipLaunchKernelGGL(sc2_hist_kernel, dim3(grid), dim3(256), 0, stream, d_tab, n_slots, prefix, shift, d_hist);
  return hipGetLastError();
}

extern "C" hipError_t mpc_launch_sc2_collect(const u64 *d_tab, u64 n_slots, u64 threshold, u64 *d_out, u32 *d_count, int grid,
                                             hipStream_t stream)
{
  hipLaunchKernelGGL(sc2_collect_kernel, dim3(grid), dim3(256), 0, stream, d_tab, n_slots, threshold, d_out, d_count);
  return hipGetLastError();
}

extern "C" hipError_t mpc_launch_sc2_size(const void *d_lines, u64 n_lines, int L, const MpcSc2Table *T, uint16_t *d_sizes,
                                          int8_t *d_sel, u64 *d_stats, int grid, hipStream_t stream)
{
  const size_t smem = ((size_t)T->mask + 1) * sizeof(uint4);
  const uint4 *l = static_cast<const uint4 *>(d_lines);
  switch (L) {
  case 16: hipLaunchKernelGGL(sc2_size_kernel<1>, dim3(grid), dim3(kSizeThreads), smem, stream, l, n_lines, *T, d_sizes, d_sel, d_stats); break;
  case 32: hipLaunchKernelGGL(sc2_size_kernel<2>, dim3(grid), dim3(kSizeThreads), smem, stream, l, n_lines, *T, d_sizes, d_sel, d_stats); break;
  case 64: hipLaunchKernelGGL(sc2_size_kernel<4>, dim3(grid), dim3(kSizeThreads), smem, stream, l, n_lines, *T, d_sizes, d_sel, d_stats); break;
  case 128: hipLaunchKernelGGL(sc2_size_kernel<8>, dim3(grid), dim3(kSizeThreads), smem, stream, l, n_lines, *T, d_sizes, d_sel, d_stats); break;
  case 256: hipLaunchKernelGGL(sc2_size_kernel<16>, dim3(grid), dim3(kSizeThreads), smem, stream, l, n_lines, *T, d_sizes, d_sel, d_stats); break;
  default:
    hipLaunchKernelGGL(sc2_size_any_kernel, dim3(grid), dim3(kSizeThreads), smem, stream, static_cast<const u32 *>(d_lines), n_lines,
                       L / 4, *T, d_sizes, d_sel, d_stats);
    break;
  }
  return hipGetLastError();
}
