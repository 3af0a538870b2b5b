// mpc_rewrite.hip -- gfx950 kernels of the rewrite accounting pass (mpc_rewrite.h): per sub-batch a keys kernel, a stable
// sort of (key, position), a kernel over the sorted elements that counts the transitions inside runs of one key, one
// keyed reduction that gives every run its largest size, length and first element, and a kernel with a lane per run
// that applies the run to the handle's map; and the one kernel of a get.
//
// Nothing here depends on how the device schedules its threads: the sort is stable, so a run lists a key's sizes in
// trace order; the transitions inside a run are sums; a key has exactly one lane in the apply kernel, which alone reads
// and writes the key's value; sub-batches are ordered by their stream or by the host's event chain.
//
// Bounds: the sorted indices are a permutation of 0 .. n - 1, so sizes[idx] stays below n; a run's first element and
// length come out of the reduction and are clamped to n before they index anything; class indices are clamped to
// 1 .. G <= 32 before they index LDS; slots are masked with the table's slot mask.
#include <cstring>      // (before rocPRIM: one of its iterator headers uses memcpy without including this)
#include <rocprim/rocprim.hpp>

#include "mpc_kernel_common.h"
#include "mpc_image_probe.h"
#include "mpc_rewrite.h"
#include "mpc_launch.h"

constexpr int kRewriteThreads = 256;
constexpr int kRewriteG = MPC_REWRITE_MAX_CLASSES;

// c(s) = min(max(1, ceil(s / (8 g))), G), as an index 0 .. G - 1
__device__ __forceinline__ u32 rewrite_class(u32 size, u32 granule_bits, u32 classes)
{
  u32 c = (size + granule_bits - 1u) / granule_bits;
  c = c < 1u ? 1u : c;
  c = c < classes ? c : classes;
  return c - 1u;
}

// the reduction's word: (largest size << 48) | (length << 24) | first element
struct RewriteRunOp {
  __host__ __device__ __forceinline__ unsigned long long operator()(unsigned long long a, unsigned long long b) const
  {
    const unsigned long long sa = a >> 48, sb = b >> 48;
    const unsigned long long la = (a >> 24) & 0xffffffull, lb = (b >> 24) & 0xffffffull;
    const unsigned long long fa = a & 0xffffffull, fb = b & 0xffffffull;
    return ((sa > sb ? sa : sb) << 48) | (((la + lb) & 0xffffffull) << 24) | (fa < fb ? fa : fb);
  }
};

__global__ void __launch_bounds__(kRewriteThreads)
rewrite_keys_kernel(const uint64_t *addrs, const uint16_t *sizes, u64 n, u32 line_size, int line_shift, u64 *keys, u32 *idx, u64 *dev)
{
  __shared__ u64 s_sum[3];
  if (threadIdx.x < 3) s_sum[threadIdx.x] = 0ull;
  __syncthreads();
  u64 bits = 0ull, lines = 0ull, mis = 0ull;
  for (u64 i = (u64)blockIdx.x * kRewriteThreads + threadIdx.x; i < n; i += (u64)gridDim.x * kRewriteThreads) {
    const u64 a = addrs[i];
    const u64 key = line_shift >= 0 ? a >> line_shift : a / line_size;
    if (keys) {
      keys[i] = key;
      idx[i] = (u32)i;
    }
    mis += a != key * line_size ? 1ull : 0ull;
    lines += 1ull;
    bits += sizes[i];
  }
  for (int o = 32; o > 0; o >>= 1) {
    bits += __shfl_xor(bits, o);
    lines += __shfl_xor(lines, o);
    mis += __shfl_xor(mis, o);
  }
  if ((threadIdx.x & 63) == 0) {
    if (lines) atomicAdd(&s_sum[0], lines);
    if (bits) atomicAdd(&s_sum[1], bits);
    if (mis) atomicAdd(&s_sum[2], mis);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    if (s_sum[0]) atomicAdd(&dev[MPC_REWRITE_CTL_LINES], s_sum[0]);
    if (s_sum[1]) atomicAdd(&dev[MPC_REWRITE_CTL_BITS], s_sum[1]);
    if (s_sum[2]) atomicAdd(&dev[MPC_REWRITE_CTL_MISALIGNED], s_sum[2]);
  }
}

// the workgroup's counts into the device table: non-zero entries only
__device__ __forceinline__ void rewrite_flush(const u32 *s_trans, const u32 *s_first, u32 s_equal, u32 classes, u64 *dev)
{
  for (u32 k = threadIdx.x; k < classes * classes; k += kRewriteThreads) {
    const u32 o = k / classes, c = k - o * classes;
    const u32 v = s_trans[o * kRewriteG + c];
    if (v) atomicAdd(&dev[MPC_REWRITE_DEV_TRANS + o * kRewriteG + c], (u64)v);
  }
  if (s_first && threadIdx.x < classes) {
    const u32 v = s_first[threadIdx.x];
    if (v) atomicAdd(&dev[MPC_REWRITE_DEV_FIRST + threadIdx.x], (u64)v);
  }
  if (threadIdx.x == 0 && s_equal) atomicAdd(&dev[MPC_REWRITE_CTL_EQUAL], (u64)s_equal);
}

// a lane per sorted element
__global__ void __launch_bounds__(kRewriteThreads)
rewrite_in_run_kernel(MpcRewriteScratch S, MpcRewriteMap M, const uint16_t *sizes, u64 n)
{
  __shared__ u32 s_trans[kRewriteG * kRewriteG];
  __shared__ u32 s_equal;
  for (u32 k = threadIdx.x; k < kRewriteG * kRewriteG; k += kRewriteThreads) s_trans[k] = 0u;
  if (threadIdx.x == 0) s_equal = 0u;
  __syncthreads();
  const u64 j = (u64)blockIdx.x * kRewriteThreads + threadIdx.x;
  if (j < n) {
    const u64 key = S.keys_out[j];
    const u32 own = sizes[S.idx_out[j]];
    S.words[j] = ((u64)own << 48) | (1ull << 24) | j;
    if (j > 0ull && S.keys_out[j - 1ull] == key) {
      const u32 prev = sizes[S.idx_out[j - 1ull]];
      atomicAdd(&s_trans[rewrite_class(prev, M.granule_bits, M.classes) * kRewriteG + rewrite_class(own, M.granule_bits, M.classes)], 1u);
      if (prev == own) atomicAdd(&s_equal, 1u);
    }
  }
  __syncthreads();
  rewrite_flush(s_trans, nullptr, s_equal, M.classes, M.dev);
}

// a lane per run
__global__ void __launch_bounds__(kRewriteThreads)
rewrite_apply_kernel(MpcRewriteScratch S, MpcRewriteMap M, const uint16_t *sizes, u64 n)
{
  __shared__ u32 s_trans[kRewriteG * kRewriteG];
  __shared__ u32 s_first[kRewriteG];
  __shared__ u32 s_equal, s_claims;
  for (u32 k = threadIdx.x; k < kRewriteG * kRewriteG; k += kRewriteThreads) s_trans[k] = 0u;
  if (threadIdx.x < kRewriteG) s_first[threadIdx.x] = 0u;
  if (threadIdx.x == 0) s_equal = s_claims = 0u;
  __syncthreads();
  u64 runs = *S.runs;
  runs = runs < n ? runs : n;
  const u64 r = (u64)blockIdx.x * kRewriteThreads + threadIdx.x;
  u64 *flag = &M.dev[MPC_REWRITE_CTL_OVERFLOW];
  // (the handle is finished once the flag is set: what the table holds no longer counts)
  const bool over = __hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0ull;
  bool claimed = false;
  if (r < runs && !over) {
    const u64 key = S.run_keys[r], agg = S.run_agg[r];
    u64 first = agg & 0xffffffull, len = (agg >> 24) & 0xffffffull;
    const u32 peak_run = (u32)(agg >> 48);
    first = first < n ? first : n - 1ull;
    len = len < 1ull ? 1ull : len;
    const u64 last = first + len - 1ull < n ? first + len - 1ull : n - 1ull;
    const u32 size_first = sizes[S.idx_out[first]], size_last = sizes[S.idx_out[last]];
    const u64 max_tries = M.capacity < M.slot_mask ? M.capacity + 1ull : M.slot_mask + 1ull;
    const u64 slot = image_slot(M.keys, M.slot_mask, M.hash_mask, key, max_tries, flag, &claimed);
    if (slot == kMpcImageEmpty) {
      atomicOr(flag, 1ull);
    } else {
      const u32 c_first = rewrite_class(size_first, M.granule_bits, M.classes);
      u32 peak = peak_run;
      u64 count = len;
      if (claimed) {
        atomicAdd(&s_first[c_first], 1u);
      } else {
        const u64 old = M.vals[slot];
        const u32 old_latest = (u32)(old >> 48), old_peak = (u32)(old >> 32) & 0xffffu;
        atomicAdd(&s_trans[rewrite_class(old_latest, M.granule_bits, M.classes) * kRewriteG + c_first], 1u);
        if (old_latest == size_first) atomicAdd(&s_equal, 1u);
        peak = old_peak > peak ? old_peak : peak;
        count += old & 0xffffffffull;
        count = count > 0xffffffffull ? 0xffffffffull : count;
      }
      M.vals[slot] = ((u64)size_last << 48) | ((u64)(peak & 0xffffu) << 32) | count;
    }
  }
  const u32 wave_claims = (u32)__popcll(__ballot(claimed));
  if ((threadIdx.x & 63) == 0 && wave_claims) atomicAdd(&s_claims, wave_claims);
  __syncthreads();
  rewrite_flush(s_trans, s_first, s_equal, M.classes, M.dev);
  if (threadIdx.x == 0 && s_claims && atomicAdd(&M.dev[MPC_REWRITE_CTL_KEYS], (u64)s_claims) + s_claims > M.capacity) atomicOr(flag, 1ull);
}

// the get: the live slots into three histograms and four sums
__global__ void __launch_bounds__(kRewriteThreads)
rewrite_get_kernel(MpcRewriteMap M)
{
  __shared__ u32 s_hist[3 * 32];
  __shared__ u64 s_sum[4];
  if (threadIdx.x < 3 * 32) s_hist[threadIdx.x] = 0u;
  if (threadIdx.x < 4) s_sum[threadIdx.x] = 0ull;
  __syncthreads();
  u64 *out = M.dev + MPC_REWRITE_DEV_OUT;
  u64 sum[4] = {0ull, 0ull, 0ull, 0ull};
  // (a workgroup's u32 histograms cannot wrap: a map has at most 2^29 slots)
  for (u64 base = (u64)blockIdx.x * kRewriteThreads; base <= M.slot_mask; base += (u64)gridDim.x * kRewriteThreads) {
    const u64 i = base + threadIdx.x;
    if (i <= M.slot_mask && M.keys[i] != kMpcImageEmpty) {
      const u64 v = M.vals[i];
      const u32 latest = (u32)(v >> 48), peak = (u32)(v >> 32) & 0xffffu, count = (u32)v;
      const u32 cl = rewrite_class(latest, M.granule_bits, M.classes), cp = rewrite_class(peak, M.granule_bits, M.classes);
      sum[0] += cl + 1u;
      sum[1] += cp + 1u;
      sum[2] += latest;
      sum[3] += peak;
      atomicAdd(&s_hist[cl], 1u);
      atomicAdd(&s_hist[32 + cp], 1u);
      atomicAdd(&s_hist[64 + (count ? 31 - __clz((int)count) : 0)], 1u);
    }
  }
  for (int k = 0; k < 4; k++) {
    u64 v = sum[k];
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(&s_sum[k], v);
  }
  __syncthreads();
  if (threadIdx.x < 3 * 32) {
    const u32 h = s_hist[threadIdx.x];
    if (h) atomicAdd(&out[MPC_REWRITE_OUT_HIST_LATEST + threadIdx.x], (u64)h);
  }
  if (threadIdx.x < 4 && s_sum[threadIdx.x]) atomicAdd(&out[MPC_REWRITE_OUT_LATEST_CLASSES + threadIdx.x], s_sum[threadIdx.x]);
}

namespace {
bool pow2(u64 v) { return v && !(v & (v - 1ull)); }
size_t up256(size_t v) { return (v + 255u) & ~(size_t)255u; }

bool map_ok(const MpcRewriteMap *M)
{
  return M->keys && M->vals && M->dev && pow2(M->slot_mask + 1ull) && M->slot_mask + 1ull >= 2ull && M->capacity != 0 &&
         M->capacity <= (M->slot_mask + 1ull) / 2ull && M->granule_bits != 0 && M->classes >= 1 && M->classes <= MPC_REWRITE_MAX_CLASSES;
}

// rocPRIM's temporary storage for a sub-batch of `lines`: the larger of the sort's and the reduction's
hipError_t temp_bytes_of(u64 lines, size_t *bytes)
{
  size_t sort_bytes = 0, reduce_bytes = 0;
  hipError_t e = rocprim::radix_sort_pairs(nullptr, sort_bytes, (u64 *)nullptr, (u64 *)nullptr, (u32 *)nullptr, (u32 *)nullptr, (size_t)lines, 0u, 64u,
                                           (hipStream_t) nullptr);
  if (e != hipSuccess) return e;
  e = rocprim::reduce_by_key(nullptr, reduce_bytes, (u64 *)nullptr, (u64 *)nullptr, (size_t)lines, (u64 *)nullptr, (u64 *)nullptr, (u64 *)nullptr, RewriteRunOp(),
                             rocprim::equal_to<u64>(), (hipStream_t) nullptr);
  if (e != hipSuccess) return e;
  *bytes = up256(sort_bytes > reduce_bytes ? sort_bytes : reduce_bytes) + 256u;
  return hipSuccess;
}

// the arrays of a scratch of `lines`, as offsets from its base; the end of the last one
size_t carve(u64 lines, size_t temp, char *base, MpcRewriteScratch *S)
{
  size_t at = 0;
  auto take = [&](size_t bytes) {
    char *p = base + at;
    at += up256(bytes);
    return p;
  };
  const size_t n = (size_t)lines;
  MpcRewriteScratch T{};
  T.keys_in = (unsigned long long *)take(n * 8);
  T.keys_out = (unsigned long long *)take(n * 8);
  T.words = (unsigned long long *)take(n * 8);
  T.run_keys = (unsigned long long *)take(n * 8);
  T.run_agg = (unsigned long long *)take(n * 8);
  T.runs = (unsigned long long *)take(8);
  T.idx_in = (unsigned *)take(n * 4);
  T.idx_out = (unsigned *)take(n * 4);
  T.temp = take(temp);
  T.temp_bytes = temp;
  T.lines = lines;
  if (S) *S = T;
  return at;
}
}  // namespace

extern "C" hipError_t mpc_rewrite_scratch_bytes(unsigned long long lines, size_t *bytes)
{
  if (lines == 0 || lines > MPC_REWRITE_BATCH || !bytes) return hipErrorInvalidValue;
  size_t temp = 0;
  const hipError_t e = temp_bytes_of(lines, &temp);
  if (e != hipSuccess) return e;
  *bytes = carve(lines, temp, nullptr, nullptr);
  return hipSuccess;
}

extern "C" hipError_t mpc_rewrite_scratch_carve(void *base, unsigned long long lines, MpcRewriteScratch *S)
{
  if (!base || lines == 0 || lines > MPC_REWRITE_BATCH || !S) return hipErrorInvalidValue;
  size_t temp = 0;
  const hipError_t e = temp_bytes_of(lines, &temp);
  if (e != hipSuccess) return e;
  (void)carve(lines, temp, static_cast<char *>(base), S);
  return hipSuccess;
}

// keys == 0: only the sums of (addrs, sizes) into dev (a further member of a group: the keys of the chunk are sorted once)
extern "C" hipError_t mpc_launch_rewrite_keys(const MpcRewriteScratch *S, const uint64_t *addrs, const uint16_t *sizes, unsigned long long n, unsigned line_size,
                                              unsigned long long *dev, int keys, int grid, hipStream_t stream)
{
  if (!S || !addrs || !sizes || !dev || line_size == 0 || n > S->lines) return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  int shift = -1;
  for (int b = 0; b < 31; b++)
    if (line_size == (1u << b)) shift = b;
  const u64 need = (n + kRewriteThreads - 1) / kRewriteThreads, cap = (u64)(grid < 1 ? 1 : grid);
  hipLaunchKernelGGL(rewrite_keys_kernel, dim3((unsigned)(need < cap ? need : cap)), dim3(kRewriteThreads), 0, stream, addrs, sizes, (u64)n, line_size, shift,
                     keys ? (u64 *)S->keys_in : (u64 *)nullptr, S->idx_in, (u64 *)dev);
  return hipGetLastError();
}

extern "C" hipError_t mpc_launch_rewrite_sort(const MpcRewriteScratch *S, unsigned long long n, hipStream_t stream)
{
  if (!S || n > S->lines) return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  size_t need = 0;
  hipError_t e = rocprim::radix_sort_pairs(nullptr, need, (u64 *)S->keys_in, (u64 *)S->keys_out, S->idx_in, S->idx_out, (size_t)n, 0u, 64u, stream);
  if (e != hipSuccess) return e;
  if (need > S->temp_bytes) return hipErrorOutOfMemory;
  need = S->temp_bytes;
  return rocprim::radix_sort_pairs(S->temp, need, (u64 *)S->keys_in, (u64 *)S->keys_out, S->idx_in, S->idx_out, (size_t)n, 0u, 64u, stream);
}

// the sorted sub-batch of S applied to map M with the sizes of M's handle
extern "C" hipError_t mpc_launch_rewrite_apply(const MpcRewriteScratch *S, const MpcRewriteMap *M, const uint16_t *sizes, unsigned long long n, hipStream_t stream)
{
  if (!S || !M || !sizes || !map_ok(M) || n > S->lines || S->lines > MPC_REWRITE_BATCH) return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  const unsigned blocks = (unsigned)((n + kRewriteThreads - 1) / kRewriteThreads);
  hipLaunchKernelGGL(rewrite_in_run_kernel, dim3(blocks), dim3(kRewriteThreads), 0, stream, *S, *M, sizes, (u64)n);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  size_t need = 0;
  e = rocprim::reduce_by_key(nullptr, need, (u64 *)S->keys_out, (u64 *)S->words, (size_t)n, (u64 *)S->run_keys, (u64 *)S->run_agg, (u64 *)S->runs, RewriteRunOp(),
                             rocprim::equal_to<u64>(), stream);
  if (e != hipSuccess) return e;
  if (need > S->temp_bytes) return hipErrorOutOfMemory;
  need = S->temp_bytes;
  e = rocprim::reduce_by_key(S->temp, need, (u64 *)S->keys_out, (u64 *)S->words, (size_t)n, (u64 *)S->run_keys, (u64 *)S->run_agg, (u64 *)S->runs, RewriteRunOp(),
                             rocprim::equal_to<u64>(), stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(rewrite_apply_kernel, dim3(blocks), dim3(kRewriteThreads), 0, stream, *S, *M, sizes, (u64)n);
  return hipGetLastError();
}

// M->dev + MPC_REWRITE_DEV_OUT is zero before the pass
extern "C" hipError_t mpc_launch_rewrite_get(const MpcRewriteMap *M, int grid, hipStream_t stream)
{
  if (!M || !map_ok(M)) return hipErrorInvalidValue;
  const u64 need = (M->slot_mask + kRewriteThreads) / kRewriteThreads, cap = (u64)(grid < 1 ? 1 : grid);
  hipLaunchKernelGGL(rewrite_get_kernel, dim3((unsigned)(need < cap ? need : cap)), dim3(kRewriteThreads), 0, stream, *M);
  return hipGetLastError();
}
