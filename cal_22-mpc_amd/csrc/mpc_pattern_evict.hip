// mpc_pattern_evict.hip -- gfx950 kernels of the Pattern analyser's EVICTING set (mpc_create_pattern_evicting): "existed
// before" as the reference answers it beyond its cache's capacity (Pattern.cpp:109-116 over LRU.h: exist, on a miss put;
// get is never called, so a hit reorders nothing and the cache is a FIFO over insertions).  The line analysis is
// mpc_pattern.hip's, untouched; so are the passes of the refusing set.  mpc_pattern.h has the layout.
//
// The rule.  A stamp is the number of insertions before an insertion.  The line at trace position t existed before iff an
// equal line was inserted earlier and the stamp s of its latest insertion satisfies s >= I_t - C (I_t: insertions before
// t, C: the capacity).  A line that did not exist is inserted with stamp I_t.  A hit changes nothing.
//
// One launch of n <= min(C, MPC_PATTERN_CHUNK) consecutive lines that starts at I0 insertions, in these passes:
//   begin     (one lane) decides whether the older table is recycled, zeroes the launch's counters
//   clear     empties the recycled table (does nothing otherwise)
//   claim, compare, tail
//             RESOLVE: the claim protocol of mpc_pattern.hip on the newer table, after which every line of the launch
//             knows its entry (ent[i]) and all equal lines share it.  The winner of an empty slot looks the line up in the
//             older table (nothing writes to it) and brings its stamp along.  Every line lowers its entry's first position.
//   classify  an entry with stamp s is GONE (none, or s < I0 - C: its first occurrence misses, every later one hits), SAFE
//             (s >= I0 + n - C: all hit) or AT RISK.  Per line: first occurrence of a gone line / occurrence of an at-risk
//             line; per 256 lines their counts.
//   scan      (one workgroup) exclusive prefix sums of those counts
//   scatter   per line A(p), the gone firsts before it, and the at-risk occurrences before it; the at-risk positions
//             compacted in ascending order
//   walk      (one workgroup) the at-risk occurrences in order: the one at p hits while s >= I0 + A(p) + r - C, r the
//             at-risk misses so far; the first that fails misses and re-stamps the entry with I0 + A(p) + r, so that the
//             later ones hit.  256 at a time are loaded by all lanes, chained to the next occurrence of their entry in
//             the batch, decided by lane 0 out of LDS and written back by all lanes.  Its loop is bounded by their
//             number.  Then the launch's totals: insertions, and hits and misses into the raw statistics.
//   finish    the stamp of a gone line's first occurrence at p: I0 + A(p) + the at-risk misses before p
// No lane waits for another, every loop is bounded by a table or by the launch, nothing spins on memory, and the host is
// not asked anything: launches of one set run back to back on the stream (mpc_capi.hip orders calls by an event).
#include "mpc_kernel_common.h"
#include "mpc_pattern.h"
#include "mpc_launch.h"

constexpr int kThreads = 256;
constexpr u64 kSeqMask = (1ull << 40) - 1ull;   // launches counted in an entry's first-position key
static_assert(MPC_PATTERN_CHUNK <= (1u << 24), "a position takes the low 24 bits of that key");

__device__ __forceinline__ u64 ev_mix(u64 x)
{
  x ^= x >> 33;
  x *= 0xff51afd7ed558ccdull;
  x ^= x >> 33;
  x *= 0xc4ceb9fe1a85ec53ull;
  x ^= x >> 33;
  return x;
}

__device__ __forceinline__ u64 ev_hash(const u64 *line, int w8, u64 tag_mask)
{
  u64 h = 0x9e3779b97f4a7c15ull;
  for (int i = 0; i < w8; i++) h = ev_mix(h ^ line[i]);
  return h & tag_mask;
}

__device__ __forceinline__ bool ev_equal(const u64 *a, const u64 *b, int w8)
{
  u64 d = 0;
  for (int i = 0; i < w8; i++) d |= a[i] ^ b[i];
  return d == 0ull;
}

__device__ __forceinline__ u64 ev_ctl(const MpcEvictSet &S, int at) { return S.ctl[at]; }
__device__ __forceinline__ MpcEvictTable ev_newer(const MpcEvictSet &S) { return S.tab[ev_ctl(S, MPC_ESET_NEWER) & 1ull]; }
__device__ __forceinline__ MpcEvictTable ev_older(const MpcEvictSet &S) { return S.tab[(ev_ctl(S, MPC_ESET_NEWER) & 1ull) ^ 1ull]; }

// the stamp of the line's entry in the older table, which no launch writes to
__device__ __forceinline__ u64 ev_older_stamp(const MpcEvictSet &S, const MpcEvictTable &O, const u64 *line, int w8, u64 tag, u32 slot)
{
  for (u32 probe = 0; probe <= S.slot_mask; probe++) {
    const u64 t = O.tags[slot];
    if (t == 0ull) return MPC_ESET_NO_STAMP;
    if (t == tag && ev_equal(line, O.store + (u64)slot * (u64)w8, w8)) return O.stamps[slot];
    slot = (slot + 1u) & S.slot_mask;
  }
  return MPC_ESET_NO_STAMP;
}

enum { EV_JOINED = 0, EV_MEET, EV_OVER };

// pat_walk of mpc_pattern.hip on the newer table, without a capacity: the table cannot fill (mpc_pattern.h)
__device__ __forceinline__ int ev_walk(const MpcEvictSet &S, const MpcEvictTable &T, const MpcEvictTable &O, const u64 *line, int w8, u64 hash, u32 &slot)
{
  const u64 tag = hash | 1ull;
  for (u32 probe = 0; probe <= S.slot_mask; probe++) {
    u64 t = __hip_atomic_load(&T.tags[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (t == 0ull) {
      t = atomicCAS(&T.tags[slot], 0ull, tag);
      if (t == 0ull) {
        u64 *dst = T.store + (u64)slot * (u64)w8;
        for (int i = 0; i < w8; i++) dst[i] = line[i];
        T.stamps[slot] = ev_older_stamp(S, O, line, w8, tag, (u32)hash & S.slot_mask);
        return EV_JOINED;
      }
    }
    if (t == tag) return EV_MEET;
    slot = (slot + 1u) & S.slot_mask;
  }
  atomicOr(&S.ctl[MPC_ESET_OVERFLOW], 2ull);
  return EV_OVER;
}

// line i of the launch has its entry
__device__ __forceinline__ void ev_settle(const MpcEvictSet &S, const MpcEvictTable &T, u32 i, u32 slot)
{
  S.ent[i] = slot;
  const u64 key = ((kSeqMask - (ev_ctl(S, MPC_ESET_SEQ) & kSeqMask)) << 24) | (u64)i;      // (i < MPC_PATTERN_CHUNK <= 2^24)
  atomicMin(&T.first[slot], key);
}

__global__ void evict_begin_kernel(MpcEvictSet S)
{
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const u64 I = S.ctl[MPC_ESET_INSERTIONS];
  const bool rotate = I - S.ctl[MPC_ESET_I_ROT] >= S.capacity;
  if (rotate) {
    S.ctl[MPC_ESET_NEWER] ^= 1ull;
    S.ctl[MPC_ESET_I_ROT] = I;
#if MPC_TESTING     // (test library only, here and below: sums over the launches for mpc_test_evict_counters, mpc_pattern.h)
    S.ctl[MPC_ESET_T_ROTATIONS] += 1ull;
#endif
  }
  S.ctl[MPC_ESET_ROTATE] = rotate ? 1ull : 0ull;
  S.ctl[MPC_ESET_I0] = I;
  S.ctl[MPC_ESET_SEQ] += 1ull;
  S.ctl[MPC_ESET_PENDING_A] = 0ull;
  S.ctl[MPC_ESET_PENDING_B] = 0ull;
  S.ctl[MPC_ESET_N_GONE] = 0ull;
  S.ctl[MPC_ESET_N_RISK] = 0ull;
}

__global__ void __launch_bounds__(kThreads)
evict_clear_kernel(MpcEvictSet S)
{
  if (ev_ctl(S, MPC_ESET_ROTATE) == 0ull) return;
  const MpcEvictTable T = ev_newer(S);
  for (u64 k = (u64)blockIdx.x * kThreads + threadIdx.x; k <= (u64)S.slot_mask; k += (u64)gridDim.x * kThreads) T.tags[k] = 0ull;
}

__global__ void __launch_bounds__(kThreads)
evict_claim_kernel(const u64 *__restrict__ lines, u32 n_lines, int w8, MpcEvictSet S)
{
  const u32 i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n_lines) return;
  const MpcEvictTable T = ev_newer(S), O = ev_older(S);
  const u64 *line = lines + (u64)i * (u64)w8;
  const u64 hash = ev_hash(line, w8, S.tag_mask);
  u32 slot = (u32)hash & S.slot_mask;
  const int r = ev_walk(S, T, O, line, w8, hash, slot);
  if (r == EV_JOINED) {
    ev_settle(S, T, i, slot);
  } else if (r == EV_MEET) {
    const u32 at = (u32)atomicAdd(&S.ctl[MPC_ESET_PENDING_A], 1ull);
    if (at < S.launch_max) S.pend_a[at] = make_uint2(i, slot);
  } else {
    S.ent[i] = 0u;          // (unreachable; the handle reports the overflow)
  }
}

// one pending line: the slot it met its tag at is complete by now
__device__ __forceinline__ int ev_resolve(const MpcEvictSet &S, const MpcEvictTable &T, const MpcEvictTable &O, const u64 *lines, int w8, uint2 e, u32 &slot)
{
  const u64 *line = lines + (u64)e.x * (u64)w8;
  slot = e.y;
  int r = EV_JOINED;
  if (!ev_equal(line, T.store + (u64)slot * (u64)w8, w8)) {
    slot = (slot + 1u) & S.slot_mask;
    r = ev_walk(S, T, O, line, w8, ev_hash(line, w8, S.tag_mask), slot);
  }
  if (r == EV_JOINED) ev_settle(S, T, e.x, slot);
  if (r == EV_OVER) S.ent[e.x] = 0u;
  return r;
}

__global__ void __launch_bounds__(kThreads)
evict_compare_kernel(const u64 *__restrict__ lines, int w8, MpcEvictSet S)
{
  const MpcEvictTable T = ev_newer(S), O = ev_older(S);
  const u64 n = min(ev_ctl(S, MPC_ESET_PENDING_A), (u64)S.launch_max);
  for (u64 k = (u64)blockIdx.x * kThreads + threadIdx.x; k < n; k += (u64)gridDim.x * kThreads) {
    const uint2 e = S.pend_a[k];
    u32 slot;
    if (ev_resolve(S, T, O, lines, w8, e, slot) == EV_MEET) {
      const u32 at = (u32)atomicAdd(&S.ctl[MPC_ESET_PENDING_B], 1ull);
      if (at < S.launch_max) S.pend_b[at] = make_uint2(e.x, slot);
#if MPC_TESTING
      atomicAdd(&S.ctl[MPC_ESET_T_LIST_B], 1ull);
#endif
    }
  }
}

// ONE workgroup: list B in rounds, the lists swapping roles (pattern_tail_kernel of mpc_pattern.hip)
__global__ void __launch_bounds__(kThreads)
evict_tail_kernel(const u64 *__restrict__ lines, int w8, MpcEvictSet S)
{
  __shared__ u32 s_next;
  const MpcEvictTable T = ev_newer(S), O = ev_older(S);
  u32 n = (u32)min(ev_ctl(S, MPC_ESET_PENDING_B), (u64)S.launch_max);
  uint2 *cur = S.pend_b, *next = S.pend_a;
  for (u32 round = 0; n > 0u && round <= S.slot_mask; round++) {
    if (threadIdx.x == 0) s_next = 0;
    __syncthreads();
    for (u32 k = threadIdx.x; k < n; k += kThreads) {
      const uint2 e = cur[k];
      u32 slot;
      if (ev_resolve(S, T, O, lines, w8, e, slot) == EV_MEET) {
        next[atomicAdd(&s_next, 1u)] = make_uint2(e.x, slot);
#if MPC_TESTING
        atomicAdd(&S.ctl[MPC_ESET_T_LIST_B], 1ull);
#endif
      }
    }
    __threadfence();
    __syncthreads();         // this round's lines, stamps and list are written: the next round may read them
    n = s_next;
    uint2 *t = cur; cur = next; next = t;
    __syncthreads();
  }
  if (n > 0u && threadIdx.x == 0) atomicOr(&S.ctl[MPC_ESET_OVERFLOW], 2ull);   // (unreachable, see ev_walk)
}

// the workgroup's sums of two flags (0 / 1 per lane), valid in every lane
__device__ __forceinline__ uint2 ev_block_sums(u32 a, u32 b, u32 *s_wave /* [8] */)
{
  const u32 wave = threadIdx.x >> 6;
  const u32 ca = (u32)__popcll(__ballot(a != 0u)), cb = (u32)__popcll(__ballot(b != 0u));
  if ((threadIdx.x & 63) == 0) { s_wave[wave] = ca; s_wave[4 + wave] = cb; }
  __syncthreads();
  return make_uint2(s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3], s_wave[4] + s_wave[5] + s_wave[6] + s_wave[7]);
}

__global__ void __launch_bounds__(kThreads)
evict_classify_kernel(u32 n_lines, MpcEvictSet S)
{
  __shared__ u32 s_wave[8];
  const u32 i = blockIdx.x * kThreads + threadIdx.x;
  u32 kind = MPC_ELINE_HIT;
  if (i < n_lines) {
    const MpcEvictTable T = ev_newer(S);
    const u32 e = S.ent[i];
    const u64 s = T.stamps[e], I0 = ev_ctl(S, MPC_ESET_I0), C = S.capacity;
    if (s == MPC_ESET_NO_STAMP || s + C < I0) kind = (u32)(T.first[e] & 0xffffffull) == i ? MPC_ELINE_GONE_FIRST : MPC_ELINE_HIT;
    else if (s + C < I0 + (u64)n_lines) kind = MPC_ELINE_RISK;
    S.kind[i] = (uint8_t)kind;
  }
  const uint2 sums = ev_block_sums(kind == MPC_ELINE_GONE_FIRST, kind == MPC_ELINE_RISK, s_wave);
  if (threadIdx.x == 0) S.block_sums[blockIdx.x] = sums;
}

// ONE workgroup: the block sums become their exclusive prefix sums; the totals go to the control block
__global__ void __launch_bounds__(kThreads)
evict_scan_kernel(u32 n_blocks, MpcEvictSet S)
{
  __shared__ uint2 s_part[kThreads];
  const u32 per = (n_blocks + kThreads - 1) / kThreads;
  const u32 lo = min(threadIdx.x * per, n_blocks), hi = min(lo + per, n_blocks);
  uint2 sum = make_uint2(0u, 0u);
  for (u32 k = lo; k < hi; k++) { const uint2 v = S.block_sums[k]; sum.x += v.x; sum.y += v.y; }
  s_part[threadIdx.x] = sum;
  __syncthreads();
  uint2 run = make_uint2(0u, 0u);
  for (u32 t = 0; t < threadIdx.x; t++) { run.x += s_part[t].x; run.y += s_part[t].y; }
  for (u32 k = lo; k < hi; k++) {
    const uint2 v = S.block_sums[k];
    S.block_sums[k] = run;
    run.x += v.x; run.y += v.y;
  }
  if (threadIdx.x == kThreads - 1) {
    S.ctl[MPC_ESET_N_GONE] = run.x;
    S.ctl[MPC_ESET_N_RISK] = run.y;
  }
}

__global__ void __launch_bounds__(kThreads)
evict_scatter_kernel(u32 n_lines, MpcEvictSet S)
{
  __shared__ u32 s_wave[8];
  const u32 i = blockIdx.x * kThreads + threadIdx.x;
  const u32 kind = i < n_lines ? S.kind[i] : MPC_ELINE_HIT;
  const u64 below = (1ull << (threadIdx.x & 63)) - 1ull;
  const u64 bg = __ballot(kind == MPC_ELINE_GONE_FIRST), br = __ballot(kind == MPC_ELINE_RISK);
  const u32 wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { s_wave[wave] = (u32)__popcll(bg); s_wave[4 + wave] = (u32)__popcll(br); }
  __syncthreads();
  uint2 at = S.block_sums[blockIdx.x];
  for (u32 w = 0; w < wave; w++) { at.x += s_wave[w]; at.y += s_wave[4 + w]; }
  at.x += (u32)__popcll(bg & below);
  at.y += (u32)__popcll(br & below);
  if (i < n_lines) {
    S.gone_before[i] = at.x;
    S.risk_before[i] = at.y;
    if (kind == MPC_ELINE_RISK) S.risk[at.y] = i;
  }
}

// ONE workgroup
__global__ void __launch_bounds__(kThreads)
evict_walk_kernel(u32 n_lines, MpcEvictSet S, u64 *gstats)
{
  __shared__ u32 s_ent[kThreads], s_gone[kThreads], s_next[kThreads], s_before[kThreads];
  __shared__ u64 s_stamp[kThreads];
  __shared__ uint8_t s_miss[kThreads];
  __shared__ u32 s_missed;
  const MpcEvictTable T = ev_newer(S);
  const u32 n_risk = (u32)min(ev_ctl(S, MPC_ESET_N_RISK), (u64)n_lines);
  const u64 I0 = ev_ctl(S, MPC_ESET_I0), C = S.capacity;
  if (threadIdx.x == 0) s_missed = 0u;
  __syncthreads();
  for (u32 base = 0; base < n_risk; base += kThreads) {
    const u32 m = min(n_risk - base, (u32)kThreads), k = threadIdx.x;
    u32 p = 0;
    if (k < m) {
      p = S.risk[base + k];
      s_ent[k] = S.ent[p];
      s_gone[k] = S.gone_before[p];
      s_stamp[k] = __hip_atomic_load(&T.stamps[s_ent[k]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (an earlier batch may have re-stamped it)
    }
    __syncthreads();
    if (k < m) {
      u32 next = kThreads;
      for (u32 j = k + 1; j < m; j++)
        if (s_ent[j] == s_ent[k]) { next = j; break; }
      s_next[k] = next;
    }
    __syncthreads();
    if (k == 0) {
      u32 missed = s_missed;
      for (u32 j = 0; j < m; j++) {
        u64 s = s_stamp[j];
        const u64 now = I0 + (u64)s_gone[j] + (u64)missed;      // insertions before this occurrence
        s_before[j] = missed;
        const bool miss = s + C < now;
        s_miss[j] = miss ? 1 : 0;
        if (miss) { s = now; s_stamp[j] = now; missed++; }
        if (s_next[j] < kThreads) s_stamp[s_next[j]] = s;
      }
      s_missed = missed;
    }
    __syncthreads();
    if (k < m) {
      S.risk_missed[base + k] = s_before[k];
      if (s_miss[k]) {
        __hip_atomic_store(&T.stamps[s_ent[k]], s_stamp[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        S.kind[p] = MPC_ELINE_RISK_MISS;
      }
    }
    __threadfence();
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    S.risk_missed[n_risk] = s_missed;
    const u64 misses = min(ev_ctl(S, MPC_ESET_N_GONE) + (u64)s_missed, (u64)n_lines);
    S.ctl[MPC_ESET_INSERTIONS] = I0 + misses;
    if (misses) atomicAdd(&gstats[MPC_PAT_JOINED], misses);
    if (n_lines - misses) atomicAdd(&gstats[MPC_PAT_EXISTED], (u64)n_lines - misses);
#if MPC_TESTING
    S.ctl[MPC_ESET_T_GONE] += ev_ctl(S, MPC_ESET_N_GONE);
    S.ctl[MPC_ESET_T_RISK] += (u64)n_risk;
    S.ctl[MPC_ESET_T_RISK_MISS] += (u64)s_missed;
#endif
  }
}

__global__ void __launch_bounds__(kThreads)
evict_finish_kernel(u32 n_lines, MpcEvictSet S)
{
  const u32 i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n_lines || S.kind[i] != MPC_ELINE_GONE_FIRST) return;
  const MpcEvictTable T = ev_newer(S);
  const u32 before = min(S.risk_before[i], n_lines);
  T.stamps[S.ent[i]] = ev_ctl(S, MPC_ESET_I0) + (u64)S.gone_before[i] + (u64)S.risk_missed[before];
}

// the passes over n_lines <= S->launch_max lines; the caller lets no other launch on the same set overlap with this one
extern "C" hipError_t mpc_launch_pattern_evict(const void *d_lines, u32 n_lines, int L, const MpcEvictSet *S, u64 *d_stats, int compare_grid,
                                               int clear_grid, hipStream_t stream)
{
  if (n_lines == 0 || n_lines > S->launch_max) return n_lines ? hipErrorInvalidValue : hipSuccess;
  const u64 *l = static_cast<const u64 *>(d_lines);
  const int w8 = L / 8;
  const u32 blocks = (n_lines + kThreads - 1) / kThreads;
  const dim3 wg(kThreads), per_line(blocks), one(1);
  hipLaunchKernelGGL(evict_begin_kernel, one, dim3(1), 0, stream, *S);
  hipLaunchKernelGGL(evict_clear_kernel, dim3(clear_grid), wg, 0, stream, *S);
  hipLaunchKernelGGL(evict_claim_kernel, per_line, wg, 0, stream, l, n_lines, w8, *S);
  hipLaunchKernelGGL(evict_compare_kernel, dim3(compare_grid), wg, 0, stream, l, w8, *S);
  hipLaunchKernelGGL(evict_tail_kernel, one, wg, 0, stream, l, w8, *S);
  hipLaunchKernelGGL(evict_classify_kernel, per_line, wg, 0, stream, n_lines, *S);
  hipLaunchKernelGGL(evict_scan_kernel, one, wg, 0, stream, blocks, *S);
  hipLaunchKernelGGL(evict_scatter_kernel, per_line, wg, 0, stream, n_lines, *S);
  hipLaunchKernelGGL(evict_walk_kernel, one, wg, 0, stream, n_lines, *S, d_stats);
  hipLaunchKernelGGL(evict_finish_kernel, per_line, wg, 0, stream, n_lines, *S);
  return hipGetLastError();
}
