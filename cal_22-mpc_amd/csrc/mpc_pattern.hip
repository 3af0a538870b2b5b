// mpc_pattern.hip -- gfx950 kernels of the Pattern analyser (reference src/compressor/Pattern.{h,cpp}, LRU.h):
//
//   pattern_kernel<NW> /       per line: Zeros, Repeat, the six base-delta scans with the returned size and the selected
//   pattern_any_kernel         PatternState, Implicit / Explicit counts, the byte histogram (Pattern.cpp:6-75, 118-346)
//   pattern_claim_kernel       the distinct-line set ("existed before", Pattern.cpp:109-116): claim pass,
//   pattern_compare_kernel     compare pass after the kernel boundary,
//   pattern_tail_kernel        and whatever still has to probe on, in one workgroup
//
// ---- the scans ------------------------------------------------------------------------------------------------------
// checkPattern is BDI's scan (the same text as BDI.cpp:108-201): values are the little-endian integers of B bytes,
// zero-extended (the "sign extension" masks with all ones); reduceSign strips the leading ones of a negative 64-bit
// value down to one sign bit and returns -1 unchanged, so "reduceSign(x) <= 2^(8D) - 1" is the range test
//        0 <= x <= 2^(8D) - 1     or     -2^(8D-1) <= x <= -2        (x as signed 64-bit)
// A scan that succeeds costs n + 8 (B + (n - 1) D) bits whatever its immediates are and a failed one more, and
// CompressLine keeps strictly smaller sizes only: a lane skips a scan whose success cost is not below its best.
//
// ---- the byte histogram ---------------------------------------------------------------------------------------------
// Only the ordinary lines (not all-word-same) are counted byte by byte; that histogram IS
// SymbolCountsExceptAllZerosAllWordSame.  A non-zero word-same line adds its word's four bytes to a second, 256-bin
// table in units of L/4; zero lines are a line count.  The host adds the three up to SymbolCounts.
// With one lane per line every lane of a wave looks at byte b of word i at the same time, and on real data those
// are equal across lines (a zero high byte in every word): 64 same-address LDS atomics.  Two things spread them:
// the lane rotates each word by (lane & 3) bytes (one v_alignbyte), so that only a quarter of the lanes is at a
// given byte position, and the histogram has 16 copies, picked by lane >> 2 and interleaved (bin * 16 + copy), so
// that those 16 lanes hit 16 different banks.  256 lines of a workgroup then meet 4 deep on a bin, one per wave.
// (DESIGN.md 4.6 has what else was considered.)
//
// ---- the set --------------------------------------------------------------------------------------------------------
// Open addressing, linear probing, in device memory: tags[slot] (0 = empty, else the line's 64-bit hash with bit 0
// set) and store[slot] (the line).  Equality is decided on the L bytes; the tag only says where to look.  No lane
// ever waits for another one:
//   claim    every line walks its chain: another tag -> next slot; empty -> compare-and-swap the tag in, the winner
//            writes the line and is done (it joined the set); the line's own tag -> the slot's line may still be on its
//            way from a winner of this very kernel, so the line is put on pending list A as (line, slot) and the lane
//            is done.
//   compare  after the kernel boundary every line stored before is complete: list A's lines compare the L bytes.
//            Equal -> "existed".  Unequal (two lines, one hash) -> the line walks on as in the claim pass; where it
//            meets its tag again it goes on list B.
//   tail     one workgroup takes list B in rounds, a workgroup barrier between rounds in the kernel boundary's place,
//            until it is empty.  Every round moves every line at least one slot down its chain, and the table is at
//            most a little over half full, so the rounds end; with 64-bit tags list B is empty in practice.
// Equal lines of one batch walk the same chain, so exactly one of them wins the slot and every other one meets its
// tag there.  The capacity (mpc_pattern.h): a lane that finds an empty slot while the set already holds the capacity
// raises the overflow flag instead of joining (the compare-and-swap of 0 for 0 there reads the slot's true value:
// an equal line may just have joined); a winner that was given a number beyond the capacity raises it too.
#include "mpc_kernel_common.h"
#include "mpc_pattern.h"
#include "mpc_launch.h"

constexpr int kThreads = 256;
// the byte histogram's spreading (development switches): interleaved copies picked by lane >> 2, and the
// lane-rotated byte order
#ifndef MPC_PAT_COPIES
#define MPC_PAT_COPIES 16
#endif
#ifndef MPC_PAT_ROTATE
#define MPC_PAT_ROTATE 1
#endif
constexpr u32 kCopies = MPC_PAT_COPIES;          // a power of two up to 16
constexpr u32 kSlotMask = (1u << MPC_PATTERN_SLOT_BITS) - 1u;

// reduceSign(x) <= 2^(8D) - 1 (Pattern.cpp:348-363)
template <int D>
__device__ __forceinline__ bool pat_fits(u64 x)
{
  constexpr u64 lim = D == 4 ? 0xffffffffull : ((1ull << (8 * D)) - 1ull);
  constexpr u64 h = 1ull << (8 * D - 1);
  return x <= lim || (x >= 0ull - h && x != ~0ull);
}

// a loop over n items, unrolled when the count N is known at compile time (the line is in registers then)
template <int N, class F>
__device__ __forceinline__ void pat_for(u32 n, F f)
{
  if constexpr (N > 0) {
#pragma unroll
    for (u32 i = 0; i < (u32)N; i++) f(i);
  } else {
    for (u32 i = 0; i < n; i++) f(i);
  }
}

template <int B, class W>
__device__ __forceinline__ u64 pat_value(const W &w, u32 i)
{
  if constexpr (B == 8) return ((u64)w[2 * i + 1] << 32) | (u64)w[2 * i];
  else if constexpr (B == 4) return (u64)w[i];
  else return (u64)((w[i >> 1] >> (16u * (i & 1u))) & 0xffffu);
}

// checkPattern (Pattern.cpp:118-211) over nw words (NW: the same at compile time, or 0); imm_out: the immediates, which
// countPattern counts again
template <int B, int D, int NW, class W>
__device__ __forceinline__ u32 pat_check(const W &w, u32 nw, u32 &imm_out)
{
  const u32 n = nw * 4u / (u32)B;
  u32 imm = 0;
  bool have_base = false, not_all = false;
  u64 base = 0;
  pat_for<NW * 4 / B>(n, [&](u32 i) {
    const u64 v = pat_value<B>(w, i);
    const bool is_imm = pat_fits<D>(v);
    imm += is_imm ? 1u : 0u;
    not_all = not_all || (!is_imm && have_base && !pat_fits<D>(base - v));
    base = (!is_imm && !have_base) ? v : base;
    have_base = have_base || !is_imm;
  });
  imm_out = imm;
  // unsigned 32-bit arithmetic as in the source, the wrap of (n - imm - 1) when every value is an immediate included
  if (not_all) return n + 8u * ((imm * (u32)D) + ((n - imm) * (u32)B));
  return n + 8u * ((imm * (u32)D) + ((u32)B + (n - imm - 1u) * (u32)D));
}

struct PatLine {
  u32 best;        // bestCSize
  int select;      // PatternState 0..5, 9 = NotDefined
  u32 imm;         // immediates of the selected scan
  bool zero, same;
};

// CompressLine without the set (Pattern.cpp:6-75)
template <int NW, class W>
__device__ __forceinline__ PatLine pat_line(const W &w, u32 nw)
{
  PatLine r;
  u32 any = 0, rep = 0;
  pat_for<NW>(nw, [&](u32 i) {
    any |= w[i];
    rep |= w[i] ^ w[0];
  });
  r.zero = any == 0u;
  r.same = rep == 0u;
  r.best = 32u * nw;
  r.select = 9;
  r.imm = 0;
#define MPC_PAT_TRY(IDX, B, D)                                                           \
  {                                                                                      \
    const u32 n_ = nw * 4u / B, ok_cost_ = n_ + 8u * ((u32)B + (n_ - 1u) * (u32)D);      \
    if (ok_cost_ < r.best) {                                                             \
      u32 imm_;                                                                          \
      const u32 c_ = pat_check<B, D, NW>(w, nw, imm_);                                       \
      if (r.best > c_) { r.best = c_; r.select = IDX; r.imm = imm_; }                    \
    }                                                                                    \
  }
  MPC_PAT_TRY(0, 8, 1)
  MPC_PAT_TRY(1, 8, 2)
  MPC_PAT_TRY(2, 8, 4)
  MPC_PAT_TRY(3, 4, 1)
  MPC_PAT_TRY(4, 4, 2)
  MPC_PAT_TRY(5, 2, 1)
#undef MPC_PAT_TRY
  return r;
}

// per-lane sums of a launch, flushed once
struct PatAcc {
  u32 lines = 0, zero = 0, same = 0, undef = 0;
  u32 imp[6] = {0, 0, 0, 0, 0, 0}, exp[6] = {0, 0, 0, 0, 0, 0};
  u64 sizes = 0;
};

struct PatShared {
  u32 hist[256 * kCopies]; // ordinary lines: bin * kCopies + copy
  u32 same[256];           // non-zero word-same lines: the four bytes of their word
  u64 stat[MPC_PAT_HIST];
};

__device__ __forceinline__ void pat_shared_init(PatShared &s)
{
  for (int i = threadIdx.x; i < 256 * (int)kCopies; i += kThreads) s.hist[i] = 0;
  for (int i = threadIdx.x; i < 256; i += kThreads) s.same[i] = 0;
  if (threadIdx.x < MPC_PAT_HIST) s.stat[threadIdx.x] = 0;
  __syncthreads();
}

__device__ __forceinline__ void pat_count_bytes(PatShared &s, u32 word, u32 rot, u32 copy)
{
  const u32 x = alignbyte(word, word, rot);       // the lane's byte order: the word rotated right by rot bytes
  atomicAdd(&s.hist[(x & 0xffu) * kCopies + copy], 1u);
  atomicAdd(&s.hist[((x >> 8) & 0xffu) * kCopies + copy], 1u);
  atomicAdd(&s.hist[((x >> 16) & 0xffu) * kCopies + copy], 1u);
  atomicAdd(&s.hist[(x >> 24) * kCopies + copy], 1u);
}

__device__ __forceinline__ void pat_account(const PatLine &r, u32 nw, PatAcc &a)
{
  a.lines++;
  a.zero += r.zero ? 1u : 0u;
  a.same += r.same ? 1u : 0u;
  a.undef += r.select == 9 ? 1u : 0u;
  a.sizes += r.best + 4u;
  // countPattern (Pattern.cpp:213-346): B bytes per immediate are implicit, B bytes per other value explicit
#pragma unroll
  for (int k = 0; k < 6; k++) {
    const u32 B = k < 3 ? 8u : k < 5 ? 4u : 2u;
    const u32 n = nw * 4u / B;
    a.imp[k] += r.select == k ? B * r.imm : 0u;
    a.exp[k] += r.select == k ? B * (n - r.imm) : 0u;
  }
}

__device__ __forceinline__ void pat_flush(PatShared &s, const PatAcc &a, u64 *gstats)
{
  auto add = [&](int at, u64 v) { if (v) atomicAdd(&s.stat[at], v); };
  add(MPC_PAT_LINES, a.lines);
  add(MPC_PAT_SIZES, a.sizes);
  add(MPC_PAT_ZERO, a.zero);
  add(MPC_PAT_SAME, a.same);
  add(MPC_PAT_UNDEF, a.undef);
#pragma unroll
  for (int k = 0; k < 6; k++) {
    add(MPC_PAT_IMPLICIT + k, a.imp[k]);
    add(MPC_PAT_EXPLICIT + k, a.exp[k]);
  }
  __syncthreads();
  if (threadIdx.x < MPC_PAT_HIST && s.stat[threadIdx.x]) atomicAdd(&gstats[threadIdx.x], s.stat[threadIdx.x]);
  {
    u32 t = 0;
#pragma unroll
    for (int c = 0; c < (int)kCopies; c++) t += s.hist[threadIdx.x * kCopies + c];
    if (t) atomicAdd(&gstats[MPC_PAT_HIST + threadIdx.x], (u64)t);
    if (s.same[threadIdx.x]) atomicAdd(&gstats[MPC_PAT_SAME_HIST + threadIdx.x], (u64)s.same[threadIdx.x]);
  }
}

template <int NW, class W>
__device__ __forceinline__ void pat_one(const W &w, u32 nw, u64 line, PatShared &s, PatAcc &a, uint16_t *sizes_out, int8_t *sel_out)
{
  const PatLine r = pat_line<NW>(w, nw);
  if (sizes_out) sizes_out[line] = (uint16_t)(r.best + 4u);
  if (sel_out) sel_out[line] = (int8_t)r.select;
  pat_account(r, nw, a);
  const u32 rot = MPC_PAT_ROTATE ? threadIdx.x & 3u : 0u, copy = (threadIdx.x >> 2) & (kCopies - 1u);
  if (!r.same) {
    pat_for<NW>(nw, [&](u32 i) { pat_count_bytes(s, w[i], rot, copy); });
  } else if (!r.zero) {
    const u32 x = w[0];
    atomicAdd(&s.same[x & 0xffu], 1u);
    atomicAdd(&s.same[(x >> 8) & 0xffu], 1u);
    atomicAdd(&s.same[(x >> 16) & 0xffu], 1u);
    atomicAdd(&s.same[x >> 24], 1u);
  }
}

// One lane per line, the line in registers (32-, 64- and 128-byte lines).  A workgroup's byte counters are 32-bit:
// the launcher keeps a launch below 2^31 bytes.
template <int NW>
__global__ void __launch_bounds__(kThreads)
pattern_kernel(const uint4 *__restrict__ lines, u64 n_lines, uint16_t *__restrict__ sizes_out, int8_t *__restrict__ sel_out, u64 *gstats)
{
  __shared__ PatShared s;
  pat_shared_init(s);
  PatAcc a;
  for (u64 line = (u64)blockIdx.x * kThreads + threadIdx.x; line < n_lines; line += (u64)gridDim.x * kThreads) {
    u32 w[NW];
    const uint4 *src = lines + line * (NW / 4);
#pragma unroll
    for (int i = 0; i < NW / 4; i++) {
      const uint4 q = src[i];
      w[4 * i] = q.x; w[4 * i + 1] = q.y; w[4 * i + 2] = q.z; w[4 * i + 3] = q.w;
    }
    pat_one<NW>(w, (u32)NW, line, s, a, sizes_out, sel_out);
  }
  pat_flush(s, a, gstats);
}

// every other multiple of 8 bytes: the scans read the line's words from memory
__global__ void __launch_bounds__(kThreads)
pattern_any_kernel(const u32 *__restrict__ words, u64 n_lines, u32 nw, uint16_t *__restrict__ sizes_out, int8_t *__restrict__ sel_out,
                   u64 *gstats)
{
  __shared__ PatShared s;
  pat_shared_init(s);
  PatAcc a;
  for (u64 line = (u64)blockIdx.x * kThreads + threadIdx.x; line < n_lines; line += (u64)gridDim.x * kThreads) {
    const u32 *w = words + line * nw;
    pat_one<0>(w, nw, line, s, a, sizes_out, sel_out);
  }
  pat_flush(s, a, gstats);
}

// ---------------------------------------------------------------------------------------------------------------------
// the set
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ u64 pat_mix(u64 x)
{
  x ^= x >> 33;
  x *= 0xff51afd7ed558ccdull;
  x ^= x >> 33;
  x *= 0xc4ceb9fe1a85ec53ull;
  x ^= x >> 33;
  return x;
}

__device__ __forceinline__ u64 pat_hash(const u64 *line, int w8, u64 tag_mask)
{
  u64 h = 0x9e3779b97f4a7c15ull;
  for (int i = 0; i < w8; i++) h = pat_mix(h ^ line[i]);
  return h & tag_mask;
}

__device__ __forceinline__ bool pat_equal(const u64 *a, const u64 *b, int w8)
{
  u64 d = 0;
  for (int i = 0; i < w8; i++) d |= a[i] ^ b[i];
  return d == 0ull;
}

enum { PAT_JOINED = 0, PAT_MEET, PAT_OVER };

// Walks the chain from `slot` until the line joined the set, met its own tag (slot = where) or ran into the
// capacity.  Bounded by the table; never waits.
__device__ __forceinline__ int pat_walk(const MpcPatternSet &S, const u64 *line, int w8, u64 tag, u32 &slot)
{
  for (u32 probe = 0; probe <= kSlotMask; probe++) {
    u64 t = __hip_atomic_load(&S.tags[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (t == 0ull) {
      const bool full = __hip_atomic_load(&S.ctl[MPC_PSET_DISTINCT], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= (u64)MPC_PATTERN_CAPACITY;
      t = atomicCAS(&S.tags[slot], 0ull, full ? 0ull : tag);
      if (t == 0ull) {
        if (full) {                 // a new line and no room for it
          atomicOr(&S.ctl[MPC_PSET_OVERFLOW], 1ull);
          return PAT_OVER;
        }
        u64 *dst = S.store + (u64)slot * (u64)w8;
        for (int i = 0; i < w8; i++) dst[i] = line[i];
        if (atomicAdd(&S.ctl[MPC_PSET_DISTINCT], 1ull) >= (u64)MPC_PATTERN_CAPACITY) {
          atomicOr(&S.ctl[MPC_PSET_OVERFLOW], 1ull);
          return PAT_OVER;
        }
        return PAT_JOINED;
      }
    }
    if (t == tag) return PAT_MEET;
    slot = (slot + 1u) & kSlotMask;
  }
  atomicOr(&S.ctl[MPC_PSET_OVERFLOW], 2ull);      // (unreachable: the table is never full)
  return PAT_OVER;
}

__device__ __forceinline__ u32 wave_sum(u32 v)
{
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__device__ __forceinline__ void pat_set_flush(u32 joined, u32 existed, u64 *gstats)
{
  joined = wave_sum(joined);
  existed = wave_sum(existed);
  if ((threadIdx.x & 63) == 0) {
    if (joined) atomicAdd(&gstats[MPC_PAT_JOINED], (u64)joined);
    if (existed) atomicAdd(&gstats[MPC_PAT_EXISTED], (u64)existed);
  }
}

__global__ void __launch_bounds__(kThreads)
pattern_claim_kernel(const u64 *__restrict__ lines, u32 n_lines, int w8, MpcPatternSet S, u64 *gstats)
{
  u32 joined = 0;
  const u32 i = blockIdx.x * kThreads + threadIdx.x;
  if (i < n_lines && __hip_atomic_load(&S.ctl[MPC_PSET_OVERFLOW], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0ull) {
    const u64 *line = lines + (u64)i * (u64)w8;
    const u64 hash = pat_hash(line, w8, S.tag_mask);
    u32 slot = (u32)hash & kSlotMask;
    const int r = pat_walk(S, line, w8, hash | 1ull, slot);
    joined = r == PAT_JOINED ? 1u : 0u;
    if (r == PAT_MEET) {
      const u32 at = (u32)atomicAdd(&S.ctl[MPC_PSET_PENDING_A], 1ull);
      if (at < MPC_PATTERN_CHUNK) S.pend_a[at] = make_uint2(i, slot);
    }
  }
  pat_set_flush(joined, 0u, gstats);
}

// one pending line: the slot it met its tag at is complete by now
__device__ __forceinline__ int pat_resolve(const MpcPatternSet &S, const u64 *lines, int w8, uint2 e, u32 &slot, u32 &joined, u32 &existed)
{
  const u64 *line = lines + (u64)e.x * (u64)w8;
  slot = e.y;
  if (pat_equal(line, S.store + (u64)slot * (u64)w8, w8)) {
    existed++;
    return PAT_JOINED;
  }
  slot = (slot + 1u) & kSlotMask;
  const int r = pat_walk(S, line, w8, pat_hash(line, w8, S.tag_mask) | 1ull, slot);
  joined += r == PAT_JOINED ? 1u : 0u;
  return r;
}

__global__ void __launch_bounds__(kThreads)
pattern_compare_kernel(const u64 *__restrict__ lines, int w8, MpcPatternSet S, u64 *gstats)
{
  u32 joined = 0, existed = 0;
  const u64 n = min(S.ctl[MPC_PSET_PENDING_A], (u64)MPC_PATTERN_CHUNK);
  for (u64 k = (u64)blockIdx.x * kThreads + threadIdx.x; k < n; k += (u64)gridDim.x * kThreads) {
    const uint2 e = S.pend_a[k];
    u32 slot;
    if (pat_resolve(S, lines, w8, e, slot, joined, existed) == PAT_MEET) {
      const u32 at = (u32)atomicAdd(&S.ctl[MPC_PSET_PENDING_B], 1ull);
      if (at < MPC_PATTERN_CHUNK) S.pend_b[at] = make_uint2(e.x, slot);
    }
  }
  pat_set_flush(joined, existed, gstats);
}

// ONE workgroup: list B in rounds, the lists swapping roles (list A's entries have all been read by then)
__global__ void __launch_bounds__(kThreads)
pattern_tail_kernel(const u64 *__restrict__ lines, int w8, MpcPatternSet S, u64 *gstats)
{
  __shared__ u32 s_next;
  u32 joined = 0, existed = 0;
  u32 n = (u32)min(S.ctl[MPC_PSET_PENDING_B], (u64)MPC_PATTERN_CHUNK);
  uint2 *cur = S.pend_b, *next = S.pend_a;
  for (u32 round = 0; n > 0u && round <= kSlotMask; round++) {
    if (threadIdx.x == 0) s_next = 0;
    __syncthreads();
    for (u32 k = threadIdx.x; k < n; k += kThreads) {
      const uint2 e = cur[k];
      u32 slot;
      if (pat_resolve(S, lines, w8, e, slot, joined, existed) == PAT_MEET) next[atomicAdd(&s_next, 1u)] = make_uint2(e.x, slot);
    }
    __threadfence();
    __syncthreads();         // this round's lines and list are written: the next round may read them
    n = s_next;
    uint2 *t = cur; cur = next; next = t;
    __syncthreads();
  }
  if (n > 0u && threadIdx.x == 0) atomicOr(&S.ctl[MPC_PSET_OVERFLOW], 2ull);   // (unreachable, see pat_walk)
  pat_set_flush(joined, existed, gstats);
}

// n_lines * L < 2^31 (the caller splits longer inputs)
extern "C" hipError_t mpc_launch_pattern(const void *d_lines, u64 n_lines, int L, uint16_t *d_sizes, int8_t *d_sel, u64 *d_stats, int grid,
                                         hipStream_t stream)
{
  const uint4 *l = static_cast<const uint4 *>(d_lines);
  switch (L) {
  case 32: hipLaunchKernelGGL(pattern_kernel<8>, dim3(grid), dim3(kThreads), 0, stream, l, n_lines, d_sizes, d_sel, d_stats); break;
  case 64: hipLaunchKernelGGL(pattern_kernel<16>, dim3(grid), dim3(kThreads), 0, stream, l, n_lines, d_sizes, d_sel, d_stats); break;
  case 128: hipLaunchKernelGGL(pattern_kernel<32>, dim3(grid), dim3(kThreads), 0, stream, l, n_lines, d_sizes, d_sel, d_stats); break;
  default:
    hipLaunchKernelGGL(pattern_any_kernel, dim3(grid), dim3(kThreads), 0, stream, static_cast<const u32 *>(d_lines), n_lines, (u32)(L / 4),
                       d_sizes, d_sel, d_stats);
    break;
  }
  return hipGetLastError();
}

// the three set passes over n_lines <= MPC_PATTERN_CHUNK lines; the caller has zeroed the two pending counters on
// `stream` and lets no other launch of these passes on the same set overlap with this one
extern "C" hipError_t mpc_launch_pattern_set(const void *d_lines, u32 n_lines, int L, const MpcPatternSet *S, u64 *d_stats, int compare_grid,
                                             hipStream_t stream)
{
  if (n_lines == 0 || n_lines > MPC_PATTERN_CHUNK) return n_lines ? hipErrorInvalidValue : hipSuccess;
  const u64 *l = static_cast<const u64 *>(d_lines);
  const int w8 = L / 8;
  hipLaunchKernelGGL(pattern_claim_kernel, dim3((n_lines + kThreads - 1) / kThreads), dim3(kThreads), 0, stream, l, n_lines, w8, *S, d_stats);
  hipLaunchKernelGGL(pattern_compare_kernel, dim3(compare_grid), dim3(kThreads), 0, stream, l, w8, *S, d_stats);
  hipLaunchKernelGGL(pattern_tail_kernel, dim3(1), dim3(kThreads), 0, stream, l, w8, *S, d_stats);
  return hipGetLastError();
}
