// mpc_baselines.h -- device code of the BDI, FPC and BPC baselines for 32-, 64- and 128-byte lines, one copy of
// each piece, used by the kernels of a single handle (bdi_kernel, fpc_kernel, bpc_kernel: mpc_kernels.hip) and by
// the group's kernel (baselines_kernel: mpc_baselines.hip) alike:
//
//   unpack, fetch_line, put_line          a line into the words of a lane; its results out
//   staged_feed (stage_*), ring_feed      how the lines of a launch reach the lanes
//   bdi_check, bdi_screen, bdi_line, BdiLane      BDI: one line; a lane's run of results and its wave's queue
//   fpc_line, FpcAcc                      FPC: one line; a lane's totals
//   bpc_line, BpcAcc                      BPC: one line; a lane's pattern counts
//   cpack_line, CpackAcc                  C-Pack with a per-line dictionary: one line; a lane's totals
//
// Device code only; gfx950.
#pragma once
#include "mpc_kernel_common.h"
#include "mpc_ring.h"

// the 16-byte pieces of a line as its 32-bit words
template <int NQ>
__device__ __forceinline__ void unpack(const uint4 (&v)[NQ], u32 (&w)[4 * NQ])
{
#pragma unroll
  for (int i = 0; i < NQ; i++) { w[4 * i] = v[i].x; w[4 * i + 1] = v[i].y; w[4 * i + 2] = v[i].z; w[4 * i + 3] = v[i].w; }
}

// one line with plain loads (BDI's queued lines, the last partial group of a ring launch)
template <int NW>
__device__ __forceinline__ void fetch_line(const uint4 *__restrict__ lines, u64 line, u32 (&w)[NW])
{
  const uint4 *src = lines + line * (NW / 4);
  uint4 v[NW / 4];
#pragma unroll
  for (int i = 0; i < NW / 4; i++) v[i] = src[i];
  unpack<NW / 4>(v, w);
}

// a line's results into the per-line outputs of a handle that asked for them
__device__ __forceinline__ void put_line(uint16_t *sizes, int8_t *sel, u64 line, u32 size, int select)
{
  if (sizes) sizes[line] = (uint16_t)size;
  if (sel) sel[line] = (int8_t)select;
}

// ---------------------------------------------------------------------------
// Staged loads.  A lane that reads "its" line with NQ
// 16-byte loads makes every load instruction touch 64 B-strided pieces of 32 cache lines; the same 64 lines read
// as NQ fully coalesced, non-temporal loads (instruction k: units k*64 + lane of the group) stream 11 % faster
// (tools/dev/membw.hip: 6.2 -> 6.9 TB/s with the transposition).  The group is brought into one-line-per-lane
// form through 64 x 16 NQ bytes of LDS per wave: unit (line, piece) at line * NQ + (piece ^ f(line)),
// f(line) = (line / (16 / NQ)) mod NQ -- no bank conflicts on either side.  Where they pay: the BPC kernel (188 vector
// instructions per 64 lines: 3.06 -> 2.78 ms per 16 GiB), the FPC kernel since its arithmetic was halved (DESIGN.md
// 4.3b) and the group's kernel at 128 bytes (4.5).  Where more arithmetic waits behind the line the LDS round trip
// costs more than the loads gain: measured slower in the BDI (+3..5 %), the earlier FPC (+4 %) and the VPC lane
// kernels (+11 %, although their all-zero traces run 5 % faster).
// ---------------------------------------------------------------------------
template <int NQ>
__device__ __forceinline__ u32 stage_unit(u32 line, u32 piece)
{
  return line * NQ + (piece ^ ((line / (16u / NQ)) & (NQ - 1u)));
}

template <int NQ>
__device__ __forceinline__ void stage_fetch_rows(uint4 (&v)[NQ], const uint4 *__restrict__ lines, u64 line0, u32 lane, u64 n_lines)
{
  typedef u32 v4u __attribute__((ext_vector_type(4)));
  const u64 last = n_lines * NQ - 1u;      // clamped: units past the end re-read the last one (never evaluated)
#pragma unroll
  for (int k = 0; k < NQ; k++) {
    const u64 u = min(line0 * NQ + (u32)(k * 64) + lane, last);
    const v4u t = __builtin_nontemporal_load(reinterpret_cast<const v4u *>(lines + u));
    v[k] = make_uint4(t.x, t.y, t.z, t.w);
  }
}

template <int NQ>
__device__ __forceinline__ void stage_rows_to_lines(uint4 (&v)[NQ], uint4 *stage, u32 lane)
{
#pragma unroll
  for (int k = 0; k < NQ; k++) {
    const u32 e = (u32)(k * 64) + lane;        // unit e of the group = piece e % NQ of line e / NQ
    stage[stage_unit<NQ>(e / NQ, e % NQ)] = v[k];
  }
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int k = 0; k < NQ; k++) v[k] = stage[stage_unit<NQ>(lane, (u32)k)];
  __builtin_amdgcn_wave_barrier();             // the next group's writes stay behind these reads
}

// The lines of a launch through staged loads, grid-stride over the waves: body(w, line, active) once per lane and
// group of 64 lines, stage = the wave's 64 * NW / 4 units of LDS.  A lane past the end of the trace is handed the
// last unit's words with active = false: a body that votes across the wave (bdi_line) needs every lane, any other
// returns at once.
template <int NW, typename Body>
__device__ __forceinline__ void staged_feed(const uint4 *__restrict__ lines, u64 n_lines, uint4 *stage, u32 lane, Body body)
{
  // (blockDim.x: read like this, a device function gets the same scalar load as a kernel does; written as blockDim.x it
  // gets the form that allows for a partial last workgroup, and every kernel two more VGPRs for the stride)
  const u32 threads = __builtin_amdgcn_workgroup_size_x();
  for (u64 line0 = (u64)blockIdx.x * threads + (threadIdx.x & ~63u); line0 < n_lines; line0 += (u64)gridDim.x * threads) {
    u32 w[NW];
    {
      uint4 v[NW / 4];
      stage_fetch_rows<NW / 4>(v, lines, line0, lane, n_lines);
      stage_rows_to_lines<NW / 4>(v, stage, lane);
      unpack<NW / 4>(v, w);
    }
    body(w, line0 + lane, line0 + lane < n_lines);
  }
}

// The lines of a launch through a per-wave ring in LDS (mpc_ring.h: LDS-DMA, non-temporal, one line per lane on the
// way out): ONE stage of 64 lines per wave (ring: 4 stages of 64 * NW / 4 units, 1 KiB-aligned), re-requested as soon
// as it has been read out, whole groups assigned grid-stride over the waves (4 per workgroup); the launch's last,
// partial group with plain loads, by one wave.  group(w, line, active) once per lane and group; qn is the caller's
// wave-uniform state that travels through the group code (see uni(), mpc_ring.h).
template <int NW, typename Group>
__device__ __forceinline__ void ring_feed(const uint4 *__restrict__ lines, u64 n_lines, uint4 *ring, u32 lane, u32 wave, u32 &qn, Group group)
{
  constexpr int NQ = NW / 4;
  constexpr u32 SB = 64u * 16u * NQ;            // bytes of a stage
  const u32 ring_lds = (u32)(uintptr_t)(__attribute__((address_space(3))) void *)ring + wave * SB;
  u32 lane_off[NQ];
#pragma unroll
  for (int j = 0; j < NQ; j++) lane_off[j] = ring_src_off<NQ>(j, lane);
  const u32 rd0 = (ring_lds + 16u * NQ * lane) | (16u * ring_swz<NQ>(lane));
  const u64 full_groups = n_lines >> 6, gstride = (u64)gridDim.x * 4u;
  u64 g = (u64)blockIdx.x * 4u + wave;
  auto request = [&](u64 gg) { ring_request<NQ>(lane_off, lines + gg * (64u * NQ), ring_lds); };
  if (g < full_groups) request(g);
  while (g < full_groups) {
    qn = uni(qn);
    ring_wait_vm<0>();
    u32 a[NQ];
#pragma unroll
    for (int j = 0; j < NQ; j++) a[j] = rd0 ^ (16u * (u32)j);
    uint4 v[NQ];
    ring_read<NQ>(v, a);
    if (uni(g + gstride < full_groups)) request(g + gstride);       // the stage is free again
    __builtin_amdgcn_sched_barrier(0);
    u32 w[NW];
    unpack<NQ>(v, w);
    group(w, g * 64u + lane, true);
    g += gstride;
  }
  if ((n_lines & 63ull) != 0ull && blockIdx.x == 0 && wave == 0u) {
    const u64 line = full_groups * 64u + lane;
    const bool active = line < n_lines;
    u32 w[NW];
    fetch_line<NW>(lines, active ? line : n_lines - 1, w);
    group(w, line, active);
  }
}

// ---------------------------------------------------------------------------
// BDI (reference BDI.cpp): one lane per line, line in registers.
//
// reduceSign (BDI.cpp:203-218) strips the leading ones of a negative 64-bit value down to
// one sign bit and returns -1 unchanged, so "reduceSign(x) <= 2^(8D)-1" is the range test
//        0 <= x <= 2^(8D)-1     or     -2^(8D-1) <= x <= -2          (x as signed 64-bit)
// (a delta of exactly -1 is rejected, +128..+255 is accepted for D = 1, as in the
// reference).  The kernel evaluates that range test directly; no bit loops.
// ---------------------------------------------------------------------------
template <int D>   // x = (hi, lo)
__device__ __forceinline__ bool bdi_fits64(u32 hi, u32 lo)
{
  if constexpr (D == 4) {
    return (hi == 0u) || (hi == 0xffffffffu && lo >= 0x80000000u && lo != 0xffffffffu);
  } else {
    constexpr u32 h = 1u << (8 * D - 1), lim = (1u << (8 * D)) - 1u;
    // t = lo + h: the accepted ranges become [0, h-2] (carry, hi = -1) and [h, h+lim] (no carry, hi = 0)
    const u32 t = lo + h;
    const u32 carry = t < lo ? 1u : 0u;
    return (hi + carry == 0u) && (t <= h + lim) && (t != h - 1u);
  }
}

// values narrower than 64 bits are zero-extended (BDI.cpp:150-151 is a no-op), so an
// immediate is simply v <= limit and a delta base - v lies in (-2^32, 2^32)
template <int D>
__device__ __forceinline__ bool bdi_fits_delta32(u32 base, u32 v)
{
  constexpr u32 h = 1u << (8 * D - 1), lim = (1u << (8 * D)) - 1u;
  const u32 d = base - v;                       // wraps when base < v
  return base >= v ? (d <= lim) : (d >= 0u - h && d <= 0xfffffffeu);
}

struct BdiScan {      // state of one (base size, delta size) scan over the values of a line
  u32 imm;
  bool have_base, not_all;
};

template <int B, int D, int NW>
__device__ __forceinline__ u32 bdi_check(const u32 *w)   // BDI.cpp:108-201
{
  constexpr u32 n = (NW * 4) / B;
  constexpr u32 lim = D == 4 ? 0xffffffffu : ((1u << (8 * D)) - 1u);
  u32 imm = 0;
  bool have_base = false, not_all = false;
  u32 base_lo = 0, base_hi = 0;
#pragma unroll
  for (u32 i = 0; i < n; i++) {
    u32 lo, hi = 0;
    if constexpr (B == 8) { lo = w[2 * i]; hi = w[2 * i + 1]; }
    else if constexpr (B == 4) lo = w[i];
    else lo = (w[i >> 1] >> (16 * (i & 1))) & 0xffffu;
    bool is_imm;
    if constexpr (B == 8) is_imm = bdi_fits64<D>(hi, lo);
    else is_imm = lo <= lim;
    imm += is_imm ? 1u : 0u;
    const bool first = !is_imm && !have_base;
    bool ok;   // base - v fits the delta width
    if constexpr (B == 8) {
      const u32 dlo = base_lo - lo;
      const u32 dhi = base_hi - hi - (base_lo < lo ? 1u : 0u);
      ok = bdi_fits64<D>(dhi, dlo);
    } else {
      ok = bdi_fits_delta32<D>(base_lo, lo);
    }
    not_all = not_all || (!is_imm && have_base && !ok);
    base_lo = first ? lo : base_lo;
    if constexpr (B == 8) base_hi = first ? hi : base_hi;
    have_base = have_base || !is_imm;
  }
  // 32-bit unsigned arithmetic incl. the wrap when every value is an immediate (BDI.cpp:200)
  if (not_all) return n + 8u * ((imm * (u32)D) + ((n - imm) * (u32)B));
  return n + 8u * ((imm * (u32)D) + ((u32)B + (n - imm - 1u) * (u32)D));
}

// ---------------------------------------------------------------------------
// Screening.  A scan that fails (some delta does not fit) with imm immediates costs
// n + 8*(imm*D + (n-imm)*B) = n + 8L - 8*imm*(B-D) bits (BDI.cpp:196-198), and
// CompressLine keeps only strictly smaller sizes (BDI.cpp:40-66): when that cost is
// not below the best size found so far the combination cannot be selected and need not
// be evaluated.  bdi_screen() finds, per lane and cheaply, combinations whose scan
// certainly fails (value 0 is the base, one of three later values is a non-immediate witness
// whose delta does not fit) and a floor of the failed cost from an upper bound of the
// immediates (exact for 4- and 2-byte bases); the kernel skips a combination when
// "fails and floor >= best" holds on every active lane of the wave and runs the exact
// scan otherwise.
// ---------------------------------------------------------------------------

// class k of a signed 64-bit value x = (hi, lo):  reduceSign(x) <= 2^(8D)-1  <=>  k <= 8D
__device__ __forceinline__ u32 bdi_class64(u32 hi, u32 lo)
{
  const u32 sx = (u32)((int)hi >> 31);
  const u32 y = lo ^ sx;                                   // magnitude bits below the sign
  const u32 k = 32u - (u32)__clz((int)y) - sx;             // + 1 sign bit for negative values
  const bool out = (hi != sx) || ((lo & hi) == 0xffffffffu);   // beyond 32 bits, or x == -1
  return out ? 64u : k;
}

// the same for base - v of two zero-extended 32-bit values
__device__ __forceinline__ u32 bdi_class_delta32(u32 base, u32 v)
{
  const u32 d = base - v;
  const u32 sx = base < v ? 0xffffffffu : 0u;
  const u32 y = d ^ sx;
  const u32 k = 32u - (u32)__clz((int)y) - sx;
  return (sx && y == 0u) ? 64u : k;                       // base - v == -1 never fits
}

// the three witness values of a screen over n values: the second, the middle and the last one (on smooth data
// -- samples of a waveform, counters -- the values far from the base show the misfitting delta first; values
// 1..3 let such lines through to the exact scans)
#ifndef MPC_BDI_WITNESS
#define MPC_BDI_WITNESS(j, n) ((j) == 0 ? 1 : (j) == 1 ? (n) / 2 : (n) - 1)
#endif

struct BdiScreen {
  u32 fails;      // bit c: the scan of combination c (B8D1, B8D2, B8D4, B4D1, B4D2, B2D1) certainly fails
  u32 allimm;     // bit c: every value is an immediate of combination c (its cost is then a constant; exact counts: c >= 3)
  u32 floor[6];   // if it fails it costs at least this many bits
};

template <int NW>
__device__ __forceinline__ BdiScreen bdi_screen(const u32 *w)
{
  constexpr u32 L8 = 32u * NW;     // 8 * L
  BdiScreen sc;
  sc.fails = 0;
  sc.allimm = 0;
  {   // 8-byte bases: a value can only be an immediate (any D) when its high word is 0 or -1
    constexpr int n = NW / 2;
    u32 cnt = 0;   // upper bound of the immediates of every D
#pragma unroll
    for (int i = 0; i < n; i++) cnt += (w[2 * i + 1] + 1u <= 1u) ? 1u : 0u;
    // value 0 is the base when it cannot be an immediate; witnesses: three later values that cannot be
    // immediates either and whose delta does not fit
    const bool base0 = w[1] + 1u > 1u;
    u32 kd = 0;
#pragma unroll
    for (int j = 0; j < (n < 4 ? n - 1 : 3); j++) {
      const int i = MPC_BDI_WITNESS(j, n);
      const u32 dlo = w[0] - w[2 * i];
      const u32 dhi = w[1] - w[2 * i + 1] - (w[0] < w[2 * i] ? 1u : 0u);
      const u32 k = bdi_class64(dhi, dlo);
      kd = max(kd, (w[2 * i + 1] + 1u > 1u) ? k : 0u);
    }
    sc.fails |= (base0 && kd > 8u) ? 1u : 0u;
    sc.fails |= (base0 && kd > 16u) ? 2u : 0u;
    sc.fails |= (base0 && kd > 32u) ? 4u : 0u;
    sc.floor[0] = (u32)n + L8 - 8u * 7u * cnt;
    sc.floor[1] = (u32)n + L8 - 8u * 6u * cnt;
    sc.floor[2] = (u32)n + L8 - 8u * 4u * cnt;
  }
  {   // 4-byte bases: exact immediate counts
    constexpr int n = NW;
    u32 i1 = 0, i2 = 0;
#pragma unroll
    for (int i = 0; i < n; i++) {
      i1 += w[i] <= 0xffu ? 1u : 0u;
      i2 += w[i] <= 0xffffu ? 1u : 0u;
    }
    bool f1 = false, f2 = false;
#pragma unroll
    for (int j = 0; j < 3; j++) {
      const int i = MPC_BDI_WITNESS(j, n);
      const u32 kd = bdi_class_delta32(w[0], w[i]);
      f1 = f1 || (w[i] > 0xffu && kd > 8u);
      f2 = f2 || (w[i] > 0xffffu && kd > 16u);
    }
    sc.fails |= (w[0] > 0xffu && f1) ? 8u : 0u;
    sc.fails |= (w[0] > 0xffffu && f2) ? 16u : 0u;
    sc.floor[3] = (u32)n + L8 - 8u * 3u * i1;
    sc.floor[4] = (u32)n + L8 - 8u * 2u * i2;
    sc.allimm |= (i1 == (u32)n ? 8u : 0u) | (i2 == (u32)n ? 16u : 0u);
  }
  {   // 2-byte bases: immediates are the 16-bit values with a zero high byte
    constexpr int n = 2 * NW;
    u32 nz = 0;   // values with a non-zero high byte
#pragma unroll
    for (int i = 0; i < NW; i++) {
      const u32 x = w[i] & 0xff00ff00u;
      nz += (u32)__popc((((x & 0x7f007f00u) + 0x7f007f00u) | x) & 0x80008000u);
    }
    const u32 v0 = w[0] & 0xffffu;
    bool f = false;
#pragma unroll
    for (int j = 0; j < 3; j++) {
      const int i = MPC_BDI_WITNESS(j, n);
      const u32 v = (w[i >> 1] >> (16 * (i & 1))) & 0xffffu;
      const u32 t = v0 - v + 128u;      // delta in [0,255] or [-128,-2]  <=>  t in [128,383] or [0,126]
      f = f || (v > 0xffu && !(t <= 383u && t != 127u));
    }
    sc.fails |= (v0 > 0xffu && f) ? 32u : 0u;
    sc.floor[5] = (u32)n + L8 - 8u * ((u32)n - nz);
    sc.allimm |= nz == 0u ? 32u : 0u;
  }
  return sc;
}

// One line (words w).  DEFER: exact scans that only a few lines of the wave's group need are not run for the
// whole wave; those lines are flagged `deferred` instead (the caller queues them) and evaluated later, 64 at a
// time, with DEFER = false.  Lanes that take no part pass active = false.
#ifndef MPC_BDI_DEFER_MAX
#define MPC_BDI_DEFER_MAX 12
#endif
template <int NW, bool DEFER>
__device__ __forceinline__ void bdi_line(const u32 (&w)[NW], bool active, bool room, u32 &best, int &select, bool &deferred)
{
  constexpr u32 uncomp = 32u * NW;
  u32 any = 0, rep = 0;
#pragma unroll
  for (int i = 0; i < NW; i++) {
    any |= w[i];
    rep |= w[i] ^ w[i & 1];
  }
  best = uncomp;
  select = 8;
  deferred = false;
  if (any == 0) {
    best = 8;
    select = 0;
  } else if (rep == 0) {
    best = 64;
    select = 1;
  } else if (active) {
    // a combination whose scan certainly fails at a cost >= the lane's best so far cannot be
    // selected; it is skipped when that holds on every active lane of the wave
    const BdiScreen sc = bdi_screen<NW>(w);
    u32 c;
    // a scan that succeeds costs n + 8*(B + (n-1)*D) bits whatever the immediates are (imm*D +
    // B + (n-imm-1)*D), and a failed one more: a combination whose success cost is not below
    // the lane's best so far cannot be selected either
#define MPC_BDI_TRY(IDX, B, D)                                                      \
    {                                                                               \
      constexpr u32 n_ = (NW * 4) / B, ok_cost_ = n_ + 8u * ((u32)B + (n_ - 1u) * (u32)D);   \
      /* every value an immediate: n + 8 (n D + B + (n - n - 1) D) in 32-bit wrap (BDI.cpp:200), no scan needed */ \
      constexpr u32 allimm_cost_ = n_ + 8u * (n_ * (u32)D + ((u32)B + (0u - 1u) * (u32)D));  \
      const bool known_ = (sc.allimm >> IDX) & 1u;                                  \
      if (known_ && best > allimm_cost_) { best = allimm_cost_; select = IDX + 2; } \
      const bool want_ = !deferred && !known_ && ok_cost_ < best && (!((sc.fails >> IDX) & 1u) || sc.floor[IDX] < best);   \
      const u64 wm_ = __ballot(want_);                                              \
      if (wm_) {                                                                    \
        if (DEFER && room && __popcll(wm_) <= MPC_BDI_DEFER_MAX) {                  \
          deferred = deferred || want_;                                             \
        } else {                                                                    \
          c = bdi_check<B, D, NW>(w);                                               \
          if (want_ && best > c) { best = c; select = IDX + 2; }                    \
        }                                                                           \
      }                                                                             \
    }
    MPC_BDI_TRY(0, 8, 1)
    MPC_BDI_TRY(1, 8, 2)
    MPC_BDI_TRY(2, 8, 4)
    MPC_BDI_TRY(3, 4, 1)
    MPC_BDI_TRY(4, 4, 2)
    MPC_BDI_TRY(5, 2, 1)
#undef MPC_BDI_TRY
    if (best == uncomp) select = 8;
  }
}

constexpr u32 kBdiQueue = 384;      // deferred lines per wave (LDS)
// A launch of more lines than this defers nothing: a queue entry is a 32-bit line index.  The test library draws the
// limit at 2^20 - 1 lines, so that a launch of a few MiB runs bdi_line's inline scans (tests/test_launch_splits_gpu.py).
constexpr u64 kBdiDeferMaxLines = MPC_TESTING ? 0xfffffull : 0xffffffffull;

// BDI's state of one lane beyond the line at hand: the run of equal results it has not counted yet, and its wave's
// queue of deferred lines.  sizes / sel: the handle's per-line outputs (or null); counts: the workgroup's raw
// statistics (LDS); queue: kBdiQueue entries of LDS per wave; routes: the test library's route counters, which sit
// behind the handle's raw statistics for bdi_kernel and for the group's BDI member alike (never read in the product
// build, which has no such code: MPC_TESTING is 0).
struct BdiLane {
  uint16_t *sizes;
  int8_t *sel;
  u64 *counts;
  u32 *queue;
  u64 *routes;
  u32 run_key = 0xffffffffu, run_cnt = 0;      // run-length accumulation: (select, size) key, count
  u32 qn = 0;                                   // queued lines of this wave (wave-uniform)

  // the run so far into the workgroup's counts
  __device__ __forceinline__ void flush()
  {
    if (run_cnt) {
      atomicAdd(&counts[run_key >> 16], (u64)run_cnt);
      atomicAdd(&counts[9], (u64)run_cnt * (u64)(run_key & 0xffffu));
    }
  }
  __device__ __forceinline__ void account(u64 line, u32 best, int select)
  {
    const u32 size = best + 4u;
    put_line(sizes, sel, line, size, select);
    const u32 key = ((u32)select << 16) | size;
    if (key != run_key) {
      flush();
      run_key = key;
      run_cnt = 0;
    }
    run_cnt++;
  }
  // the lines of the wave's group that want to be deferred, in lane order (every lane calls)
  __device__ __forceinline__ void push(u64 line, bool want)
  {
    const u64 dmask = __ballot(want);
    if (dmask) {
      const u32 rank = __builtin_amdgcn_mbcnt_hi((u32)(dmask >> 32), __builtin_amdgcn_mbcnt_lo((u32)dmask, 0u));
      if (want) queue[qn + rank] = (u32)line;
      qn += (u32)__popcll(dmask);
    }
  }
  // the queued lines, 64 at a time, every scan they need
  template <int NW>
  __device__ __forceinline__ void drain(const uint4 *__restrict__ lines, u32 lane)
  {
    while (qn > 0u) {
      const u32 take = qn < 64u ? qn : 64u;
      qn -= take;
      if (MPC_TESTING && routes && lane == 0) {
        route_add(routes, MPC_RT_BDI_DRAINS, 1u);
        route_add(routes, MPC_RT_BDI_DEFERRED, take);
      }
      const bool active = lane < take;
      const u64 line = active ? (u64)queue[qn + lane] : 0ull;
      u32 w[NW];
      fetch_line<NW>(lines, line, w);
      u32 best;
      int select;
      bool deferred;
      bdi_line<NW, false>(w, active, false, best, select, deferred);
      if (active) account(line, best, select);
    }
  }
  // one group of 64 lines held in w (every lane stays in: bdi_line votes across the wave and qn must stay uniform).
  // DEFER: exact scans that few lines of the group need are queued (can_defer: the queue's 32-bit entries can hold
  // the launch's line indices) and run once the queue may not have room for another group's; without it no line is
  // ever flagged and the queue stays empty.
  template <int NW, bool DEFER>
  __device__ __forceinline__ void group(const uint4 *__restrict__ lines, u32 lane, const u32 (&w)[NW], u64 line, bool active, bool can_defer)
  {
    u32 best;
    int select;
    bool deferred;
    bdi_line<NW, DEFER>(w, active, can_defer, best, select, deferred);
    push(line, active && deferred);
    if (active && !deferred) account(line, best, select);
    if (qn + 64u > kBdiQueue) drain<NW>(lines, lane);        // wave-uniform: room for the next group's deferrals
  }
};

// ---------------------------------------------------------------------------
// FPC (reference FPC.cpp:7-88): frequent pattern compression of the line's 32-bit
// little-endian words; one lane per line, line in registers.  The sign-extension tests of
// the reference are range tests: (v & 0xFFFFFFF8) in {0, 0xFFFFFFF8}  <=>  v + 8 < 16, etc.
// A zero run costs 3 + 3 bits once, its further words nothing (FPC.cpp:20-32); a run ends
// at the end of the line (the reference reads past it there: undefined behaviour, see
// DESIGN.md "Deliberate deviations").
// ---------------------------------------------------------------------------
// prefix number of one word (the reference's tests in their order; used by the any-line-size kernel below)
__device__ __forceinline__ u32 fpc_prefix(u32 v)
{
  // width of v as a sign-extended number: nb significant bits below the sign
  const u32 nb = 32u - (u32)__clz((int)(v ^ (u32)((int)v >> 31)));
  const u32 lo = v & 0xffffu, hi = v >> 16;
  const bool halves = (((lo + 128u) & 0xffffu) < 256u) && (((hi + 128u) & 0xffffu) < 256u);
  const bool rep = v == (v & 0xffu) * 0x01010101u;
  return v == 0u ? 0u : nb <= 3u ? 1u : nb <= 7u ? 2u : nb <= 15u ? 3u : lo == 0u ? 4u : halves ? 5u : rep ? 6u : 7u;
}

// Classification without a prefix number (the unrolled kernels).  With y = v ^ (v << 1), bit i+1 of y says "bits i+1 and i of v differ", so
// "v is a sign-extended k-bit number" (bits 31 .. k-1 all equal) is y < 2^k: prefixes 1, 2, 3 are y < 16, y < 256,
// y < 65536 -- nested, and zero lies inside all of them -- and "both halfwords are sign-extended bytes" is
// (y & 0xff00ff00) == 0.  Nested tests need no exclusivity: the kernel counts how many words pass each of them and
// takes differences when it flushes.  The size of a line is linear in its counts:
//   35 NW + 6 runs - 7 n(zero) - 4 n(y<16) - 8 n(y<256) - 16 (n(y<65536) + n4 + n5) - 24 n6
// (n4, n5, n6: padded halfword / two sign-extended bytes / repeated bytes, each exclusive of the tests before it).
struct FpcCounts { u32 z, c1, c2, c3, e4, e5, e6, runs; };

__device__ __forceinline__ void fpc_word(u32 v, bool &prev_zero, FpcCounts &n)
{
  const u32 y = v ^ (v << 1);
  const bool z = v == 0u;
  const bool c1 = y < 16u, c2 = y < 256u, c3 = y < 65536u;
  const bool c4 = (v << 16) == 0u;                                   // low halfword zero (FPC.cpp: padded halfword)
  const bool c5 = (y & 0xff00ff00u) == 0u;
  const bool c6 = v == __builtin_amdgcn_alignbit(v, v, 8);           // four equal bytes
  const bool e4 = c4 && !c3, e5 = c5 && !c3 && !c4, e6 = c6 && !c3 && !c4 && !c5;
  n.z += z ? 1u : 0u;
  n.c1 += c1 ? 1u : 0u;
  n.c2 += c2 ? 1u : 0u;
  n.c3 += c3 ? 1u : 0u;
  n.e4 += e4 ? 1u : 0u;
  n.e5 += e5 ? 1u : 0u;
  n.e6 += e6 ? 1u : 0u;
  n.runs += (z && !prev_zero) ? 1u : 0u;
  prev_zero = z;
}

// one line: its counts into n (zeroed by the caller), its size in bits returned
template <int NW>
__device__ __forceinline__ u32 fpc_line(const u32 (&w)[NW], FpcCounts &n)
{
  bool prev_zero = false;
#pragma unroll
  for (int i = 0; i < NW; i++) fpc_word(w[i], prev_zero, n);
  // bits per prefix: 6, 7, 11, 19, 19, 19, 11, 35 (PREFIX_SIZE + payload, FPC.h:8 + FPC.cpp); a zero run pays once
  return 35u * NW + 6u * n.runs - 7u * n.z - 4u * n.c1 - 8u * n.c2 - 16u * (n.c3 + n.e4 + n.e5) - 24u * n.e6;
}
// FPC's totals of one lane: counts of the words that passed each test, words, bits
struct FpcAcc {
  FpcCounts tot = {0, 0, 0, 0, 0, 0, 0, 0};
  u32 words = 0;
  u64 bits = 0;

  // per-lane totals -> the workgroup's prefix counts (Prefix0..7) and bits
  __device__ __forceinline__ void flush(u64 *s_counts)
  {
    const FpcCounts &t = tot;
    const u32 c[8] = {t.z, t.c1 - t.z, t.c2 - t.c1, t.c3 - t.c2, t.e4, t.e5, t.e6, words - t.c3 - t.e4 - t.e5 - t.e6};
#pragma unroll
    for (int k = 0; k < 8; k++)
      if (c[k]) atomicAdd(&s_counts[k], (u64)c[k]);
    if (bits) atomicAdd(&s_counts[8], bits);
    tot = FpcCounts{0, 0, 0, 0, 0, 0, 0, 0};
    words = 0;
    bits = 0;
  }
  // one line of nw words: its counts n and its size
  __device__ __forceinline__ void add(const FpcCounts &n, u32 size, u32 nw, u64 *s_counts)
  {
    tot.z += n.z; tot.c1 += n.c1; tot.c2 += n.c2; tot.c3 += n.c3; tot.e4 += n.e4; tot.e5 += n.e5; tot.e6 += n.e6;
    words += nw;
    bits += size;
    if (words >= (1u << 30)) flush(s_counts);      // far from overflow of the 32-bit totals
  }
};

// ---------------------------------------------------------------------------
// BPC (reference BPC.cpp:20-185): deltas of consecutive 32-bit words (33-bit two's
// complement: the words are zero-extended, see DESIGN.md "Deliberate deviations"), the 33
// delta bit planes DBP[c] (bit r = bit c of delta r), DBX[c] = DBP[c] ^ DBP[c+1], coded from
// plane 32 down: zero-DBX runs (3 bits for one plane, 7 for 2..33), zero DBP 5, all ones
// (0x7fffffff, i.e. only with 31 deltas) 5, one 1 / two adjacent 1s 10, anything else 32
// bits; the first word always costs 3 + 4 bits (BPC.cpp:96-108 assigns in its first test).
//
// One lane per line, and no bit transpose: the planes are classified where they lie.  Per delta r
// the word X_r = d_r ^ (d_r >> 1) (33-bit shift) holds bit c of DBX[c] at bit c, so "how many ones
// has DBX[c]" is a count per bit POSITION over the X_r -- carry-save adders on v_bitop3_b32, all 32
// low planes at once -- "two adjacent ones" is the OR of X_r & X_(r+1), "DBP[c] == 0" the OR of the
// d_r, "all ones" their AND.  Plane 32 (the borrows) is a single word and handled on its own.
// ---------------------------------------------------------------------------
// One line: its pattern counts added into the 16-bit fields of even / odd (patterns 0,2,4,6 / 1,3,5), its size in
// bits returned.
template <int NW>
__device__ __forceinline__ u32 bpc_line(const u32 (&w)[NW], u64 &even, u64 &odd)
{
  constexpr int ND = NW - 1;                           // deltas = bits of a plane
  // deltas (low words d_r, sign s_r = 0 / ~0 = bits 32.. of the 33-bit delta) and X_r
  u32 X[ND];
  u32 orD = 0, andX = ~0u, top = 0, adj = 0;
  u32 b0 = 0, b1 = 0, hi = 0, pend = 0;       // ones per plane: bit 0, bit 1, "4 or more"; a waiting carry of weight 2
#pragma unroll
  for (int r = 0; r < ND; r++) {
    const u32 d = w[r + 1] - w[r];
    const u32 sgn = w[r + 1] < w[r] ? ~0u : 0u;
    X[r] = d ^ __builtin_amdgcn_alignbit(sgn, d, 1);          // d ^ ((sign : d) >> 1)
    top = bitop3<((BO_A & BO_B) | BO_C)>(sgn, 1u << r, top);  // plane 32: bit r = the borrow of delta r
    orD |= d;
    if (ND == 31) andX &= X[r];
  }
#pragma unroll
  for (int r = 0; r + 1 < ND; r += 2) {
    // two more planes-words into the count: full adder at weight 1, its carry joins the weight-2 column
    const u32 s = xor3(b0, X[r], X[r + 1]), c = maj3(b0, X[r], X[r + 1]);
    b0 = s;
    if ((r / 2) & 1) {
      const u32 s2 = xor3(b1, pend, c), c4 = maj3(b1, pend, c);
      b1 = s2;
      hi |= c4;
    } else {
      pend = c;
    }
    adj = bitop3<((BO_A & BO_B) | BO_C)>(X[r], X[r + 1], adj);
    if (r + 2 < ND) adj = bitop3<((BO_A & BO_B) | BO_C)>(X[r + 1], X[r + 2], adj);
  }
  {
    // ND is odd (7, 15, 31): one X left, and possibly a waiting carry
    constexpr int last = ND - 1;
    const u32 c = b0 & X[last];
    b0 ^= X[last];
    if ((((ND - 1) / 2) & 1) != 0) {          // a carry is waiting
      const u32 s2 = xor3(b1, pend, c), c4 = maj3(b1, pend, c);
      b1 = s2;
      hi |= c4;
    } else {
      hi |= b1 & c;
      b1 ^= c;
    }
  }
  // classes of the 32 low planes, as bit masks (bit c = plane c)
  const u32 nz = or3(b0, b1, hi);                                   // DBX[c] != 0
  const u32 single = bitop3<(BO_A & ~BO_B & ~BO_C) & 0xFFu>(b0, b1, hi);
  const u32 two = bitop3<(~BO_A & BO_B & ~BO_C) & 0xFFu>(b0, b1, hi) & adj;
  const u32 zero_dbp = nz & ~orD;                                   // DBP[c] == 0 is tested first (BPC.cpp:127)
  const u32 allones = ND == 31 ? (nz & orD & andX) : 0u;            // then DBX[c] == 0x7fffffff
  const u32 rest = nz & ~zero_dbp & ~allones;
  const u32 one_two = rest & (single | two);
  const u32 unc = rest & ~(single | two);
  // plane 32: DBX[32] = DBP[32] = the borrows
  const u32 t_ones = (u32)__popc(top);
  const bool t_nz = top != 0u;
  const bool t_all = ND == 31 && top == 0x7fffffffu;
  const bool t_one = !t_all && t_ones == 1u;
  const bool t_two = !t_all && t_ones == 2u && (top & (top >> 1)) != 0u;
  const bool t_unc = t_nz && !t_all && !t_one && !t_two;
  // zero-DBX runs in coding order 32 .. 0: bit c of Z = DBX[c] == 0
  const u64 Z = ((u64)(t_nz ? 0u : 1u) << 32) | (u64)(~nz);
  const u64 starts = Z & ~(Z >> 1);                 // the plane above is not zero (or there is none)
  const u64 longer = starts & (Z << 1);             // ... and the plane below is zero too: a run of 2 or more
  const u32 n_runs = (u32)__popcll(starts);
  const u32 n_zero = (u32)__popc(zero_dbp), n_all = (u32)__popc(allones) + (t_all ? 1u : 0u);
  const u32 n_one = (u32)__popc(rest & single) + (t_one ? 1u : 0u);
  const u32 n_two = (u32)__popc(rest & two & ~single) + (t_two ? 1u : 0u);
  const u32 n_unc = (u32)__popc(unc) + (t_unc ? 1u : 0u);
  (void)one_two;
  const u32 length = 3u + 4u + 3u * n_runs + 4u * (u32)__popcll(longer) + 5u * (n_zero + n_all) + 10u * (n_one + n_two) + 32u * n_unc;
  // BPCPattern order: Uncomp, ZRLE, Zero, SingleOne, ConsecTwoOnes, ZeroDBP (never), AllOnes
  even += (u64)n_unc | ((u64)n_zero << 16) | ((u64)n_two << 32) | ((u64)n_all << 48);
  odd += (u64)n_runs | ((u64)n_one << 16);
  return length;
}
// BPC's pattern counts of one lane, in 16-bit fields of even / odd (what bpc_line adds to), planes and bits.  A line
// adds at most 34 to a field (33 planes and the run behind them), so the fields are flushed every 1023 lines:
// 1023 x 34 < 2^16.
struct BpcAcc {
  u64 even = 0, odd = 0;
  u64 words = 0, bits = 0;
  u32 since_flush = 0;

  __device__ __forceinline__ void flush(u64 *s_counts)
  {
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const u64 e = (even >> (16 * k)) & 0xffffull, o = (odd >> (16 * k)) & 0xffffull;
      if (e) atomicAdd(&s_counts[2 * k], e);
      if (o && k < 3) atomicAdd(&s_counts[2 * k + 1], o);
    }
    if (words) atomicAdd(&s_counts[7], words);
    if (bits) atomicAdd(&s_counts[8], bits);
    even = odd = words = bits = 0;
  }
  // one line whose counts bpc_line has added to even / odd: its size
  __device__ __forceinline__ void add(u32 length, u64 *s_counts)
  {
    words += 33u;                                  // every plane is counted once: as a pattern or inside a run
    bits += length;
    if (++since_flush == 1023u) {
      flush(s_counts);
      since_flush = 0;
    }
  }
};

// ---------------------------------------------------------------------------
// C-Pack with a PER-LINE dictionary (reference CPACK.cpp:7-101 with a fresh comp::CPACK per line; the reference's own
// driver carries the dictionary from line to line, which is not evaluated here: DESIGN.md 8).  The dictionary is a
// FIFO of 16 words, all zero when the line starts.  Per 32-bit word b0 b1 b2 b3 (memory order; b0 = the low byte):
//   b0 = b1 = b2 = 0                       ZZZZ 2 bits if b3 = 0, else ZZZX 12; no dictionary access
//   the FIRST entry from the front with the same (b0, b1) decides: b2 differs MMXX 24, b3 differs MMMX 16, equal MMMM 6;
//     a hit changes nothing
//   no such entry                          XXXX 34; the word is pushed at the back and the front entry leaves
// One lane per line, the line in registers, and no dictionary: with the key of a word = its (b0, b1) and C = the misses
// before it in the line,
//   - pushed entries that are still in the FIFO have pairwise different keys (a word is pushed only when no entry has
//     its key), so at most one entry can match: the LATEST earlier miss with the word's key, if it is still there;
//   - the entry pushed as miss number p (from 0) leaves with miss number p + 16: it is there at a word iff C - p <= 16;
//   - the zero entries are at the front while C < 16: a word with key 0 that is not ZZZ* then gets MMXX (its b2 is not
//     0), and nothing with key 0 has been pushed;
//   - up to 16 words (64 bytes) C <= 15 throughout: nothing is ever evicted, and a word with a non-zero key is decided by
//     the FIRST earlier word with its key (that one missed) -- pairwise compares of the words, no serial dependence.
// The size is linear in nested counts, as FPC's: with a = ZZZ* words, b = ZZZZ, c = hits, d = hits whose b2 is equal,
// e = hits whose b2 and b3 are equal:  34 NW - 22 a - 10 b - 10 c - 8 d - 10 e.  It is not capped (16 misses: 544 bits).
// ---------------------------------------------------------------------------
struct CpackCounts { u32 a, b, c, d, e; };

// one word: zzz = its (b0, b1, b2) are 0; hit and, for a hit, x = (b2, b3) of the word XOR those of the deciding entry
__device__ __forceinline__ void cpack_count(u32 v, bool zzz, bool hit, u32 x, CpackCounts &n)
{
  n.a += zzz ? 1u : 0u;
  n.b += v == 0u ? 1u : 0u;
  n.c += hit ? 1u : 0u;
  n.d += (hit && (x & 0xffu) == 0u) ? 1u : 0u;
  n.e += (hit && x == 0u) ? 1u : 0u;
}

// one line: its counts into n (zeroed by the caller), its size in bits returned
template <int NW>
__device__ __forceinline__ u32 cpack_line(const u32 (&w)[NW], CpackCounts &n)
{
  if constexpr (NW <= 16) {
#pragma unroll
    for (int i = 0; i < NW; i++) {
      const u32 key = w[i] & 0xffffu;
      u32 m = ~w[i];                                   // (no earlier word with this key: the XOR below has a key part)
#pragma unroll
      for (int j = i - 1; j >= 0; j--) m = (w[j] & 0xffffu) == key ? w[j] : m;      // ends at the first such word
      const u32 y = m ^ w[i];
      const bool zzz = (w[i] & 0xffffffu) == 0u;
      const bool zero_entry = key == 0u && !zzz;       // decided by a zero entry: MMXX
      const bool hit = !zzz && (key == 0u || (y & 0xffffu) == 0u);
      cpack_count(w[i], zzz, hit, zero_entry ? 1u : (y >> 16), n);
    }
  } else {
    // the misses so far as (key | none) and ((b2, b3) | miss number << 16); C = their number
    u32 dk[NW], pay[NW];
    u32 C = 0;
#pragma unroll
    for (int i = 0; i < NW; i++) {
      const u32 key = w[i] & 0xffffu, hi = w[i] >> 16;
      u32 m = 0xffff0000u;                             // (no miss with this key: a miss number that is never "still there")
#pragma unroll
      for (int j = 0; j < i; j++) m = dk[j] == key ? pay[j] : m;                     // ends at the latest such miss
      const bool zzz = (w[i] & 0xffffffu) == 0u;
      const bool zero_entry = key == 0u && !zzz && C < 16u;
      const bool there = C - (m >> 16) <= 16u;         // (unsigned: no miss found gives a huge difference)
      const bool hit = !zzz && (zero_entry || there);
      cpack_count(w[i], zzz, hit, zero_entry ? 1u : ((m & 0xffffu) ^ hi), n);
      const bool miss = !zzz && !hit;
      dk[i] = miss ? key : 0xffffffffu;
      pay[i] = hi | (C << 16);
      C += miss ? 1u : 0u;
    }
  }
  return 34u * NW - 22u * n.a - 10u * n.b - 10u * n.c - 8u * n.d - 10u * n.e;
}
// C-Pack's totals of one lane: the nested counts, words, bits
struct CpackAcc {
  CpackCounts tot = {0, 0, 0, 0, 0};
  u32 words = 0;
  u64 bits = 0;

  // per-lane totals -> the workgroup's pattern counts (CPACKPattern order: ZZZZ ZZZX MMMM MMMX MMXX XXXX) and bits
  __device__ __forceinline__ void flush(u64 *s_counts)
  {
    const CpackCounts &t = tot;
    const u32 c[6] = {t.b, t.a - t.b, t.e, t.d - t.e, t.c - t.d, words - t.a - t.c};
#pragma unroll
    for (int k = 0; k < 6; k++)
      if (c[k]) atomicAdd(&s_counts[k], (u64)c[k]);
    if (bits) atomicAdd(&s_counts[6], bits);
    tot = CpackCounts{0, 0, 0, 0, 0};
    words = 0;
    bits = 0;
  }
  // one line of nw words: its counts n and its size
  __device__ __forceinline__ void add(const CpackCounts &n, u32 size, u32 nw, u64 *s_counts)
  {
    tot.a += n.a; tot.b += n.b; tot.c += n.c; tot.d += n.d; tot.e += n.e;
    words += nw;
    bits += size;
    if (words >= (1u << 30)) flush(s_counts);      // far from overflow of the 32-bit totals
  }
};
