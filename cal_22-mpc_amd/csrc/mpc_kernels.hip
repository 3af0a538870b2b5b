// mpc_kernels.hip -- gfx950 (MI355X, CDNA4) kernels of the per-line evaluator other
// than the fast VPC kernel (mpc_vpc_lane.hip):
//
//   vpc_generic_kernel     VPC, any configuration the reference can run
//   bdi_kernel             BDI baseline (reference src/compressor/BDI.cpp)
//   fpc_kernel             FPC baseline (reference src/compressor/FPC.cpp)
//   bpc_kernel             BPC baseline (reference src/compressor/BPC.cpp)
//   synth_kernel / read_probe_kernel   measurement helpers
#include "mpc_kernel_common.h"
#include "mpc_ring.h"
#include "mpc_launch.h"

// ---------------------------------------------------------------------------
// generic VPC kernel: one lane per line, byte loops, any configuration.
// Follows the reference stage by stage; the XOR stage is done on bytes.  The line and the transformed residue
// of the module at hand live in LDS, one padded slice per lane (they are indexed by table entries; as private
// arrays they would sit in scratch memory and every bit of the scan would be a memory access), and so do the
// module tables when they fit (LDSTAB).  Per module the scanned rows are produced in order and fed straight to
// the selector's leading-zero-row count and to the common encoder (FPCModule.cpp:19-85), so only (z, encoded
// size) of the winner so far is kept -- the reference encodes the winner alone, with the same result.
// ---------------------------------------------------------------------------
constexpr int kGenericThreads = 128;

// threads per workgroup: fewer for long lines, whose slices are larger
__host__ __device__ static inline int generic_threads(int L) { return L > 128 ? 64 : kGenericThreads; }
__host__ __device__ static inline size_t generic_lane_smem(int L) { return (size_t)generic_threads(L) * 2u * (size_t)(L + 4); }

template <bool LDSTAB>
__global__ void __launch_bounds__(kGenericThreads)
vpc_generic_kernel(const uint8_t *__restrict__ lines, u64 n_lines, MpcVpcParams P,
                   uint16_t *__restrict__ sizes_out, int8_t *__restrict__ sel_out, u64 *gstats)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int K = P.M + 1, bins = P.hist_bins, L = P.L, R = (8 * L) / 16;
  WgStats st;
  st.sums = reinterpret_cast<u64 *>(smem);
  st.hist = reinterpret_cast<u32 *>(smem + 16 * ((2 * K * 8 + 15) / 16));
  const int slice = L + 4;
  uint8_t *d = smem + vpc_stats_smem(K, bins) + (size_t)threadIdx.x * 2u * (size_t)slice;
  uint8_t *t = d + slice;
  const uint8_t *gt = P.gtab;
  if (LDSTAB) {
    uint8_t *tabs = smem + vpc_stats_smem(K, bins) + generic_lane_smem(L);
    for (int i = threadIdx.x; i < P.gtab_bytes / 4; i += blockDim.x)
      reinterpret_cast<u32 *>(tabs)[i] = reinterpret_cast<const u32 *>(P.gtab)[i];
    gt = tabs;
  }
  stats_init(st, K, bins);      // ends with __syncthreads()

  for (u64 line = (u64)blockIdx.x * blockDim.x + threadIdx.x; line < n_lines; line += (u64)gridDim.x * blockDim.x) {
    const uint8_t *src = lines + line * (u64)L;
    bool zero = true, same = true;
    for (int i = 0; i < L; i += 4) {
      const u32 w = *reinterpret_cast<const u32 *>(src + i);
      *reinterpret_cast<u32 *>(d + i) = w;
      zero = zero && w == 0u;
    }
    for (int i = 4; i < L; i++) same = same && (d[i] == d[i & 3]);
    int chosen;
    u32 size;
    u32 sum_r = 0, sum_r2 = 0;
    bool residue_stat = false;
    if (zero) {
      chosen = 0;
      size = (u32)P.enc_bits[1];
    } else if (P.has_aws && same) {
      chosen = 1;
      size = 32u + (u32)P.enc_bits[2];
    } else {
      int best_q = -1, best_z = 0;
      u32 best_enc = 0;
      for (int q = 0; q < P.n_pred; q++) {
        const MpcGenModule gm = P.gm[q];
        const uint8_t *base = gt + gm.off_base, *dif = gt + gm.off_diff;
        const int8_t *shf = reinterpret_cast<const int8_t *>(gt + gm.off_shift);
        // residue array (root first), already XOR-transformed per byte
        int j = 1;
        for (int i = 0; i < L; i++) {
          if (i == gm.root) continue;
          uint8_t p;
          if (gm.pred_kind == 0) {
            const int s = shf[i];
            const uint8_t b = d[base[i]];
            p = s < 0 ? (uint8_t)(b >> (-s)) : (uint8_t)(b << s);
          } else if (gm.pred_kind == 1) {
            p = (uint8_t)(dif[i] + d[base[i]]);
          } else if (gm.pred_kind == 2) {
            p = d[gm.root];
          } else {
            // inp[i-1]: inp index n -> byte (3 - n / W) of word n % W
            const int n = i - 1, Wd = L / 4;
            p = d[4 * (n % Wd) + (3 - n / Wd)];
          }
          const uint8_t r = (uint8_t)(d[i] - p);
          t[j++] = gm.cx ? (uint8_t)(r ^ (r >> 1)) : (uint8_t)(r ^ ((r & 0x80) ? 0x7f : 0));
        }
        t[0] = d[gm.root];
        // scan (ScanModule.cpp:13-19) row by row; selector count and common encoder on the fly
        const uint16_t *sc = reinterpret_cast<const uint16_t *>(gt + gm.off_scan);
        int z = 0;
        bool leading = true;
        u32 enc = 0, run = 0;
        for (int r = 0; r < R; r++) {
          u32 v = 0;
          const int i0 = 16 * r;
          const int nb = gm.table_size - i0 < 16 ? gm.table_size - i0 : 16;      // entries of this row (rest of the array stays 0)
          if (nb == 16) {
            // a full row: the 16 table entries as 8 words, then 16 independent reads of t (the loads overlap)
            const u32 *sw = reinterpret_cast<const u32 *>(sc + i0);
            u32 ew[8];
#pragma unroll
            for (int k = 0; k < 8; k++) ew[k] = sw[k];
#pragma unroll
            for (int c = 0; c < 16; c++) {
              const u32 e = (ew[c >> 1] >> (16 * (c & 1))) & 0xffffu;
              v |= (u32)((t[e & 0xffu] >> (7u - (e >> 8))) & 1u) << (15 - c);
            }
          } else {
            for (int c = 0; c < nb; c++) {
              const u32 e = sc[i0 + c];
              v |= (u32)((t[e & 0xffu] >> (7u - (e >> 8))) & 1u) << (15 - c);
            }
          }
          if (leading && v == 0) z++; else leading = false;
          if (v == 0) { run++; continue; }
          if (run) enc += run > 1 ? 7u : 4u;
          run = 0;
          const int ones = __popc(v);
          if (ones == 1) enc += 7u;
          else if (ones == 2 && (v & (v >> 1))) enc += 8u;
          else if ((v & 0xff00u) == 0 || (v & 0x00ffu) == 0) enc += 12u;
          else enc += 17u;
        }
        if (run) enc += run > 1 ? 7u : 4u;
        if (best_z <= z) {     // ties go to the later module (VPC.cpp:389)
          best_z = z;
          best_q = q;
          best_enc = enc;
        }
      }
      // with no prediction module the empty array encodes to 0 bits (VPC.cpp:397 with an empty maxScanned)
      const u32 enc = best_q >= 0 ? best_enc : 0u;
      residue_stat = true;
      if (enc < 8u * (u32)L) {
        // note: with no prediction module the empty array encodes to 0 bits, cluster -1
        chosen = best_q >= 0 ? P.start + best_q : -1;
        size = enc;
      } else {
        chosen = -1;
        size = 8u * (u32)L;
      }
      if (chosen >= 0) {
        const MpcGenModule gm = P.gm[best_q];
        const uint8_t *base = gt + gm.off_base, *dif = gt + gm.off_diff;
        const int8_t *shf = reinterpret_cast<const int8_t *>(gt + gm.off_shift);
        for (int i = 0; i < L; i++) {
          uint8_t p;
          if (gm.pred_kind == 2) p = d[gm.root];
          else if (gm.pred_kind == 3) p = (i == 0) ? d[3] : d[4 * ((i - 1) % (L / 4)) + (3 - (i - 1) / (L / 4))];
          else if (i == gm.root) p = d[i];
          else if (gm.pred_kind == 0) {
            const int s = shf[i];
            const uint8_t b = d[base[i]];
            p = s < 0 ? (uint8_t)(b >> (-s)) : (uint8_t)(b << s);
          } else p = (uint8_t)(dif[i] + d[base[i]]);
          const u32 r = (uint8_t)(d[i] - p);
          sum_r += r;
          sum_r2 += r * r;
        }
      } else {
        for (int i = 0; i < L; i++) {
          sum_r += d[i];
          sum_r2 += (u32)d[i] * d[i];
        }
      }
      size += (u32)P.enc_bits[chosen + 1];
    }
    if (sizes_out) sizes_out[line] = (uint16_t)size;
    if (sel_out) sel_out[line] = (int8_t)chosen;
    const int k = chosen + 1;
    atomicAdd(&st.hist[k * bins + (int)size], 1u);
    if (residue_stat) {
      atomicAdd(&st.sums[k], (u64)sum_r);
      atomicAdd(&st.sums[K + k], (u64)sum_r2);
    }
  }
  stats_flush(st, K, bins, gstats);
}

// ---------------------------------------------------------------------------
// Staged loads (MPC_BPC_STAGE).  A lane that reads "its" line with NQ
// 16-byte loads makes every load instruction touch 64 B-strided pieces of 32 cache lines; the same 64 lines read
// as NQ fully coalesced, non-temporal loads (instruction k: units k*64 + lane of the group) stream 11 % faster
// (tools/dev/membw.hip: 6.2 -> 6.9 TB/s with the transposition).  The group is brought into one-line-per-lane
// form through 64 x 16 NQ bytes of LDS per wave: unit (line, piece) at line * NQ + (piece ^ f(line)),
// f(line) = (line / (16 / NQ)) mod NQ -- no bank conflicts on either side.  Used by the BPC kernel (188 vector
// instructions per 64 lines: 3.06 -> 2.78 ms per 16 GiB).  Where more arithmetic waits behind the line the LDS
// round trip costs more than the loads gain: measured slower in the BDI (+3..5 %), FPC (+4 %) and VPC lane kernels
// (+11 %, although their all-zero traces run 5 % faster).
// ---------------------------------------------------------------------------
#ifndef MPC_BPC_STAGE
#define MPC_BPC_STAGE 1
#endif
#ifndef MPC_FPC_STAGE
#define MPC_FPC_STAGE 1
#endif
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

// Lines stream through a per-wave ring in LDS (mpc_ring.h: LDS-DMA, non-temporal, one line per lane on the way out):
// ONE stage of 64 lines per wave, re-requested as soon as it has been read out, groups assigned grid-stride.  With so
// little arithmetic behind a line (random data: every scan is screened out) the kernel sits on the floor of its access
// pattern, and that floor is higher for the ring than for lane-per-line register loads: same box, ms per 16 GiB,
// random 3.07 -> 2.84, sine 3.29 -> 3.12, mixed 3.27 -> 3.06, 128-byte pointers 2.82 -> 2.69.  (Two stages per wave
// leave room for 4 instead of 7 workgroups per CU and measured slower on every trace; FPC and BPC, which already
// transposed coalesced non-temporal loads through LDS, gain nothing from the ring and keep their form.)
template <int NW>   // words per line
__global__ void __launch_bounds__(256)
bdi_kernel(const uint4 *__restrict__ lines, u64 n_lines, uint16_t *__restrict__ sizes_out,
           int8_t *__restrict__ sel_out, u64 *gstats)
{
  constexpr int NQ = NW / 4;
  constexpr u32 SB = 64u * 16u * NQ;            // bytes of a stage
  __shared__ u64 s_counts[MPC_BDI_RAW_LEN];
  __shared__ u32 s_queue[4][kBdiQueue];
  __shared__ __attribute__((aligned(1024))) uint4 s_ring[4 * 64 * NQ];
  if (threadIdx.x < MPC_BDI_RAW_LEN) s_counts[threadIdx.x] = 0;
  __syncthreads();
  // run-length accumulation per lane: (select, size) key, count
  u32 run_key = 0xffffffffu, run_cnt = 0;
  auto account = [&](u64 line, u32 best, int select) {
    const u32 size = best + 4u;
    if (sizes_out) sizes_out[line] = (uint16_t)size;
    if (sel_out) sel_out[line] = (int8_t)select;
    const u32 key = ((u32)select << 16) | size;
    if (key != run_key) {
      if (run_cnt) {
        atomicAdd(&s_counts[run_key >> 16], (u64)run_cnt);
        atomicAdd(&s_counts[9], (u64)run_cnt * (u64)(run_key & 0xffffu));
      }
      run_key = key;
      run_cnt = 0;
    }
    run_cnt++;
  };
  auto fetch = [&](u32 (&w)[NW], u64 line) {
    const uint4 *src = lines + line * (NW / 4);
#pragma unroll
    for (int i = 0; i < NW / 4; i++) {
      const uint4 q = src[i];
      w[4 * i] = q.x; w[4 * i + 1] = q.y; w[4 * i + 2] = q.z; w[4 * i + 3] = q.w;
    }
  };
  const u32 lane = threadIdx.x & 63u;
  const u32 wave = uni(threadIdx.x >> 6);
  u32 *queue = s_queue[wave];

  u32 qn = 0;                                   // queued lines of this wave (wave-uniform)
  const bool can_defer = n_lines <= 0xffffffffull;      // queue entries are 32-bit line indices
  // the queued lines, 64 at a time, every scan they need
  auto drain = [&]() __attribute__((always_inline)) {
    while (qn > 0u) {
      const u32 take = qn < 64u ? qn : 64u;
      qn -= take;
      if (MPC_TESTING && lane == 0) {      // (test library only: route counters behind the statistics)
        route_add(gstats + MPC_BDI_RAW_LEN, MPC_RT_BDI_DRAINS, 1u);
        route_add(gstats + MPC_BDI_RAW_LEN, MPC_RT_BDI_DEFERRED, take);
      }
      const bool active = lane < take;
      const u64 line = active ? (u64)queue[qn + lane] : 0ull;
      u32 w[NW];
      fetch(w, line);
      u32 best;
      int select;
      bool deferred;
      bdi_line<NW, false>(w, active, false, best, select, deferred);
      if (active) account(line, best, select);
    }
  };
  // one group of 64 lines held in w (every lane stays in: qn must stay uniform)
  auto group = [&](const u32 (&w)[NW], u64 line, bool active) __attribute__((always_inline)) {
    u32 best;
    int select;
    bool deferred;
    bdi_line<NW, (NW <= 16)>(w, active, can_defer, best, select, deferred);     // (128-byte lines: deferral measured slower)
    const u64 dmask = __ballot(active && deferred);
    if (dmask) {
      const u32 rank = __builtin_amdgcn_mbcnt_hi((u32)(dmask >> 32), __builtin_amdgcn_mbcnt_lo((u32)dmask, 0u));
      if (active && deferred) queue[qn + rank] = (u32)line;
      qn += (u32)__popcll(dmask);
    }
    if (active && !deferred) account(line, best, select);
    if (qn + 64u > kBdiQueue) drain();        // wave-uniform: room for the next group's deferrals
  };

  // ---- whole groups of 64 lines through the ring, grid-stride over the waves ----
  const u32 ring_lds = (u32)(uintptr_t)(__attribute__((address_space(3))) void *)s_ring + wave * SB;
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
#pragma unroll
    for (int i = 0; i < NQ; i++) { w[4 * i] = v[i].x; w[4 * i + 1] = v[i].y; w[4 * i + 2] = v[i].z; w[4 * i + 3] = v[i].w; }
    group(w, g * 64u + lane, true);
    g += gstride;
  }
  // ---- the launch's last, partial group: plain loads, by one wave ----
  if ((n_lines & 63ull) != 0ull && blockIdx.x == 0 && wave == 0u) {
    const u64 line = full_groups * 64u + lane;
    const bool active = line < n_lines;
    u32 w[NW];
    fetch(w, active ? line : n_lines - 1);
    group(w, line, active);
  }
  drain();
  if (run_cnt) {
    atomicAdd(&s_counts[run_key >> 16], (u64)run_cnt);
    atomicAdd(&s_counts[9], (u64)run_cnt * (u64)(run_key & 0xffffu));
  }
  __syncthreads();
  if (threadIdx.x < MPC_BDI_RAW_LEN && s_counts[threadIdx.x]) atomicAdd(&gstats[threadIdx.x], s_counts[threadIdx.x]);
}

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

// per-lane totals -> the workgroup's prefix counts (Prefix0..7) and bits
__device__ __forceinline__ void fpc_flush(FpcCounts &t, u32 &words, u64 &bits, u64 *s_counts)
{
  const u32 c[8] = {t.z, t.c1 - t.z, t.c2 - t.c1, t.c3 - t.c2, t.e4, t.e5, t.e6, words - t.c3 - t.e4 - t.e5 - t.e6};
#pragma unroll
  for (int k = 0; k < 8; k++)
    if (c[k]) atomicAdd(&s_counts[k], (u64)c[k]);
  if (bits) atomicAdd(&s_counts[8], bits);
  t = FpcCounts{0, 0, 0, 0, 0, 0, 0, 0};
  words = 0;
  bits = 0;
}

// one line: its counts into n (zeroed by the caller), its size in bits returned (fpc_kernel, baselines_kernel)
template <int NW>
__device__ __forceinline__ u32 fpc_line(const u32 (&w)[NW], FpcCounts &n)
{
  bool prev_zero = false;
#pragma unroll
  for (int i = 0; i < NW; i++) fpc_word(w[i], prev_zero, n);
  // bits per prefix: 6, 7, 11, 19, 19, 19, 11, 35 (PREFIX_SIZE + payload, FPC.h:8 + FPC.cpp); a zero run pays once
  return 35u * NW + 6u * n.runs - 7u * n.z - 4u * n.c1 - 8u * n.c2 - 16u * (n.c3 + n.e4 + n.e5) - 24u * n.e6;
}

template <int NW>   // words per line
__global__ void __launch_bounds__(256)
fpc_kernel(const uint4 *__restrict__ lines, u64 n_lines, uint16_t *__restrict__ sizes_out,
           int8_t *__restrict__ sel_out, u64 *gstats)
{
  __shared__ u64 s_counts[MPC_FPC_RAW_LEN];
  if (threadIdx.x < MPC_FPC_RAW_LEN) s_counts[threadIdx.x] = 0;
  __syncthreads();
  FpcCounts tot = {0, 0, 0, 0, 0, 0, 0, 0};
  u32 words = 0;
  u64 bits_acc = 0;
#if MPC_FPC_STAGE
  __shared__ uint4 s_stage[4][64 * (NW / 4)];
  const u32 lane = threadIdx.x & 63u;
  uint4 *stage = s_stage[__builtin_amdgcn_readfirstlane(threadIdx.x >> 6)];
  for (u64 line0 = (u64)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); line0 < n_lines; line0 += (u64)gridDim.x * blockDim.x) {
    const u64 line = line0 + lane;
    u32 w[NW];
    {
      uint4 v[NW / 4];
      stage_fetch_rows<NW / 4>(v, lines, line0, lane, n_lines);
      stage_rows_to_lines<NW / 4>(v, stage, lane);
#pragma unroll
      for (int i = 0; i < NW / 4; i++) { w[4 * i] = v[i].x; w[4 * i + 1] = v[i].y; w[4 * i + 2] = v[i].z; w[4 * i + 3] = v[i].w; }
    }
    if (line >= n_lines) continue;
#else
  for (u64 line = (u64)blockIdx.x * blockDim.x + threadIdx.x; line < n_lines; line += (u64)gridDim.x * blockDim.x) {
    u32 w[NW];
    const uint4 *src = lines + line * (NW / 4);
#pragma unroll
    for (int i = 0; i < NW / 4; i++) {
      const uint4 q = src[i];
      w[4 * i] = q.x; w[4 * i + 1] = q.y; w[4 * i + 2] = q.z; w[4 * i + 3] = q.w;
    }
#endif
    FpcCounts n = {0, 0, 0, 0, 0, 0, 0, 0};      // this line's counts
    const u32 size = fpc_line<NW>(w, n);
    tot.z += n.z; tot.c1 += n.c1; tot.c2 += n.c2; tot.c3 += n.c3; tot.e4 += n.e4; tot.e5 += n.e5; tot.e6 += n.e6;
    words += NW;
    bits_acc += size;
    if (sizes_out) sizes_out[line] = (uint16_t)size;
    if (sel_out) sel_out[line] = 0;
    if (words >= (1u << 30)) fpc_flush(tot, words, bits_acc, s_counts);      // far from overflow of the 32-bit totals
  }
  fpc_flush(tot, words, bits_acc, s_counts);
  __syncthreads();
  if (threadIdx.x < MPC_FPC_RAW_LEN && s_counts[threadIdx.x]) atomicAdd(&gstats[threadIdx.x], s_counts[threadIdx.x]);
}

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
// One line for baselines_kernel: its pattern counts added into the 16-bit fields of even / odd (patterns 0,2,4,6 /
// 1,3,5), its size in bits returned.  The same text as the loop body of bpc_kernel below, which keeps its own copy:
// called from there, the 128-byte instantiation allocates 107 instead of 150 VGPRs, and a solo handle's kernel is
// not to change with the group's (profiles/group_kernel_resource_usage.txt).
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

template <int NW>   // words per line: 8, 16 or 32
__global__ void __launch_bounds__(256)
bpc_kernel(const uint4 *__restrict__ lines, u64 n_lines, uint16_t *__restrict__ sizes_out,
           int8_t *__restrict__ sel_out, u64 *gstats)
{
  __shared__ u64 s_counts[MPC_BPC_RAW_LEN];
  if (threadIdx.x < MPC_BPC_RAW_LEN) s_counts[threadIdx.x] = 0;
  __syncthreads();
  constexpr int ND = NW - 1;                           // deltas = bits of a plane
  u64 even = 0, odd = 0;                               // pattern counts 0,2,4,6 / 1,3,5 in 16-bit fields
  u64 words_acc = 0, bits_acc = 0;
  u32 since_flush = 0;
  auto flush = [&]() {
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const u64 e = (even >> (16 * k)) & 0xffffull, o = (odd >> (16 * k)) & 0xffffull;
      if (e) atomicAdd(&s_counts[2 * k], e);
      if (o && k < 3) atomicAdd(&s_counts[2 * k + 1], o);
    }
    if (words_acc) atomicAdd(&s_counts[7], words_acc);
    if (bits_acc) atomicAdd(&s_counts[8], bits_acc);
    even = odd = words_acc = bits_acc = 0;
  };
#if MPC_BPC_STAGE
  __shared__ uint4 s_stage[4][64 * (NW / 4)];
  const u32 lane = threadIdx.x & 63u;
  uint4 *stage = s_stage[__builtin_amdgcn_readfirstlane(threadIdx.x >> 6)];
  for (u64 line0 = (u64)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); line0 < n_lines; line0 += (u64)gridDim.x * blockDim.x) {
    const u64 line = line0 + lane;
    u32 w[NW];
    {
      uint4 v[NW / 4];
      stage_fetch_rows<NW / 4>(v, lines, line0, lane, n_lines);
      stage_rows_to_lines<NW / 4>(v, stage, lane);
#pragma unroll
      for (int i = 0; i < NW / 4; i++) { w[4 * i] = v[i].x; w[4 * i + 1] = v[i].y; w[4 * i + 2] = v[i].z; w[4 * i + 3] = v[i].w; }
    }
    if (line >= n_lines) continue;
#else
  for (u64 line = (u64)blockIdx.x * blockDim.x + threadIdx.x; line < n_lines; line += (u64)gridDim.x * blockDim.x) {
    u32 w[NW];
    const uint4 *src = lines + line * (NW / 4);
#pragma unroll
    for (int i = 0; i < NW / 4; i++) {
      const uint4 q = src[i];
      w[4 * i] = q.x; w[4 * i + 1] = q.y; w[4 * i + 2] = q.z; w[4 * i + 3] = q.w;
    }
#endif
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
    words_acc += 33u;                                  // every plane is counted once: as a pattern or inside a run
    bits_acc += length;
    if (sizes_out) sizes_out[line] = (uint16_t)length;
    if (sel_out) sel_out[line] = 0;
    if (++since_flush == 1023u) {      // 1023 lines x 34 counts < 2^16 per field
      flush();
      since_flush = 0;
    }
  }
  flush();
  __syncthreads();
  if (threadIdx.x < MPC_BPC_RAW_LEN && s_counts[threadIdx.x]) atomicAdd(&gstats[threadIdx.x], s_counts[threadIdx.x]);
}

// ---------------------------------------------------------------------------
// This file is compiled twice (build.py).  Without MPC_BASELINES_UNIT: every kernel a handle launches on its own, the
// measurement helpers and their launchers (the kernel templates above are instantiated by the launchers).  With it:
// only baselines_kernel, the group's kernel, on the device functions above -- in a unit of its own so that the code
// and the register allocation of bdi_kernel / fpc_kernel / bpc_kernel cannot depend on it
// (profiles/group_kernel_resource_usage.txt).
// ---------------------------------------------------------------------------
#ifndef MPC_BASELINES_UNIT
#define MPC_BASELINES_UNIT 0
#endif
#if !MPC_BASELINES_UNIT
// ---------------------------------------------------------------------------
// BDI / FPC / BPC at line sizes without an unrolled kernel (the reference takes any line a loader
// hands it: BDI.cpp:8, FPC.cpp:10, BPC.cpp:35).  One lane per line, byte and word loops straight
// from the definitions; exact, slow, and only ever used for line sizes other than 32 / 64 / 128.
// ---------------------------------------------------------------------------
__device__ __forceinline__ bool gen_bdi_fits(u64 x, int D)     // reduceSign(x) <= 2^(8D)-1, see bdi_fits64
{
  const u64 lim = D == 4 ? 0xffffffffull : ((1ull << (8 * D)) - 1ull);
  const long long sx = (long long)x, h = 1ll << (8 * D - 1);
  return x <= lim || (sx >= -h && sx <= -2);
}

__device__ u32 gen_bdi_check(const uint8_t *d, int L, int B, int D)   // BDI.cpp:108-201
{
  const u32 n = (u32)(L / B);
  u32 imm = 0;
  bool have_base = false, not_all = false;
  u64 base = 0;
  for (u32 i = 0; i < n; i++) {
    u64 v = 0;
    for (int j = B - 1; j >= 0; j--) v = (v << 8) | d[i * B + j];
    const bool is_imm = gen_bdi_fits(v, D);
    imm += is_imm ? 1u : 0u;
    if (!is_imm) {
      if (!have_base) { base = v; have_base = true; }
      else if (!gen_bdi_fits(base - v, D)) not_all = true;
    }
  }
  if (not_all) return n + 8u * ((imm * (u32)D) + ((n - imm) * (u32)B));
  return n + 8u * ((imm * (u32)D) + ((u32)B + (n - imm - 1u) * (u32)D));     // 32-bit wrap when every value is an immediate
}

__global__ void __launch_bounds__(128)
baseline_generic_kernel(int algo, const uint8_t *__restrict__ lines, u64 n_lines, int L, uint16_t *__restrict__ sizes_out,
                        int8_t *__restrict__ sel_out, u64 *gstats)
{
  __shared__ u64 s_counts[16];
  if (threadIdx.x < 16) s_counts[threadIdx.x] = 0;
  __syncthreads();
  for (u64 line = (u64)blockIdx.x * blockDim.x + threadIdx.x; line < n_lines; line += (u64)gridDim.x * blockDim.x) {
    uint8_t d[MPC_MAX_LINE];
    const uint8_t *src = lines + line * (u64)L;
    for (int i = 0; i < L; i++) d[i] = src[i];
    u32 size = 0;
    int select = 0;
    if (algo == 1) {                       // ---- BDI (BDI.cpp:6-74)
      bool zeros = true, rep = true;
      for (int i = 0; i < L; i++) zeros = zeros && d[i] == 0;
      for (int i = 8; i < (L / 8) * 8; i++) rep = rep && d[i] == d[i % 8];
      u32 best = 8u * (u32)L;
      select = 8;
      if (zeros) { best = 8; select = 0; }
      else if (rep) { best = 64; select = 1; }
      else {
        const int combos[6][2] = {{8, 1}, {8, 2}, {8, 4}, {4, 1}, {4, 2}, {2, 1}};
        for (int k = 0; k < 6; k++) {
          const u32 c = gen_bdi_check(d, L, combos[k][0], combos[k][1]);
          if (best > c) { best = c; select = 2 + k; }
        }
        if (best == 8u * (u32)L) select = 8;
      }
      size = best + 4u;
      atomicAdd(&s_counts[select], 1ull);
      atomicAdd(&s_counts[9], (u64)size);
    } else if (algo == 2) {                // ---- FPC (FPC.cpp:7-88)
      const u32 kBits[8] = {6, 7, 11, 19, 19, 19, 11, 35};
      bool prev_zero = false;
      for (int i = 0; i < L / 4; i++) {
        const u32 v = (u32)d[4 * i] | ((u32)d[4 * i + 1] << 8) | ((u32)d[4 * i + 2] << 16) | ((u32)d[4 * i + 3] << 24);
        const u32 p = fpc_prefix(v);
        size += (p == 0u && prev_zero) ? 0u : kBits[p];
        prev_zero = p == 0u;
        atomicAdd(&s_counts[p], 1ull);
      }
      atomicAdd(&s_counts[8], (u64)size);
    } else {                               // ---- BPC (BPC.cpp:20-185)
      const int n = L / 4, nd = n - 1;
      long long delta[MPC_MAX_LINE / 4];
      for (int r = 1; r < n; r++) {
        const u32 a = (u32)d[4 * r] | ((u32)d[4 * r + 1] << 8) | ((u32)d[4 * r + 2] << 16) | ((u32)d[4 * r + 3] << 24);
        const u32 b = (u32)d[4 * r - 4] | ((u32)d[4 * r - 3] << 8) | ((u32)d[4 * r - 2] << 16) | ((u32)d[4 * r - 1] << 24);
        delta[r - 1] = (long long)a - (long long)b;
      }
      u32 length = 3 + 4, run = 0, prev = 0;
      for (int c = 32; c >= 0; c--) {
        u32 dbp = 0;
        for (int r = nd - 1; r >= 0; r--) dbp = (dbp << 1) | (u32)((delta[r] >> c) & 1);
        const u32 dbx = c == 32 ? dbp : (dbp ^ prev);
        prev = dbp;
        if (dbx == 0u) { run++; continue; }
        if (run) {
          length += run == 1u ? 3u : 7u;
          atomicAdd(&s_counts[1], 1ull);
        }
        run = 0;
        const u32 ones = (u32)__popc(dbx);
        int pat;
        if (dbp == 0u) { length += 5; pat = 2; }
        else if (dbx == 0x7fffffffu) { length += 5; pat = 6; }
        else if (ones == 1u) { length += 10; pat = 3; }
        else if (ones == 2u && (dbx & (dbx >> 1)) != 0u) { length += 10; pat = 4; }
        else { length += 32; pat = 0; }
        atomicAdd(&s_counts[pat], 1ull);
      }
      if (run) {
        length += run == 1u ? 3u : 7u;
        atomicAdd(&s_counts[1], 1ull);
      }
      size = length;
      atomicAdd(&s_counts[7], 33ull);
      atomicAdd(&s_counts[8], (u64)size);
    }
    if (sizes_out) sizes_out[line] = (uint16_t)size;
    if (sel_out) sel_out[line] = (int8_t)(algo == 1 ? select : 0);
  }
  __syncthreads();
  const int len = algo == 1 ? MPC_BDI_RAW_LEN : (algo == 2 ? MPC_FPC_RAW_LEN : MPC_BPC_RAW_LEN);
  if ((int)threadIdx.x < len && s_counts[threadIdx.x]) atomicAdd(&gstats[threadIdx.x], s_counts[threadIdx.x]);
}

// ---------------------------------------------------------------------------
// measurement helpers
// ---------------------------------------------------------------------------
__device__ __forceinline__ u64 splitmix64(u64 x)
{
  u64 z = x + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__device__ __forceinline__ u32 rand_u32(u64 idx, u64 seed) { return (u32)(splitmix64(idx + seed * 0xD1342543DE82EF95ull) >> 32); }

// One thread per 32-bit word (64-bit word for kind 4).  sine = float32 table of one period.
__global__ void synth_kernel(u32 *__restrict__ out, u64 n_words, u32 words_per_line, int kind,
                             u64 first_line, u64 seed, const u32 *__restrict__ sine)
{
  const u64 first_word = first_line * words_per_line;
  for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n_words; i += (u64)gridDim.x * blockDim.x) {
    const u64 gi = first_word + i;          // global word index
    u32 v = 0;
    if (kind == 1) {
      v = rand_u32(gi, seed);
    } else if (kind == 2) {
      v = sine[gi & 1023u];
    } else if (kind == 3) {
      const u64 line = gi / words_per_line, j = gi % words_per_line;
      v = (line & 1ull) ? sine[gi & 1023u] : (u32)((line * 16ull + j) % 1000ull);
    } else if (kind == 4) {
      const u64 qi = gi >> 1;               // global qword index
      const u64 u = (u64)(rand_u32(qi, seed) & 0xfffffu);
      const u64 qv = 0x00007f3a5c000000ull + 8ull * u;
      v = (gi & 1ull) ? (u32)(qv >> 32) : (u32)qv;
    }
    out[i] = v;
  }
}

__global__ void __launch_bounds__(256) read_probe_kernel(const uint4 *__restrict__ p, u64 n16, u32 *sink)
{
  u32 acc = 0;
  for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += (u64)gridDim.x * blockDim.x) {
    const uint4 v = p[i];
    acc ^= v.x ^ v.y ^ v.z ^ v.w;
  }
  if (acc == 0x9e3779b9u) *sink = acc;   // practically never; keeps the loads alive
}

// ---------------------------------------------------------------------------
// host-callable launchers (used by mpc_capi.hip)
// ---------------------------------------------------------------------------
// statistics + per lane (128 lanes) the line and one transformed residue, padded
// statistics + per lane the line and one transformed residue (+ the module tables when all of it stays below 150 KiB)
static inline bool generic_tabs_fit(const MpcVpcParams *P)
{
  return vpc_stats_smem(P->M + 1, P->hist_bins) + generic_lane_smem(P->L) + (size_t)P->gtab_bytes <= 150u * 1024u;
}
extern "C" size_t mpc_vpc_generic_smem(const MpcVpcParams *P)
{
  return vpc_stats_smem(P->M + 1, P->hist_bins) + generic_lane_smem(P->L) + (generic_tabs_fit(P) ? (size_t)P->gtab_bytes : 0u);
}

extern "C" hipError_t mpc_launch_vpc_generic(const void *d_lines, u64 n_lines, const MpcVpcParams *P, uint16_t *d_sizes,
                                             int8_t *d_sel, u64 *d_stats, int grid, hipStream_t stream)
{
  const size_t smem = mpc_vpc_generic_smem(P);
  const bool tabs = generic_tabs_fit(P);
  const void *fn = tabs ? reinterpret_cast<const void *>(&vpc_generic_kernel<true>) : reinterpret_cast<const void *>(&vpc_generic_kernel<false>);
  if (smem > (64u << 10))   // more than the default LDS allowance
    (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
  if (tabs)
    hipLaunchKernelGGL(vpc_generic_kernel<true>, dim3(grid), dim3(generic_threads(P->L)), smem, stream, static_cast<const uint8_t *>(d_lines),
                       n_lines, *P, d_sizes, d_sel, d_stats);
  else
    hipLaunchKernelGGL(vpc_generic_kernel<false>, dim3(grid), dim3(generic_threads(P->L)), smem, stream, static_cast<const uint8_t *>(d_lines),
                       n_lines, *P, d_sizes, d_sel, d_stats);
  return hipGetLastError();
}

extern "C" hipError_t mpc_launch_bdi(const void *d_lines, u64 n_lines, int L, uint16_t *d_sizes, int8_t *d_sel,
                                     u64 *d_stats, int grid, hipStream_t stream)
{
  const uint4 *l = static_cast<const uint4 *>(d_lines);
  switch (L) {
  case 32: hipLaunchKernelGGL(bdi_kernel<8>, dim3(grid), dim3(256), 0, stream, l, n_lines, d_sizes, d_sel, d_stats); break;
  case 64: hipLaunchKernelGGL(bdi_kernel<16>, dim3(grid), dim3(256), 0, stream, l, n_lines, d_sizes, d_sel, d_stats); break;
  case 128: hipLaunchKernelGGL(bdi_kernel<32>, dim3(grid), dim3(256), 0, stream, l, n_lines, d_sizes, d_sel, d_stats); break;
  default:     // any other line size: the loop kernel
    hipLaunchKernelGGL(baseline_generic_kernel, dim3(grid), dim3(128), 0, stream, 1, static_cast<const uint8_t *>(d_lines), n_lines, L,
                       d_sizes, d_sel, d_stats);
    break;
  }
  return hipGetLastError();
}

extern "C" hipError_t mpc_launch_fpc(const void *d_lines, u64 n_lines, int L, uint16_t *d_sizes, int8_t *d_sel,
                                     u64 *d_stats, int grid, hipStream_t stream)
{
  const uint4 *l = static_cast<const uint4 *>(d_lines);
  switch (L) {
  case 32: hipLaunchKernelGGL(fpc_kernel<8>, dim3(grid), dim3(256), 0, stream, l, n_lines, d_sizes, d_sel, d_stats); break;
  case 64: hipLaunchKernelGGL(fpc_kernel<16>, dim3(grid), dim3(256), 0, stream, l, n_lines, d_sizes, d_sel, d_stats); break;
  case 128: hipLaunchKernelGGL(fpc_kernel<32>, dim3(grid), dim3(256), 0, stream, l, n_lines, d_sizes, d_sel, d_stats); break;
  default:     // any other line size: the loop kernel
    hipLaunchKernelGGL(baseline_generic_kernel, dim3(grid), dim3(128), 0, stream, 2, static_cast<const uint8_t *>(d_lines), n_lines, L,
                       d_sizes, d_sel, d_stats);
    break;
  }
  return hipGetLastError();
}

extern "C" hipError_t mpc_launch_bpc(const void *d_lines, u64 n_lines, int L, uint16_t *d_sizes, int8_t *d_sel,
                                     u64 *d_stats, int grid, hipStream_t stream)
{
  const uint4 *l = static_cast<const uint4 *>(d_lines);
  switch (L) {
  case 32: hipLaunchKernelGGL(bpc_kernel<8>, dim3(grid), dim3(256), 0, stream, l, n_lines, d_sizes, d_sel, d_stats); break;
  case 64: hipLaunchKernelGGL(bpc_kernel<16>, dim3(grid), dim3(256), 0, stream, l, n_lines, d_sizes, d_sel, d_stats); break;
  case 128: hipLaunchKernelGGL(bpc_kernel<32>, dim3(grid), dim3(256), 0, stream, l, n_lines, d_sizes, d_sel, d_stats); break;
  default:     // any other line size: the loop kernel
    hipLaunchKernelGGL(baseline_generic_kernel, dim3(grid), dim3(128), 0, stream, 3, static_cast<const uint8_t *>(d_lines), n_lines, L,
                       d_sizes, d_sel, d_stats);
    break;
  }
  return hipGetLastError();
}

extern "C" hipError_t mpc_launch_synth(void *d_out, u64 n_lines, unsigned L, int kind, u64 first_line, u64 seed,
                                       const u32 *d_sine, hipStream_t stream)
{
  const u64 n_words = n_lines * (L / 4);
  hipLaunchKernelGGL(synth_kernel, dim3(4096), dim3(256), 0, stream, static_cast<u32 *>(d_out), n_words, L / 4, kind,
                     first_line, seed, d_sine);
  return hipGetLastError();
}

extern "C" hipError_t mpc_launch_read_probe(const void *d_buf, u64 bytes, u32 *d_sink, int grid, hipStream_t stream)
{
  hipLaunchKernelGGL(read_probe_kernel, dim3(grid), dim3(256), 0, stream, static_cast<const uint4 *>(d_buf), bytes / 16,
                     d_sink);
  return hipGetLastError();
}
#else      // MPC_BASELINES_UNIT
// ---------------------------------------------------------------------------
// BDI, FPC and BPC in one pass (a group of handles, mpc_capi.hip): the three map a line the same way -- one lane per
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
  // BDI: run-length accumulation per lane, (select, size) key and count (bdi_kernel)
  u32 run_key = 0xffffffffu, run_cnt = 0;
  auto bdi_run_flush = [&]() {
    if (run_cnt) {
      atomicAdd(&s_bdi[run_key >> 16], (u64)run_cnt);
      atomicAdd(&s_bdi[9], (u64)run_cnt * (u64)(run_key & 0xffffu));
    }
  };
  auto bdi_account = [&](u64 line, u32 best, int select) {
    const u32 size = best + 4u;
    if (A.bdi.sizes) A.bdi.sizes[line] = (uint16_t)size;
    if (A.bdi.sel) A.bdi.sel[line] = (int8_t)select;
    const u32 key = ((u32)select << 16) | size;
    if (key != run_key) {
      bdi_run_flush();
      run_key = key;
      run_cnt = 0;
    }
    run_cnt++;
  };
  const u32 lane = threadIdx.x & 63u;
  auto fetch = [&](u32 (&w)[NW], u64 line) {      // plain loads: queued lines, the launch's last partial group
    const uint4 *src = lines + line * (NW / 4);
#pragma unroll
    for (int i = 0; i < NW / 4; i++) {
      const uint4 q = src[i];
      w[4 * i] = q.x; w[4 * i + 1] = q.y; w[4 * i + 2] = q.z; w[4 * i + 3] = q.w;
    }
  };
  // BDI's queued lines, 64 at a time, every scan they need (the other members have seen them already)
  u32 *queue = s_queue[DEFER ? uni(threadIdx.x >> 6) : 0u];
  u32 qn = 0;                                   // queued lines of this wave (wave-uniform)
  const bool can_defer = n_lines <= 0xffffffffull;      // queue entries are 32-bit line indices
  auto drain = [&]() __attribute__((always_inline)) {
    while (qn > 0u) {
      const u32 take = qn < 64u ? qn : 64u;
      qn -= take;
      const bool active = lane < take;
      const u64 line = active ? (u64)queue[qn + lane] : 0ull;
      u32 w[NW];
      fetch(w, line);
      u32 best;
      int select;
      bool deferred;
      bdi_line<NW, false>(w, active, false, best, select, deferred);
      if (active) bdi_account(line, best, select);
    }
  };
  // FPC: per-lane totals (fpc_kernel)
  FpcCounts f_tot = {0, 0, 0, 0, 0, 0, 0, 0};
  u32 f_words = 0;
  u64 f_bits = 0;
  // BPC: pattern counts in 16-bit fields (bpc_kernel)
  u64 even = 0, odd = 0, p_words = 0, p_bits = 0;
  u32 since_flush = 0;
  auto bpc_flush = [&]() {
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const u64 e = (even >> (16 * k)) & 0xffffull, o = (odd >> (16 * k)) & 0xffffull;
      if (e) atomicAdd(&s_bpc[2 * k], e);
      if (o && k < 3) atomicAdd(&s_bpc[2 * k + 1], o);
    }
    if (p_words) atomicAdd(&s_bpc[7], p_words);
    if (p_bits) atomicAdd(&s_bpc[8], p_bits);
    even = odd = p_words = p_bits = 0;
  };
  // every member on one line held in w (every lane stays in: bdi_line votes across the wave)
  auto evaluate = [&](const u32 (&w)[NW], u64 line, bool active) __attribute__((always_inline)) {
    if (FPC && active) {
      FpcCounts n = {0, 0, 0, 0, 0, 0, 0, 0};
      const u32 size = fpc_line<NW>(w, n);
      f_tot.z += n.z; f_tot.c1 += n.c1; f_tot.c2 += n.c2; f_tot.c3 += n.c3; f_tot.e4 += n.e4; f_tot.e5 += n.e5; f_tot.e6 += n.e6;
      f_words += NW;
      f_bits += size;
      if (A.fpc.sizes) A.fpc.sizes[line] = (uint16_t)size;
      if (A.fpc.sel) A.fpc.sel[line] = 0;
      if (f_words >= (1u << 30)) fpc_flush(f_tot, f_words, f_bits, s_fpc);
    }
    if (BPC && active) {
      const u32 length = bpc_line<NW>(w, even, odd);
      p_words += 33u;
      p_bits += length;
      if (A.bpc.sizes) A.bpc.sizes[line] = (uint16_t)length;
      if (A.bpc.sel) A.bpc.sel[line] = 0;
      if (++since_flush == 1023u) {      // 1023 lines x 34 counts < 2^16 per field
        bpc_flush();
        since_flush = 0;
      }
    }
    if (BDI) {
      u32 best;
      int select;
      bool deferred;
      bdi_line<NW, DEFER>(w, active, can_defer, best, select, deferred);
      if (DEFER) {
        const u64 dmask = __ballot(active && deferred);
        if (dmask) {
          const u32 rank = __builtin_amdgcn_mbcnt_hi((u32)(dmask >> 32), __builtin_amdgcn_mbcnt_lo((u32)dmask, 0u));
          if (active && deferred) queue[qn + rank] = (u32)line;
          qn += (u32)__popcll(dmask);
        }
      }
      if (active && !deferred) bdi_account(line, best, select);
      if (DEFER && qn + 64u > kBdiQueue) drain();        // wave-uniform: room for the next group's deferrals
    }
  };
  if constexpr (RING) {
  // whole groups of 64 lines through a one-stage ring per wave (bdi_kernel), grid-stride over the waves
  constexpr int NQ = NW / 4;
  constexpr u32 SB = 64u * 16u * NQ;            // bytes of a stage
  const u32 wave = uni(threadIdx.x >> 6);
  const u32 ring_lds = (u32)(uintptr_t)(__attribute__((address_space(3))) void *)s_stage + wave * SB;
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
#pragma unroll
    for (int i = 0; i < NQ; i++) { w[4 * i] = v[i].x; w[4 * i + 1] = v[i].y; w[4 * i + 2] = v[i].z; w[4 * i + 3] = v[i].w; }
    evaluate(w, g * 64u + lane, true);
    g += gstride;
  }
  // the launch's last, partial group: plain loads, by one wave
  if ((n_lines & 63ull) != 0ull && blockIdx.x == 0 && wave == 0u) {
    const u64 line = full_groups * 64u + lane;
    const bool active = line < n_lines;
    u32 w[NW];
    fetch(w, active ? line : n_lines - 1);
    evaluate(w, line, active);
  }
  } else {
  uint4 *stage = s_stage[__builtin_amdgcn_readfirstlane(threadIdx.x >> 6)];
  for (u64 line0 = (u64)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); line0 < n_lines; line0 += (u64)gridDim.x * blockDim.x) {
    u32 w[NW];
    {
      uint4 v[NW / 4];
      stage_fetch_rows<NW / 4>(v, lines, line0, lane, n_lines);
      stage_rows_to_lines<NW / 4>(v, stage, lane);
#pragma unroll
      for (int i = 0; i < NW / 4; i++) { w[4 * i] = v[i].x; w[4 * i + 1] = v[i].y; w[4 * i + 2] = v[i].z; w[4 * i + 3] = v[i].w; }
    }
    evaluate(w, line0 + lane, line0 + lane < n_lines);
  }
  }
  if (DEFER) drain();
  if (BDI) bdi_run_flush();
  if (FPC) fpc_flush(f_tot, f_words, f_bits, s_fpc);
  if (BPC) bpc_flush();
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
#endif     // MPC_BASELINES_UNIT
