// mpc_kernels.hip -- gfx950 (MI355X, CDNA4) kernels that a single handle launches, other than the fast VPC kernel
// (mpc_vpc_lane.hip), and their launchers:
//
//   vpc_generic_kernel       VPC, any configuration the reference can run
//   bdi_kernel               BDI baseline (reference src/compressor/BDI.cpp), 32- / 64- / 128-byte lines
//   fpc_kernel               FPC baseline (reference src/compressor/FPC.cpp)
//   bpc_kernel               BPC baseline (reference src/compressor/BPC.cpp)
//   baseline_generic_kernel  the three baselines at any other line size
//   synth_kernel / read_probe_kernel   measurement helpers
//
// What the three baseline kernels share with each other and with the kernel of a group of handles (mpc_baselines.hip)
// is in mpc_baselines.h, once.
#include "mpc_baselines.h"
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
// BDI, FPC and BPC of a single handle at 32-, 64- and 128-byte lines: one lane per line, the line in registers.  The
// evaluation of a line, the two feeds and the per-lane accumulators are mpc_baselines.h's, shared with the group's
// kernel (mpc_baselines.hip); a kernel here is its LDS, its choice of feed and what it does with a line.
// ---------------------------------------------------------------------------

// BDI.  Lines stream through the ring (ring_feed).  With so little arithmetic behind a line (random data: every scan
// is screened out) the kernel sits on the floor of its access pattern, and that floor is higher for the ring than for
// lane-per-line register loads: same box, ms per 16 GiB, random 3.07 -> 2.84, sine 3.29 -> 3.12, mixed 3.27 -> 3.06,
// 128-byte pointers 2.82 -> 2.69.  (Two stages per wave leave room for 4 instead of 7 workgroups per CU and measured
// slower on every trace; FPC and BPC, which already transposed coalesced non-temporal loads through LDS, gain nothing
// from the ring and keep their form.)
template <int NW>   // words per line
__global__ void __launch_bounds__(256)
bdi_kernel(const uint4 *__restrict__ lines, u64 n_lines, uint16_t *__restrict__ sizes_out,
           int8_t *__restrict__ sel_out, u64 *gstats)
{
  __shared__ u64 s_counts[MPC_BDI_RAW_LEN];
  __shared__ u32 s_queue[4][kBdiQueue];
  __shared__ __attribute__((aligned(1024))) uint4 s_ring[4 * 64 * (NW / 4)];
  if (threadIdx.x < MPC_BDI_RAW_LEN) s_counts[threadIdx.x] = 0;
  __syncthreads();
  const u32 lane = threadIdx.x & 63u;
  const u32 wave = uni(threadIdx.x >> 6);
  BdiLane bdi = {sizes_out, sel_out, s_counts, s_queue[wave], gstats + MPC_BDI_RAW_LEN};      // (route counters behind the statistics)
  const bool can_defer = n_lines <= kBdiDeferMaxLines;      // queue entries are 32-bit line indices
  ring_feed<NW>(lines, n_lines, s_ring, lane, wave, bdi.qn, [&](const u32 (&w)[NW], u64 line, bool active) __attribute__((always_inline)) {
    bdi.group<NW, (NW <= 16)>(lines, lane, w, line, active, can_defer);     // (128-byte lines: deferral measured slower)
  });
  bdi.drain<NW>(lines, lane);
  bdi.flush();
  __syncthreads();
  if (threadIdx.x < MPC_BDI_RAW_LEN && s_counts[threadIdx.x]) atomicAdd(&gstats[threadIdx.x], s_counts[threadIdx.x]);
}

// FPC: staged loads (staged_feed)
template <int NW>   // words per line
__global__ void __launch_bounds__(256)
fpc_kernel(const uint4 *__restrict__ lines, u64 n_lines, uint16_t *__restrict__ sizes_out,
           int8_t *__restrict__ sel_out, u64 *gstats)
{
  __shared__ u64 s_counts[MPC_FPC_RAW_LEN];
  __shared__ uint4 s_stage[4][64 * (NW / 4)];
  if (threadIdx.x < MPC_FPC_RAW_LEN) s_counts[threadIdx.x] = 0;
  __syncthreads();
  FpcAcc acc;
  staged_feed<NW>(lines, n_lines, s_stage[uni(threadIdx.x >> 6)], threadIdx.x & 63u, [&](const u32 (&w)[NW], u64 line, bool active) __attribute__((always_inline)) {
    if (!active) return;
    FpcCounts n = {0, 0, 0, 0, 0, 0, 0, 0};      // this line's counts
    const u32 size = fpc_line<NW>(w, n);
    put_line(sizes_out, sel_out, line, size, 0);
    acc.add(n, size, NW, s_counts);
  });
  acc.flush(s_counts);
  __syncthreads();
  if (threadIdx.x < MPC_FPC_RAW_LEN && s_counts[threadIdx.x]) atomicAdd(&gstats[threadIdx.x], s_counts[threadIdx.x]);
}

// BPC: staged loads (staged_feed)
template <int NW>   // words per line: 8, 16 or 32
__global__ void __launch_bounds__(256)
bpc_kernel(const uint4 *__restrict__ lines, u64 n_lines, uint16_t *__restrict__ sizes_out,
           int8_t *__restrict__ sel_out, u64 *gstats)
{
  __shared__ u64 s_counts[MPC_BPC_RAW_LEN];
  __shared__ uint4 s_stage[4][64 * (NW / 4)];
  if (threadIdx.x < MPC_BPC_RAW_LEN) s_counts[threadIdx.x] = 0;
  __syncthreads();
  BpcAcc acc;
  staged_feed<NW>(lines, n_lines, s_stage[uni(threadIdx.x >> 6)], threadIdx.x & 63u, [&](const u32 (&w)[NW], u64 line, bool active) __attribute__((always_inline)) {
    if (!active) return;
    const u32 length = bpc_line<NW>(w, acc.even, acc.odd);
    put_line(sizes_out, sel_out, line, length, 0);
    acc.add(length, s_counts);
  });
  acc.flush(s_counts);
  __syncthreads();
  if (threadIdx.x < MPC_BPC_RAW_LEN && s_counts[threadIdx.x]) atomicAdd(&gstats[threadIdx.x], s_counts[threadIdx.x]);
}

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

// BDI / FPC / BPC: the unrolled kernel of a 32-, 64- or 128-byte line, the loop kernel (its algorithm number: algo) for any other
typedef void (*BaselineKernel)(const uint4 *, u64, uint16_t *, int8_t *, u64 *);
static hipError_t launch_baseline(BaselineKernel k32, BaselineKernel k64, BaselineKernel k128, int algo, const void *d_lines, u64 n_lines, int L,
                                  uint16_t *d_sizes, int8_t *d_sel, u64 *d_stats, int grid, hipStream_t stream)
{
  const BaselineKernel k = L == 32 ? k32 : L == 64 ? k64 : L == 128 ? k128 : nullptr;
  if (k)
    hipLaunchKernelGGL(k, dim3(grid), dim3(256), 0, stream, static_cast<const uint4 *>(d_lines), n_lines, d_sizes, d_sel, d_stats);
  else
    hipLaunchKernelGGL(baseline_generic_kernel, dim3(grid), dim3(128), 0, stream, algo, static_cast<const uint8_t *>(d_lines), n_lines, L,
                       d_sizes, d_sel, d_stats);
  return hipGetLastError();
}

extern "C" hipError_t mpc_launch_bdi(const void *d_lines, u64 n_lines, int L, uint16_t *d_sizes, int8_t *d_sel,
                                     u64 *d_stats, int grid, hipStream_t stream)
{
  return launch_baseline(bdi_kernel<8>, bdi_kernel<16>, bdi_kernel<32>, 1, d_lines, n_lines, L, d_sizes, d_sel, d_stats, grid, stream);
}

extern "C" hipError_t mpc_launch_fpc(const void *d_lines, u64 n_lines, int L, uint16_t *d_sizes, int8_t *d_sel,
                                     u64 *d_stats, int grid, hipStream_t stream)
{
  return launch_baseline(fpc_kernel<8>, fpc_kernel<16>, fpc_kernel<32>, 2, d_lines, n_lines, L, d_sizes, d_sel, d_stats, grid, stream);
}

extern "C" hipError_t mpc_launch_bpc(const void *d_lines, u64 n_lines, int L, uint16_t *d_sizes, int8_t *d_sel,
                                     u64 *d_stats, int grid, hipStream_t stream)
{
  return launch_baseline(bpc_kernel<8>, bpc_kernel<16>, bpc_kernel<32>, 3, d_lines, n_lines, L, d_sizes, d_sel, d_stats, grid, stream);
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
