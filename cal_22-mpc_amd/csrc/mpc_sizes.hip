// mpc_sizes.hip -- gfx950 kernel of the accounting pass over per-line sizes (mpc_sizes.h): per-member size histograms and
// the per-line best-of of a set.  It runs on the stream of the evaluators' launches, directly behind them, and reads
// only what they wrote: 2 bytes per line and member.
//
// Persistent and grid-stride.  A lane takes a chunk of 8 consecutive lines: one 16-byte load per member (the last,
// partial chunk and arrays that are not 16-byte aligned take 2-byte loads, every one bounds-checked).  A workgroup
// keeps one histogram of MPC_SIZE_BINS uint32 bins (16 KiB) in LDS per member that has one, and one more for the
// best-of; at the end it adds its non-empty bins to the uint64 device accumulators with vector atomics.  The launcher
// cuts a call into launches of at most 2^31 lines, so no LDS bin can wrap.
//
// All-zero and random traces put every line into ONE bin, and 64 lanes adding to one LDS address serialise.  Before
// the LDS add a wave therefore aggregates: the first lane's size is broadcast, the lanes that hold the same size are
// counted with a ballot and one lane adds their number; a second round does the same for the lanes left over; only
// what is left after two rounds adds lane by lane.  A wave that agrees sends one add per chunk position, a wave with
// two sizes two.
#include "mpc_kernel_common.h"
#include "mpc_sizes.h"
#include "mpc_launch.h"

constexpr int kSizesThreads = 256;
constexpr u32 kLastBin = MPC_SIZE_BINS - 1;

struct SizesSlots {
  int hist[MPC_SIZES_MAX];   // LDS histogram of member i (-1: none)
  int best;                  // ... of the best-of (-1: none)
};

// sizes 8c .. 8c+7 of one member, two per dword; `vec`: the array is 16-byte aligned
__device__ __forceinline__ uint4 sizes_load8(const uint16_t *__restrict__ p, u64 c, u64 n, bool vec)
{
  const u64 first = c * 8ull;
  if (vec && first + 8ull <= n) return *reinterpret_cast<const uint4 *>(p + first);
  u32 w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int j = 0; j < 8; j++)
    if (first + (u64)j < n) w[j >> 1] |= (u32)p[first + (u64)j] << (16 * (j & 1));
  return make_uint4(w[0], w[1], w[2], w[3]);
}

template <int J>
__device__ __forceinline__ u32 size_at(const uint4 &q)
{
  const u32 w = (J >> 1) == 0 ? q.x : (J >> 1) == 1 ? q.y : (J >> 1) == 2 ? q.z : q.w;
  return (J & 1) ? (w >> 16) : (w & 0xffffu);
}

// one add per line into an LDS histogram; called by every lane of the wave (valid: this lane has a line)
__device__ __forceinline__ void wave_hist_add(u32 *hist, u32 bin, bool valid, int lane)
{
  u64 rem = __ballot(valid);
#pragma unroll
  for (int round = 0; round < 2; round++) {
    if (rem == 0ull) return;                                 // (wave-uniform)
    const int leader = __ffsll((long long)rem) - 1;
    const u32 lead_bin = (u32)__shfl((int)bin, leader);
    const u64 same = __ballot(valid && bin == lead_bin) & rem;
    if (lane == leader) atomicAdd(&hist[lead_bin], (u32)__popcll(same));
    rem &= ~same;
  }
  if ((rem >> lane) & 1ull) atomicAdd(&hist[bin], 1u);
}

template <int M, int J>
__device__ __forceinline__ void account_position(const uint4 (&q)[M], int cnt, const SizesSlots &S, u32 *s_hist, bool best,
                                                 u32 (&wins)[M], u64 &bits, int lane)
{
  const bool valid = J < cnt;
  u32 b = 0u, w = 0u;
#pragma unroll
  for (int i = 0; i < M; i++) {
    const u32 v = size_at<J>(q[i]);
    if (S.hist[i] >= 0) wave_hist_add(s_hist + S.hist[i] * MPC_SIZE_BINS, min(v, kLastBin), valid, lane);
    if (i == 0 || v < b) {        // strict: the first minimal member wins a tie
      b = v;
      w = (u32)i;
    }
  }
  if (best) {
#pragma unroll
    for (int i = 0; i < M; i++) wins[i] += (valid && w == (u32)i) ? 1u : 0u;
    bits += valid ? (u64)b : 0ull;
    wave_hist_add(s_hist + S.best * MPC_SIZE_BINS, min(b, kLastBin), valid, lane);
  }
}

template <int M>
__global__ void __launch_bounds__(kSizesThreads)
sizes_account_kernel(MpcSizesArgs A, SizesSlots S, int n_hist, u64 n, int vec)
{
  extern __shared__ u32 s_hist[];            // [n_hist][MPC_SIZE_BINS]
  __shared__ u64 s_sum[MPC_SIZES_MAX + 1];   // wins, bits
  for (int i = threadIdx.x; i < n_hist * MPC_SIZE_BINS; i += kSizesThreads) s_hist[i] = 0u;
  if (threadIdx.x <= MPC_SIZES_MAX) s_sum[threadIdx.x] = 0ull;
  __syncthreads();

  const int lane = threadIdx.x & 63;
  const bool best = S.best >= 0;
  const u64 n_chunks = (n + 7ull) / 8ull;
  u32 wins[M];
#pragma unroll
  for (int i = 0; i < M; i++) wins[i] = 0u;
  u64 bits = 0ull;
  // every lane of a wave stays in the loop while the wave's first chunk exists (the ballots need the whole wave)
  const u64 wave_first = (u64)blockIdx.x * kSizesThreads + (u64)(threadIdx.x & ~63);
  for (u64 base = wave_first; base < n_chunks; base += (u64)gridDim.x * kSizesThreads) {
    const u64 c = base + (u64)lane;
    const u64 first = c * 8ull;
    const int cnt = first >= n ? 0 : (n - first < 8ull ? (int)(n - first) : 8);
    uint4 q[M];
#pragma unroll
    for (int i = 0; i < M; i++) q[i] = cnt ? sizes_load8(A.sizes[i], c, n, vec != 0) : make_uint4(0u, 0u, 0u, 0u);
    account_position<M, 0>(q, cnt, S, s_hist, best, wins, bits, lane);
    account_position<M, 1>(q, cnt, S, s_hist, best, wins, bits, lane);
    account_position<M, 2>(q, cnt, S, s_hist, best, wins, bits, lane);
    account_position<M, 3>(q, cnt, S, s_hist, best, wins, bits, lane);
    account_position<M, 4>(q, cnt, S, s_hist, best, wins, bits, lane);
    account_position<M, 5>(q, cnt, S, s_hist, best, wins, bits, lane);
    account_position<M, 6>(q, cnt, S, s_hist, best, wins, bits, lane);
    account_position<M, 7>(q, cnt, S, s_hist, best, wins, bits, lane);
  }

  if (best) {
#pragma unroll
    for (int i = 0; i < M; i++) {
      u32 v = wins[i];
      for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
      if (lane == 0 && v) atomicAdd(&s_sum[i], (u64)v);
    }
    for (int o = 32; o > 0; o >>= 1) bits += __shfl_xor(bits, o);
    if (lane == 0 && bits) atomicAdd(&s_sum[MPC_SIZES_MAX], bits);
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < M; i++) {
    if (S.hist[i] < 0) continue;
    const u32 *h = s_hist + S.hist[i] * MPC_SIZE_BINS;
    for (int b = threadIdx.x; b < MPC_SIZE_BINS; b += kSizesThreads)
      if (h[b]) atomicAdd(&A.hist[i][b], (u64)h[b]);
  }
  if (best) {
    const u32 *h = s_hist + S.best * MPC_SIZE_BINS;
    for (int b = threadIdx.x; b < MPC_SIZE_BINS; b += kSizesThreads)
      if (h[b]) atomicAdd(&A.best[b], (u64)h[b]);
    if (threadIdx.x <= MPC_SIZES_MAX && s_sum[threadIdx.x]) atomicAdd(&A.best[MPC_SIZES_WINS + threadIdx.x], s_sum[threadIdx.x]);
  }
}

namespace {

int sizes_slots(const MpcSizesArgs *A, SizesSlots *S)
{
  int n_hist = 0;
  for (int i = 0; i < MPC_SIZES_MAX; i++) S->hist[i] = (i < A->m && A->hist[i]) ? n_hist++ : -1;
  S->best = A->best ? n_hist++ : -1;
  return n_hist;
}

template <int M>
hipError_t sizes_launch(const MpcSizesArgs &A, const SizesSlots &S, int n_hist, u64 n, int vec, int grid, hipStream_t stream)
{
  const size_t smem = (size_t)n_hist * MPC_SIZE_BINS * sizeof(u32);
  if (smem > (64u << 10))   // more than the default LDS allowance
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&sizes_account_kernel<M>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
  hipLaunchKernelGGL(sizes_account_kernel<M>, dim3(grid), dim3(kSizesThreads), smem, stream, A, S, n_hist, n, vec);
  return hipGetLastError();
}

}  // namespace

// workgroups of the pass that fit a CU beside each other (their LDS histograms), at most 8
extern "C" int mpc_sizes_wg_per_cu(const MpcSizesArgs *A)
{
  SizesSlots S;
  const int n_hist = sizes_slots(A, &S);
  if (n_hist == 0) return 0;
  const int fit = (160 * 1024) / (n_hist * MPC_SIZE_BINS * (int)sizeof(u32) + 128);
  return fit > 8 ? 8 : fit;
}

extern "C" hipError_t mpc_launch_sizes(const MpcSizesArgs *A, u64 n_lines, int grid, hipStream_t stream)
{
  if (A->m < 1 || A->m > MPC_SIZES_MAX || (A->best && A->m < 2)) return hipErrorInvalidValue;
  SizesSlots S;
  const int n_hist = sizes_slots(A, &S);
  if (n_hist == 0 || n_lines == 0) return hipSuccess;
  int vec = 1;
  for (int i = 0; i < A->m; i++) vec &= (reinterpret_cast<uintptr_t>(A->sizes[i]) & 15u) == 0 ? 1 : 0;
  const u64 kMaxLines = mpc_launch_cap(1ull << 31);     // per launch: a uint32 LDS bin cannot wrap (and a piece's first line keeps the alignment)
  for (u64 at = 0; at < n_lines; at += kMaxLines) {
    const u64 take = n_lines - at < kMaxLines ? n_lines - at : kMaxLines;
    MpcSizesArgs P = *A;
    for (int i = 0; i < A->m; i++) P.sizes[i] = A->sizes[i] + at;
    mpc_count_launch();
    const u64 chunks = (take + 7) / 8;
    const u64 need = (chunks + kSizesThreads - 1) / kSizesThreads;
    const int g = (int)(need < (u64)(grid < 1 ? 1 : grid) ? need : (u64)(grid < 1 ? 1 : grid));
    hipError_t e;
    switch (A->m) {
    case 1: e = sizes_launch<1>(P, S, n_hist, take, vec, g, stream); break;
    case 2: e = sizes_launch<2>(P, S, n_hist, take, vec, g, stream); break;
    case 3: e = sizes_launch<3>(P, S, n_hist, take, vec, g, stream); break;
    case 4: e = sizes_launch<4>(P, S, n_hist, take, vec, g, stream); break;
    case 5: e = sizes_launch<5>(P, S, n_hist, take, vec, g, stream); break;
    case 6: e = sizes_launch<6>(P, S, n_hist, take, vec, g, stream); break;
    case 7: e = sizes_launch<7>(P, S, n_hist, take, vec, g, stream); break;
    default: e = sizes_launch<8>(P, S, n_hist, take, vec, g, stream); break;
    }
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

#if MPC_TESTING
// test library only (not part of include/mpc_hip.h): the kernel launches that mpc_launch_vpc_lane,
// mpc_launch_vpc_lane_jit, mpc_launch_sizes and mpc_launch_classes have made in this process, one per piece of a batch
// (mpc_kernel_common.h: mpc_count_launch)
extern "C" unsigned long long mpc_test_launches(void) { return __atomic_load_n(&mpc_test_launch_counter(), __ATOMIC_RELAXED); }
#endif
