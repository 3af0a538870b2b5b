// mpc_snapshot.hip -- snapshots (mpc_snapshot.h, include/mpc_hip_snapshot.h): the gfx950 kernels that keep, per distinct
// unit address, the bytes of the latest unit added there and that write the address-aligned lines of that memory out, and
// the snapshot object of the C ABI behind them.  mpc_snapshot_evaluate, which needs a handle's insides, is mpc_capi.hip's.
//
// Add, two kernels on one stream.  Stamp: persistent, grid-stride, a lane per unit, image_update_kernel's shape -- 8 bytes
// of address in, one 64-bit compare-and-swap where a key is new, one 64-bit atomic max of p + 1 per unit that goes to the
// table, 4 bytes of slot index out.  A lane whose right neighbour in the wave holds the same key stays off the table (the
// neighbour's unit is later).  What an overflowing trace may cost is bounded as there: a probe gives up after capacity + 1
// slots, waves add their claims in lots and the add that passes the capacity raises the flag, every wave reads the flag in
// every 16th round and leaves when it is set.  Copy: U / 16 lanes per unit, each moves 16 bytes of the unit whose p + 1 the
// slot's stamp holds; exactly one unit per key and launch does, so no two lanes write the same bytes.
//
// Plan: the live (key, slot) pairs are appended wave by wave to an array (one atomic add per wave and round), sorted by
// key with rocPRIM's radix sort and kept; mark, scan (rocPRIM) and heads number the emitted lines of a line size.  rocPRIM
// is used for the sort and the scan alone; the stamp, copy, compact, mark, heads and gather kernels are this file's.
//
// All table indices are masked with the slot mask; units, sorted keys and emitted lines are read only below their counts.
#include <cstring>      // (before rocPRIM: one of its iterator headers uses memcpy without including this)
#include <rocprim/rocprim.hpp>

#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <string>
#include <vector>

#include "mpc_kernel_common.h"
#include "mpc_snapshot.h"
#include "mpc_trace_files.h"
#include "../../include/mpc_hip.h"

constexpr int kSnapThreads = 256;

// image_slot of mpc_image.hip: the slot of `key`, found or claimed (then *claimed); ~0 when max_tries slots in a row were
// taken by other keys, or when a long probe finds *stop set (looked at every 64 slots)
__device__ __forceinline__ u64 snap_slot(u64 *keys, u64 mask, u64 hash_mask, u64 key, u64 max_tries, const u64 *stop, bool *claimed)
{
  u64 slot = mpc_image_mix(key) & hash_mask & mask;
  for (u64 tries = 0; tries < max_tries; tries++, slot = (slot + 1ull) & mask) {
    if ((tries & 63ull) == 63ull && __hip_atomic_load(stop, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0ull) break;
    u64 cur = __hip_atomic_load(&keys[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == kMpcImageEmpty) {
      cur = atomicCAS(&keys[slot], kMpcImageEmpty, key);
      if (cur == kMpcImageEmpty) {
        *claimed = true;
        return slot;
      }
    }
    if (cur == key) return slot;
  }
  return kMpcImageEmpty;
}

__global__ void __launch_bounds__(kSnapThreads)
snapshot_stamp_kernel(MpcSnapAddArgs A, u64 n)
{
  __shared__ u64 s_sum[2];
  if (threadIdx.x < 2) s_sum[threadIdx.x] = 0ull;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  u64 mis = 0ull;
  u64 claims = 0ull;                             // of the wave, not yet added to the device's count (the same in every lane)
  u32 round = 0u;
  const u64 max_tries = A.capacity < A.slot_mask ? A.capacity + 1ull : A.slot_mask + 1ull;
  // (uniform over the wave: the shuffle, the ballot, the way out)
  for (u64 base = (u64)blockIdx.x * kSnapThreads; base < n; base += (u64)gridDim.x * kSnapThreads) {
    u64 over = 0ull;
    if ((round++ & 15u) == 0u) over = __hip_atomic_load(&A.ctl[MPC_SNAP_CTL_OVERFLOW], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const u64 i = base + threadIdx.x;
    const bool have = i < n;
    u64 key = kMpcImageEmpty;
    if (have) {
      const u64 a = A.addrs[i];
      key = a >> A.unit_shift;
      mis += (a & ((u64)A.unit_bytes - 1ull)) ? 1ull : 0ull;
    }
    const u64 next = (u64)__shfl_down((long long)key, 1);
    bool claimed = false;
    u32 mine = kMpcSnapNoSlot;
    if (have && (lane == 63 || next != key)) {
      const u64 slot = snap_slot(A.keys, A.slot_mask, A.hash_mask, key, max_tries, &A.ctl[MPC_SNAP_CTL_OVERFLOW], &claimed);
      if (slot == kMpcImageEmpty) atomicOr(&A.ctl[MPC_SNAP_CTL_OVERFLOW], 1ull);
      else {
        atomicMax(&A.stamp[slot], A.pos + i + 1ull);
        mine = (u32)slot;                        // (slots <= 2^29)
      }
    }
    if (have) A.unit_slot[i] = mine;
    claims += (u64)__popcll(__ballot(claimed));
    if (claims >= A.flush_claims) {
      if (lane == 0 && atomicAdd(&A.ctl[MPC_SNAP_CTL_KEYS], claims) + claims > A.capacity) atomicOr(&A.ctl[MPC_SNAP_CTL_OVERFLOW], 1ull);
      claims = 0ull;
    }
    if (__any(over != 0ull)) break;              // the snapshot is finished: what the table holds no longer counts
  }
  for (int o = 32; o > 0; o >>= 1) mis += __shfl_xor(mis, o);
  if (lane == 0) {
    if (mis) atomicAdd(&s_sum[0], mis);
    if (claims) atomicAdd(&s_sum[1], claims);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    if (s_sum[0]) atomicAdd(&A.ctl[MPC_SNAP_CTL_MISALIGNED], s_sum[0]);
    if (s_sum[1] && atomicAdd(&A.ctl[MPC_SNAP_CTL_KEYS], s_sum[1]) + s_sum[1] > A.capacity) atomicOr(&A.ctl[MPC_SNAP_CTL_OVERFLOW], 1ull);
  }
}

// The unit that won its slot goes into the payload, 16 bytes per lane.  unit_slot[i] of a unit that a wave left unwritten
// when it met the overflow flag is whatever an earlier launch wrote: the index is masked, and its stamp cannot be p + 1,
// which only unit i's own atomic max writes -- after it wrote unit_slot[i].
__global__ void __launch_bounds__(kSnapThreads)
snapshot_copy_kernel(MpcSnapAddArgs A, u64 n)
{
  const int part_shift = A.unit_shift - 4;                     // 16-byte parts per unit: 2, 4 or 8
  const u64 parts = 1ull << part_shift, work = n << part_shift;
  const uint4 *src = reinterpret_cast<const uint4 *>(A.units);
  uint4 *dst = reinterpret_cast<uint4 *>(A.payload);
  for (u64 g = (u64)blockIdx.x * kSnapThreads + threadIdx.x; g < work; g += (u64)gridDim.x * kSnapThreads) {
    const u64 i = g >> part_shift, part = g & (parts - 1ull);
    const u32 us = A.unit_slot[i];
    if (us == kMpcSnapNoSlot) continue;
    const u64 slot = (u64)us & A.slot_mask;
    if (A.stamp[slot] != A.pos + i + 1ull) continue;
    dst[(slot << part_shift) + part] = src[g];
  }
}

// the live slots appended to (okeys, oslot) in any order; *counter ends as their number
__global__ void __launch_bounds__(kSnapThreads)
snapshot_compact_kernel(const u64 *keys, u64 slots, u64 *okeys, u32 *oslot, u64 cap, u64 *counter)
{
  const int lane = threadIdx.x & 63;
  for (u64 base = (u64)blockIdx.x * kSnapThreads; base < slots; base += (u64)gridDim.x * kSnapThreads) {
    const u64 i = base + threadIdx.x;
    const u64 key = i < slots ? keys[i] : kMpcImageEmpty;
    const bool live = key != kMpcImageEmpty;
    const u64 b = __ballot(live);
    if (b == 0ull) continue;                     // (uniform over the wave)
    u64 off = 0ull;
    if (lane == 0) off = atomicAdd(counter, (u64)__popcll(b));
    off = (u64)__shfl((long long)off, 0);
    if (live) {
      const u64 at = off + (u64)__popcll(b & ((1ull << lane) - 1ull));
      if (at < cap) {
        okeys[at] = key;
        oslot[at] = (u32)i;
      }
    }
  }
}

// a lane per sorted unit: the units that begin a line, the sums of a plan, the flags of the emitted lines
__global__ void __launch_bounds__(kSnapThreads)
snapshot_mark_kernel(MpcSnapLinesArgs A)
{
  __shared__ u64 s_sum[3];
  if (threadIdx.x < 3) s_sum[threadIdx.x] = 0ull;
  __syncthreads();
  const u64 k = A.k;
  const int ks = __ffs((int)A.k) - 1;                           // k is 1, 2, 4 or 8: key / k is a shift
  u64 touched = 0ull, complete = 0ull, punits = 0ull;
  for (u64 base = (u64)blockIdx.x * kSnapThreads; base < A.D; base += (u64)gridDim.x * kSnapThreads) {
    const u64 i = base + threadIdx.x;
    if (i >= A.D) continue;
    const u64 lk = A.skeys[i] >> ks;
    u32 flag = 0u;
    if (i == 0ull || A.skeys[i - 1ull] >> ks != lk) {
      u64 cnt = 1ull;
      while (cnt < k && i + cnt < A.D && A.skeys[i + cnt] >> ks == lk) cnt++;
      touched += 1ull;
      if (cnt == k) complete += 1ull; else punits += cnt;
      flag = (A.zero_fill || cnt == k) ? 1u : 0u;
    }
    A.flags[i] = flag;
  }
  for (int o = 32; o > 0; o >>= 1) {
    touched += __shfl_xor(touched, o);
    complete += __shfl_xor(complete, o);
    punits += __shfl_xor(punits, o);
  }
  if ((threadIdx.x & 63) == 0) {
    if (touched) atomicAdd(&s_sum[0], touched);
    if (complete) atomicAdd(&s_sum[1], complete);
    if (punits) atomicAdd(&s_sum[2], punits);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    if (s_sum[0]) atomicAdd(&A.plan[MPC_SNAP_PLAN_TOUCHED], s_sum[0]);
    if (s_sum[1]) atomicAdd(&A.plan[MPC_SNAP_PLAN_COMPLETE], s_sum[1]);
    if (s_sum[2]) atomicAdd(&A.plan[MPC_SNAP_PLAN_PARTIAL_UNITS], s_sum[2]);
  }
}

// heads[j] = the sorted index of the first unit of emitted line j (A.n: the emitted lines, the bound of the write)
__global__ void __launch_bounds__(kSnapThreads)
snapshot_heads_kernel(MpcSnapLinesArgs A)
{
  for (u64 i = (u64)blockIdx.x * kSnapThreads + threadIdx.x; i < A.D; i += (u64)gridDim.x * kSnapThreads) {
    if (!A.flags[i]) continue;
    const u64 j = A.index[i];
    if (j < A.n) A.heads[j] = (u32)i;
  }
}

// emitted lines [first, first + n): L / 16 lanes per line, 16 bytes each, from the payload of the unit or zero
__global__ void __launch_bounds__(kSnapThreads)
snapshot_gather_kernel(MpcSnapLinesArgs A)
{
  const u64 k = A.k;
  const int ks = __ffs((int)A.k) - 1, ps = __ffs((int)(A.unit_bytes / 16u)) - 1;      // k and the parts are powers of two: shifts and masks
  const u64 parts = 1ull << ps;                                // 16-byte parts per unit
  const u64 lpl = parts << ks;                                 // ... per line
  const u64 work = A.n << (ps + ks);
  const uint4 *src = reinterpret_cast<const uint4 *>(A.payload);
  uint4 *dst = reinterpret_cast<uint4 *>(A.lines_out);
  for (u64 g = (u64)blockIdx.x * kSnapThreads + threadIdx.x; g < work; g += (u64)gridDim.x * kSnapThreads) {
    const u64 j = g >> (ps + ks), q = g & (lpl - 1ull);
    const u64 h = A.heads[A.first + j];
    const u64 lk = A.skeys[h] >> ks;
    const u64 want = (lk << ks) + (q >> ps);
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    u32 mask = 0u;
    for (u64 t = 0; t < k && h + t < A.D; t++) {
      const u64 key = A.skeys[h + t];
      if (key >> ks != lk) break;
      mask |= 1u << (u32)(key & (k - 1ull));
      if (key == want) v = src[((u64)A.sslot[h + t] << ps) + (q & (parts - 1ull))];
    }
    dst[g] = v;
    if (q == 0ull) {
      if (A.addrs_out) A.addrs_out[j] = (lk << ks) * (u64)A.unit_bytes;
      if (A.presence_out) A.presence_out[j] = (uint8_t)mask;
    }
  }
}

namespace {
bool pow2(u64 v) { return v && !(v & (v - 1ull)); }
int grid_of(u64 work, int grid)
{
  const u64 need = (work + kSnapThreads - 1) / kSnapThreads;
  const u64 cap = (u64)(grid < 1 ? 1 : grid);
  return (int)(need < cap ? need : cap);
}
bool lines_ok(const MpcSnapLinesArgs *A)
{
  return A->skeys && A->D && (A->unit_bytes == 32u || A->unit_bytes == 64u || A->unit_bytes == 128u) &&
         (A->k == 1u || A->k == 2u || A->k == 4u || A->k == 8u) && A->k * A->unit_bytes <= MPC_SNAP_MAX_LINE;
}
}  // namespace

extern "C" hipError_t mpc_launch_snapshot_add(const MpcSnapAddArgs *A, unsigned long long n, int grid, hipStream_t stream)
{
  if (!A->units || !A->addrs || !A->keys || !A->stamp || !A->payload || !A->unit_slot || !A->ctl || !pow2(A->slot_mask + 1ull) ||
      A->slot_mask + 1ull < 2ull || A->slot_mask + 1ull > (1ull << 29) || A->capacity == 0 || A->capacity > (A->slot_mask + 1ull) / 2ull ||
      (A->unit_bytes != 32u && A->unit_bytes != 64u && A->unit_bytes != 128u) || A->unit_bytes != (1u << A->unit_shift) ||
      (((uintptr_t)A->units) & 15u) || (((uintptr_t)A->addrs) & 7u))
    return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  const int g = grid_of(n, grid);
  MpcSnapAddArgs B = *A;
  // all waves of the launch together hold back at most capacity / 4 claims (mpc_launch_image_update)
  const u64 share = A->capacity / (4ull * (u64)g * (kSnapThreads / 64));
  B.flush_claims = share < 1ull ? 1ull : share > 1024ull ? 1024ull : share;
  hipLaunchKernelGGL(snapshot_stamp_kernel, dim3(g), dim3(kSnapThreads), 0, stream, B, n);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(snapshot_copy_kernel, dim3(grid_of(n * (A->unit_bytes / 16u), grid)), dim3(kSnapThreads), 0, stream, B, n);
  return hipGetLastError();
}

extern "C" hipError_t mpc_launch_snapshot_compact(const unsigned long long *keys, unsigned long long slots, unsigned long long *okeys, uint32_t *oslot,
                                                  unsigned long long cap, unsigned long long *counter, int grid, hipStream_t stream)
{
  if (!keys || !okeys || !oslot || !counter || !pow2(slots) || cap == 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(snapshot_compact_kernel, dim3(grid_of(slots, grid)), dim3(kSnapThreads), 0, stream, keys, slots, okeys, oslot, cap, counter);
  return hipGetLastError();
}

extern "C" hipError_t mpc_launch_snapshot_mark(const MpcSnapLinesArgs *A, int grid, hipStream_t stream)
{
  if (!lines_ok(A) || !A->flags || !A->plan) return hipErrorInvalidValue;
  hipLaunchKernelGGL(snapshot_mark_kernel, dim3(grid_of(A->D, grid)), dim3(kSnapThreads), 0, stream, *A);
  return hipGetLastError();
}

extern "C" hipError_t mpc_launch_snapshot_heads(const MpcSnapLinesArgs *A, int grid, hipStream_t stream)
{
  if (!lines_ok(A) || !A->flags || !A->index || !A->heads || A->n == 0 || A->n > A->D) return hipErrorInvalidValue;
  hipLaunchKernelGGL(snapshot_heads_kernel, dim3(grid_of(A->D, grid)), dim3(kSnapThreads), 0, stream, *A);
  return hipGetLastError();
}

extern "C" hipError_t mpc_launch_snapshot_gather(const MpcSnapLinesArgs *A, int grid, hipStream_t stream)
{
  if (!lines_ok(A) || !A->sslot || !A->heads || !A->payload || !A->lines_out || (((uintptr_t)A->lines_out) & 15u) || (((uintptr_t)A->addrs_out) & 7u))
    return hipErrorInvalidValue;
  if (A->n == 0) return hipSuccess;
  hipLaunchKernelGGL(snapshot_gather_kernel, dim3(grid_of(A->n * (u64)(A->k * A->unit_bytes / 16u), grid)), dim3(kSnapThreads), 0, stream, *A);
  return hipGetLastError();
}

// ---- the snapshot object (include/mpc_hip_snapshot.h) ------------------------------------------------------------------

constexpr u64 kPieceLines = 4ull << 20;        // of an evaluation, a read and an add's scratch
constexpr u64 kStageUnits = 1ull << 20;        // of a host add

struct mpc_snapshot {
  int device = 0, num_cus = 256;
  unsigned U = 0;
  int shift = 0;
  u64 capacity = 0, slots = 0, hash_mask = ~0ull;
  hipStream_t stream = nullptr;
  u64 *d_keys = nullptr, *d_stamp = nullptr;   // [slots] each, one allocation
  uint8_t *d_payload = nullptr;                // [slots x U]
  u64 *d_ctl = nullptr;                        // [MPC_SNAP_CTL_LEN] | plan sums [MPC_SNAP_PLAN_LEN] | the compaction's counter
  u64 seen = 0;                                // units added: the next unit's position
  u64 ctl[MPC_SNAP_CTL_LEN] = {};              // what status() last read
  bool over = false;                           // a key beyond the capacity arrived
  uint32_t *d_unit_slot = nullptr;             // the add kernels' scratch
  u64 unit_slot_cap = 0;
  uint8_t *d_in = nullptr;                     // a host add's chunk on the device: units | addresses
  u64 in_cap = 0;
  // the sorted live (key, slot) pairs, valid until the next add or reset
  bool sorted = false;
  u64 D = 0;
  u64 *d_skeys = nullptr;
  uint32_t *d_sslot = nullptr;
  // the plan of one (line size, partial), valid as long as the sorted pairs
  bool planned = false;
  unsigned plan_L = 0;
  int plan_partial = 0;
  u64 plan[MPC_SNAPSHOT_TABLE_LEN] = {};
  uint32_t *d_heads = nullptr;
  uint8_t *d_out = nullptr;                    // pieces of emitted lines for an evaluation or a read
  u64 out_cap = 0;
  std::string error;
};

namespace {

thread_local std::string g_snapshot_error;

int fail(mpc_snapshot *s, int code, const std::string &msg)
{
  if (s) s->error = msg; else g_snapshot_error = msg;
  return code;
}

#define SNAPCHK(s, call)                                                                           \
  do {                                                                                             \
    const hipError_t e_ = (call);                                                                  \
    if (e_ != hipSuccess) return fail((s), MPC_E_HIP, std::string(#call ": ") + hipGetErrorString(e_)); \
  } while (0)

std::string refusal_of(unsigned U, u64 capacity, unsigned L)
{
  if (U != 32u && U != 64u && U != 128u) return "snapshot: unit_bytes must be 32, 64 or 128, not " + std::to_string(U);
  if (capacity == 0) return "snapshot: capacity_units must be at least 1";
  if (capacity > MPC_SNAPSHOT_MAX_CAPACITY)
    return "snapshot: capacity_units above " + std::to_string(MPC_SNAPSHOT_MAX_CAPACITY) + " (2^28; the table takes 2 x (16 + unit_bytes) bytes per unit of capacity)";
  if (L == 0) return "";
  if (L > MPC_SNAPSHOT_MAX_LINE) return "snapshot: line_size " + std::to_string(L) + " is above 256";
  const unsigned k = L / U;
  if (L % U != 0 || (k != 1u && k != 2u && k != 4u && k != 8u))
    return "snapshot: line_size " + std::to_string(L) + " is not 1, 2, 4 or 8 units of " + std::to_string(U) + " bytes";
  return "";
}

u64 slots_of(u64 capacity)
{
  u64 s = 2;
  while (s < 2 * capacity) s <<= 1;
  return s;
}

int grid_cap(const mpc_snapshot *s)
{
  long cap = (long)s->num_cus * 8;
#if MPC_TESTING
  // test library only: MPC_TEST_GRID caps the grid so that the kernels' loops stride on small inputs
  static const long test_cap = []() { const char *e = getenv("MPC_TEST_GRID"); return e ? atol(e) : 0L; }();
  if (test_cap > 0 && cap > test_cap) cap = test_cap;
#endif
  return (int)cap;
}

void drop_plan(mpc_snapshot *s)
{
  s->sorted = s->planned = false;
  if (s->d_skeys) (void)hipFree(s->d_skeys);
  if (s->d_sslot) (void)hipFree(s->d_sslot);
  if (s->d_heads) (void)hipFree(s->d_heads);
  s->d_skeys = nullptr;
  s->d_sslot = nullptr;
  s->d_heads = nullptr;
  s->D = 0;
}

int over_error(mpc_snapshot *s)
{
  return fail(s, MPC_E_INVAL, "snapshot: more than " + std::to_string(s->capacity) +
                                  " distinct unit addresses (capacity_units of mpc_snapshot_create): the snapshot is incomplete and takes no more units");
}

// at a point where the device is idle: has a key beyond the capacity arrived?
int status(mpc_snapshot *s)
{
  if (!s->over) {
    SNAPCHK(s, hipMemcpy(s->ctl, s->d_ctl, sizeof(s->ctl), hipMemcpyDeviceToHost));
    s->over = s->ctl[MPC_SNAP_CTL_KEYS] > s->capacity || s->ctl[MPC_SNAP_CTL_OVERFLOW] != 0;
  }
  return s->over ? over_error(s) : MPC_OK;
}

int wait_status(mpc_snapshot *s)
{
  SNAPCHK(s, hipSetDevice(s->device));
  SNAPCHK(s, hipDeviceSynchronize());            // (adds may have been queued on caller streams)
  return status(s);
}

int clear(mpc_snapshot *s)
{
  SNAPCHK(s, hipMemset(s->d_keys, 0xff, s->slots * sizeof(u64)));
  SNAPCHK(s, hipMemset(s->d_stamp, 0, s->slots * sizeof(u64)));
  SNAPCHK(s, hipMemset(s->d_ctl, 0, (MPC_SNAP_CTL_LEN + MPC_SNAP_PLAN_LEN + 1) * sizeof(u64)));
  SNAPCHK(s, hipDeviceSynchronize());            // (the kernels run on non-blocking streams)
  s->seen = 0;
  s->over = false;
  std::fill(s->ctl, s->ctl + MPC_SNAP_CTL_LEN, 0ull);
  return MPC_OK;
}

// units already in device memory: pieces of kPieceLines units over the slot scratch, on `stream`
int add_device(mpc_snapshot *s, const uint8_t *d_units, u64 n, const uint64_t *d_addrs, hipStream_t stream)
{
  const u64 want = std::min<u64>(n, kPieceLines);
  if (s->unit_slot_cap < want) {
    if (s->d_unit_slot) SNAPCHK(s, hipFree(s->d_unit_slot));     // (waits for the launches that use it)
    s->d_unit_slot = nullptr;
    s->unit_slot_cap = 0;
    if (hipMalloc((void **)&s->d_unit_slot, want * sizeof(uint32_t)) != hipSuccess) {
      s->d_unit_slot = nullptr;
      return fail(s, MPC_E_NOMEM, "hipMalloc(snapshot add scratch, " + std::to_string(want * sizeof(uint32_t)) + " bytes) failed");
    }
    s->unit_slot_cap = want;
  }
  drop_plan(s);
  for (u64 at = 0; at < n; at += kPieceLines) {
    const u64 take = std::min<u64>(n - at, kPieceLines);
    MpcSnapAddArgs A{};
    A.units = d_units + at * (u64)s->U;
    A.addrs = d_addrs + at;
    A.keys = s->d_keys;
    A.stamp = s->d_stamp;
    A.payload = s->d_payload;
    A.unit_slot = s->d_unit_slot;
    A.ctl = s->d_ctl;
    A.slot_mask = s->slots - 1ull;
    A.hash_mask = s->hash_mask;
    A.pos = s->seen;
    A.capacity = s->capacity;
    A.unit_bytes = s->U;
    A.unit_shift = s->shift;
    const hipError_t e = mpc_launch_snapshot_add(&A, take, grid_cap(s), stream);
    if (e != hipSuccess) return fail(s, MPC_E_HIP, std::string("kernel launch (snapshot add): ") + hipGetErrorString(e));
    s->seen += take;
  }
  return MPC_OK;
}

// units in host memory: chunks of kStageUnits through one device buffer, on the snapshot's stream; does not wait
int add_host(mpc_snapshot *s, const uint8_t *units, u64 n, const uint64_t *addrs)
{
  const u64 want = std::min<u64>(n, kStageUnits);
  if (s->in_cap < want) {
    if (s->d_in) SNAPCHK(s, hipFree(s->d_in));
    s->d_in = nullptr;
    s->in_cap = 0;
    if (hipMalloc((void **)&s->d_in, want * ((u64)s->U + 8ull)) != hipSuccess) {
      s->d_in = nullptr;
      return fail(s, MPC_E_NOMEM, "hipMalloc(snapshot staging, " + std::to_string(want * ((u64)s->U + 8ull)) + " bytes) failed");
    }
    s->in_cap = want;
  }
  uint64_t *d_adr = reinterpret_cast<uint64_t *>(s->d_in + s->in_cap * (u64)s->U);
  for (u64 at = 0; at < n; at += kStageUnits) {
    const u64 take = std::min<u64>(n - at, kStageUnits);
    SNAPCHK(s, hipMemcpyAsync(s->d_in, units + at * (u64)s->U, take * (u64)s->U, hipMemcpyHostToDevice, s->stream));
    SNAPCHK(s, hipMemcpyAsync(d_adr, addrs + at, take * sizeof(uint64_t), hipMemcpyHostToDevice, s->stream));
    if (const int rc = add_device(s, s->d_in, take, d_adr, s->stream)) return rc;
  }
  return MPC_OK;
}

int finish_add(mpc_snapshot *s)
{
  SNAPCHK(s, hipStreamSynchronize(s->stream));
  return status(s);
}

// the live (key, slot) pairs sorted by key; the device is idle and the snapshot within its capacity
int ensure_sorted(mpc_snapshot *s)
{
  if (s->sorted) return MPC_OK;
  drop_plan(s);
  const u64 D = s->ctl[MPC_SNAP_CTL_KEYS];
  if (D == 0) {
    s->sorted = true;
    return MPC_OK;
  }
  u64 *d_k = nullptr, *d_counter = s->d_ctl + MPC_SNAP_CTL_LEN + MPC_SNAP_PLAN_LEN;
  uint32_t *d_v = nullptr;
  void *d_tmp = nullptr;
  size_t tmp_bytes = 0;
  int rc = MPC_OK;
  u64 counted = 0;
  auto hip = [&](hipError_t e, const char *what) {
    if (e != hipSuccess && rc == MPC_OK) rc = fail(s, e == hipErrorOutOfMemory ? MPC_E_NOMEM : MPC_E_HIP, std::string("snapshot plan, ") + what + ": " + hipGetErrorString(e));
    return e == hipSuccess && rc == MPC_OK;
  };
  if (hip(hipMalloc((void **)&d_k, D * sizeof(u64)), "hipMalloc(keys)") && hip(hipMalloc((void **)&d_v, D * sizeof(uint32_t)), "hipMalloc(slots)") &&
      hip(hipMalloc((void **)&s->d_skeys, D * sizeof(u64)), "hipMalloc(sorted keys)") &&
      hip(hipMalloc((void **)&s->d_sslot, D * sizeof(uint32_t)), "hipMalloc(sorted slots)") &&
      hip(rocprim::radix_sort_pairs(nullptr, tmp_bytes, d_k, s->d_skeys, d_v, s->d_sslot, (size_t)D, 0u, 64u, s->stream), "sizing the sort") &&
      hip(hipMalloc(&d_tmp, tmp_bytes ? tmp_bytes : 16), "hipMalloc(sort scratch)") &&
      hip(hipMemsetAsync(d_counter, 0, sizeof(u64), s->stream), "hipMemsetAsync") &&
      hip(mpc_launch_snapshot_compact(s->d_keys, s->slots, d_k, d_v, D, d_counter, grid_cap(s), s->stream), "kernel launch (compact)") &&
      hip(rocprim::radix_sort_pairs(d_tmp, tmp_bytes, d_k, s->d_skeys, d_v, s->d_sslot, (size_t)D, 0u, 64u, s->stream), "the sort") &&
      hip(hipMemcpyAsync(&counted, d_counter, sizeof(u64), hipMemcpyDeviceToHost, s->stream), "hipMemcpyAsync"))
    (void)hip(hipStreamSynchronize(s->stream), "hipStreamSynchronize");
  if (d_k) (void)hipFree(d_k);
  if (d_v) (void)hipFree(d_v);
  if (d_tmp) (void)hipFree(d_tmp);
  if (rc == MPC_OK && counted != D)
    rc = fail(s, MPC_E_HIP, "snapshot plan: the table holds " + std::to_string(counted) + " units, the count says " + std::to_string(D) + " (internal error)");
  if (rc != MPC_OK) {
    drop_plan(s);
    return rc;
  }
  s->D = D;
  s->sorted = true;
  return MPC_OK;
}

MpcSnapLinesArgs lines_args(const mpc_snapshot *s, unsigned L, int partial)
{
  MpcSnapLinesArgs A{};
  A.skeys = s->d_skeys;
  A.sslot = s->d_sslot;
  A.D = s->D;
  A.heads = s->d_heads;
  A.payload = s->d_payload;
  A.unit_bytes = s->U;
  A.k = L / s->U;
  A.zero_fill = partial == MPC_SNAPSHOT_PARTIAL_ZERO;
  return A;
}

// the plan of (L, partial): waits, then counts and numbers the emitted lines unless that plan is still current
int ensure_plan(mpc_snapshot *s, unsigned L, int partial)
{
  const std::string why = L ? refusal_of(s->U, s->capacity, L) : std::string("snapshot: line_size must be at least one unit");
  if (!why.empty()) return fail(s, MPC_E_INVAL, why);
  if (partial != MPC_SNAPSHOT_PARTIAL_SKIP && partial != MPC_SNAPSHOT_PARTIAL_ZERO)
    return fail(s, MPC_E_INVAL, "snapshot: partial is MPC_SNAPSHOT_PARTIAL_SKIP (0) or MPC_SNAPSHOT_PARTIAL_ZERO (1)");
  if (const int rc = wait_status(s)) return rc;
  if (s->sorted && s->planned && s->plan_L == L && s->plan_partial == partial) return MPC_OK;
  if (const int rc = ensure_sorted(s)) return rc;
  s->planned = false;
  if (s->d_heads) (void)hipFree(s->d_heads);
  s->d_heads = nullptr;
  std::fill(s->plan, s->plan + MPC_SNAPSHOT_TABLE_LEN, 0ull);
  const u64 k = L / s->U;
  if (s->D) {
    uint32_t *d_flags = nullptr, *d_index = nullptr;
    void *d_tmp = nullptr;
    size_t tmp_bytes = 0;
    u64 *d_plan = s->d_ctl + MPC_SNAP_CTL_LEN, sums[MPC_SNAP_PLAN_LEN] = {};
    int rc = MPC_OK;
    auto hip = [&](hipError_t e, const char *what) {
      if (e != hipSuccess && rc == MPC_OK) rc = fail(s, e == hipErrorOutOfMemory ? MPC_E_NOMEM : MPC_E_HIP, std::string("snapshot plan, ") + what + ": " + hipGetErrorString(e));
      return e == hipSuccess && rc == MPC_OK;
    };
    MpcSnapLinesArgs A = lines_args(s, L, partial);
    u64 n_out = 0;
    if (hip(hipMalloc((void **)&d_flags, s->D * sizeof(uint32_t)), "hipMalloc(flags)") && hip(hipMalloc((void **)&d_index, s->D * sizeof(uint32_t)), "hipMalloc(index)") &&
        hip(rocprim::exclusive_scan(nullptr, tmp_bytes, d_flags, d_index, 0u, (size_t)s->D, rocprim::plus<uint32_t>(), s->stream), "sizing the scan") &&
        hip(hipMalloc(&d_tmp, tmp_bytes ? tmp_bytes : 16), "hipMalloc(scan scratch)")) {
      A.flags = d_flags;
      A.index = d_index;
      A.plan = d_plan;
      if (hip(hipMemsetAsync(d_plan, 0, MPC_SNAP_PLAN_LEN * sizeof(u64), s->stream), "hipMemsetAsync") &&
          hip(mpc_launch_snapshot_mark(&A, grid_cap(s), s->stream), "kernel launch (mark)") &&
          hip(rocprim::exclusive_scan(d_tmp, tmp_bytes, d_flags, d_index, 0u, (size_t)s->D, rocprim::plus<uint32_t>(), s->stream), "the scan") &&
          hip(hipMemcpyAsync(sums, d_plan, sizeof(sums), hipMemcpyDeviceToHost, s->stream), "hipMemcpyAsync") &&
          hip(hipStreamSynchronize(s->stream), "hipStreamSynchronize")) {
        n_out = A.zero_fill ? sums[MPC_SNAP_PLAN_TOUCHED] : sums[MPC_SNAP_PLAN_COMPLETE];
        if (n_out > s->D || sums[MPC_SNAP_PLAN_TOUCHED] > s->D) rc = fail(s, MPC_E_HIP, "snapshot plan: more lines than units (internal error)");
        if (rc == MPC_OK && n_out && hip(hipMalloc((void **)&s->d_heads, n_out * sizeof(uint32_t)), "hipMalloc(heads)")) {
          A.heads = s->d_heads;
          A.n = n_out;
          if (hip(mpc_launch_snapshot_heads(&A, grid_cap(s), s->stream), "kernel launch (heads)")) (void)hip(hipStreamSynchronize(s->stream), "hipStreamSynchronize");
        }
      }
    }
    if (d_flags) (void)hipFree(d_flags);
    if (d_index) (void)hipFree(d_index);
    if (d_tmp) (void)hipFree(d_tmp);
    if (rc != MPC_OK) {
      if (s->d_heads) (void)hipFree(s->d_heads);
      s->d_heads = nullptr;
      return rc;
    }
    const u64 touched = sums[MPC_SNAP_PLAN_TOUCHED], complete = sums[MPC_SNAP_PLAN_COMPLETE], punits = sums[MPC_SNAP_PLAN_PARTIAL_UNITS];
    s->plan[0] = touched;
    s->plan[1] = complete;
    s->plan[2] = touched - complete;
    s->plan[3] = punits;
    s->plan[4] = k * (touched - complete) - punits;
    s->plan[5] = n_out;
  }
  s->plan_L = L;
  s->plan_partial = partial;
  s->planned = true;
  return MPC_OK;
}

// emitted lines [first, first + n) of the current plan, on `stream`
int write_planned(mpc_snapshot *s, u64 first, u64 n, void *d_lines, uint64_t *d_addrs, uint8_t *d_presence, hipStream_t stream)
{
  if (first > s->plan[5] || n > s->plan[5] - first)
    return fail(s, MPC_E_INVAL, "snapshot: lines [" + std::to_string(first) + ", " + std::to_string(first) + " + " + std::to_string(n) + ") lie beyond the " +
                                    std::to_string(s->plan[5]) + " emitted lines of the plan");
  if (n == 0) return MPC_OK;
  if (!d_lines) return fail(s, MPC_E_INVAL, "snapshot: no buffer for the lines");
  if (((uintptr_t)d_lines) & 15u) return fail(s, MPC_E_INVAL, "device line buffer must be 16-byte aligned");
  if (((uintptr_t)d_addrs) & 7u) return fail(s, MPC_E_INVAL, "device address buffer must be 8-byte aligned");
  MpcSnapLinesArgs A = lines_args(s, s->plan_L, s->plan_partial);
  A.first = first;
  A.n = n;
  A.lines_out = static_cast<uint8_t *>(d_lines);
  A.addrs_out = d_addrs;
  A.presence_out = d_presence;
  const hipError_t e = mpc_launch_snapshot_gather(&A, grid_cap(s), stream);
  return e == hipSuccess ? MPC_OK : fail(s, MPC_E_HIP, std::string("kernel launch (snapshot gather): ") + hipGetErrorString(e));
}

}  // namespace

int mpc_snapshot_piece_lines() { return (int)kPieceLines; }
int mpc_snapshot_device_of(const mpc_snapshot *s) { return s->device; }
int mpc_snapshot_fail(mpc_snapshot *s, int code, const char *msg) { return fail(s, code, msg ? msg : ""); }

// a piece of at most kPieceLines emitted lines in the scratch buffer: lines | addresses | presence masks, written on the
// snapshot's stream behind whatever read the buffer last on that stream
int mpc_snapshot_piece(mpc_snapshot *s, unsigned L, int partial, unsigned long long first, unsigned long long n, const void **d_lines, const uint64_t **d_addrs,
                       const uint8_t **d_presence, void **stream)
{
  if (n > kPieceLines) return fail(s, MPC_E_INVAL, "snapshot: a piece has at most 4 Mi lines");
  if (const int rc = ensure_plan(s, L, partial)) return rc;
  const u64 cap = std::min<u64>(std::max<u64>(s->plan[5], 1ull), kPieceLines);
  const u64 need = cap * ((u64)L + 9ull) + 16ull;
  if (s->out_cap < need) {
    if (s->d_out) SNAPCHK(s, hipFree(s->d_out));
    s->d_out = nullptr;
    s->out_cap = 0;
    if (hipMalloc((void **)&s->d_out, need) != hipSuccess) {
      s->d_out = nullptr;
      return fail(s, MPC_E_NOMEM, "hipMalloc(snapshot lines scratch, " + std::to_string(need) + " bytes) failed");
    }
    s->out_cap = need;
  }
  uint8_t *lines = s->d_out;
  uint64_t *addrs = reinterpret_cast<uint64_t *>(s->d_out + ((n * (u64)L + 15ull) & ~15ull));
  uint8_t *presence = reinterpret_cast<uint8_t *>(addrs + n);
  if (const int rc = write_planned(s, first, n, lines, addrs, presence, s->stream)) return rc;
  *d_lines = lines;
  *d_addrs = addrs;
  *d_presence = presence;
  *stream = s->stream;
  return MPC_OK;
}

extern "C" {

const char *mpc_snapshot_last_error(const mpc_snapshot *s) { return s ? s->error.c_str() : g_snapshot_error.c_str(); }

int mpc_snapshot_check_values(unsigned unit_bytes, uint64_t capacity_units, unsigned line_size)
{
  const std::string why = refusal_of(unit_bytes, capacity_units, line_size);
  return why.empty() ? MPC_OK : fail(nullptr, MPC_E_INVAL, why);
}

void mpc_snapshot_destroy(mpc_snapshot *s)
{
  if (!s) return;
  (void)hipSetDevice(s->device);
  (void)hipDeviceSynchronize();
  drop_plan(s);
  if (s->d_keys) (void)hipFree(s->d_keys);
  if (s->d_payload) (void)hipFree(s->d_payload);
  if (s->d_ctl) (void)hipFree(s->d_ctl);
  if (s->d_unit_slot) (void)hipFree(s->d_unit_slot);
  if (s->d_in) (void)hipFree(s->d_in);
  if (s->d_out) (void)hipFree(s->d_out);
  if (s->stream) (void)hipStreamDestroy(s->stream);
  delete s;
}

int mpc_snapshot_create(unsigned unit_bytes, uint64_t capacity_units, int device, mpc_snapshot **out)
{
  if (!out) return MPC_E_INVAL;
  *out = nullptr;
  const std::string why = refusal_of(unit_bytes, capacity_units, 0);
  if (!why.empty()) return fail(nullptr, MPC_E_INVAL, why);
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(nullptr, MPC_E_NODEVICE, "no HIP device available (libmpc_hip has no CPU fallback)");
  if (device < 0 && hipGetDevice(&device) != hipSuccess) device = 0;
  if (device >= n) return fail(nullptr, MPC_E_INVAL, "device ordinal out of range");
  if (hipSetDevice(device) != hipSuccess) return fail(nullptr, MPC_E_NODEVICE, "hipSetDevice failed");
  mpc_snapshot *s = new (std::nothrow) mpc_snapshot;
  if (!s) return fail(nullptr, MPC_E_NOMEM, "out of memory");
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) == hipSuccess) s->num_cus = prop.multiProcessorCount;
  s->device = device;
  s->U = unit_bytes;
  s->shift = unit_bytes == 32u ? 5 : unit_bytes == 64u ? 6 : 7;
  s->capacity = capacity_units;
  s->slots = slots_of(capacity_units);
#if MPC_TESTING
  // chains through most of the table at any capacity: keep only the low bits of the hash
  if (const char *e = getenv("MPC_TEST_SNAPSHOT_HASH_BITS")) {
    const long bits = atol(e);
    if (bits >= 0 && bits < 64) s->hash_mask = (1ull << bits) - 1ull;
  }
#endif
  int rc = MPC_OK;
  if (hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking) != hipSuccess) {
    s->stream = nullptr;
    rc = fail(nullptr, MPC_E_NODEVICE, "hipStreamCreate failed");
  }
  if (rc == MPC_OK && hipMalloc((void **)&s->d_keys, 2 * s->slots * sizeof(u64)) != hipSuccess) {
    s->d_keys = nullptr;
    rc = fail(nullptr, MPC_E_NOMEM, "hipMalloc(snapshot table, " + std::to_string(2 * s->slots * sizeof(u64)) + " bytes) failed");
  }
  if (rc == MPC_OK && hipMalloc((void **)&s->d_payload, s->slots * (u64)s->U) != hipSuccess) {
    s->d_payload = nullptr;
    rc = fail(nullptr, MPC_E_NOMEM, "hipMalloc(snapshot payload, " + std::to_string(s->slots * (u64)s->U) + " bytes) failed");
  }
  if (rc == MPC_OK && hipMalloc((void **)&s->d_ctl, (MPC_SNAP_CTL_LEN + MPC_SNAP_PLAN_LEN + 1) * sizeof(u64)) != hipSuccess) {
    s->d_ctl = nullptr;
    rc = fail(nullptr, MPC_E_NOMEM, "hipMalloc(snapshot counters) failed");
  }
  if (rc == MPC_OK) {
    s->d_stamp = s->d_keys + s->slots;
    rc = clear(s);
    if (rc != MPC_OK) g_snapshot_error = s->error;
  }
  if (rc != MPC_OK) {
    mpc_snapshot_destroy(s);
    return rc;
  }
  *out = s;
  return MPC_OK;
}

int mpc_snapshot_reset(mpc_snapshot *s)
{
  if (!s) return MPC_E_INVAL;
  SNAPCHK(s, hipSetDevice(s->device));
  SNAPCHK(s, hipDeviceSynchronize());
  drop_plan(s);
  return clear(s);
}

int mpc_snapshot_add(mpc_snapshot *s, const uint8_t *units, uint64_t n, const uint64_t *addresses)
{
  if (!s) return MPC_E_INVAL;
  if (n && (!units || !addresses)) return fail(s, MPC_E_INVAL, "snapshot: an add needs the units and one address per unit");
  if (s->over) return over_error(s);
  if (n == 0) return MPC_OK;
  SNAPCHK(s, hipSetDevice(s->device));
  if (const int rc = add_host(s, units, n, addresses)) return rc;
  return finish_add(s);
}

int mpc_snapshot_add_device(mpc_snapshot *s, const void *d_units, uint64_t n, const uint64_t *d_addresses, void *hip_stream)
{
  if (!s) return MPC_E_INVAL;
  if (n && (!d_units || !d_addresses)) return fail(s, MPC_E_INVAL, "snapshot: an add needs the units and one address per unit");
  if (s->over) return over_error(s);
  if (n == 0) return MPC_OK;
  if (((uintptr_t)d_units) & 15u) return fail(s, MPC_E_INVAL, "device unit buffer must be 16-byte aligned");
  if (((uintptr_t)d_addresses) & 7u) return fail(s, MPC_E_INVAL, "device address buffer must be 8-byte aligned");
  SNAPCHK(s, hipSetDevice(s->device));
  return add_device(s, static_cast<const uint8_t *>(d_units), n, d_addresses, (hipStream_t)hip_stream);
}

// a walk over the mapped log (mpc_trace_files.h) that fills chunks for the host add; the stager is not involved
int mpc_snapshot_add_gpgpusim_log(mpc_snapshot *s, const char *log_path, uint64_t *units_added)
{
  if (units_added) *units_added = 0;
  if (!s || !log_path) return MPC_E_INVAL;
  if (s->over) return over_error(s);
  mpctrace::LogMap log;
  std::string err;
  int rc = log.open(log_path, err);
  if (rc != MPC_OK) return fail(s, rc, err);
  SNAPCHK(s, hipSetDevice(s->device));
  const u64 U = s->U;
  std::vector<uint8_t> units;
  std::vector<uint64_t> addrs;
  try {
    units.reserve((size_t)(kStageUnits * U));
    addrs.reserve((size_t)kStageUnits);
  } catch (const std::bad_alloc &) {
    return fail(s, MPC_E_NOMEM, "out of memory");
  }
  u64 added = 0;
  bool first = true;
  uint32_t req_type, req_size;
  const unsigned char *payload;
  auto flush = [&]() {
    int frc = MPC_OK;
    if (!addrs.empty()) {
      frc = add_host(s, units.data(), addrs.size(), addrs.data());
      if (frc == MPC_OK) frc = finish_add(s);      // (the chunk is reused)
      added += addrs.size();
    }
    units.clear();
    addrs.clear();
    return frc;
  };
  while (log.next(&req_type, &req_size, &payload)) {
    if (first && req_size != U)
      return fail(s, MPC_E_INVAL, "trace line size " + std::to_string(req_size) + " differs from the snapshot's unit size " + std::to_string(U));
    first = false;
    if (!payload) break;                           // incomplete trailing request
    if (req_type != 0u && req_type != 4u) continue;   // GLOBAL_ACC_R, GLOBAL_ACC_W
    if (req_size != U)
      return fail(s, MPC_E_INVAL, "the GPGPU-sim trace mixes request sizes (" + std::to_string(req_size) + " after " + std::to_string(U) + " bytes)");
    uint64_t a;
    std::memcpy(&a, payload - mpctrace::kLogRecordHeader + mpctrace::kLogRecordAddr, sizeof(a));   // mem_addr
    units.insert(units.end(), payload, payload + U);
    addrs.push_back(a);
    if (addrs.size() == kStageUnits)
      if ((rc = flush()) != MPC_OK) return rc;
  }
  if ((rc = flush()) != MPC_OK) return rc;
  if (units_added) *units_added = added;
  return MPC_OK;
}

int mpc_snapshot_stats(mpc_snapshot *s, uint64_t *t)
{
  if (!s || !t) return MPC_E_INVAL;
  if (const int rc = wait_status(s)) return rc;
  std::fill(t, t + MPC_SNAPSHOT_TABLE_LEN, 0ull);
  t[0] = s->seen;
  t[1] = s->ctl[MPC_SNAP_CTL_KEYS];
  t[2] = s->ctl[MPC_SNAP_CTL_MISALIGNED];
  t[3] = s->capacity;
  t[4] = s->U;
  return MPC_OK;
}

int mpc_snapshot_plan(mpc_snapshot *s, unsigned line_size, int partial, uint64_t *p)
{
  if (!s || !p) return MPC_E_INVAL;
  if (const int rc = ensure_plan(s, line_size, partial)) return rc;
  std::copy(s->plan, s->plan + MPC_SNAPSHOT_TABLE_LEN, p);
  return MPC_OK;
}

int mpc_snapshot_write_lines(mpc_snapshot *s, unsigned line_size, int partial, uint64_t first, uint64_t n, void *d_lines_out, uint64_t *d_addresses_out,
                             uint8_t *d_presence_out, void *hip_stream)
{
  if (!s) return MPC_E_INVAL;
  if (const int rc = ensure_plan(s, line_size, partial)) return rc;
  return write_planned(s, first, n, d_lines_out, d_addresses_out, d_presence_out, (hipStream_t)hip_stream);
}

int mpc_snapshot_read_lines(mpc_snapshot *s, unsigned line_size, int partial, uint64_t first, uint64_t n, uint8_t *lines_out, uint64_t *addresses_out,
                            uint8_t *presence_out)
{
  if (!s) return MPC_E_INVAL;
  if (const int rc = ensure_plan(s, line_size, partial)) return rc;
  if (first > s->plan[5] || n > s->plan[5] - first) return write_planned(s, first, n, nullptr, nullptr, nullptr, s->stream);   // (the refusal)
  if (n && !lines_out) return fail(s, MPC_E_INVAL, "snapshot: no buffer for the lines");
  for (u64 at = 0; at < n; at += kPieceLines) {
    const u64 take = std::min<u64>(n - at, kPieceLines);
    const void *d_lines;
    const uint64_t *d_addrs;
    const uint8_t *d_presence;
    void *stream;
    if (const int rc = mpc_snapshot_piece(s, line_size, partial, first + at, take, &d_lines, &d_addrs, &d_presence, &stream)) return rc;
    SNAPCHK(s, hipMemcpyAsync(lines_out + at * (u64)line_size, d_lines, take * (u64)line_size, hipMemcpyDeviceToHost, s->stream));
    if (addresses_out) SNAPCHK(s, hipMemcpyAsync(addresses_out + at, d_addrs, take * sizeof(uint64_t), hipMemcpyDeviceToHost, s->stream));
    if (presence_out) SNAPCHK(s, hipMemcpyAsync(presence_out + at, d_presence, take, hipMemcpyDeviceToHost, s->stream));
    SNAPCHK(s, hipStreamSynchronize(s->stream));
  }
  return MPC_OK;
}

}  // extern "C"
