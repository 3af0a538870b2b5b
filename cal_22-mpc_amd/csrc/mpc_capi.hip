// mpc_capi.hip -- the C ABI of include/mpc_hip.h: handles, the pinned
// double-buffered host->device stager, .npy streaming, statistics.
//
// There is no CPU evaluation path in this library: every size it reports was
// computed by a gfx950 kernel in mpc_kernels.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <system_error>
#include <thread>
#include <vector>

#include "../../include/mpc_hip.h"
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include "mpc_config.h"
#include "mpc_device.h"
#include "mpc_sc2.h"
#include "mpc_pattern.h"

// libmpc_hip_test.so (build.py, -DMPC_TESTING=1): route counters behind the raw statistics and a cap on the launch grid,
// see mpc_kernel_common.h.  Must agree with the kernels' translation units.
#ifndef MPC_TESTING
#define MPC_TESTING 0
#endif
constexpr size_t kRouteWords = MPC_TESTING ? 16 : 0;

typedef unsigned long long u64;

#include "mpc_jit.h"

extern "C" {
hipError_t mpc_launch_vpc_generic(const void *, u64, const MpcVpcParams *, uint16_t *, int8_t *, u64 *, int, hipStream_t);
hipError_t mpc_launch_bdi(const void *, u64, int, uint16_t *, int8_t *, u64 *, int, hipStream_t);
hipError_t mpc_launch_fpc(const void *, u64, int, uint16_t *, int8_t *, u64 *, int, hipStream_t);
hipError_t mpc_launch_bpc(const void *, u64, int, uint16_t *, int8_t *, u64 *, int, hipStream_t);
hipError_t mpc_launch_baselines(const void *, u64, int, const MpcBaselinesArgs *, int, hipStream_t);
hipError_t mpc_launch_synth(void *, u64, unsigned, int, u64, u64, const uint32_t *, hipStream_t);
hipError_t mpc_launch_read_probe(const void *, u64, uint32_t *, int, hipStream_t);
hipError_t mpc_launch_vpc_lane(const void *, u64, const MpcVpcParams *, uint16_t *, int8_t *, u64 *, int, hipStream_t);
hipError_t mpc_launch_vpc_lane_jit(hipFunction_t, hipFunction_t, const void *, u64, const MpcVpcParams *, uint16_t *, int8_t *, u64 *, int,
                                   hipStream_t);
size_t mpc_vpc_lane_smem(const MpcVpcParams *);
int mpc_vpc_lane_unrolled(const MpcVpcParams *);
size_t mpc_vpc_generic_smem(const MpcVpcParams *);
hipError_t mpc_launch_sc2_count(const void *, u64, int, u64 *, u64, uint16_t *, int8_t *, u64 *, hipStream_t);
hipError_t mpc_launch_sc2_hist(const u64 *, u64, u64, int, uint32_t *, int, hipStream_t);
hipError_t mpc_launch_sc2_collect(const u64 *, u64, u64, u64 *, uint32_t *, int, hipStream_t);
hipError_t mpc_launch_sc2_size(const void *, u64, int, const MpcSc2Table *, uint16_t *, int8_t *, u64 *, int, hipStream_t);
hipError_t mpc_launch_pattern(const void *, u64, int, uint16_t *, int8_t *, u64 *, int, hipStream_t);
hipError_t mpc_launch_pattern_set(const void *, uint32_t, int, const MpcPatternSet *, u64 *, int, hipStream_t);
}

namespace {

thread_local std::string g_create_error;

// staging: two slots, each a pinned host buffer + device buffer + stream
constexpr size_t kStageBytes = 64ull << 20;   // per slot
constexpr size_t kMiniLines = 512;            // batches up to this many lines take the small path

struct Slot {
  hipStream_t stream = nullptr;
  hipEvent_t done = nullptr;
  uint8_t *h_in = nullptr;       // pinned
  uint8_t *d_in = nullptr;
  uint16_t *d_sizes = nullptr, *h_sizes = nullptr;
  int8_t *d_sel = nullptr, *h_sel = nullptr;
  uint16_t *user_sizes = nullptr;  // where the pending results go
  int8_t *user_sel = nullptr;
  u64 pending_lines = 0;
  bool busy = false;
};

// the kernel a VPC configuration runs (route_vpc), and why it is the generic one
enum class VpcKernel { BuiltIn, BuiltInGeneral, AtCreation, RuntimeLoop, Generic };
struct VpcRoute { VpcKernel kernel = VpcKernel::Generic; std::string why_generic; };

}  // namespace

struct mpc_handle {
  int algorithm = 0;   // 0 VPC, 1 BDI, 2 FPC, 3 BPC, 4 SC2, 5 Pattern
  int device = 0;
  int L = 0;
  int num_cus = 256;
  mpc::VpcConfig cfg;
  mpc::VpcPlan plan;
  MpcVpcParams params;           // VPC: plan.params with the device addresses of the tables, what the kernels get
  VpcRoute route;                // VPC: decided once, at creation
  hipStream_t stream = nullptr;
  uint32_t *d_tab = nullptr;
  uint8_t *d_gtab = nullptr;
  u64 *d_raw = nullptr;          // device raw statistics
  u64 raw_len = 0;
  std::vector<u64> extra;        // merged-in statistics (ABI layout)
  u64 stats_len = 0;
  Slot slots[2];
  bool slots_ready = false;
  size_t stage_lines = 0;
  // small batches (the per-line CompressLine of the reference's interface above all): one pinned,
  // device-visible buffer the kernel reads the lines from and writes the results to directly --
  // no staging copies, no 64 MiB slots; a call is one launch and one stream synchronisation
  uint8_t *mini = nullptr;       // [kMiniLines * L] lines | [kMiniLines] uint16 sizes | [kMiniLines] int8 clusters
  mpcjit::Kernels jit;           // VPC: the unrolled kernels compiled at creation (mpc_jit.h; route AtCreation)
  // SC2: lines 0 .. S-1 of the trace (counted across calls) are warm-up lines, the table is built when line S arrives
  struct {
    u64 S = 0;                   // warm-up lines (the reference's m_maxSamplingCnt)
    u64 seen = 0;                // lines evaluated since creation (m_samplingCnt, not capped); not reset by mpc_stats_reset
    u64 lines = 0, warm = 0;     // statistics [0] and [3] since creation or the last reset (counted on the host)
    u64 *d_hash = nullptr;       // warm-up frequency table (mpc_sc2.hip), freed once the code table is built
    u64 hash_mask = 0;
    uint4 *d_buckets = nullptr;  // the code table's bucket image
    MpcSc2Table tab{};
    bool built = false;
    std::vector<uint32_t> symbols;   // the table, ascending symbol order
    std::vector<uint16_t> lengths;
  } sc2;
  // Pattern: the set of distinct lines (mpc_pattern.h).  Its passes must not overlap on one set: every call waits, on its
  // own stream, for the event the call before it recorded behind its passes -- whichever stream that was.
  struct {
    MpcPatternSet set{};
    hipEvent_t done = nullptr;
    bool recorded = false;
    bool over = false;           // a line beyond the capacity arrived: the handle takes no more lines
  } pat;
  std::vector<hipStream_t> group_streams;   // the slot streams of the groups this handle is a member of (sc2_build waits for them)
  std::string error;
};

namespace {

// a group's staging slot: the chunk is copied once, every member's launch follows on the slot's stream
struct GroupSlot {
  hipStream_t stream = nullptr;
  hipEvent_t done = nullptr;
  uint8_t *h_in = nullptr;       // pinned
  uint8_t *d_in = nullptr;
  // per member, allocated when a call first asks for that member's per-line output
  std::vector<uint16_t *> d_sizes, h_sizes, user_sizes;
  std::vector<int8_t *> d_sel, h_sel, user_sel;
  u64 pending_lines = 0;
  bool busy = false;
};

}  // namespace

struct mpc_group {
  std::vector<mpc_handle *> m;   // borrowed, in the caller's order
  int device = 0;
  int L = 0;
  int shared[3] = {-1, -1, -1};  // member index of the BDI, FPC, BPC handle that baselines_kernel evaluates (all -1: no shared launch)
  int first_shared = -1;         // ... the first of them in member order: where the shared launch is enqueued
  GroupSlot slots[2];            // the streams and events exist from creation, the buffers from the first staged call
  bool slots_ready = false;
  size_t stage_lines = 0;
  uint8_t *mini = nullptr;       // [kMiniLines * L] lines | per member [kMiniLines] uint16 | per member [kMiniLines] int8
  std::string form, error;
};

namespace {

int set_err(mpc_handle *h, int code, const std::string &msg)
{
  if (h) h->error = msg; else g_create_error = msg;
  return code;
}

#define HIPCHK(h, call)                                                                         \
  do {                                                                                          \
    hipError_t e_ = (call);                                                                     \
    if (e_ != hipSuccess)                                                                       \
      return set_err((h), MPC_E_HIP, std::string(#call) + ": " + hipGetErrorString(e_));        \
  } while (0)

int pick_device(int device, int *out, int *cus)
{
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0) {
    g_create_error = "no HIP device available (libmpc_hip has no CPU fallback)";
    return MPC_E_NODEVICE;
  }
  if (device < 0) {
    if (hipGetDevice(&device) != hipSuccess) device = 0;
  }
  if (device >= n) {
    g_create_error = "device ordinal out of range";
    return MPC_E_INVAL;
  }
  if (hipSetDevice(device) != hipSuccess) {
    g_create_error = "hipSetDevice failed";
    return MPC_E_NODEVICE;
  }
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) == hipSuccess) *cus = prop.multiProcessorCount;
  *out = device;
  return MPC_OK;
}

int finish_create(mpc_handle *h)
{
  if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess)
    return set_err(nullptr, MPC_E_NODEVICE, "hipStreamCreate failed");
  if (hipMalloc(&h->d_raw, (h->raw_len + kRouteWords) * sizeof(u64)) != hipSuccess)
    return set_err(nullptr, MPC_E_NOMEM, "hipMalloc(stats) failed");
  if (hipMemsetAsync(h->d_raw, 0, (h->raw_len + kRouteWords) * sizeof(u64), h->stream) != hipSuccess ||
      hipStreamSynchronize(h->stream) != hipSuccess)
    return set_err(nullptr, MPC_E_NODEVICE, "hipMemset(stats) failed");
  h->extra.assign(h->stats_len, 0);
  return MPC_OK;
}

// The one place that picks the kernel of a VPC configuration.  `jit`: a compilation at creation (mpc_jit.h) is only
// predicted (describe, compile check), still to be tried or tried and failed (a handle).
enum class Jit { Predicted, Pending, Failed };

VpcRoute route_vpc(const mpc::VpcPlan &plan, Jit jit)
{
  const MpcVpcParams &P = plan.params;
  if (!plan.fast) return {VpcKernel::Generic, plan.why_generic};
  if (mpc_vpc_lane_unrolled(&P)) return {P.gen_layout ? VpcKernel::BuiltInGeneral : VpcKernel::BuiltIn, ""};  // (never runtime_only)
  // switched on, a layout the generated source has, a sequence not too long, rings that fit beside the histogram with some
  // workgroup size (a fast plan has 32-, 64- or 128-byte lines)
  const char *env = std::getenv("MPC_JIT");
  const bool compilable = !(env && std::strcmp(env, "0") == 0) && (!P.runtime_only || plan.jit_needs) && P.n_pred >= 1 &&
                          P.n_pred <= mpcjit::max_modules() && mpc_vpc_lane_ring_plan(&P, nullptr, nullptr) != 0;
  if (compilable && jit != Jit::Failed) return {VpcKernel::AtCreation, ""};
  const unsigned no_loop = plan.jit_needs & mpc::JIT_NO_LOOP;      // (layouts the run-time module loop lacks too)
  if (!no_loop) return {VpcKernel::RuntimeLoop, ""};
  const std::string it = (no_loop & mpc::JIT_PLANES) ? "them" : "it";
  return {VpcKernel::Generic, mpc::jit_need_text(no_loop) + (jit == Jit::Predicted ? ", and run-time compilation is not available for " + it
                                                                                   : ", and the kernel for " + it + " could not be compiled at creation")};
}

int create_vpc_from_text(const std::string &text, int device, mpc_handle **out)
{
  if (!out) return MPC_E_INVAL;
  *out = nullptr;
  mpc_handle *h = new (std::nothrow) mpc_handle();
  if (!h) return MPC_E_NOMEM;
  std::string err;
  int rc = mpc::parse_vpc_config(text, h->cfg, err);
  if (rc != 0) {
    g_create_error = err;
    delete h;
    return rc;
  }
  mpc::build_vpc_plan(h->cfg, h->plan);
  h->algorithm = 0;
  h->L = h->cfg.L;
  const int K = h->cfg.M + 1;
  h->raw_len = mpc_vpc_raw_len(K, h->cfg.hist_bins);
  h->stats_len = 3ull + 6ull * K + (u64)K * h->cfg.hist_bins;
  rc = pick_device(device, &h->device, &h->num_cus);
  if (rc == MPC_OK) {
    const size_t tb = h->plan.tab.size() * sizeof(uint32_t), gb = h->plan.gtab.size();
    if (hipMalloc(&h->d_tab, tb) != hipSuccess || hipMalloc(&h->d_gtab, gb ? gb : 16) != hipSuccess ||
        hipMemcpy(h->d_tab, h->plan.tab.data(), tb, hipMemcpyHostToDevice) != hipSuccess ||
        (gb && hipMemcpy(h->d_gtab, h->plan.gtab.data(), gb, hipMemcpyHostToDevice) != hipSuccess)) {
      g_create_error = "hipMalloc/hipMemcpy of the predictor tables failed";
      rc = MPC_E_NOMEM;
    }
  }
  if (rc == MPC_OK) {
    h->params = h->plan.params;
    h->params.tab = h->d_tab;
    h->params.gtab = h->d_gtab;
    // no built-in instantiation: compile it now (mpc_jit.h); when that fails, the configuration is routed without it and says so
    h->route = route_vpc(h->plan, Jit::Pending);
    if (h->route.kernel == VpcKernel::AtCreation) {
      std::string why;
      (void)hipSetDevice(h->device);
      if (!mpcjit::build(h->plan, MPC_TESTING, h->jit, why)) {
        h->route = route_vpc(h->plan, Jit::Failed);
        std::fprintf(stderr, "libmpc_hip: module sequence [%s] runs the %s: %s\n", mpcjit::kinds_of(h->plan.params).c_str(),
                     h->route.kernel == VpcKernel::Generic ? "generic kernel (some hundred times slower)" : "run-time module loop (several times slower)",
                     why.c_str());
      }
    }
    // the statistics accumulators of a workgroup live in LDS
    const size_t smem = h->route.kernel == VpcKernel::AtCreation ? mpc_vpc_lane_ring_plan(&h->plan.params, nullptr, nullptr)
                        : h->route.kernel == VpcKernel::Generic ? mpc_vpc_generic_smem(&h->plan.params) : mpc_vpc_lane_smem(&h->plan.params);
    if (smem > 160 * 1024) {
      g_create_error = "histogram does not fit the 160 KiB LDS (too many clusters x bins)";
      rc = MPC_E_INVAL;
    }
  }
  if (rc == MPC_OK) rc = finish_create(h);
  if (rc != MPC_OK) {
    mpc_destroy(h);
    return rc;
  }
  *out = h;
  return MPC_OK;
}

// Staging copies (caller's buffer -> pinned slot) are memory-bandwidth work on the host: one
// thread moves ~12-24 GB/s, less than the PCIe link takes, so large copies are split over a
// few threads.
constexpr size_t kCopySlice = 8u << 20;
constexpr unsigned kCopyThreads = 4;

void parallel_copy(void *dst, const void *src, size_t bytes)
{
  const size_t want = (bytes + kCopySlice - 1) / kCopySlice;
  unsigned hw = std::thread::hardware_concurrency();
  if (hw == 0) hw = 1;
  const unsigned nt = (unsigned)std::min<size_t>(std::min<size_t>(want, kCopyThreads), hw);
  if (nt <= 1) { std::memcpy(dst, src, bytes); return; }
  const size_t per = ((bytes + nt - 1) / nt + 63) & ~(size_t)63;
  std::vector<std::thread> th;
  for (unsigned i = 0; i < nt; i++) {
    const size_t off = (size_t)i * per;
    if (off >= bytes) break;
    const size_t n = std::min(per, bytes - off);
    // (no exception may leave the library: a thread that cannot be started -- the host's thread limit -- copies here instead)
    try {
      th.emplace_back([=]() { std::memcpy((char *)dst + off, (const char *)src + off, n); });
    } catch (const std::system_error &) {
      std::memcpy((char *)dst + off, (const char *)src + off, n);
    }
  }
  for (auto &t : th) t.join();
}

// the same for page cache -> pinned slot; false on a short read / error
bool parallel_pread(int fd, void *dst, size_t bytes, u64 file_off)
{
  const size_t want = (bytes + kCopySlice - 1) / kCopySlice;
  unsigned hw = std::thread::hardware_concurrency();
  if (hw == 0) hw = 1;
  const unsigned nt = (unsigned)std::max<size_t>(1, std::min<size_t>(std::min<size_t>(want, kCopyThreads), hw));
  const size_t per = ((bytes + nt - 1) / nt + 4095) & ~(size_t)4095;
  std::vector<int> ok(nt, 1);
  auto work = [&](unsigned i) {
    size_t off = (size_t)i * per;
    const size_t end = std::min(bytes, off + per);
    while (off < end) {
      const ssize_t got = pread(fd, (char *)dst + off, end - off, (off_t)(file_off + off));
      if (got <= 0) { ok[i] = 0; return; }
      off += (size_t)got;
    }
  };
  std::vector<std::thread> th;
  for (unsigned i = 1; i < nt; i++) {
    try {
      th.emplace_back(work, i);
    } catch (const std::system_error &) {
      work(i);          // (the host's thread limit: read this part here)
    }
  }
  work(0);
  for (auto &t : th) t.join();
  for (int v : ok) if (!v) return false;
  return true;
}

// Workgroups per CU of the grid-stride VPC and BDI kernels.  2-8 are resident; a grid of 32 per
// CU lets CUs that finish early pick up more work (same-box A/B against 8 per CU: VPC random
// -3.5 %, mixed -5 %, 128-byte lines -9 %, all-zero traces +3 %; BDI random -8 %, pointers -10 %).
#ifndef MPC_WG_PER_CU
#define MPC_WG_PER_CU 32
#endif
constexpr int kWgPerCu = MPC_WG_PER_CU;

int grid_for(const mpc_handle *h, u64 work_items, int block, int per_cu)
{
  u64 need = (work_items + (u64)block - 1) / (u64)block;
  u64 cap = (u64)h->num_cus * (u64)per_cu;
#if MPC_TESTING
  // test library only: MPC_TEST_GRID caps the grid so that a wave walks many groups of lines (the kernels' deferred-line
  // queues then fill and drain inside the loop even on small inputs)
  static const long test_cap = []() { const char *e = getenv("MPC_TEST_GRID"); return e ? atol(e) : 0L; }();
  if (test_cap > 0 && cap > (u64)test_cap) cap = (u64)test_cap;
#endif
  if (need < 1) need = 1;
  return (int)(need < cap ? need : cap);
}

int launch_sc2(mpc_handle *h, const void *d_lines, u64 n, uint16_t *d_sizes, int8_t *d_sel, hipStream_t s);
int launch_pattern(mpc_handle *h, const void *d_lines, u64 n, uint16_t *d_sizes, int8_t *d_sel, hipStream_t s);

int launch(mpc_handle *h, const void *d_lines, u64 n, uint16_t *d_sizes, int8_t *d_sel, hipStream_t s)
{
  if (n == 0) return MPC_OK;
  if (h->algorithm == 4) return launch_sc2(h, d_lines, n, d_sizes, d_sel, s);
  if (h->algorithm == 5) return launch_pattern(h, d_lines, n, d_sizes, d_sel, s);
  hipError_t e;
  if (h->algorithm == 3) {
    e = mpc_launch_bpc(d_lines, n, h->L, d_sizes, d_sel, h->d_raw, grid_for(h, n, 256, kWgPerCu), s);
  } else if (h->algorithm == 2) {
    e = mpc_launch_fpc(d_lines, n, h->L, d_sizes, d_sel, h->d_raw, grid_for(h, n, 256, kWgPerCu), s);
  } else if (h->algorithm == 1) {
    e = mpc_launch_bdi(d_lines, n, h->L, d_sizes, d_sel, h->d_raw, grid_for(h, n, 256, kWgPerCu), s);
  } else if (h->route.kernel == VpcKernel::AtCreation) {
    e = mpc_launch_vpc_lane_jit(h->jit.stats, h->jit.lines, d_lines, n, &h->params, d_sizes, d_sel, h->d_raw,
                                grid_for(h, n, 256, kWgPerCu), s);
  } else if (h->route.kernel == VpcKernel::Generic) {
    e = mpc_launch_vpc_generic(d_lines, n, &h->params, d_sizes, d_sel, h->d_raw, grid_for(h, n, 128, 8), s);
  } else {     // built in or the run-time module loop: the lane launcher finds which
    e = mpc_launch_vpc_lane(d_lines, n, &h->params, d_sizes, d_sel, h->d_raw, grid_for(h, n, 256, kWgPerCu), s);
  }
  if (e != hipSuccess) return set_err(h, MPC_E_HIP, std::string("kernel launch: ") + hipGetErrorString(e));
  return MPC_OK;
}

// SC2: the code table from the warm-up counts.  The one blocking point of an SC2 handle: every stream that may still
// run a warm-up count (the call's, the handle's, both staging slots', the slots of the groups it belongs to) is synchronised, the 1024 largest slots are
// selected on the device (radix select, 8 bits per pass from the top), only those <= 1024 (symbol, count) pairs come
// to the host, the heap is replayed there (mpc_sc2.h) and the bucket image goes back to the device.
int sc2_build(mpc_handle *h, hipStream_t s)
{
  HIPCHK(h, hipStreamSynchronize(s));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  for (int i = 0; i < 2; i++)
    if (h->slots[i].stream) HIPCHK(h, hipStreamSynchronize(h->slots[i].stream));
  // a member of a group: the warm-up chunk may be counting on the group's other slot
  for (hipStream_t gs : h->group_streams) HIPCHK(h, hipStreamSynchronize(gs));
  const u64 n_slots = h->sc2.hash_mask + 1;
  const int grid = (int)std::min<u64>((n_slots + 255) / 256, (u64)h->num_cus * 8);
  uint32_t *d_work = nullptr;           // [256] histogram | [1] count | pad | [1024] uint64 slots
  HIPCHK(h, hipMalloc((void **)&d_work, 272 * sizeof(uint32_t) + MPC_SC2_ENTRIES * sizeof(u64)));
  u64 *d_out = reinterpret_cast<u64 *>(d_work + 272);
  auto fail = [&](const char *what, hipError_t e) {
    (void)hipFree(d_work);
    return set_err(h, MPC_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
  };
  hipError_t e;
  uint32_t hist[256];
  u64 need = MPC_SC2_ENTRIES, prefix = 0, threshold = 1;
  for (int shift = 56; shift >= 0; shift -= 8) {
    if ((e = hipMemsetAsync(d_work, 0, 256 * sizeof(uint32_t), h->stream)) != hipSuccess) return fail("hipMemsetAsync", e);
    if ((e = mpc_launch_sc2_hist(h->sc2.d_hash, n_slots, prefix, shift, d_work, grid, h->stream)) != hipSuccess) return fail("sc2 select", e);
    if ((e = hipMemcpyAsync(hist, d_work, sizeof(hist), hipMemcpyDeviceToHost, h->stream)) != hipSuccess ||
        (e = hipStreamSynchronize(h->stream)) != hipSuccess)
      return fail("sc2 select", e);
    if (shift == 56) {
      u64 total = 0;
      for (int d = 0; d < 256; d++) total += hist[d];
      if (total <= MPC_SC2_ENTRIES) break;          // no eviction: every nonzero slot (threshold 1)
    }
    int d = 255;
    for (; d > 0 && hist[d] < need; d--) need -= hist[d];
    prefix = (prefix << 8) | (u64)d;
    if (shift == 0) threshold = prefix;             // the 1024th largest slot (slots are distinct)
  }
  if ((e = hipMemsetAsync(d_work + 256, 0, sizeof(uint32_t), h->stream)) != hipSuccess ||
      (e = mpc_launch_sc2_collect(h->sc2.d_hash, n_slots, threshold, d_out, d_work + 256, grid, h->stream)) != hipSuccess)
    return fail("sc2 collect", e);
  uint32_t count = 0;
  std::vector<u64> kept(MPC_SC2_ENTRIES);
  if ((e = hipMemcpyAsync(&count, d_work + 256, sizeof(count), hipMemcpyDeviceToHost, h->stream)) != hipSuccess ||
      (e = hipMemcpyAsync(kept.data(), d_out, kept.size() * sizeof(u64), hipMemcpyDeviceToHost, h->stream)) != hipSuccess ||
      (e = hipStreamSynchronize(h->stream)) != hipSuccess)
    return fail("sc2 collect", e);
  (void)hipFree(d_work);
  if (count == 0 || count > MPC_SC2_ENTRIES) return set_err(h, MPC_E_HIP, "sc2: selection returned " + std::to_string(count) + " symbols");
  kept.resize(count);
  std::sort(kept.begin(), kept.end(), [](u64 a, u64 b) { return (uint32_t)a < (uint32_t)b; });
  std::vector<uint32_t> sym(count);
  std::vector<uint64_t> freq(count);
  for (uint32_t i = 0; i < count; i++) {
    sym[i] = (uint32_t)kept[i];
    freq[i] = kept[i] >> 32;
  }
  std::vector<uint16_t> len(count);
  if (mpcsc2::code_lengths(sym.data(), freq.data(), count, len.data()) != 0) return set_err(h, MPC_E_INVAL, "sc2: empty warm-up sample");
  std::vector<uint32_t> image;
  MpcSc2Table t{};
  if (!mpcsc2::layout(sym, len, image, t)) return set_err(h, MPC_E_HIP, "sc2: no bucket layout found for the code table");
  HIPCHK(h, hipMemcpy(h->sc2.d_buckets, image.data(), image.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  t.buckets = h->sc2.d_buckets;
  h->sc2.tab = t;
  h->sc2.symbols = std::move(sym);
  h->sc2.lengths = std::move(len);
  h->sc2.built = true;
  (void)hipFree(h->sc2.d_hash);                     // the counts are not needed again
  h->sc2.d_hash = nullptr;
  return MPC_OK;
}

// SC2: a call's lines split at line S of the trace -- warm-up counts before it, the table build at it, sizing after
int launch_sc2(mpc_handle *h, const void *d_lines, u64 n, uint16_t *d_sizes, int8_t *d_sel, hipStream_t s)
{
  const u64 warm = h->sc2.seen < h->sc2.S ? std::min<u64>(n, h->sc2.S - h->sc2.seen) : 0;
  if (warm) {
    hipError_t e = mpc_launch_sc2_count(d_lines, warm, h->L, h->sc2.d_hash, h->sc2.hash_mask, d_sizes, d_sel, h->d_raw, s);
    if (e != hipSuccess) return set_err(h, MPC_E_HIP, std::string("kernel launch: ") + hipGetErrorString(e));
    h->sc2.seen += warm;
    h->sc2.lines += warm;
    h->sc2.warm += warm;
  }
  if (warm == n) return MPC_OK;
  if (!h->sc2.built) {
    int rc = sc2_build(h, s);
    if (rc != MPC_OK) return rc;
  }
  const u64 rest = n - warm;
  // persistent: a workgroup loads the table once; 32 KiB of LDS for the largest table leaves room for 4 per CU
  const int per_cu = h->sc2.tab.mask + 1 > 1024 ? 4 : 8;
  hipError_t e = mpc_launch_sc2_size(static_cast<const uint8_t *>(d_lines) + warm * (u64)h->L, rest, h->L, &h->sc2.tab,
                                     d_sizes ? d_sizes + warm : nullptr, d_sel ? d_sel + warm : nullptr, h->d_raw,
                                     grid_for(h, rest * (u64)h->L / 16 + 1, 256 * 4, per_cu), s);
  if (e != hipSuccess) return set_err(h, MPC_E_HIP, std::string("kernel launch: ") + hipGetErrorString(e));
  h->sc2.seen += rest;
  h->sc2.lines += rest;
  return MPC_OK;
}

// Pattern: the line analysis, then the set passes behind those of every earlier call
const char *const kPatternLimit = "Pattern: more than 16777215 (2^24 - 1) distinct lines: the reference starts evicting there, which is not modelled";

int launch_pattern(mpc_handle *h, const void *d_lines, u64 n, uint16_t *d_sizes, int8_t *d_sel, hipStream_t s)
{
  if (h->pat.over) return set_err(h, MPC_E_INVAL, kPatternLimit);
  const uint8_t *base = static_cast<const uint8_t *>(d_lines);
  auto failed = [&](hipError_t e) { return set_err(h, MPC_E_HIP, std::string("kernel launch: ") + hipGetErrorString(e)); };
  // (a launch stays below 2^31 bytes: the workgroups count bytes in 32 bits)
  for (u64 at = 0; at < n; at += MPC_PATTERN_CHUNK) {
    const u64 take = std::min<u64>(n - at, MPC_PATTERN_CHUNK);
    const hipError_t e = mpc_launch_pattern(base + at * (u64)h->L, take, h->L, d_sizes ? d_sizes + at : nullptr, d_sel ? d_sel + at : nullptr,
                                            h->d_raw, grid_for(h, take, 256, kWgPerCu), s);
    if (e != hipSuccess) return failed(e);
  }
  if (h->pat.recorded) HIPCHK(h, hipStreamWaitEvent(s, h->pat.done, 0));
  for (u64 at = 0; at < n; at += MPC_PATTERN_CHUNK) {
    const u64 take = std::min<u64>(n - at, MPC_PATTERN_CHUNK);
    HIPCHK(h, hipMemsetAsync(h->pat.set.ctl + MPC_PSET_PENDING_A, 0, 2 * sizeof(u64), s));
    const hipError_t e = mpc_launch_pattern_set(base + at * (u64)h->L, (uint32_t)take, h->L, &h->pat.set, h->d_raw, grid_for(h, take, 256, 8), s);
    if (e != hipSuccess) return failed(e);
  }
  HIPCHK(h, hipEventRecord(h->pat.done, s));
  h->pat.recorded = true;
  return MPC_OK;
}

// Pattern, at a point where the handle's work is complete: has a line beyond the capacity arrived?
int pattern_status(mpc_handle *h)
{
  if (h->algorithm != 5) return MPC_OK;
  if (!h->pat.over) {
    u64 ctl[2] = {0, 0};
    HIPCHK(h, hipMemcpy(ctl, h->pat.set.ctl, sizeof(ctl), hipMemcpyDeviceToHost));
    h->pat.over = ctl[MPC_PSET_OVERFLOW] != 0;
  }
  return h->pat.over ? set_err(h, MPC_E_INVAL, kPatternLimit) : MPC_OK;
}

int ensure_slots(mpc_handle *h)
{
  if (h->slots_ready) return MPC_OK;
  h->stage_lines = kStageBytes / (size_t)h->L;
  for (int i = 0; i < 2; i++) {
    Slot &s = h->slots[i];
    HIPCHK(h, hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking));
    HIPCHK(h, hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
    HIPCHK(h, hipHostMalloc((void **)&s.h_in, kStageBytes, hipHostMallocDefault));
    HIPCHK(h, hipMalloc((void **)&s.d_in, kStageBytes));
    HIPCHK(h, hipMalloc((void **)&s.d_sizes, h->stage_lines * sizeof(uint16_t)));
    HIPCHK(h, hipMalloc((void **)&s.d_sel, h->stage_lines));
    HIPCHK(h, hipHostMalloc((void **)&s.h_sizes, h->stage_lines * sizeof(uint16_t), hipHostMallocDefault));
    HIPCHK(h, hipHostMalloc((void **)&s.h_sel, h->stage_lines, hipHostMallocDefault));
  }
  h->slots_ready = true;
  return MPC_OK;
}

int ensure_mini(mpc_handle *h)
{
  if (h->mini) return MPC_OK;
  const size_t bytes = kMiniLines * ((size_t)h->L + sizeof(uint16_t) + 1);
  HIPCHK(h, hipHostMalloc((void **)&h->mini, bytes, hipHostMallocDefault));
  return MPC_OK;
}

// n <= kMiniLines lines, evaluated in place from pinned host memory on the handle's own stream
int compress_small(mpc_handle *h, const uint8_t *lines, uint64_t n, uint16_t *sizes, int8_t *sel)
{
  int rc = ensure_mini(h);
  if (rc != MPC_OK) return rc;
  uint8_t *in = h->mini;
  uint16_t *out_sizes = reinterpret_cast<uint16_t *>(h->mini + kMiniLines * (size_t)h->L);
  int8_t *out_sel = reinterpret_cast<int8_t *>(out_sizes + kMiniLines);
  std::memcpy(in, lines, (size_t)(n * (uint64_t)h->L));
  rc = launch(h, in, n, sizes ? out_sizes : nullptr, sel ? out_sel : nullptr, h->stream);
  if (rc != MPC_OK) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));   // (polling hipStreamQuery instead was slower: 46 k vs 58 k lines/s)
  if (sizes) std::memcpy(sizes, out_sizes, (size_t)n * sizeof(uint16_t));
  if (sel) std::memcpy(sel, out_sel, (size_t)n);
  return pattern_status(h);
}

// wait for a slot's in-flight chunk and hand its per-line results to the caller
int retire(mpc_handle *h, Slot &s)
{
  if (!s.busy) return MPC_OK;
  HIPCHK(h, hipEventSynchronize(s.done));
  if (s.user_sizes) std::memcpy(s.user_sizes, s.h_sizes, s.pending_lines * sizeof(uint16_t));
  if (s.user_sel) std::memcpy(s.user_sel, s.h_sel, s.pending_lines);
  s.busy = false;
  return MPC_OK;
}

// submit the chunk already sitting in s.h_in
int submit(mpc_handle *h, Slot &s, u64 lines, uint16_t *user_sizes, int8_t *user_sel)
{
  HIPCHK(h, hipMemcpyAsync(s.d_in, s.h_in, lines * (u64)h->L, hipMemcpyHostToDevice, s.stream));
  int rc = launch(h, s.d_in, lines, user_sizes ? s.d_sizes : nullptr, user_sel ? s.d_sel : nullptr, s.stream);
  if (rc != MPC_OK) return rc;
  if (user_sizes) HIPCHK(h, hipMemcpyAsync(s.h_sizes, s.d_sizes, lines * sizeof(uint16_t), hipMemcpyDeviceToHost, s.stream));
  if (user_sel) HIPCHK(h, hipMemcpyAsync(s.h_sel, s.d_sel, lines, hipMemcpyDeviceToHost, s.stream));
  HIPCHK(h, hipEventRecord(s.done, s.stream));
  s.user_sizes = user_sizes;
  s.user_sel = user_sel;
  s.pending_lines = lines;
  s.busy = true;
  return MPC_OK;
}

// After an error: nothing of the failed call may be delivered later.  Wait for both slots' streams
// and forget their pending results (the caller's output pointers may be gone by the next call).
void abandon_slots(mpc_handle *h)
{
  for (int i = 0; i < 2; i++) {
    Slot &s = h->slots[i];
    if (s.stream) (void)hipStreamSynchronize(s.stream);
    s.busy = false;
    s.user_sizes = nullptr;
    s.user_sel = nullptr;
    s.pending_lines = 0;
  }
}

int sync_all(mpc_handle *h)
{
  for (int i = 0; i < 2; i++) {
    int rc = retire(h, h->slots[i]);
    if (rc != MPC_OK) return rc;
  }
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return pattern_status(h);
}

// raw device statistics -> ABI vector (added into `vec`)
void derive_stats(const mpc_handle *h, const std::vector<u64> &raw, std::vector<u64> &vec)
{
  if (h->algorithm == 5) {
    const u64 L = (u64)h->L;
    vec[0] += raw[MPC_PAT_LINES];
    vec[3] += raw[MPC_PAT_SIZES];
    vec[4] += L * raw[MPC_PAT_ZERO];
    vec[5] += L * raw[MPC_PAT_SAME];
    vec[6] += L * raw[MPC_PAT_EXISTED];
    vec[7] += L * raw[MPC_PAT_UNDEF];
    vec[8] += L * raw[MPC_PAT_LINES];
    for (int k = 0; k < 6; k++) {
      vec[9 + k] += raw[MPC_PAT_IMPLICIT + k];
      vec[15 + k] += raw[MPC_PAT_EXPLICIT + k];
    }
    vec[21] += raw[MPC_PAT_JOINED];
    // SymbolCounts = the ordinary lines' bytes + L/4 of each byte of a word-same line's word + L zero bytes per zero line
    for (int b = 0; b < 256; b++) {
      vec[22 + b] += raw[MPC_PAT_HIST + b] + (L / 4) * raw[MPC_PAT_SAME_HIST + b];
      vec[278 + b] += raw[MPC_PAT_HIST + b];
    }
    vec[22] += L * raw[MPC_PAT_ZERO];
    return;
  }
  if (h->algorithm == 4) {
    // lines and warm-up lines are counted by the host (it splits every call at line S); bits and hits on the device
    vec[0] += h->sc2.lines;
    vec[1] += h->sc2.lines * 8ull * (u64)h->L;
    vec[2] += raw[0];
    vec[3] += h->sc2.warm;
    vec[4] += h->sc2.symbols.size();
    vec[5] += raw[1];
    return;
  }
  if (h->algorithm == 3) {
    // lines are not recoverable from the pattern counts: the kernel counts compressed bits per line,
    // and every line contributes exactly 33 planes = TotalWords / 33
    const u64 lines = raw[7] / 33ull;
    vec[0] += lines;
    vec[1] += lines * 8ull * (u64)h->L;
    vec[2] += raw[8];
    vec[3] += raw[7];
    for (int i = 0; i < 7; i++) vec[4 + i] += raw[i];
    return;
  }
  if (h->algorithm == 2) {
    u64 words = 0;
    for (int i = 0; i < 8; i++) {
      vec[3 + i] += raw[i];
      words += raw[i];
    }
    vec[0] += words / (u64)(h->L / 4);
    vec[1] += words * 32ull;
    vec[2] += raw[8];
    return;
  }
  if (h->algorithm == 1) {
    u64 lines = 0;
    for (int i = 0; i < 9; i++) {
      vec[3 + i] += raw[i];
      lines += raw[i];
    }
    vec[0] += lines;
    vec[1] += lines * 8ull * (u64)h->L;
    vec[2] += raw[9];
    return;
  }
  const int K = h->cfg.M + 1, B = h->cfg.hist_bins;
  const u64 uncomp = 8ull * (u64)h->L;
  for (int k = 0; k < K; k++) {
    u64 count = 0, comp = 0;
    for (int s = 0; s < B; s++) {
      const u64 c = raw[2 * K + (u64)k * B + s];
      count += c;
      comp += c * (u64)s;
      vec[3 + 6 * K + (u64)k * B + s] += c;
    }
    vec[3 + 6 * k + 0] += count;
    vec[3 + 6 * k + 1] += count * uncomp;
    vec[3 + 6 * k + 2] += comp;
    // residue statistics are kept for lines that reached checkOtherPatterns (VPC.cpp:412):
    // every cluster except AllZero (0) and AllWordSame (1)
    const int cluster = k - 1;
    const bool early = (cluster == 0) || (cluster == 1 && h->cfg.has_aws);
    vec[3 + 6 * k + 3] += early ? 0 : count;
    vec[3 + 6 * k + 4] += raw[k];
    vec[3 + 6 * k + 5] += raw[K + k];
    vec[0] += count;
    vec[1] += count * uncomp;
    vec[2] += comp;
  }
}

// ---- .npy header (format spec: magic, version, header length, python dict) ----
int parse_npy_header(FILE *f, u64 *rows, u64 *cols, u64 *data_off, std::string &err)
{
  unsigned char pre[12];
  if (fread(pre, 1, 10, f) != 10 || std::memcmp(pre, "\x93NUMPY", 6) != 0) { err = "not a .npy file"; return MPC_E_PARSE; }
  size_t hlen, off;
  if (pre[6] == 1) {
    hlen = (size_t)pre[8] | ((size_t)pre[9] << 8);
    off = 10;
  } else {
    if (fread(pre + 10, 1, 2, f) != 2) { err = "truncated .npy header"; return MPC_E_PARSE; }
    hlen = (size_t)pre[8] | ((size_t)pre[9] << 8) | ((size_t)pre[10] << 16) | ((size_t)pre[11] << 24);
    off = 12;
  }
  if (hlen > (1u << 20)) { err = "unreasonable .npy header length"; return MPC_E_PARSE; }
  std::string hdr(hlen, '\0');
  if (fread(&hdr[0], 1, hlen, f) != hlen) { err = "truncated .npy header"; return MPC_E_PARSE; }
  auto find_val = [&](const char *key) -> size_t {
    size_t p = hdr.find(key);
    if (p == std::string::npos) return p;
    p = hdr.find(':', p);
    return p == std::string::npos ? p : p + 1;
  };
  size_t p = find_val("'descr'");
  if (p == std::string::npos) { err = ".npy header has no descr"; return MPC_E_PARSE; }
  size_t q1 = hdr.find('\'', p), q2 = q1 == std::string::npos ? q1 : hdr.find('\'', q1 + 1);
  if (q2 == std::string::npos) { err = ".npy descr malformed"; return MPC_E_PARSE; }
  std::string descr = hdr.substr(q1 + 1, q2 - q1 - 1);
  if (!(descr == "|u1" || descr == "<u1" || descr == "u1" || descr == "=u1")) { err = ".npy dtype is " + descr + ", expected uint8"; return MPC_E_INVAL; }
  p = find_val("'fortran_order'");
  {
    const size_t v = p == std::string::npos ? p : hdr.find_first_not_of(' ', p);
    if (v == std::string::npos) { err = ".npy header has no fortran_order value"; return MPC_E_PARSE; }
    if (hdr.compare(v, 5, "False") != 0) { err = ".npy array must be C-order"; return MPC_E_INVAL; }
  }
  p = find_val("'shape'");
  size_t a = p == std::string::npos ? p : hdr.find('(', p), b = a == std::string::npos ? a : hdr.find(')', a);
  if (b == std::string::npos) { err = ".npy shape malformed"; return MPC_E_PARSE; }
  std::vector<u64> dims;
  const char *c = hdr.c_str() + a + 1, *e = hdr.c_str() + b;
  while (c < e) {
    while (c < e && (*c < '0' || *c > '9')) c++;
    if (c >= e) break;
    u64 v = 0;
    while (c < e && *c >= '0' && *c <= '9') v = v * 10 + (u64)(*c++ - '0');
    dims.push_back(v);
  }
  if (dims.size() != 2) { err = ".npy array must be 2-D [lines, line_size]"; return MPC_E_INVAL; }
  *rows = dims[0];
  *cols = dims[1];
  *data_off = off + hlen;
  return MPC_OK;
}

// ---- streaming a trace file through the staging slots.  The file walkers below are written once, against a
// "feed": who owns the two slots and what a submitted chunk is launched on -- one handle, or a group of them.
struct HandleFeed {
  mpc_handle *h;
  int L() const { return h->L; }
  int device() const { return h->device; }
  int fail(int code, const std::string &msg) const { return set_err(h, code, msg); }
  int ensure() const { return ensure_slots(h); }
  u64 stage_lines() const { return (u64)h->stage_lines; }
  uint8_t *buffer(int which) const { return h->slots[which].h_in; }
  int retire(int which) const { return ::retire(h, h->slots[which]); }
  int submit(int which, u64 lines) const { return ::submit(h, h->slots[which], lines, nullptr, nullptr); }
  int finish() const { return sync_all(h); }
  void abandon() const { abandon_slots(h); }
};

template <class Feed>
int feed_npy(Feed fd_, const char *path, uint64_t first_row, uint64_t n_rows, int skip_last_row, uint64_t *rows_done)
{
  if (rows_done) *rows_done = 0;
  FILE *f = fopen(path, "rb");
  if (!f) return fd_.fail(MPC_E_NOENT, std::string("cannot open ") + path);
  u64 rows, cols, off;
  std::string err;
  int rc = parse_npy_header(f, &rows, &cols, &off, err);
  if (rc != MPC_OK) { fclose(f); return fd_.fail(rc, err); }
  if (cols != (u64)fd_.L()) {
    fclose(f);
    return fd_.fail(MPC_E_INVAL, "trace line size " + std::to_string(cols) + " differs from the evaluator's " + std::to_string(fd_.L()));
  }
  // the reference driver drops the final row (LoaderNPY.cpp:28-32 + main.cpp:240)
  u64 usable = (skip_last_row && rows > 0) ? rows - 1 : rows;
  u64 begin = first_row < usable ? first_row : usable;
  u64 end = (n_rows > usable - begin) ? usable : begin + n_rows;
  if (hipSetDevice(fd_.device()) != hipSuccess) { fclose(f); return fd_.fail(MPC_E_HIP, "hipSetDevice failed"); }
  rc = fd_.ensure();
  if (rc != MPC_OK) { fclose(f); return rc; }
  const int fd = fileno(f);
  u64 done = begin;
  int which = 0;
  while (done < end) {
    rc = fd_.retire(which);
    if (rc != MPC_OK) break;
    const u64 take = (end - done) < fd_.stage_lines() ? (end - done) : fd_.stage_lines();
    if (!parallel_pread(fd, fd_.buffer(which), (size_t)(take * cols), off + done * cols)) { rc = fd_.fail(MPC_E_PARSE, "short read: .npy file is truncated"); break; }
    rc = fd_.submit(which, take);
    if (rc != MPC_OK) break;
    done += take;
    which ^= 1;
  }
  fclose(f);
  if (rc == MPC_OK) rc = fd_.finish();
  if (rc != MPC_OK) fd_.abandon();
  if (rc == MPC_OK && rows_done) *rows_done = end - begin;
  return rc;
}

constexpr int kLogKeys = 17, kLogRecordHeader = 62;

template <class Feed>
int feed_gpgpusim_log(Feed fd_, const char *log_path, uint64_t *requests_read, uint64_t *lines_done)
{
  if (requests_read) *requests_read = 0;
  if (lines_done) *lines_done = 0;
  // the file is mapped and walked in memory (per-request stdio calls cap the rate at ~35 M requests/s)
  const int fd = open(log_path, O_RDONLY);
  if (fd < 0) return fd_.fail(MPC_E_NOENT, std::string("Failed to open a file. Check the path of the file: ") + log_path);
  struct stat st;
  if (fstat(fd, &st) != 0) { close(fd); return fd_.fail(MPC_E_NOENT, std::string("cannot stat ") + log_path); }
  const u64 size = (u64)st.st_size;
  constexpr u64 kFileHeader = 1 + 7 * kLogKeys;
  const unsigned char *base = nullptr;
  if (size > 0) {
    void *m = mmap(nullptr, (size_t)size, PROT_READ, MAP_PRIVATE, fd, 0);
    if (m == MAP_FAILED) { close(fd); return fd_.fail(MPC_E_NOMEM, std::string("cannot map ") + log_path); }
    base = static_cast<const unsigned char *>(m);
    (void)madvise(m, (size_t)size, MADV_SEQUENTIAL);
  }
  close(fd);
  auto unmap = [&]() { if (base) munmap(const_cast<unsigned char *>(base), (size_t)size); };
  if (size < kFileHeader || base[0] != kLogKeys) {
    unmap();
    return fd_.fail(MPC_E_PARSE, "The header of the GPGPU-sim trace file is not valid.");
  }
  if (hipSetDevice(fd_.device()) != hipSuccess) { unmap(); return fd_.fail(MPC_E_HIP, "hipSetDevice failed"); }
  int rc = fd_.ensure();
  if (rc != MPC_OK) { unmap(); return rc; }
  const u64 L = (u64)fd_.L();
  u64 requests = 0, lines = 0, fill = 0, pos = kFileHeader;
  bool first = true;
  int which = 0;
  rc = fd_.retire(which);
  while (rc == MPC_OK && pos + kLogRecordHeader <= size) {
    uint32_t req_type, req_size;
    std::memcpy(&req_type, base + pos + 38, 4);
    std::memcpy(&req_size, base + pos + 58, 4);
    if (first && req_size != L) {
      rc = fd_.fail(MPC_E_INVAL, "trace line size " + std::to_string(req_size) + " differs from the evaluator's " + std::to_string(L));
      break;
    }
    first = false;
    const u64 next = pos + kLogRecordHeader + (u64)req_size;
    if (next > size) break;                                      // incomplete trailing request
    if (req_type == 0u || req_type == 4u) {                      // GLOBAL_ACC_R, GLOBAL_ACC_W
      if (req_size != L) {
        rc = fd_.fail(MPC_E_INVAL, "the GPGPU-sim trace mixes request sizes (" + std::to_string(req_size) + " after " + std::to_string(L) + " bytes)");
        break;
      }
      std::memcpy(fd_.buffer(which) + fill * L, base + pos + kLogRecordHeader, (size_t)L);
      fill++;
    }
    pos = next;
    requests++;
    if (fill == fd_.stage_lines()) {
      rc = fd_.submit(which, fill);
      if (rc != MPC_OK) break;
      lines += fill;
      fill = 0;
      which ^= 1;
      rc = fd_.retire(which);
    }
  }
  if (rc == MPC_OK && fill) {
    rc = fd_.submit(which, fill);
    if (rc == MPC_OK) lines += fill;
  }
  if (rc == MPC_OK) rc = fd_.finish();
  if (rc != MPC_OK) fd_.abandon();
  unmap();
  if (rc == MPC_OK) {
    if (requests_read) *requests_read = requests;
    if (lines_done) *lines_done = lines;
  }
  return rc;
}

// ---------------------------------------------------------------------------
// groups: several handles of one line size on one device, fed together
// ---------------------------------------------------------------------------
int group_err(mpc_group *g, int code, const std::string &msg)
{
  if (g) g->error = msg; else g_create_error = msg;
  return code;
}

#define GHIPCHK(g, call)                                                                        \
  do {                                                                                          \
    hipError_t e_ = (call);                                                                     \
    if (e_ != hipSuccess)                                                                       \
      return group_err((g), MPC_E_HIP, std::string(#call) + ": " + hipGetErrorString(e_));      \
  } while (0)

const char *algorithm_name(int algorithm)
{
  static const char *const name[] = {"VPC", "BDI", "FPC", "BPC", "SC2", "PATTERN"};
  return name[algorithm];
}

// Which members share baselines_kernel: the first BDI, FPC and BPC handle of the group when the line size has an
// instantiation and at least two of the three are there; every other member launches its own kernel.
void group_route(mpc_group *g)
{
  int found[3] = {-1, -1, -1}, n = 0;
  for (size_t i = 0; i < g->m.size(); i++) {
    const int a = g->m[i]->algorithm;
    if (a >= 1 && a <= 3 && found[a - 1] < 0) {
      found[a - 1] = (int)i;
      n++;
    }
  }
  if (n >= 2 && (g->L == 32 || g->L == 64 || g->L == 128)) {
    for (int k = 0; k < 3; k++) {
      g->shared[k] = found[k];
      if (found[k] >= 0 && (g->first_shared < 0 || found[k] < g->first_shared)) g->first_shared = found[k];
    }
  }
  auto is_shared = [&](int i) { return i == g->shared[0] || i == g->shared[1] || i == g->shared[2]; };
  std::string form;
  for (int i = 0; i < (int)g->m.size(); i++) {
    const mpc_handle *h = g->m[(size_t)i];
    std::string part;
    if (is_shared(i)) {
      if (i != g->first_shared) continue;
      for (int j = i; j < (int)g->m.size(); j++)
        if (is_shared(j)) part += (part.empty() ? "" : "+") + std::string(algorithm_name(g->m[(size_t)j]->algorithm));
      part += ": one kernel";
    } else {
      part = std::string(algorithm_name(h->algorithm)) + ": " + (h->algorithm == 0 ? mpc_kernel_form(h) : h->algorithm == 5 ? "own kernels" : "own kernel");
    }
    form += (form.empty() ? "" : "; ") + part;
  }
  g->form = form;
}

// every member over the same device-resident lines, in member order on one stream; d_sizes / d_sel: arrays of one
// pointer per member (the array or any entry may be null)
int group_launch(mpc_group *g, const void *d_lines, u64 n, uint16_t *const *d_sizes, int8_t *const *d_sel, hipStream_t s)
{
  if (n == 0) return MPC_OK;
  for (int i = 0; i < (int)g->m.size(); i++) {
    mpc_handle *h = g->m[(size_t)i];
    const bool in_shared = i == g->shared[0] || i == g->shared[1] || i == g->shared[2];
    if (in_shared) {
      if (i != g->first_shared) continue;
      MpcBaselinesArgs A{};
      MpcBaselineOut *out[3] = {&A.bdi, &A.fpc, &A.bpc};
      for (int k = 0; k < 3; k++) {
        const int j = g->shared[k];
        if (j < 0) continue;
        out[k]->sizes = d_sizes ? d_sizes[j] : nullptr;
        out[k]->sel = d_sel ? d_sel[j] : nullptr;
        out[k]->raw = g->m[(size_t)j]->d_raw;
      }
      const hipError_t e = mpc_launch_baselines(d_lines, n, g->L, &A, grid_for(h, n, 256, kWgPerCu), s);
      if (e != hipSuccess) return group_err(g, MPC_E_HIP, std::string("kernel launch: ") + hipGetErrorString(e));
      continue;
    }
    const int rc = launch(h, d_lines, n, d_sizes ? d_sizes[i] : nullptr, d_sel ? d_sel[i] : nullptr, s);
    if (rc != MPC_OK) return group_err(g, rc, "member " + std::to_string(i) + " (" + algorithm_name(h->algorithm) + "): " + h->error);
  }
  return MPC_OK;
}

int group_ensure_slots(mpc_group *g)
{
  if (g->slots_ready) return MPC_OK;
  g->stage_lines = kStageBytes / (size_t)g->L;
  for (int i = 0; i < 2; i++) {
    GroupSlot &s = g->slots[i];
    if (!s.h_in) GHIPCHK(g, hipHostMalloc((void **)&s.h_in, kStageBytes, hipHostMallocDefault));
    if (!s.d_in) GHIPCHK(g, hipMalloc((void **)&s.d_in, kStageBytes));
  }
  g->slots_ready = true;
  return MPC_OK;
}

// the per-line output buffers of member i in a slot, when a call asks for them for the first time
int group_ensure_outputs(mpc_group *g, GroupSlot &s, size_t i, bool sizes, bool sel)
{
  if (sizes && !s.d_sizes[i]) {
    GHIPCHK(g, hipMalloc((void **)&s.d_sizes[i], g->stage_lines * sizeof(uint16_t)));
    GHIPCHK(g, hipHostMalloc((void **)&s.h_sizes[i], g->stage_lines * sizeof(uint16_t), hipHostMallocDefault));
  }
  if (sel && !s.d_sel[i]) {
    GHIPCHK(g, hipMalloc((void **)&s.d_sel[i], g->stage_lines));
    GHIPCHK(g, hipHostMalloc((void **)&s.h_sel[i], g->stage_lines, hipHostMallocDefault));
  }
  return MPC_OK;
}

int group_retire(mpc_group *g, GroupSlot &s)
{
  if (!s.busy) return MPC_OK;
  GHIPCHK(g, hipEventSynchronize(s.done));
  for (size_t i = 0; i < g->m.size(); i++) {
    if (s.user_sizes[i]) std::memcpy(s.user_sizes[i], s.h_sizes[i], s.pending_lines * sizeof(uint16_t));
    if (s.user_sel[i]) std::memcpy(s.user_sel[i], s.h_sel[i], s.pending_lines);
  }
  s.busy = false;
  return MPC_OK;
}

// submit the chunk already sitting in s.h_in: one copy, then every member's launch on the slot's stream.
// sizes / sel: the callers' arrays of per-member pointers (or null), `first` the chunk's first line in them.
int group_submit(mpc_group *g, GroupSlot &s, u64 lines, uint16_t *const *sizes, int8_t *const *sel, u64 first)
{
  const size_t n = g->m.size();
  std::vector<uint16_t *> ds(n, nullptr);
  std::vector<int8_t *> dl(n, nullptr);
  for (size_t i = 0; i < n; i++) {
    s.user_sizes[i] = (sizes && sizes[i]) ? sizes[i] + first : nullptr;
    s.user_sel[i] = (sel && sel[i]) ? sel[i] + first : nullptr;
    const int rc = group_ensure_outputs(g, s, i, s.user_sizes[i] != nullptr, s.user_sel[i] != nullptr);
    if (rc != MPC_OK) return rc;
    if (s.user_sizes[i]) ds[i] = s.d_sizes[i];
    if (s.user_sel[i]) dl[i] = s.d_sel[i];
  }
  GHIPCHK(g, hipMemcpyAsync(s.d_in, s.h_in, lines * (u64)g->L, hipMemcpyHostToDevice, s.stream));
  const int rc = group_launch(g, s.d_in, lines, ds.data(), dl.data(), s.stream);
  if (rc != MPC_OK) return rc;
  for (size_t i = 0; i < n; i++) {
    if (ds[i]) GHIPCHK(g, hipMemcpyAsync(s.h_sizes[i], ds[i], lines * sizeof(uint16_t), hipMemcpyDeviceToHost, s.stream));
    if (dl[i]) GHIPCHK(g, hipMemcpyAsync(s.h_sel[i], dl[i], lines, hipMemcpyDeviceToHost, s.stream));
  }
  GHIPCHK(g, hipEventRecord(s.done, s.stream));
  s.pending_lines = lines;
  s.busy = true;
  return MPC_OK;
}

// after an error: nothing of the failed call may be delivered later (abandon_slots)
void group_abandon(mpc_group *g)
{
  for (int i = 0; i < 2; i++) {
    GroupSlot &s = g->slots[i];
    if (s.stream) (void)hipStreamSynchronize(s.stream);
    s.busy = false;
    s.pending_lines = 0;
    std::fill(s.user_sizes.begin(), s.user_sizes.end(), nullptr);
    std::fill(s.user_sel.begin(), s.user_sel.end(), nullptr);
  }
}

int group_members_status(mpc_group *g);

int group_finish(mpc_group *g)
{
  for (int i = 0; i < 2; i++) {
    const int rc = group_retire(g, g->slots[i]);
    if (rc != MPC_OK) return rc;
  }
  for (int i = 0; i < 2; i++) GHIPCHK(g, hipStreamSynchronize(g->slots[i].stream));
  return group_members_status(g);
}

// a Pattern member that ran into its capacity fails the group call (checked wherever the group has synchronised)
int group_members_status(mpc_group *g)
{
  for (size_t i = 0; i < g->m.size(); i++) {
    const int rc = pattern_status(g->m[i]);
    if (rc != MPC_OK) return group_err(g, rc, "member " + std::to_string(i) + " (" + algorithm_name(g->m[i]->algorithm) + "): " + g->m[i]->error);
  }
  return MPC_OK;
}

// n <= kMiniLines lines, evaluated in place from pinned host memory: one launch per member or per shared launch on the
// first slot's stream (idle: every group call ends synchronised), one synchronisation
int group_small(mpc_group *g, const uint8_t *lines, u64 n, uint16_t *const *sizes, int8_t *const *sel)
{
  const size_t nm = g->m.size();
  if (!g->mini) GHIPCHK(g, hipHostMalloc((void **)&g->mini, kMiniLines * ((size_t)g->L + nm * (sizeof(uint16_t) + 1)), hipHostMallocDefault));
  uint16_t *out_sizes = reinterpret_cast<uint16_t *>(g->mini + kMiniLines * (size_t)g->L);
  int8_t *out_sel = reinterpret_cast<int8_t *>(out_sizes + nm * kMiniLines);
  std::vector<uint16_t *> ds(nm, nullptr);
  std::vector<int8_t *> dl(nm, nullptr);
  for (size_t i = 0; i < nm; i++) {
    if (sizes && sizes[i]) ds[i] = out_sizes + i * kMiniLines;
    if (sel && sel[i]) dl[i] = out_sel + i * kMiniLines;
  }
  std::memcpy(g->mini, lines, (size_t)(n * (u64)g->L));
  hipStream_t s = g->slots[0].stream;
  const int rc = group_launch(g, g->mini, n, ds.data(), dl.data(), s);
  if (rc != MPC_OK) { (void)hipStreamSynchronize(s); return rc; }
  GHIPCHK(g, hipStreamSynchronize(s));
  for (size_t i = 0; i < nm; i++) {
    if (ds[i]) std::memcpy(sizes[i], ds[i], (size_t)n * sizeof(uint16_t));
    if (dl[i]) std::memcpy(sel[i], dl[i], (size_t)n);
  }
  return group_members_status(g);
}

struct GroupFeed {
  mpc_group *g;
  int L() const { return g->L; }
  int device() const { return g->device; }
  int fail(int code, const std::string &msg) const { return group_err(g, code, msg); }
  int ensure() const { return group_ensure_slots(g); }
  u64 stage_lines() const { return (u64)g->stage_lines; }
  uint8_t *buffer(int which) const { return g->slots[which].h_in; }
  int retire(int which) const { return group_retire(g, g->slots[which]); }
  int submit(int which, u64 lines) const { return group_submit(g, g->slots[which], lines, nullptr, nullptr, 0); }
  int finish() const { return group_finish(g); }
  void abandon() const { group_abandon(g); }
};

uint32_t *g_sine_dev[16] = {nullptr};   // per device float32 sine period for mpc_synth_fill

}  // namespace

// ===========================================================================
// C ABI
// ===========================================================================
extern "C" {

int mpc_create_vpc_from_string(const char *text, int device, mpc_handle **out)
{
  if (!text) return MPC_E_INVAL;
  return create_vpc_from_text(text, device, out);
}

int mpc_create_vpc(const char *path, int device, mpc_handle **out)
{
  if (!path || !out) return MPC_E_INVAL;
  std::string text;
  if (!mpc::read_file(path, text)) {
    g_create_error = std::string("Invalid File! \"") + path + "\" is not valid path.";
    return MPC_E_NOENT;
  }
  return create_vpc_from_text(text, device, out);
}

int mpc_create_bdi(unsigned line_size, int device, mpc_handle **out)
{
  if (!out) return MPC_E_INVAL;
  *out = nullptr;
  // BDI.cpp:8 takes any dataLine.size(); values are 8, 4 and 2 bytes wide, so a multiple of 8
  if (line_size < 8 || line_size > MPC_MAX_LINE || (line_size % 8)) {
    g_create_error = "BDI line size must be a multiple of 8 in 8.." + std::to_string(MPC_MAX_LINE) + " bytes";
    return MPC_E_INVAL;
  }
  mpc_handle *h = new (std::nothrow) mpc_handle();
  if (!h) return MPC_E_NOMEM;
  h->algorithm = 1;
  h->L = (int)line_size;
  h->raw_len = MPC_BDI_RAW_LEN;
  h->stats_len = 12;
  int rc = pick_device(device, &h->device, &h->num_cus);
  if (rc == MPC_OK) rc = finish_create(h);
  if (rc != MPC_OK) {
    mpc_destroy(h);
    return rc;
  }
  *out = h;
  return MPC_OK;
}

int mpc_create_bpc(unsigned line_size, int device, mpc_handle **out)
{
  if (!out) return MPC_E_INVAL;
  *out = nullptr;
  // 32-bit words; a plane has one bit per delta and is held in an int32_t (BPC.cpp:53-63): 2..32 words
  if (line_size < 8 || line_size > 128 || (line_size % 4)) {
    g_create_error = "BPC line size must be a multiple of 4 in 8..128 bytes";
    return MPC_E_INVAL;
  }
  mpc_handle *h = new (std::nothrow) mpc_handle();
  if (!h) return MPC_E_NOMEM;
  h->algorithm = 3;
  h->L = (int)line_size;
  h->raw_len = MPC_BPC_RAW_LEN;
  h->stats_len = 11;
  int rc = pick_device(device, &h->device, &h->num_cus);
  if (rc == MPC_OK) rc = finish_create(h);
  if (rc != MPC_OK) {
    mpc_destroy(h);
    return rc;
  }
  *out = h;
  return MPC_OK;
}

int mpc_create_fpc(unsigned line_size, int device, mpc_handle **out)
{
  if (!out) return MPC_E_INVAL;
  *out = nullptr;
  if (line_size < 4 || line_size > MPC_MAX_LINE || (line_size % 4)) {
    g_create_error = "FPC line size must be a multiple of 4 in 4.." + std::to_string(MPC_MAX_LINE) + " bytes";
    return MPC_E_INVAL;
  }
  mpc_handle *h = new (std::nothrow) mpc_handle();
  if (!h) return MPC_E_NOMEM;
  h->algorithm = 2;
  h->L = (int)line_size;
  h->raw_len = MPC_FPC_RAW_LEN;
  h->stats_len = 11;
  int rc = pick_device(device, &h->device, &h->num_cus);
  if (rc == MPC_OK) rc = finish_create(h);
  if (rc != MPC_OK) {
    mpc_destroy(h);
    return rc;
  }
  *out = h;
  return MPC_OK;
}

int mpc_create_pattern(unsigned line_size, int device, mpc_handle **out)
{
  if (!out) return MPC_E_INVAL;
  *out = nullptr;
  // 8-, 4- and 2-byte values (Pattern.cpp:26-58): a multiple of 8, or checkPattern reads past the line
  if (line_size < 8 || line_size > MPC_MAX_LINE || (line_size % 8)) {
    g_create_error = "Pattern line size must be a multiple of 8 in 8.." + std::to_string(MPC_MAX_LINE) + " bytes";
    return MPC_E_INVAL;
  }
  mpc_handle *h = new (std::nothrow) mpc_handle();
  if (!h) return MPC_E_NOMEM;
  h->algorithm = 5;
  h->L = (int)line_size;
  h->raw_len = MPC_PATTERN_RAW_LEN;
  h->stats_len = 534;
  int rc = pick_device(device, &h->device, &h->num_cus);
  if (rc == MPC_OK) rc = finish_create(h);
  if (rc == MPC_OK) {
    MpcPatternSet &S = h->pat.set;
    const size_t slots = (size_t)1 << MPC_PATTERN_SLOT_BITS;
    S.tag_mask = ~0ull;
#if MPC_TESTING
    // test library only: a hash of a few bits, so that unequal lines meet on the tag and in the chains
    if (const char *e = getenv("MPC_TEST_PATTERN_TAG_BITS")) {
      const long bits = atol(e);
      if (bits >= 1 && bits < 64) S.tag_mask = (1ull << bits) - 1ull;
    }
#endif
    if (hipMalloc((void **)&S.tags, slots * sizeof(u64)) != hipSuccess || hipMalloc((void **)&S.store, slots * (size_t)line_size) != hipSuccess ||
        hipMalloc((void **)&S.ctl, MPC_PSET_WORDS * sizeof(u64)) != hipSuccess ||
        hipMalloc((void **)&S.pend_a, (size_t)MPC_PATTERN_CHUNK * sizeof(uint2)) != hipSuccess ||
        hipMalloc((void **)&S.pend_b, (size_t)MPC_PATTERN_CHUNK * sizeof(uint2)) != hipSuccess) {
      g_create_error = "hipMalloc of the Pattern line set (" + std::to_string(slots * (sizeof(u64) + line_size)) + " bytes) failed";
      rc = MPC_E_NOMEM;
    } else if (hipMemset(S.tags, 0, slots * sizeof(u64)) != hipSuccess || hipMemset(S.ctl, 0, MPC_PSET_WORDS * sizeof(u64)) != hipSuccess ||
               hipDeviceSynchronize() != hipSuccess ||          // (the kernels run on non-blocking streams)
               hipEventCreateWithFlags(&h->pat.done, hipEventDisableTiming) != hipSuccess) {
      g_create_error = "initialising the Pattern line set failed";
      rc = MPC_E_NODEVICE;
    }
  }
  if (rc != MPC_OK) {
    mpc_destroy(h);
    return rc;
  }
  *out = h;
  return MPC_OK;
}

int mpc_pattern_distinct_lines(mpc_handle *h, uint64_t *n)
{
  if (!h || !n || h->algorithm != 5) return MPC_E_INVAL;
  HIPCHK(h, hipSetDevice(h->device));
  int rc = sync_all(h);
  if (rc != MPC_OK) return rc;
  HIPCHK(h, hipDeviceSynchronize());   // callers may have used their own streams
  rc = pattern_status(h);
  if (rc != MPC_OK) return rc;
  u64 v = 0;
  HIPCHK(h, hipMemcpy(&v, h->pat.set.ctl + MPC_PSET_DISTINCT, sizeof(v), hipMemcpyDeviceToHost));
  *n = v;
  return MPC_OK;
}

uint64_t mpc_sc2_sampling_lines(uint64_t num_lines)
{
  // main.cpp:110-113: max(10000, min(numLines / 100, WARM_UP_CNT))
  return std::max<uint64_t>(10000, std::min<uint64_t>(num_lines / 100, 1000000));
}

int mpc_sc2_code_lengths(const uint32_t *symbols, const uint64_t *freqs, size_t n, uint16_t *len_out)
{
  if (n == 0 || !symbols || !freqs || !len_out) return MPC_E_INVAL;
  std::vector<uint32_t> sorted(symbols, symbols + n);
  std::sort(sorted.begin(), sorted.end());
  if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) return MPC_E_INVAL;   // a frequency map has distinct keys
  return mpcsc2::code_lengths(symbols, freqs, n, len_out) == 0 ? MPC_OK : MPC_E_INVAL;
}

int mpc_create_sc2(unsigned line_size, uint64_t sampling_lines, int device, mpc_handle **out)
{
  if (!out) return MPC_E_INVAL;
  *out = nullptr;
  if (line_size < 4 || line_size > MPC_MAX_LINE || (line_size % 4)) {
    g_create_error = "SC2 line size must be a multiple of 4 in 4.." + std::to_string(MPC_MAX_LINE) + " bytes";
    return MPC_E_INVAL;
  }
  if (sampling_lines == 0) {
    g_create_error = "SC2 needs at least one warm-up line (the reference builds its table from an empty map otherwise)";
    return MPC_E_INVAL;
  }
  const u64 words = sampling_lines * (u64)(line_size / 4);
  if (sampling_lines > (1ull << 28) || words > (1ull << 28)) {
    g_create_error = "SC2 warm-up sample of more than 2^28 words (its frequency table would exceed 4 GiB)";
    return MPC_E_INVAL;
  }
  mpc_handle *h = new (std::nothrow) mpc_handle();
  if (!h) return MPC_E_NOMEM;
  h->algorithm = 4;
  h->L = (int)line_size;
  h->raw_len = MPC_SC2_RAW_LEN;
  h->stats_len = 6;
  h->sc2.S = sampling_lines;
  u64 slots = 2;
  while (slots < 2 * words) slots <<= 1;
  h->sc2.hash_mask = slots - 1;
  int rc = pick_device(device, &h->device, &h->num_cus);
  if (rc == MPC_OK) rc = finish_create(h);
  if (rc == MPC_OK && (hipMalloc((void **)&h->sc2.d_hash, slots * sizeof(u64)) != hipSuccess ||
                       hipMalloc((void **)&h->sc2.d_buckets, MPC_SC2_MAX_BUCKETS * sizeof(uint4)) != hipSuccess ||
                       hipMemset(h->sc2.d_hash, 0, slots * sizeof(u64)) != hipSuccess ||
                       hipDeviceSynchronize() != hipSuccess)) {        // (the kernels run on non-blocking streams)
    g_create_error = "hipMalloc of the SC2 frequency table (" + std::to_string(slots * sizeof(u64)) + " bytes) failed";
    rc = MPC_E_NOMEM;
  }
  if (rc != MPC_OK) {
    mpc_destroy(h);
    return rc;
  }
  *out = h;
  return MPC_OK;
}

int mpc_sc2_table(mpc_handle *h, uint32_t *symbols, uint16_t *lengths, size_t cap, size_t *n)
{
  if (!h || !n || h->algorithm != 4) return MPC_E_INVAL;
  const size_t m = h->sc2.symbols.size();
  *n = m;
  if (m == 0) return MPC_OK;
  if (cap < m || !symbols || !lengths) return MPC_E_INVAL;
  std::memcpy(symbols, h->sc2.symbols.data(), m * sizeof(uint32_t));
  std::memcpy(lengths, h->sc2.lengths.data(), m * sizeof(uint16_t));
  return MPC_OK;
}

void mpc_destroy(mpc_handle *h)
{
  if (!h) return;
  (void)hipSetDevice(h->device);
  for (int i = 0; i < 2; i++) {
    Slot &s = h->slots[i];
    if (s.stream) (void)hipStreamSynchronize(s.stream);
    if (s.h_in) (void)hipHostFree(s.h_in);
    if (s.d_in) (void)hipFree(s.d_in);
    if (s.d_sizes) (void)hipFree(s.d_sizes);
    if (s.d_sel) (void)hipFree(s.d_sel);
    if (s.h_sizes) (void)hipHostFree(s.h_sizes);
    if (s.h_sel) (void)hipHostFree(s.h_sel);
    if (s.done) (void)hipEventDestroy(s.done);
    if (s.stream) (void)hipStreamDestroy(s.stream);
  }
  if (h->stream) {
    (void)hipStreamSynchronize(h->stream);
    (void)hipStreamDestroy(h->stream);
  }
  if (h->mini) (void)hipHostFree(h->mini);
  if (h->d_tab) (void)hipFree(h->d_tab);
  if (h->d_gtab) (void)hipFree(h->d_gtab);
  if (h->d_raw) (void)hipFree(h->d_raw);
  if (h->sc2.d_hash) (void)hipFree(h->sc2.d_hash);
  if (h->sc2.d_buckets) (void)hipFree(h->sc2.d_buckets);
  if (h->pat.set.tags) (void)hipFree(h->pat.set.tags);
  if (h->pat.set.store) (void)hipFree(h->pat.set.store);
  if (h->pat.set.ctl) (void)hipFree(h->pat.set.ctl);
  if (h->pat.set.pend_a) (void)hipFree(h->pat.set.pend_a);
  if (h->pat.set.pend_b) (void)hipFree(h->pat.set.pend_b);
  if (h->pat.done) (void)hipEventDestroy(h->pat.done);
  delete h;
}

int mpc_get_info(const mpc_handle *h, mpc_info *info)
{
  if (!h || !info) return MPC_E_INVAL;
  info->abi_version = MPC_ABI_VERSION;
  info->algorithm = h->algorithm;
  info->line_size = h->L;
  info->num_modules = h->algorithm == 0 ? h->cfg.M : 0;
  info->num_clusters = h->algorithm == 0 ? h->cfg.M + 1 : (h->algorithm == 1 ? 9 : (h->algorithm == 2 ? 8 : h->algorithm == 3 ? 7 : h->algorithm == 5 ? 10 : 2));
  info->hist_bins = h->algorithm == 0 ? h->cfg.hist_bins : 0;
  info->kernel_path = h->algorithm == 5 ? MPC_PATH_PATTERN : h->algorithm == 4 ? MPC_PATH_SC2 : h->algorithm == 3 ? MPC_PATH_BPC : h->algorithm == 2 ? MPC_PATH_FPC
                      : h->algorithm == 1 ? MPC_PATH_BDI : (h->route.kernel != VpcKernel::Generic ? MPC_PATH_VPC_FAST : MPC_PATH_VPC_GENERIC);
  info->device = h->device;
  info->stats_len = h->stats_len;
  return MPC_OK;
}

const char *mpc_last_error(const mpc_handle *h) { return h ? h->error.c_str() : g_create_error.c_str(); }

// Needs no device: parses the configuration and, when its module sequence would be compiled at creation, runs that
// compilation for gfx950 (nothing is loaded).  Returns the size of the code object, 0 when the sequence is built in or
// takes the run-time loop, or a negative MPC_E_* with the compiler's log in `log`.
long long mpc_jit_compile_check(const char *json_text, char *log, size_t cap)
{
  if (log && cap) log[0] = 0;
  mpc::VpcConfig cfg;
  std::string err;
  int rc = mpc::parse_vpc_config(json_text ? json_text : "", cfg, err);
  if (rc == 0) {
    mpc::VpcPlan plan;
    mpc::build_vpc_plan(cfg, plan);
    if (route_vpc(plan, Jit::Predicted).kernel != VpcKernel::AtCreation) return 0;
    const size_t smem = mpc_vpc_lane_ring_plan(&plan.params, nullptr, nullptr);
    std::string code;
    if (mpcjit::compile(mpcjit::source_of(plan, smem, MPC_TESTING), "gfx950", mpcjit::source_dir(), code, err)) return (long long)code.size();
    rc = MPC_E_HIP;
  }
  if (log && cap) {
    std::strncpy(log, err.c_str(), cap - 1);
    log[cap - 1] = 0;
  }
  return rc;
}

const char *mpc_kernel_form(const mpc_handle *h)
{
  if (!h) return "";
  if (h->algorithm == 4) return h->sc2.built ? "table sizing" : "warm-up counting";
  if (h->algorithm == 5) return (h->L == 32 || h->L == 64 || h->L == 128) ? "unrolled, then the set passes" : "run-time loop, then the set passes";
  if (h->algorithm != 0) return "unrolled";
  if (h->route.kernel == VpcKernel::AtCreation && h->jit.from_cache) return "unrolled, compiled at creation (from the cache)";
  static const char *const form[] = {"unrolled", "unrolled, general layout", "unrolled, compiled at creation", "run-time loop", "generic"};
  return form[(int)h->route.kernel];      // (VpcKernel order)
}

const char *mpc_path_reason(const mpc_handle *h)
{
  return (h && h->algorithm == 0) ? h->route.why_generic.c_str() : "";
}

int mpc_compress_batch_device(mpc_handle *h, const void *d_lines, uint64_t n, uint16_t *d_sizes, int8_t *d_sel,
                              void *hip_stream)
{
  if (!h || (!d_lines && n)) return MPC_E_INVAL;
  if (((uintptr_t)d_lines) & 15u) return set_err(h, MPC_E_INVAL, "device line buffer must be 16-byte aligned");
  HIPCHK(h, hipSetDevice(h->device));
  return launch(h, d_lines, n, d_sizes, d_sel, (hipStream_t)hip_stream);
}

int mpc_sync(mpc_handle *h)
{
  if (!h) return MPC_E_INVAL;
  HIPCHK(h, hipSetDevice(h->device));
  int rc = sync_all(h);
  if (rc != MPC_OK) return rc;
  HIPCHK(h, hipDeviceSynchronize());   // batches may have been queued on caller streams
  return pattern_status(h);
}

int mpc_compress_batch(mpc_handle *h, const uint8_t *lines, uint64_t n, uint16_t *sizes, int8_t *sel)
{
  if (!h || (!lines && n)) return MPC_E_INVAL;
  if (n == 0) return MPC_OK;
  if (n <= kMiniLines) {
    HIPCHK(h, hipSetDevice(h->device));
    return compress_small(h, lines, n, sizes, sel);
  }
  HIPCHK(h, hipSetDevice(h->device));
  int rc = ensure_slots(h);
  if (rc != MPC_OK) return rc;
  u64 done = 0;
  int which = 0;
  while (done < n) {
    Slot &s = h->slots[which];
    rc = retire(h, s);   // the slot's previous chunk (overlapped with the other slot's work)
    if (rc != MPC_OK) break;
    const u64 take = (n - done) < (u64)h->stage_lines ? (n - done) : (u64)h->stage_lines;
    parallel_copy(s.h_in, lines + done * (u64)h->L, (size_t)(take * (u64)h->L));
    rc = submit(h, s, take, sizes ? sizes + done : nullptr, sel ? sel + done : nullptr);
    if (rc != MPC_OK) break;
    done += take;
    which ^= 1;
  }
  if (rc == MPC_OK) rc = sync_all(h);
  if (rc != MPC_OK) abandon_slots(h);
  return rc;
}

int mpc_npy_shape(const char *path, uint64_t *rows, uint64_t *cols)
{
  if (!path || !rows || !cols) return MPC_E_INVAL;
  FILE *f = fopen(path, "rb");
  if (!f) { g_create_error = std::string("cannot open ") + path; return MPC_E_NOENT; }
  u64 r, c, off;
  std::string err;
  int rc = parse_npy_header(f, &r, &c, &off, err);
  fclose(f);
  if (rc != MPC_OK) { g_create_error = err; return rc; }
  *rows = r;
  *cols = c;
  return MPC_OK;
}

int mpc_compress_npy(mpc_handle *h, const char *path, uint64_t first_row, uint64_t n_rows, int skip_last_row,
                     uint64_t *rows_done)
{
  if (!h || !path) return MPC_E_INVAL;
  return feed_npy(HandleFeed{h}, path, first_row, n_rows, skip_last_row, rows_done);
}

namespace {

// validates the file header of a GPGPU-Sim trace (LoaderGPGPU.cpp:93-119)
int log_open(const char *path, FILE **out, std::string &err)
{
  FILE *f = fopen(path, "rb");
  if (!f) { err = std::string("Failed to open a file. Check the path of the file: ") + path; return MPC_E_NOENT; }
  unsigned char hdr[1 + 7 * kLogKeys];
  if (fread(hdr, 1, sizeof(hdr), f) != sizeof(hdr) || hdr[0] != kLogKeys) {
    fclose(f);
    err = "The header of the GPGPU-sim trace file is not valid.";
    return MPC_E_PARSE;
  }
  *out = f;
  return MPC_OK;
}

// one request header; false at the end of the file (or inside an incomplete header)
bool log_next(FILE *f, uint32_t *req_type, uint32_t *req_size)
{
  unsigned char h[kLogRecordHeader];
  if (fread(h, 1, sizeof(h), f) != sizeof(h)) return false;
  std::memcpy(req_type, h + 38, 4);
  std::memcpy(req_size, h + 58, 4);
  return true;
}

}  // namespace

int mpc_gpgpusim_log_line_size(const char *log_path, uint32_t *line_size)
{
  if (!log_path || !line_size) return MPC_E_INVAL;
  *line_size = 0;
  FILE *f = nullptr;
  std::string err;
  int rc = log_open(log_path, &f, err);
  if (rc != MPC_OK) return set_err(nullptr, rc, err);
  uint32_t t = 0, sz = 0;
  if (log_next(f, &t, &sz)) *line_size = sz;
  fclose(f);
  return MPC_OK;
}

int mpc_compress_gpgpusim_log(mpc_handle *h, const char *log_path, uint64_t *requests_read, uint64_t *lines_done)
{
  if (!h || !log_path) return MPC_E_INVAL;
  return feed_gpgpusim_log(HandleFeed{h}, log_path, requests_read, lines_done);
}

// ---- groups ---------------------------------------------------------------
int mpc_group_create(mpc_handle *const *members, size_t n, mpc_group **out)
{
  if (!out) return MPC_E_INVAL;
  *out = nullptr;
  if (!members || n == 0) return group_err(nullptr, MPC_E_INVAL, "a group needs at least one member");
  for (size_t i = 0; i < n; i++) {
    if (!members[i]) return group_err(nullptr, MPC_E_INVAL, "member " + std::to_string(i) + " is NULL");
    for (size_t j = 0; j < i; j++)
      if (members[j] == members[i])
        return group_err(nullptr, MPC_E_INVAL, "member " + std::to_string(i) + " repeats member " + std::to_string(j) + " (a handle is fed once)");
    if (members[i]->L != members[0]->L)
      return group_err(nullptr, MPC_E_INVAL, "members of different line sizes: member " + std::to_string(i) + " has " + std::to_string(members[i]->L) +
                                                 "-byte lines, member 0 " + std::to_string(members[0]->L));
    if (members[i]->device != members[0]->device)
      return group_err(nullptr, MPC_E_INVAL, "members on different devices: member " + std::to_string(i) + " is bound to device " +
                                                 std::to_string(members[i]->device) + ", member 0 to " + std::to_string(members[0]->device));
  }
  mpc_group *g = new (std::nothrow) mpc_group();
  if (!g) return MPC_E_NOMEM;
  g->m.assign(members, members + n);
  g->L = members[0]->L;
  g->device = members[0]->device;
  group_route(g);
  bool ok = hipSetDevice(g->device) == hipSuccess;
  for (int i = 0; i < 2 && ok; i++) {
    GroupSlot &s = g->slots[i];
    ok = hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking) == hipSuccess &&
         hipEventCreateWithFlags(&s.done, hipEventDisableTiming) == hipSuccess;
    s.d_sizes.assign(n, nullptr); s.h_sizes.assign(n, nullptr); s.user_sizes.assign(n, nullptr);
    s.d_sel.assign(n, nullptr); s.h_sel.assign(n, nullptr); s.user_sel.assign(n, nullptr);
  }
  if (!ok) {
    mpc_group_destroy(g);
    return group_err(nullptr, MPC_E_HIP, "hipStreamCreate / hipEventCreate failed for the group's slots");
  }
  for (mpc_handle *h : g->m)
    for (int i = 0; i < 2; i++) h->group_streams.push_back(g->slots[i].stream);
  *out = g;
  return MPC_OK;
}

void mpc_group_destroy(mpc_group *g)
{
  if (!g) return;
  (void)hipSetDevice(g->device);
  for (int i = 0; i < 2; i++) {
    GroupSlot &s = g->slots[i];
    if (s.stream) (void)hipStreamSynchronize(s.stream);
    for (mpc_handle *h : g->m)
      h->group_streams.erase(std::remove(h->group_streams.begin(), h->group_streams.end(), s.stream), h->group_streams.end());
    if (s.h_in) (void)hipHostFree(s.h_in);
    if (s.d_in) (void)hipFree(s.d_in);
    for (uint16_t *p : s.d_sizes) if (p) (void)hipFree(p);
    for (uint16_t *p : s.h_sizes) if (p) (void)hipHostFree(p);
    for (int8_t *p : s.d_sel) if (p) (void)hipFree(p);
    for (int8_t *p : s.h_sel) if (p) (void)hipHostFree(p);
    if (s.done) (void)hipEventDestroy(s.done);
    if (s.stream) (void)hipStreamDestroy(s.stream);
  }
  if (g->mini) (void)hipHostFree(g->mini);
  delete g;
}

const char *mpc_group_last_error(const mpc_group *g) { return g ? g->error.c_str() : g_create_error.c_str(); }

const char *mpc_group_form(const mpc_group *g) { return g ? g->form.c_str() : ""; }

int mpc_group_compress_batch(mpc_group *g, const uint8_t *lines, uint64_t n, uint16_t *const *sizes, int8_t *const *sel)
{
  if (!g || (!lines && n)) return MPC_E_INVAL;
  if (n == 0) return MPC_OK;
  GHIPCHK(g, hipSetDevice(g->device));
  if (n <= kMiniLines) return group_small(g, lines, n, sizes, sel);
  int rc = group_ensure_slots(g);
  if (rc != MPC_OK) return rc;
  u64 done = 0;
  int which = 0;
  while (done < n) {
    GroupSlot &s = g->slots[which];
    rc = group_retire(g, s);   // the slot's previous chunk (overlapped with the other slot's work)
    if (rc != MPC_OK) break;
    const u64 take = (n - done) < (u64)g->stage_lines ? (n - done) : (u64)g->stage_lines;
    parallel_copy(s.h_in, lines + done * (u64)g->L, (size_t)(take * (u64)g->L));
    rc = group_submit(g, s, take, sizes, sel, done);
    if (rc != MPC_OK) break;
    done += take;
    which ^= 1;
  }
  if (rc == MPC_OK) rc = group_finish(g);
  if (rc != MPC_OK) group_abandon(g);
  return rc;
}

int mpc_group_compress_batch_device(mpc_group *g, const void *d_lines, uint64_t n, uint16_t *const *d_sizes, int8_t *const *d_sel,
                                    void *hip_stream)
{
  if (!g || (!d_lines && n)) return MPC_E_INVAL;
  if (((uintptr_t)d_lines) & 15u) return group_err(g, MPC_E_INVAL, "device line buffer must be 16-byte aligned");
  GHIPCHK(g, hipSetDevice(g->device));
  return group_launch(g, d_lines, n, d_sizes, d_sel, (hipStream_t)hip_stream);
}

int mpc_group_compress_npy(mpc_group *g, const char *path, uint64_t first_row, uint64_t n_rows, int skip_last_row, uint64_t *rows_done)
{
  if (!g || !path) return MPC_E_INVAL;
  return feed_npy(GroupFeed{g}, path, first_row, n_rows, skip_last_row, rows_done);
}

int mpc_group_compress_gpgpusim_log(mpc_group *g, const char *log_path, uint64_t *requests_read, uint64_t *lines_done)
{
  if (!g || !log_path) return MPC_E_INVAL;
  return feed_gpgpusim_log(GroupFeed{g}, log_path, requests_read, lines_done);
}

int mpc_group_sync(mpc_group *g)
{
  if (!g) return MPC_E_INVAL;
  GHIPCHK(g, hipSetDevice(g->device));
  const int rc = group_finish(g);
  if (rc != MPC_OK) return rc;
  GHIPCHK(g, hipDeviceSynchronize());   // batches may have been queued on caller streams
  return group_members_status(g);
}

int mpc_stats_len(const mpc_handle *h, uint64_t *len)
{
  if (!h || !len) return MPC_E_INVAL;
  *len = h->stats_len;
  return MPC_OK;
}

int mpc_stats_get(mpc_handle *h, uint64_t *vec, size_t n)
{
  if (!h || !vec || n < h->stats_len) return MPC_E_INVAL;
  HIPCHK(h, hipSetDevice(h->device));
  int rc = sync_all(h);
  if (rc != MPC_OK) return rc;
  HIPCHK(h, hipDeviceSynchronize());   // callers may have used their own streams
  rc = pattern_status(h);
  if (rc != MPC_OK) return rc;
  std::vector<u64> raw(h->raw_len);
  HIPCHK(h, hipMemcpy(raw.data(), h->d_raw, h->raw_len * sizeof(u64), hipMemcpyDeviceToHost));
  std::vector<u64> out(h->extra);
  derive_stats(h, raw, out);
  std::memcpy(vec, out.data(), h->stats_len * sizeof(u64));
  return MPC_OK;
}

int mpc_stats_raw_len(const mpc_handle *h, uint64_t *raw_len)
{
  if (!h || !raw_len) return MPC_E_INVAL;
  *raw_len = h->raw_len;
  return MPC_OK;
}

int mpc_stats_copy_raw_device(mpc_handle *h, void *d_dst, void *hip_stream)
{
  if (!h || !d_dst) return MPC_E_INVAL;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipMemcpyAsync(d_dst, h->d_raw, h->raw_len * sizeof(u64), hipMemcpyDeviceToDevice,
                           static_cast<hipStream_t>(hip_stream)));
  return MPC_OK;
}

int mpc_stats_from_raw(const mpc_handle *h, const uint64_t *raw, size_t raw_len, uint64_t *vec, size_t n)
{
  if (!h || !raw || !vec || raw_len != h->raw_len || n < h->stats_len) return MPC_E_INVAL;
  std::vector<u64> r(raw, raw + raw_len), out(h->stats_len, 0);
  derive_stats(h, r, out);
  std::memcpy(vec, out.data(), h->stats_len * sizeof(u64));
  return MPC_OK;
}

int mpc_stats_merge(mpc_handle *h, const uint64_t *vec, size_t n)
{
  if (!h || !vec || n != h->stats_len) return MPC_E_INVAL;
  for (size_t i = 0; i < n; i++) h->extra[i] += vec[i];
  return MPC_OK;
}

int mpc_stats_reset(mpc_handle *h)
{
  if (!h) return MPC_E_INVAL;
  HIPCHK(h, hipSetDevice(h->device));
  int rc = sync_all(h);
  if (rc != MPC_OK) return rc;
  HIPCHK(h, hipDeviceSynchronize());
  HIPCHK(h, hipMemset(h->d_raw, 0, (h->raw_len + kRouteWords) * sizeof(u64)));
  h->extra.assign(h->stats_len, 0);
  h->sc2.lines = h->sc2.warm = 0;     // SC2: the table and the line counter stay
  return MPC_OK;
}

int mpc_stats_set(mpc_handle *h, const uint64_t *vec, size_t n)
{
  if (!h || !vec || n != h->stats_len) return MPC_E_INVAL;
  int rc = mpc_stats_reset(h);
  if (rc != MPC_OK) return rc;
  for (size_t i = 0; i < n; i++) h->extra[i] = vec[i];
  return MPC_OK;
}

int mpc_config_describe(const char *json_text, char *out, size_t cap)
{
  if (!json_text || !out || cap < 2) return MPC_E_INVAL;
  mpc::VpcConfig cfg;
  std::string err;
  int rc = mpc::parse_vpc_config(json_text, cfg, err);
  std::string s;
  if (rc != 0) {
    s = "{\"error\": \"";
    for (char c : err) s += (c == '"' || c == '\\') ? '\'' : c;
    s += "\"}";
  } else {
    mpc::VpcPlan plan;
    mpc::build_vpc_plan(cfg, plan);
    const VpcRoute r = route_vpc(plan, Jit::Predicted);
    const bool fast = r.kernel != VpcKernel::Generic, unrolled = fast && r.kernel != VpcKernel::RuntimeLoop;
    s = "{\"L\": " + std::to_string(cfg.L) + ", \"M\": " + std::to_string(cfg.M) + ", \"n_pred\": " + std::to_string(cfg.n_pred) +
        ", \"has_aws\": " + (cfg.has_aws ? "true" : "false") + ", \"hist_bins\": " + std::to_string(cfg.hist_bins) + ", \"enc_bits\": [";
    for (size_t i = 0; i < cfg.enc_bits.size(); i++) s += (i ? ", " : "") + std::to_string(cfg.enc_bits[i]);
    s += "], \"path\": \"" + std::string(fast ? "fast" : "generic") + "\", \"why_generic\": \"" + r.why_generic +
         "\", \"sequence\": \"" + std::string(!fast ? "" : unrolled ? "unrolled" : "run-time loop") +
         "\", \"compiled\": \"" + std::string(!unrolled ? "" : r.kernel == VpcKernel::AtCreation ? "at creation" : "built in") +
         "\", \"general_layout\": \"" + std::string(unrolled && plan.params.gen_layout ? "yes" : "no") +
         "\", \"scan_order\": \"" + std::string(!fast ? "" : (plan.params.byte_major ? "byte-major" : "plane-major")) +
         "\", \"modules\": [";
    for (int i = 0; i < cfg.M; i++) {
      const mpc::Module &m = cfg.modules[(size_t)i];
      s += (i ? ", " : "");
      s += "{\"kind\": " + std::to_string(m.kind) + ", \"pred_kind\": " + std::to_string(m.pred_kind) + ", \"root\": " + std::to_string(m.root) +
           ", \"cx\": " + (m.consecutive_xor ? "1" : "0") + ", \"table_size\": " + std::to_string(m.table_size) + ", \"shifts\": [";
      for (size_t j = 0; j < m.weight.size(); j++)
        s += (j ? "," : "") + std::to_string(m.pred_kind == mpc::PRED_WEIGHT && (int)j != m.root ? mpc::weight_shift(m.weight[j]) : 0);
      s += "]}";
    }
    s += "]}";
  }
  if (s.size() + 1 > cap) return MPC_E_NOMEM;
  std::memcpy(out, s.c_str(), s.size() + 1);
  return rc;
}

int mpc_synth_fill(void *d_lines, uint64_t n_lines, unsigned L, int kind, uint64_t first_line, uint64_t seed, void *stream)
{
  if (!d_lines || L % 8 || kind < 0 || kind > 4) return MPC_E_INVAL;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return MPC_E_NODEVICE;
  if (!g_sine_dev[dev]) {
    // float32(sin(2*pi*t/1024)) computed in double on the host: the same
    // values as cal_22-mpc_amd/traces.py:sine_table()
    float tabf[1024];
    for (int t = 0; t < 1024; t++) tabf[t] = (float)sin(2.0 * 3.14159265358979323846 * (double)t / 1024.0);
    if (hipMalloc((void **)&g_sine_dev[dev], sizeof(tabf)) != hipSuccess) return MPC_E_NOMEM;
    if (hipMemcpy(g_sine_dev[dev], tabf, sizeof(tabf), hipMemcpyHostToDevice) != hipSuccess) return MPC_E_HIP;
  }
  hipError_t e = mpc_launch_synth(d_lines, n_lines, L, kind, first_line, seed, g_sine_dev[dev], (hipStream_t)stream);
  return e == hipSuccess ? MPC_OK : MPC_E_HIP;
}

int mpc_read_bandwidth_probe(const void *d_buf, uint64_t bytes, void *stream)
{
  static uint32_t *sink[16] = {nullptr};
  int dev = 0;
  if (!d_buf || hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return MPC_E_INVAL;
  if (!sink[dev] && hipMalloc((void **)&sink[dev], 64) != hipSuccess) return MPC_E_NOMEM;
  hipError_t e = mpc_launch_read_probe(d_buf, bytes, sink[dev], 256 * 8, (hipStream_t)stream);
  return e == hipSuccess ? MPC_OK : MPC_E_HIP;
}

#if MPC_TESTING
// test library only (not part of include/mpc_hip.h): the kernels' route counters since the handle was created or
// its statistics were last reset; out[i] for i < n, order of the MPC_RT_* enumeration (mpc_kernel_common.h)
int mpc_test_routes(mpc_handle *h, uint64_t *out, size_t n)
{
  if (!h || !out) return MPC_E_INVAL;
  if (hipSetDevice(h->device) != hipSuccess) return MPC_E_HIP;
  HIPCHK(h, hipDeviceSynchronize());
  uint64_t tmp[kRouteWords];
  HIPCHK(h, hipMemcpy(tmp, h->d_raw + h->raw_len, sizeof(tmp), hipMemcpyDeviceToHost));
  for (size_t i = 0; i < n; i++) out[i] = i < kRouteWords ? tmp[i] : 0;
  return MPC_OK;
}
#endif

}  // extern "C"
