// mpc_capi.hip -- the C ABI of include/mpc_hip.h: handles and groups, which kernel a handle launches, statistics.
// The staging pipeline behind the host-buffer and file calls is mpc_stage.h, the trace files mpc_trace_files.h.
//
// There is no CPU evaluation path in this library: every size it reports was
// computed by a gfx950 kernel in mpc_kernels.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "../../include/mpc_hip.h"

#include "mpc_config.h"
#include "mpc_device.h"
#include "mpc_sc2.h"
#include "mpc_pattern.h"
#include "mpc_sizes.h"
#include "mpc_classes.h"
#include "mpc_pack.h"
#include "mpc_image.h"
#include "mpc_rewrite.h"
#include "mpc_snapshot.h"
#include "mpc_fit.h"
#include "mpc_launch.h"

// libmpc_hip_test.so (build.py, -DMPC_TESTING=1): route counters behind the raw statistics and a cap on the launch grid,
// see mpc_kernel_common.h.  Must agree with the kernels' translation units.
#ifndef MPC_TESTING
#define MPC_TESTING 0
#endif
constexpr size_t kRouteWords = (MPC_TESTING || MPC_STAMPS) ? 16 : 0;
constexpr size_t kTestWords = kRouteWords + (MPC_STAMPS ? MPC_STAMP_WORDS : 0);      // route counters, then the workgroup stamps

typedef unsigned long long u64;

// Size, class, pack or image accounting on mpc_compress_batch_device without a sizes array of the caller's: the batch is evaluated in
// pieces of this many lines, each evaluator launch followed by the accounting passes over ONE scratch array (8 MiB per member).
constexpr u64 kAccountLines = 4ull << 20;

#include "mpc_jit.h"
#include "mpc_stage.h"

using mpcstage::Sink;
using mpcstage::Stager;

namespace {

thread_local std::string g_create_error;

// The ABI's algorithm numbers (mpc_info.algorithm) and, per algorithm, the facts that do not depend on a handle.
enum class Algo { VPC, BDI, FPC, BPC, SC2, Pattern, CPack, Fit };

struct AlgoFacts {
  const char *name;                        // in a group's form and error texts
  const char *label;                       // in the refusal of a line size
  u64 raw_len, stats_len;                  // device raw statistics, ABI statistics vector (VPC computes its own from the configuration)
  int clusters;                            // mpc_info.num_clusters (VPC: modules + 1)
  int path;                                // mpc_info.kernel_path (VPC: MPC_PATH_VPC_GENERIC when routed there)
  unsigned min_line, multiple, max_line;   // line sizes a handle is created for (VPC: the configuration's checks)
};
constexpr AlgoFacts kAlgo[] = {
  {"VPC", "VPC", 0, 0, 0, MPC_PATH_VPC_FAST, 0, 0, 0},
  // BDI.cpp:8 takes any dataLine.size(); values are 8, 4 and 2 bytes wide, so a multiple of 8
  {"BDI", "BDI", MPC_BDI_RAW_LEN, 12, 9, MPC_PATH_BDI, 8, 8, MPC_MAX_LINE},
  {"FPC", "FPC", MPC_FPC_RAW_LEN, 11, 8, MPC_PATH_FPC, 4, 4, MPC_MAX_LINE},
  // 32-bit words; a plane has one bit per delta and is held in an int32_t (BPC.cpp:53-63): 2..32 words
  {"BPC", "BPC", MPC_BPC_RAW_LEN, 11, 7, MPC_PATH_BPC, 8, 4, 128},
  {"SC2", "SC2", MPC_SC2_RAW_LEN, 6, 2, MPC_PATH_SC2, 4, 4, MPC_MAX_LINE},
  // 8-, 4- and 2-byte values (Pattern.cpp:26-58): a multiple of 8, or checkPattern reads past the line
  {"PATTERN", "Pattern", MPC_PATTERN_RAW_LEN, 534, 10, MPC_PATH_PATTERN, 8, 8, MPC_MAX_LINE},
  // C-Pack with a per-line dictionary: 32-bit words (CPACK.cpp:14)
  {"CPACK", "C-Pack", MPC_CPACK_RAW_LEN, 10, 6, MPC_PATH_CPACK, 4, 4, MPC_MAX_LINE},
  // the two Fit analyses: lengths, clusters and path depend on the line size and the analysis (create_fit); 32, 64 or 128 bytes
  {"FIT", "Fit", 0, 0, 9, MPC_PATH_FIT_PAIRS, 32, 32, 128},
};
constexpr const AlgoFacts &facts(Algo a) { return kAlgo[(int)a]; }
const char *algorithm_name(Algo a) { return facts(a).name; }

// the kernel a VPC configuration runs (route_vpc), and why it is the generic one
enum class VpcKernel { BuiltIn, BuiltInGeneral, AtCreation, RuntimeLoop, Generic };
struct VpcRoute { VpcKernel kernel = VpcKernel::Generic; std::string why_generic; };

}  // namespace

struct mpc_handle {
  Algo algorithm = Algo::VPC;
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
  Stager stage;                  // one member: this handle (mpc_stage.h); nothing of it exists before the first host-buffer call
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
    bool evicting = false;       // mpc_create_pattern_evicting: `evict` is the set, `set` is unused
    MpcEvictSet evict{};
  } pat;
  // C-Pack with a dictionary per block of N lines (mpc_create_cpack_blocks; N == 0: the per-line handle of mpc_create_cpack).
  // A launch may end inside a block: the open block's dictionary stays on the device, and every launch that reads or
  // writes it waits, on its own stream, for the event the one before it recorded -- whichever stream that was.
  struct {
    u64 N = 0;                   // lines per block
    u64 pos = 0;                 // lines of the open block already evaluated (lines seen modulo N); not reset by mpc_stats_reset
    uint32_t *d_state = nullptr; // [2][MPC_CPACK_STATE_WORDS]: a launch reads half `cur` and writes the other
    int cur = 0;
    hipEvent_t done = nullptr;
    bool recorded = false;
    std::string form;            // mpc_kernel_form
  } cpk;
  // Fit (mpc_fit.h): which of the two analyses; the residue analysis's base table (its device copy is d_gtab)
  struct {
    bool residues = false;
    std::vector<uint8_t> base;
  } fit;
  std::vector<Stager *> fed_by;  // every stager that feeds this handle: its own, then those of the groups it is a member of (sc2_build)
  // size accounting (mpc_sizes.h): nothing of it exists before mpc_size_hist_enable
  struct {
    bool on = false;
    u64 *d_hist = nullptr;             // [MPC_SIZE_BINS]; not for VPC, whose histogram is in its statistics
    std::vector<u64> vpc_base;         // VPC: that histogram when accounting was switched on (only later lines count)
    uint16_t *d_scratch = nullptr;     // [kAccountLines] sizes of a piece of a device batch (class accounting reads the same array)
    hipEvent_t scratch_done = nullptr; // behind the last pass that read the scratch, whichever stream that was
    bool recorded = false;
  } acct;
  // per-class accounting (mpc_classes.h): nothing of it exists before mpc_class_stats_enable
  struct {
    bool on = false;
    unsigned sector_bytes = 0;
    u64 *d_tab = nullptr;              // [MPC_CLASS_TABLE_LEN]
    std::vector<u64> extra;            // merged-in tables
  } cls;
  // pack accounting (mpc_pack.h): nothing of it exists before mpc_pack_stats_enable.  A launch may begin or end inside a
  // block: the open block's payload stays on the device, double-buffered, and every launch that reads or writes it waits,
  // on its own stream, for the event the one before it recorded -- whichever stream that was (as cpk above).
  struct {
    bool on = false;
    u64 N = 0;
    unsigned sector_bytes = 0, header_bits = 0;
    u64 seen = 0;                      // lines evaluated since accounting was switched on or last reset; the open block has seen % N
    u64 *d_tab = nullptr;              // [MPC_PACK_DEV_LEN]
    uint32_t *d_carry = nullptr;       // [2]: a launch reads word `cur` and writes the other
    int cur = 0;
    hipEvent_t done = nullptr;
    bool recorded = false;
    std::vector<u64> extra;            // merged-in tables, device layout
  } pack;
  // image accounting (mpc_image.h): nothing of it exists before mpc_image_stats_enable.  Its update passes are atomic
  // and stamped with the line's position, so launches on different streams need no order between them.
  struct {
    bool on = false;
    u64 capacity = 0, N = 0;
    unsigned sector_bytes = 0, header_bits = 0;
    u64 seen = 0;                      // lines evaluated since accounting was switched on or last reset: the next line's position
    u64 slots = 0;                     // the smallest power of two >= 2 x capacity
    u64 hash_mask = ~0ull;             // (the test library: MPC_TEST_IMAGE_HASH_BITS)
    u64 *d_keys = nullptr, *d_vals = nullptr;   // [slots]
    u64 *d_ctl = nullptr;              // [MPC_IMAGE_CTL_LEN], then [MPC_IMAGE_OUT_LEN]: the table of a get's pass
    u64 ctl[MPC_IMAGE_CTL_LEN] = {};   // what image_status last read of it
    bool over = false;                 // a key beyond the capacity arrived: the handle takes no more lines
  } img;
  // rewrite accounting (mpc_rewrite.h): nothing of it exists before mpc_rewrite_stats_enable.  Its passes depend on
  // order: every pass waits, on its own stream, for the event the pass before it recorded -- whichever stream that was
  // (the stager's two slot streams run one handle's chunks side by side).
  struct {
    bool on = false;
    u64 capacity = 0;
    unsigned granule = 0, G = 0;
    u64 seen = 0;                      // lines evaluated since accounting was switched on or last reset: the next line's position
    u64 slots = 0;                     // the smallest power of two >= 2 x capacity
    u64 hash_mask = ~0ull;             // (the test library: MPC_TEST_REWRITE_HASH_BITS)
    u64 batch = MPC_REWRITE_BATCH;     // lines of a sub-batch (the test library: MPC_TEST_REWRITE_BATCH)
    u64 *d_keys = nullptr, *d_vals = nullptr;   // [slots]
    u64 *d_dev = nullptr;              // [MPC_REWRITE_DEV_LEN]
    void *d_scratch = nullptr;         // the arrays of a sub-batch
    MpcRewriteScratch scratch{};
    hipEvent_t done = nullptr;
    bool recorded = false;
    u64 ctl[MPC_REWRITE_CTL_LEN] = {}; // what rewrite_status last read of the counters
    bool over = false;                 // a key beyond the capacity arrived: the handle takes no more lines
  } rw;
  std::string error;
};

struct mpc_group {
  std::vector<mpc_handle *> m;   // borrowed, in the caller's order
  int shared[3] = {-1, -1, -1};  // member index of the BDI, FPC, BPC handle that baselines_kernel evaluates (all -1: no shared launch)
  int first_shared = -1;         // ... the first of them in member order: where the shared launch is enqueued
  Stager stage;                  // m.size() members; its streams and events exist from creation (the members' fed_by), the rest as for a handle
  // best-of (mpc_sizes.h): nothing of it exists before mpc_group_best_enable
  struct {
    bool on = false;
    std::vector<int> set;              // member indices that take part, in member order (every member but Pattern ones)
    u64 *d_acc = nullptr;              // [MPC_SIZES_BEST_LEN]: histogram | wins in the order of `set` | bits
  } best;
  // device batches with accounting: per member the scratch sizes of a piece (null until needed), the pointers of the piece
  std::vector<uint16_t *> d_scratch, piece_sizes;
  std::vector<int8_t *> piece_sel;
  // per-class accounting of the group (mpc_classes.h): the members' tables are their handles'
  struct {
    bool on = false;
    unsigned sector_bytes = 0;
    u64 *d_best = nullptr;             // [MPC_CLASS_TABLE_LEN] of the per-line minimum; exists while this and the best-of are both on
    int from_member = -1;              // the class of a line is this member's selected + 1 (-1: the caller's classes or a .log field)
    int log_field = MPC_CLASS_LOG_NONE;
    int8_t *d_scratch_sel = nullptr;   // [kAccountLines] that member's selected values of a piece of a device batch
  } cls;
  // pack accounting of the group (mpc_pack.h): the members' tables are their handles'; the per-line minimum's is the group's
  struct {
    bool on = false;
    u64 N = 0;
    unsigned sector_bytes = 0, header_bits = 0, best_header_bits = 0;
    u64 *d_best = nullptr;             // [MPC_PACK_DEV_LEN]; exists if the best-of was on when this was switched on
    uint32_t *d_carry = nullptr;       // [2], as a handle's
    int cur = 0;
    u64 best_seen = 0;                 // lines that table has seen
    hipEvent_t done = nullptr;
    bool recorded = false;
  } pack;
  // image accounting of the group (mpc_image.h): the members' images are their handles'
  struct {
    bool on = false;
    u64 capacity = 0, N = 0;
    unsigned sector_bytes = 0, header_bits = 0;
  } img;
  // rewrite accounting of the group (mpc_rewrite.h): the members' maps are their handles'
  struct {
    bool on = false;
    u64 capacity = 0;
    unsigned granule = 0;
  } rw;
  hipEvent_t scratch_done = nullptr;
  bool recorded = false;
  std::string form, error;
};

namespace {

int set_err(mpc_handle *h, int code, const std::string &msg)
{
  if (h) h->error = msg; else g_create_error = msg;
  return code;
}

int group_err(mpc_group *g, int code, const std::string &msg)
{
  if (g) g->error = msg; else g_create_error = msg;
  return code;
}

// The two sinks of the stager (mpc_stage.h), which HIPCHK reports through as well: set_err and group_err are the two
// places a message lands.
int launch(mpc_handle *h, const void *d_lines, u64 n, uint16_t *d_sizes, int8_t *d_sel, hipStream_t s);
int pattern_status(mpc_handle *h);
int group_launch(mpc_group *g, const void *d_lines, u64 n, uint16_t *const *d_sizes, int8_t *const *d_sel, hipStream_t s);
int group_members_status(mpc_group *g);
int launch_accounted(mpc_handle *h, const void *d_lines, u64 n, uint16_t *d_sizes, int8_t *d_sel, const uint8_t *d_classes, const uint64_t *d_addrs,
                     hipStream_t s);
int group_launch_accounted(mpc_group *g, const void *d_lines, u64 n, uint16_t *const *d_sizes, int8_t *const *d_sel, const uint8_t *d_classes,
                           const uint64_t *d_addrs, hipStream_t s);

Sink sink_of(mpc_handle *h)
{
  return {h,
          [](void *c, const void *d, u64 n, uint16_t *const *ds, int8_t *const *dl, const uint8_t *dc, const uint64_t *da, hipStream_t s) {
            return launch_accounted(static_cast<mpc_handle *>(c), d, n, ds ? ds[0] : nullptr, dl ? dl[0] : nullptr, dc, da, s);
          },
          [](void *c, int code, const std::string &msg) { return set_err(static_cast<mpc_handle *>(c), code, msg); },
          [](void *c) { return pattern_status(static_cast<mpc_handle *>(c)); }};
}

Sink sink_of(mpc_group *g)
{
  return {g,
          [](void *c, const void *d, u64 n, uint16_t *const *ds, int8_t *const *dl, const uint8_t *dc, const uint64_t *da, hipStream_t s) {
            return group_launch_accounted(static_cast<mpc_group *>(c), d, n, ds, dl, dc, da, s);
          },
          [](void *c, int code, const std::string &msg) { return group_err(static_cast<mpc_group *>(c), code, msg); },
          [](void *c) { return group_members_status(static_cast<mpc_group *>(c)); }};
}

// a handle's slots retired, its own stream idle, Pattern's capacity checked
int sync_all(mpc_handle *h) { return mpcstage::finish(h->stage, sink_of(h), h->stream); }

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
  if (hipMalloc(&h->d_raw, (h->raw_len + kTestWords) * sizeof(u64)) != hipSuccess)
    return set_err(nullptr, MPC_E_NOMEM, "hipMalloc(stats) failed");
  if (hipMemsetAsync(h->d_raw, 0, (h->raw_len + kTestWords) * sizeof(u64), h->stream) != hipSuccess ||
      hipStreamSynchronize(h->stream) != hipSuccess)
    return set_err(nullptr, MPC_E_NODEVICE, "hipMemset(stats) failed");
  h->extra.assign(h->stats_len, 0);
  mpcstage::init(h->stage, h->device, h->L, 1);
  h->fed_by.assign(1, &h->stage);
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
  h->algorithm = Algo::VPC;
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
int launch_cpack_blocks(mpc_handle *h, const void *d_lines, u64 n, uint16_t *d_sizes, int8_t *d_sel, hipStream_t s);

const char *const kFitNoPerLine = "Fit: an analysis has no per-line result: size_bits_out and selected_out must be NULL";

int launch(mpc_handle *h, const void *d_lines, u64 n, uint16_t *d_sizes, int8_t *d_sel, hipStream_t s)
{
  if (n == 0) return MPC_OK;
  hipError_t e;
  switch (h->algorithm) {
  case Algo::Fit:
    if (d_sizes || d_sel) return set_err(h, MPC_E_INVAL, kFitNoPerLine);
    if (h->fit.residues)
      e = mpc_launch_fit_residues(d_lines, n, h->L, h->d_gtab, h->d_raw, grid_for(h, n, 1, mpc_fit_residues_wg_per_cu(h->L)), s);
    else      // (persistent grids: the launchers size them down to the work of a short batch)
      e = mpc_launch_fit_pairs(d_lines, n, h->L, h->d_raw, grid_for(h, n, 1, mpc_fit_pairs_wg_per_cu(h->L)), s);
    break;
  case Algo::SC2: return launch_sc2(h, d_lines, n, d_sizes, d_sel, s);
  case Algo::Pattern: return launch_pattern(h, d_lines, n, d_sizes, d_sel, s);
  case Algo::CPack:
    if (h->cpk.N) return launch_cpack_blocks(h, d_lines, n, d_sizes, d_sel, s);
    e = mpc_launch_cpack(d_lines, n, h->L, d_sizes, d_sel, h->d_raw, grid_for(h, n, 256, kWgPerCu), s); break;
  case Algo::BPC: e = mpc_launch_bpc(d_lines, n, h->L, d_sizes, d_sel, h->d_raw, grid_for(h, n, 256, kWgPerCu), s); break;
  case Algo::FPC: e = mpc_launch_fpc(d_lines, n, h->L, d_sizes, d_sel, h->d_raw, grid_for(h, n, 256, kWgPerCu), s); break;
  case Algo::BDI: e = mpc_launch_bdi(d_lines, n, h->L, d_sizes, d_sel, h->d_raw, grid_for(h, n, 256, kWgPerCu), s); break;
  default:
    if (h->route.kernel == VpcKernel::AtCreation) {
      e = mpc_launch_vpc_lane_jit(h->jit.stats, h->jit.lines, d_lines, n, &h->params, d_sizes, d_sel, h->d_raw,
                                  grid_for(h, n, 256, kWgPerCu), s);
    } else if (h->route.kernel == VpcKernel::Generic) {
      e = mpc_launch_vpc_generic(d_lines, n, &h->params, d_sizes, d_sel, h->d_raw, grid_for(h, n, 128, 8), s);
    } else {     // built in or the run-time module loop: the lane launcher finds which
      e = mpc_launch_vpc_lane(d_lines, n, &h->params, d_sizes, d_sel, h->d_raw, grid_for(h, n, 256, kWgPerCu), s);
    }
  }
  if (e != hipSuccess) return set_err(h, MPC_E_HIP, std::string("kernel launch: ") + hipGetErrorString(e));
  return MPC_OK;
}

// SC2: the code table from the warm-up counts.  The one blocking point of an SC2 handle: every stream that may still
// run a warm-up count (the call's, the handle's, the slot streams of every stager that feeds the handle: its own and
// those of the groups it belongs to, whose other slot may still be counting) is synchronised, the 1024 largest slots are
// selected on the device (radix select, 8 bits per pass from the top), only those <= 1024 (symbol, count) pairs come
// to the host, the heap is replayed there (mpc_sc2.h) and the bucket image goes back to the device.
int sc2_build(mpc_handle *h, hipStream_t s)
{
  HIPCHK(h, hipStreamSynchronize(s));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  for (Stager *st : h->fed_by) {
    const int rc = mpcstage::sync_slots(*st, sink_of(h));
    if (rc != MPC_OK) return rc;
  }
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

// C-Pack in blocks: one launch; the host keeps where in a block the next line falls.  Only a launch that begins or ends
// inside a block touches the dictionary kept on the device, and only those are chained.
int launch_cpack_blocks(mpc_handle *h, const void *d_lines, u64 n, uint16_t *d_sizes, int8_t *d_sel, hipStream_t s)
{
  auto &K = h->cpk;
  const bool loads = K.pos != 0, stores = (K.pos + n) % K.N != 0;
  if ((loads || stores) && K.recorded) HIPCHK(h, hipStreamWaitEvent(s, K.done, 0));
  const u64 n_blocks = (K.pos + n + K.N - 1) / K.N;
  const hipError_t e = mpc_launch_cpack_blocks(d_lines, n, h->L, K.N, K.pos, d_sizes, d_sel, h->d_raw, K.d_state + K.cur * MPC_CPACK_STATE_WORDS,
                                               K.d_state + (K.cur ^ 1) * MPC_CPACK_STATE_WORDS,
                                               grid_for(h, n_blocks, MPC_CPACK_BLOCK_THREADS, kWgPerCu), s);
  if (e != hipSuccess) return set_err(h, MPC_E_HIP, std::string("kernel launch: ") + hipGetErrorString(e));
  if (loads || stores) {
    HIPCHK(h, hipEventRecord(K.done, s));
    K.recorded = true;
  }
  if (stores) K.cur ^= 1;
  K.pos = (K.pos + n) % K.N;
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
  // the evicting set: launches of at most min(capacity, MPC_PATTERN_CHUNK) lines, in trace order
  for (u64 at = 0; h->pat.evicting && at < n; at += h->pat.evict.launch_max) {
    const u64 take = std::min<u64>(n - at, h->pat.evict.launch_max);
    const hipError_t e = mpc_launch_pattern_evict(base + at * (u64)h->L, (uint32_t)take, h->L, &h->pat.evict, h->d_raw, grid_for(h, take, 256, 8),
                                                  grid_for(h, (u64)h->pat.evict.slot_mask + 1, 256, 8), s);
    if (e != hipSuccess) return failed(e);
  }
  for (u64 at = 0; !h->pat.evicting && at < n; at += MPC_PATTERN_CHUNK) {
    const u64 take = std::min<u64>(n - at, MPC_PATTERN_CHUNK);
    HIPCHK(h, hipMemsetAsync(h->pat.set.ctl + MPC_PSET_PENDING_A, 0, 2 * sizeof(u64), s));
    const hipError_t e = mpc_launch_pattern_set(base + at * (u64)h->L, (uint32_t)take, h->L, &h->pat.set, h->d_raw, grid_for(h, take, 256, 8), s);
    if (e != hipSuccess) return failed(e);
  }
  HIPCHK(h, hipEventRecord(h->pat.done, s));
  h->pat.recorded = true;
  return MPC_OK;
}

// image accounting, at a point where the handle's work is complete: has a key beyond the capacity arrived?
int image_status(mpc_handle *h)
{
  if (!h->img.on) return MPC_OK;
  if (!h->img.over) {
    u64 *ctl = h->img.ctl;            // more claims than the capacity (the device's flag says the same, earlier)
    HIPCHK(h, hipMemcpy(ctl, h->img.d_ctl, sizeof(h->img.ctl), hipMemcpyDeviceToHost));
    h->img.over = ctl[MPC_IMAGE_CTL_KEYS] > h->img.capacity || ctl[MPC_IMAGE_CTL_OVERFLOW] != 0;
  }
  return h->img.over ? set_err(h, MPC_E_INVAL, "image accounting: more than " + std::to_string(h->img.capacity) +
                                                   " distinct line addresses (capacity_lines of mpc_image_stats_enable): the image is incomplete, the handle takes no more lines")
                     : MPC_OK;
}

// rewrite accounting, at a point where the handle's work is complete: has a key beyond the capacity arrived?
int rewrite_status(mpc_handle *h)
{
  if (!h->rw.on) return MPC_OK;
  if (!h->rw.over) {
    u64 *ctl = h->rw.ctl;
    HIPCHK(h, hipMemcpy(ctl, h->rw.d_dev, sizeof(h->rw.ctl), hipMemcpyDeviceToHost));
    h->rw.over = ctl[MPC_REWRITE_CTL_KEYS] > h->rw.capacity || ctl[MPC_REWRITE_CTL_OVERFLOW] != 0;
  }
  return h->rw.over ? set_err(h, MPC_E_INVAL, "rewrite accounting: more than " + std::to_string(h->rw.capacity) +
                                                  " distinct line addresses (capacity_lines of mpc_rewrite_stats_enable): the map is incomplete, the handle takes no more lines")
                    : MPC_OK;
}

// Pattern, at a point where the handle's work is complete: has a line beyond the capacity arrived?  (Image and rewrite
// accounting's capacities are checked at the same points, for every kind of handle.)
int pattern_status(mpc_handle *h)
{
  if (const int rc = image_status(h)) return rc;
  if (const int rc = rewrite_status(h)) return rc;
  if (h->algorithm != Algo::Pattern) return MPC_OK;
  if (h->pat.evicting) {       // nothing to run into: the flag says that a probe went round a whole table, which its sizing excludes
    u64 flag = 0;
    HIPCHK(h, hipMemcpy(&flag, h->pat.evict.ctl + MPC_ESET_OVERFLOW, sizeof(flag), hipMemcpyDeviceToHost));
    return flag ? set_err(h, MPC_E_HIP, "Pattern: the evicting set's table is full (internal error)") : MPC_OK;
  }
  if (!h->pat.over) {
    u64 ctl[2] = {0, 0};
    HIPCHK(h, hipMemcpy(ctl, h->pat.set.ctl, sizeof(ctl), hipMemcpyDeviceToHost));
    h->pat.over = ctl[MPC_PSET_OVERFLOW] != 0;
  }
  return h->pat.over ? set_err(h, MPC_E_INVAL, kPatternLimit) : MPC_OK;
}

// raw device statistics -> ABI vector (added into `vec`)
void derive_stats(const mpc_handle *h, const std::vector<u64> &raw, std::vector<u64> &vec)
{
  switch (h->algorithm) {
  case Algo::Fit: {
    const u64 L = (u64)h->L, lines = raw[0];
    vec[0] += lines;
    if (h->fit.residues) {
      for (u64 i = 0; i < L; i++)
        for (u64 v = 0; v < 256; v++) vec[3 + i * 256 + v] += raw[1 + v * L + i];
      return;
    }
    for (u64 i = 0; i < L; i++)
      for (u64 j = 0; j < L; j++) {
        u64 others = 0;
        for (u64 k = 1; k <= MPC_FIT_PAIR_BINS; k++) {
          const u64 c = raw[1 + (i * MPC_FIT_PAIR_BINS + (k - 1)) * L + j];
          vec[3 + (i * L + j) * 9 + k] += c;
          others += c;
        }
        vec[3 + (i * L + j) * 9] += lines - others;      // bin 0 is what the eight counted bins leave
      }
    return;
  }
  case Algo::Pattern: {
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
  case Algo::SC2: {
    // lines and warm-up lines are counted by the host (it splits every call at line S); bits and hits on the device
    vec[0] += h->sc2.lines;
    vec[1] += h->sc2.lines * 8ull * (u64)h->L;
    vec[2] += raw[0];
    vec[3] += h->sc2.warm;
    vec[4] += h->sc2.symbols.size();
    vec[5] += raw[1];
    return;
  }
  case Algo::CPack: {
    u64 words = 0;
    for (int i = 0; i < 6; i++) {
      vec[4 + i] += raw[i];
      words += raw[i];
    }
    vec[0] += words / (u64)(h->L / 4);
    vec[1] += words * 32ull;
    vec[2] += raw[6];
    vec[3] += words;
    return;
  }
  case Algo::BPC: {
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
  case Algo::FPC: {
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
  case Algo::BDI: {
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
  case Algo::VPC: break;
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

// ---------------------------------------------------------------------------
// groups: several handles of one line size on one device, fed together
// ---------------------------------------------------------------------------
// Which members share baselines_kernel: the first BDI, FPC and BPC handle of the group when the line size has an
// instantiation and at least two of the three are there; every other member launches its own kernel.
void group_route(mpc_group *g)
{
  int found[3] = {-1, -1, -1}, n = 0;
  for (size_t i = 0; i < g->m.size(); i++) {
    const int a = (int)g->m[i]->algorithm;
    if (a >= (int)Algo::BDI && a <= (int)Algo::BPC && found[a - 1] < 0) {
      found[a - 1] = (int)i;
      n++;
    }
  }
  if (n >= 2 && (g->stage.L == 32 || g->stage.L == 64 || g->stage.L == 128)) {
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
      part = std::string(algorithm_name(h->algorithm)) + ": " + (h->algorithm == Algo::VPC ? mpc_kernel_form(h) : h->algorithm == Algo::Pattern ? "own kernels" : "own kernel");
      if (h->cpk.N) part += ", dictionary per block of " + std::to_string(h->cpk.N) + " lines";
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
      const hipError_t e = mpc_launch_baselines(d_lines, n, g->stage.L, &A, grid_for(h, n, 256, kWgPerCu), s);
      if (e != hipSuccess) return group_err(g, MPC_E_HIP, std::string("kernel launch: ") + hipGetErrorString(e));
      continue;
    }
    const int rc = launch(h, d_lines, n, d_sizes ? d_sizes[i] : nullptr, d_sel ? d_sel[i] : nullptr, s);
    if (rc != MPC_OK) return group_err(g, rc, "member " + std::to_string(i) + " (" + algorithm_name(h->algorithm) + "): " + h->error);
  }
  return MPC_OK;
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

// ---------------------------------------------------------------------------
// size accounting (mpc_sizes.h): one pass over the sizes the evaluators of a chunk wrote, on the same stream behind them
// ---------------------------------------------------------------------------
// a handle whose sizes feed the pass for its own histogram (a VPC handle's histogram is in its statistics)
bool accounts(const mpc_handle *h) { return h->acct.on && h->algorithm != Algo::VPC; }

bool in_best(const mpc_group *g, int i) { return g->best.on && std::find(g->best.set.begin(), g->best.set.end(), i) != g->best.set.end(); }

// a handle whose sizes are wanted on the device, asked for by the caller or not
bool needs_sizes(const mpc_handle *h) { return accounts(h) || h->cls.on || h->pack.on || h->img.on || h->rw.on; }

// ... a member whose sizes a group needs on the device, asked for by the caller or not
bool group_accounts(const mpc_group *g, int i) { return needs_sizes(g->m[(size_t)i]) || in_best(g, i); }

// (a handle's accounting may have been switched on since the group's last call)
void group_refresh(mpc_group *g)
{
  for (int i = 0; i < (int)g->m.size(); i++) {
    g->stage.account[(size_t)i] = group_accounts(g, i) ? 1 : 0;
    g->stage.need_sel[(size_t)i] = g->cls.from_member == i ? 1 : 0;
  }
  g->stage.log_field = (g->cls.on && g->cls.from_member < 0) ? g->cls.log_field : MPC_CLASS_LOG_NONE;
  g->stage.log_addrs = g->img.on || g->rw.on;
}

hipError_t sizes_pass(const mpc_handle *h, const MpcSizesArgs &A, u64 n, hipStream_t s)
{
  return mpc_launch_sizes(&A, n, grid_for(h, n / 8 + 1, 256, mpc_sizes_wg_per_cu(&A)), s);
}

int account(mpc_handle *h, const uint16_t *d_sizes, u64 n, hipStream_t s)
{
  MpcSizesArgs A{};
  A.m = 1;
  A.sizes[0] = d_sizes;
  A.hist[0] = h->acct.d_hist;
  const hipError_t e = sizes_pass(h, A, n, s);
  if (e != hipSuccess) return set_err(h, MPC_E_HIP, std::string("kernel launch (size accounting): ") + hipGetErrorString(e));
  return MPC_OK;
}

// the per-class pass (mpc_classes.h) behind the evaluators' launches of a chunk
hipError_t classes_pass(const mpc_handle *h, const MpcClassArgs &A, u64 n, hipStream_t s)
{
  return mpc_launch_classes(&A, n, grid_for(h, n / 8 + 1, 256, mpc_classes_wg_per_cu(&A)), s);
}

void class_sectors(MpcClassArgs &A, unsigned L, unsigned sector_bytes)
{
  A.sector_bits = 8u * sector_bytes;
  A.max_sectors = (L + sector_bytes - 1) / sector_bytes;
}

// the refusals of mpc_class_stats_enable that need no device
const char *class_sector_refusal(unsigned L, unsigned sector_bytes)
{
  if (sector_bytes == 0 || sector_bytes > L) return "class accounting: sector_bytes must be 1 .. line_size";
  if ((L + sector_bytes - 1) / sector_bytes > MPC_CLASS_MAX_SECTORS) return "class accounting: a line of more than 8 sectors (sector_bytes is too small for the line size)";
  return nullptr;
}

// ---- pack accounting (mpc_pack.h) ----
// the refusals of mpc_pack_stats_enable that need no device
std::string pack_refusal(unsigned L, u64 block_lines, unsigned sector_bytes, unsigned header_bits)
{
  if (block_lines == 0) return "pack accounting: block_lines must be at least 1";
  if (block_lines > MPC_PACK_MAX_BLOCK_LINES)
    return "pack accounting: block_lines above " + std::to_string(MPC_PACK_MAX_BLOCK_LINES) + " (a block's bits are summed in 32 bits)";
  const u64 block_bytes = block_lines * (u64)L;
  if (sector_bytes == 0 || (u64)sector_bytes > block_bytes)
    return "pack accounting: sector_bytes must be 1 .. block_lines x line_size (" + std::to_string(block_bytes) + ")";
  if ((block_bytes + sector_bytes - 1) / sector_bytes > MPC_PACK_MAX_SECTORS)
    return "pack accounting: a block of more than " + std::to_string(MPC_PACK_MAX_SECTORS) + " sectors (sector_bytes is too small for block_lines x line_size = " +
           std::to_string(block_bytes) + ")";
  if (header_bits > 65535u) return "pack accounting: header_bits must be 0 .. 65535";
  return "";
}

std::string pack_values(u64 N, unsigned sb, unsigned hb)
{
  return "block_lines " + std::to_string(N) + ", sector_bytes " + std::to_string(sb) + ", header_bits " + std::to_string(hb);
}

// ---- image accounting (mpc_image.h): its values ----
// the refusals of mpc_image_stats_enable that need no device
std::string image_refusal_of(unsigned L, u64 capacity, u64 block_lines, unsigned sector_bytes, unsigned header_bits)
{
  if (capacity == 0) return "image accounting: capacity_lines must be at least 1";
  if (capacity > MPC_IMAGE_MAX_CAPACITY) return "image accounting: capacity_lines above " + std::to_string(MPC_IMAGE_MAX_CAPACITY) + " (2^28; the table takes 32 bytes per line of capacity)";
  std::string why = pack_refusal(L, block_lines, sector_bytes, header_bits);
  if (!why.empty()) why.replace(0, 4, "image");        // "pack accounting: ..." -> "image accounting: ..."
  return why;
}

std::string image_values(u64 cap, u64 N, unsigned sb, unsigned hb) { return "capacity_lines " + std::to_string(cap) + ", " + pack_values(N, sb, hb); }

u64 image_slots(u64 capacity)
{
  u64 slots = 2;
  while (slots < 2 * capacity) slots <<= 1;
  return slots;
}

// ---- rewrite accounting (mpc_rewrite.h): its values ----
// the refusals of mpc_rewrite_stats_enable that need no device
std::string rewrite_refusal_of(unsigned L, u64 capacity, unsigned granule)
{
  if (capacity == 0) return "rewrite accounting: capacity_lines must be at least 1";
  if (capacity > MPC_REWRITE_MAX_CAPACITY) return "rewrite accounting: capacity_lines above " + std::to_string(MPC_REWRITE_MAX_CAPACITY) + " (2^28; the map takes 32 bytes per line of capacity)";
  if (granule == 0) return "rewrite accounting: granule_bytes must be at least 1";
  if (granule > L) return "rewrite accounting: granule_bytes " + std::to_string(granule) + " above the line size " + std::to_string(L);
  if ((L + granule - 1) / granule > MPC_REWRITE_MAX_CLASSES)
    return "rewrite accounting: granule_bytes " + std::to_string(granule) + " gives " + std::to_string((L + granule - 1) / granule) + " size classes for lines of " +
           std::to_string(L) + " bytes, more than " + std::to_string(MPC_REWRITE_MAX_CLASSES);
  return "";
}

std::string rewrite_values(u64 cap, unsigned granule) { return "capacity_lines " + std::to_string(cap) + ", granule_bytes " + std::to_string(granule); }
// device table (mpc_pack.h) -> the ABI's table; open_lines / open_bits: the open block
void pack_table_out(const std::vector<u64> &dev, u64 N, unsigned L, unsigned sb, unsigned hb, u64 open_lines, u64 open_bits, uint64_t *table)
{
  std::fill(table, table + MPC_PACK_TABLE_LEN, 0);
  const u64 S = (N * (u64)L + sb - 1) / sb;
  for (u64 k = 1; k <= S; k++) {
    table[8 + k - 1] = dev[k];
    table[0] += dev[k];
    table[2] += dev[k] * k;
  }
  table[1] = dev[0];
  table[3] = open_lines;
  table[4] = open_bits;
  table[5] = N;
  table[6] = sb;
  table[7] = hb;
}

// One pass behind the evaluators' launches of a chunk for `m` handles that count with the same values and stand at the
// same line (the caller has checked), with the group's table of the per-line minimum over them when `g` is given.
// Only a launch that begins or ends inside a block touches the carries, and only those are chained.
int pack_pass(const Sink &k, const mpc_handle *grid_of, mpc_handle *const *hs, const uint16_t *const *d_sizes, int m, mpc_group *g, u64 n, hipStream_t s)
{
  const auto &P0 = hs[0]->pack;
  const u64 N = P0.N, pos = P0.seen % N;
  const bool loads = pos != 0, stores = (pos + n) % N != 0;
  MpcPackArgs A{};
  A.m = m;
  A.block_lines = N;
  A.pos = pos;
  A.sector_bits = 8u * P0.sector_bytes;
  A.max_sectors = (unsigned)((N * (u64)hs[0]->L + P0.sector_bytes - 1) / P0.sector_bytes);
  A.header_bits = P0.header_bits;
  for (int i = 0; i < m; i++) {
    auto &P = hs[i]->pack;
    A.sizes[i] = d_sizes[i];
    if (!P.on) continue;
    A.table[i] = P.d_tab;
    A.carry_in[i] = P.d_carry + P.cur;
    A.carry_out[i] = P.d_carry + (P.cur ^ 1);
    if ((loads || stores) && P.recorded) HIPCHK(k, hipStreamWaitEvent(s, P.done, 0));
  }
  if (g) {
    A.best = g->pack.d_best;
    A.best_carry_in = g->pack.d_carry + g->pack.cur;
    A.best_carry_out = g->pack.d_carry + (g->pack.cur ^ 1);
    A.best_header_bits = g->pack.best_header_bits;
    if ((loads || stores) && g->pack.recorded) HIPCHK(k, hipStreamWaitEvent(s, g->pack.done, 0));
  }
  const u64 blocks = (pos + n + N - 1) / N;
  const u64 per_wg = N <= MPC_PACK_LANE_MAX ? 256 : N <= MPC_PACK_WAVE_MAX ? 4 : 1;
  const hipError_t e = mpc_launch_pack(&A, n, grid_for(grid_of, (blocks + per_wg - 1) / per_wg, 1, 4), s);      // (the launcher sizes it down further)
  if (e != hipSuccess) return k.fail(k.ctx, MPC_E_HIP, std::string("kernel launch (pack accounting): ") + hipGetErrorString(e));
  for (int i = 0; i < m; i++) {
    auto &P = hs[i]->pack;
    if (!P.on) continue;
    if (loads || stores) {
      HIPCHK(k, hipEventRecord(P.done, s));
      P.recorded = true;
    }
    if (stores) P.cur ^= 1;
    P.seen += n;
  }
  if (g) {
    if (loads || stores) {
      HIPCHK(k, hipEventRecord(g->pack.done, s));
      g->pack.recorded = true;
    }
    if (stores) g->pack.cur ^= 1;
    g->pack.best_seen += n;
  }
  return MPC_OK;
}

// ---- image accounting (mpc_image.h) ----
// before a chunk is evaluated: a handle with the accounting on takes only lines that bring an address, and none once
// its capacity was exceeded; a handle without it takes no addresses
int image_refusal(mpc_handle *h, u64 n, const uint64_t *d_addrs)
{
  if (!h->img.on && !h->rw.on)
    return d_addrs ? set_err(h, MPC_E_INVAL, "image accounting is not switched on for this handle (mpc_image_stats_enable): the call must not bring addresses") : MPC_OK;
  if (h->img.on && h->img.over) return image_status(h);
  if (h->rw.on && h->rw.over) return rewrite_status(h);
  if (n && !d_addrs)
    return h->img.on ? set_err(h, MPC_E_INVAL, "image accounting is on: every line needs an address (mpc_compress_batch_addressed, mpc_compress_batch_device_addressed or a "
                                               "GPGPU-Sim .log); this call brings none, and a hole in the image is not counted silently")
                     : set_err(h, MPC_E_INVAL, "rewrite accounting is on: every line needs an address (mpc_compress_batch_addressed, mpc_compress_batch_device_addressed or a "
                                               "GPGPU-Sim .log); this call brings none, and a hole in the sequences is not counted silently");
  return MPC_OK;
}

// ---- rewrite accounting (mpc_rewrite.h) ----
MpcRewriteMap rewrite_map(const mpc_handle *h)
{
  const auto &R = h->rw;
  MpcRewriteMap M{};
  M.keys = R.d_keys;
  M.vals = R.d_vals;
  M.dev = R.d_dev;
  M.slot_mask = R.slots - 1;
  M.hash_mask = R.hash_mask;
  M.capacity = R.capacity;
  M.granule_bits = 8u * R.granule;
  M.classes = R.G;
  return M;
}

// The passes behind the evaluators' launches of a chunk for the `m` handles that account (all at one line; a handle alone:
// m == 1).  The chunk's keys are sorted once, in the first handle's scratch, and applied to each handle's map with its own
// sizes.  Every pass of a handle is chained to the one before it: stream s waits for the event recorded behind it, and
// the event is recorded again behind this one.
int rewrite_pass(const Sink &k, mpc_handle *const *hs, const uint16_t *const *d_sizes, int m, const uint64_t *d_addrs, u64 n, hipStream_t s)
{
  mpc_handle *h0 = hs[0];
  const MpcRewriteScratch &S = h0->rw.scratch;
  for (int i = 0; i < m; i++)
    if (hs[i]->rw.recorded) HIPCHK(k, hipStreamWaitEvent(s, hs[i]->rw.done, 0));
  for (u64 at = 0; at < n; at += h0->rw.batch) {
    const u64 take = std::min<u64>(n - at, h0->rw.batch);
    hipError_t e = hipSuccess;
    for (int i = 0; i < m && e == hipSuccess; i++)
      e = mpc_launch_rewrite_keys(&S, d_addrs + at, d_sizes[i] + at, take, (unsigned)h0->L, hs[i]->rw.d_dev, i == 0, grid_for(h0, take, 256, 8), s);
    if (e == hipSuccess) e = mpc_launch_rewrite_sort(&S, take, s);
    for (int i = 0; i < m && e == hipSuccess; i++) {
      const MpcRewriteMap M = rewrite_map(hs[i]);
      e = mpc_launch_rewrite_apply(&S, &M, d_sizes[i] + at, take, s);
    }
    if (e != hipSuccess) return k.fail(k.ctx, MPC_E_HIP, std::string("kernel launch (rewrite accounting): ") + hipGetErrorString(e));
  }
  for (int i = 0; i < m; i++) {
    HIPCHK(k, hipEventRecord(hs[i]->rw.done, s));
    hs[i]->rw.recorded = true;
    hs[i]->rw.seen += n;
  }
  return MPC_OK;
}

// the update pass behind the evaluator's launch of a chunk
int image_pass(const Sink &k, mpc_handle *h, const uint16_t *d_sizes, const uint64_t *d_addrs, u64 n, hipStream_t s)
{
  auto &I = h->img;
  MpcImageArgs A{};
  A.addrs = d_addrs;
  A.sizes = d_sizes;
  A.keys = I.d_keys;
  A.vals = I.d_vals;
  A.ctl = I.d_ctl;
  A.slot_mask = I.slots - 1;
  A.hash_mask = I.hash_mask;
  A.pos = I.seen;
  A.capacity = I.capacity;
  A.line_size = (unsigned)h->L;
  A.line_shift = -1;
  for (int b = 0; b < 31; b++)
    if ((unsigned)h->L == (1u << b)) A.line_shift = b;
  const hipError_t e = mpc_launch_image_update(&A, n, grid_for(h, n, 256, 8), s);
  if (e != hipSuccess) return k.fail(k.ctx, MPC_E_HIP, std::string("kernel launch (image accounting): ") + hipGetErrorString(e));
  I.seen += n;
  return MPC_OK;
}

// a staged or in-place chunk of a handle: the stager has asked for the sizes of a handle that accounts
int launch_accounted(mpc_handle *h, const void *d_lines, u64 n, uint16_t *d_sizes, int8_t *d_sel, const uint8_t *d_classes, const uint64_t *d_addrs,
                     hipStream_t s)
{
  if (const int irc = image_refusal(h, n, d_addrs)) return irc;
  int rc = launch(h, d_lines, n, d_sizes, d_sel, s);
  if (rc != MPC_OK || n == 0 || !needs_sizes(h)) return rc;
  if (!d_sizes) return set_err(h, MPC_E_INVAL, "size accounting: the chunk has no sizes array");
  if (accounts(h)) rc = account(h, d_sizes, n, s);
  if (rc == MPC_OK && h->cls.on) {
    MpcClassArgs A{};
    A.m = 1;
    A.sizes[0] = d_sizes;
    A.table[0] = h->cls.d_tab;
    A.classes = d_classes;
    class_sectors(A, (unsigned)h->L, h->cls.sector_bytes);
    const hipError_t e = classes_pass(h, A, n, s);
    if (e != hipSuccess) return set_err(h, MPC_E_HIP, std::string("kernel launch (class accounting): ") + hipGetErrorString(e));
  }
  if (rc == MPC_OK && h->pack.on) {
    mpc_handle *one[1] = {h};
    const uint16_t *arr[1] = {d_sizes};
    rc = pack_pass(sink_of(h), h, one, arr, 1, nullptr, n, s);
  }
  if (rc == MPC_OK && h->img.on) rc = image_pass(sink_of(h), h, d_sizes, d_addrs, n, s);
  if (rc != MPC_OK || !h->rw.on) return rc;
  mpc_handle *one[1] = {h};
  const uint16_t *arr[1] = {d_sizes};
  return rewrite_pass(sink_of(h), one, arr, 1, d_addrs, n, s);
}

// The members' sizes of one chunk (one pointer per member, non-null for every member that group_accounts): first the
// best-of set in one launch, with the histograms of its members that have one; then the other histograms (Pattern
// members, or every member when best-of is off), MPC_SIZES_MAX arrays a launch.
int group_account(mpc_group *g, uint16_t *const *d_sizes, u64 n, hipStream_t s)
{
  const mpc_handle *h0 = g->m[0];
  auto pass = [&](const MpcSizesArgs &A) {
    const hipError_t e = sizes_pass(h0, A, n, s);
    return e == hipSuccess ? MPC_OK : group_err(g, MPC_E_HIP, std::string("kernel launch (size accounting): ") + hipGetErrorString(e));
  };
  if (g->best.on) {
    MpcSizesArgs A{};
    for (int i : g->best.set) {
      A.sizes[A.m] = d_sizes[i];
      A.hist[A.m] = accounts(g->m[(size_t)i]) ? g->m[(size_t)i]->acct.d_hist : nullptr;
      A.m++;
    }
    A.best = g->best.d_acc;
    const int rc = pass(A);
    if (rc != MPC_OK) return rc;
  }
  MpcSizesArgs A{};
  for (int i = 0; i < (int)g->m.size(); i++) {
    if (!accounts(g->m[(size_t)i]) || in_best(g, i)) continue;
    A.sizes[A.m] = d_sizes[i];
    A.hist[A.m] = g->m[(size_t)i]->acct.d_hist;
    if (++A.m == MPC_SIZES_MAX) {
      const int rc = pass(A);
      if (rc != MPC_OK) return rc;
      A = MpcSizesArgs{};
    }
  }
  return A.m ? pass(A) : MPC_OK;
}

// The per-class tables of one chunk, behind every member's launch and the size pass: the best-of set in one launch
// (the minimum's table, with the tables of its members), then the other members, MPC_SIZES_MAX arrays a launch.
int group_class_account(mpc_group *g, uint16_t *const *d_sizes, int8_t *const *d_sel, const uint8_t *d_classes, u64 n, hipStream_t s)
{
  const mpc_handle *h0 = g->m[0];
  MpcClassArgs base{};
  unsigned sb = 0;
  for (const mpc_handle *h : g->m) {
    if (!h->cls.on) continue;
    if (sb && h->cls.sector_bytes != sb)
      return group_err(g, MPC_E_INVAL, "class accounting: the members of a group count with different sector_bytes (" + std::to_string(sb) + " and " +
                                           std::to_string(h->cls.sector_bytes) + ")");
    sb = h->cls.sector_bytes;
  }
  if (!sb) return MPC_OK;
  class_sectors(base, (unsigned)g->stage.L, sb);
  base.classes = d_classes;
  if (g->cls.from_member >= 0) {
    if (!d_sel || !d_sel[g->cls.from_member])
      return group_err(g, MPC_E_INVAL, "class accounting: the chunk has no selected array for member " + std::to_string(g->cls.from_member));
    base.classes = reinterpret_cast<const uint8_t *>(d_sel[g->cls.from_member]);
    base.class_bias = 1;
  }
  auto pass = [&](const MpcClassArgs &A) {
    const hipError_t e = classes_pass(h0, A, n, s);
    return e == hipSuccess ? MPC_OK : group_err(g, MPC_E_HIP, std::string("kernel launch (class accounting): ") + hipGetErrorString(e));
  };
  const bool with_best = g->best.on && g->cls.d_best;
  if (with_best) {
    MpcClassArgs A = base;
    for (int i : g->best.set) {
      A.sizes[A.m] = d_sizes[i];
      A.table[A.m] = g->m[(size_t)i]->cls.on ? g->m[(size_t)i]->cls.d_tab : nullptr;
      A.m++;
    }
    A.best = g->cls.d_best;
    const int rc = pass(A);
    if (rc != MPC_OK) return rc;
  }
  MpcClassArgs A = base;
  for (int i = 0; i < (int)g->m.size(); i++) {
    if (!g->m[(size_t)i]->cls.on || (with_best && in_best(g, i))) continue;
    A.sizes[A.m] = d_sizes[i];
    A.table[A.m] = g->m[(size_t)i]->cls.d_tab;
    if (++A.m == MPC_SIZES_MAX) {
      const int rc = pass(A);
      if (rc != MPC_OK) return rc;
      A = base;
    }
  }
  return A.m ? pass(A) : MPC_OK;
}

// The pack tables of one chunk, behind the other accounting passes.  A group with pack accounting on has its members at
// one line with one set of values (group_pack_check): the best-of set in one launch (the minimum's table with the tables
// of its members), then the other members, MPC_SIZES_MAX arrays a launch.  Else every member that counts on its own
// takes a launch of its own, with its own values.
int group_pack_account(mpc_group *g, uint16_t *const *d_sizes, u64 n, hipStream_t s)
{
  const Sink k = sink_of(g);
  mpc_handle *hs[MPC_SIZES_MAX];
  const uint16_t *arr[MPC_SIZES_MAX];
  if (!g->pack.on) {
    for (size_t i = 0; i < g->m.size(); i++) {
      if (!g->m[i]->pack.on) continue;
      hs[0] = g->m[i];
      arr[0] = d_sizes[i];
      const int rc = pack_pass(k, g->m[0], hs, arr, 1, nullptr, n, s);
      if (rc != MPC_OK) return rc;
    }
    return MPC_OK;
  }
  const bool with_best = g->pack.d_best != nullptr;
  int m = 0;
  if (with_best) {
    for (int i : g->best.set) {
      hs[m] = g->m[(size_t)i];
      arr[m++] = d_sizes[i];
    }
    const int rc = pack_pass(k, g->m[0], hs, arr, m, g, n, s);
    if (rc != MPC_OK) return rc;
    m = 0;
  }
  for (int i = 0; i < (int)g->m.size(); i++) {
    if (with_best && in_best(g, i)) continue;
    hs[m] = g->m[(size_t)i];
    arr[m] = d_sizes[i];
    if (++m == MPC_SIZES_MAX) {
      const int rc = pack_pass(k, g->m[0], hs, arr, m, nullptr, n, s);
      if (rc != MPC_OK) return rc;
      m = 0;
    }
  }
  return m ? pack_pass(k, g->m[0], hs, arr, m, nullptr, n, s) : MPC_OK;
}

// Before a group call feeds its members: with the group's pack accounting on they stand at one common line.
int group_pack_check(mpc_group *g)
{
  if (!g->pack.on) return MPC_OK;
  const u64 at = g->m[0]->pack.seen;
  for (size_t i = 0; i < g->m.size(); i++) {
    const auto &P = g->m[i]->pack;
    if (!P.on || P.N != g->pack.N || P.sector_bytes != g->pack.sector_bytes || P.header_bits != g->pack.header_bits)
      return group_err(g, MPC_E_INVAL, "pack accounting: member " + std::to_string(i) + " does not count with the group's values (" +
                                           pack_values(g->pack.N, g->pack.sector_bytes, g->pack.header_bits) + ")");
    if (P.seen != at)
      return group_err(g, MPC_E_INVAL, "pack accounting: member " + std::to_string(i) + " (" + algorithm_name(g->m[i]->algorithm) + ") is at line " +
                                           std::to_string(P.seen) + ", member 0 at line " + std::to_string(at) +
                                           ": a member was fed outside the group, its blocks no longer line up with the others' (reset the members to start over)");
  }
  if (g->pack.d_best && g->pack.best_seen != at)
    return group_err(g, MPC_E_INVAL, "pack accounting: the members are at line " + std::to_string(at) + ", the table of the best-of at line " +
                                         std::to_string(g->pack.best_seen) + ": the members were fed or reset outside the group (reset the members and mpc_group_best_reset to start over)");
  return MPC_OK;
}

// Before a group call feeds its members: with the group's image accounting on they stand at one common line.
int group_image_check(mpc_group *g)
{
  if (!g->img.on) return MPC_OK;
  const u64 at = g->m[0]->img.seen;
  for (size_t i = 0; i < g->m.size(); i++) {
    const auto &I = g->m[i]->img;
    if (!I.on || I.capacity != g->img.capacity || I.N != g->img.N || I.sector_bytes != g->img.sector_bytes || I.header_bits != g->img.header_bits)
      return group_err(g, MPC_E_INVAL, "image accounting: member " + std::to_string(i) + " does not count with the group's values");
    if (I.seen != at)
      return group_err(g, MPC_E_INVAL, "image accounting: member " + std::to_string(i) + " (" + algorithm_name(g->m[i]->algorithm) + ") is at line " +
                                           std::to_string(I.seen) + ", member 0 at line " + std::to_string(at) +
                                           ": a member was fed outside the group, its positions no longer line up with the others' (reset the members to start over)");
  }
  return MPC_OK;
}

// Before a group call feeds its members: with the group's rewrite accounting on they stand at one common line.
int group_rewrite_check(mpc_group *g)
{
  if (!g->rw.on) return MPC_OK;
  const u64 at = g->m[0]->rw.seen;
  for (size_t i = 0; i < g->m.size(); i++) {
    const auto &R = g->m[i]->rw;
    if (!R.on || R.capacity != g->rw.capacity || R.granule != g->rw.granule)
      return group_err(g, MPC_E_INVAL, "rewrite accounting: member " + std::to_string(i) + " does not count with the group's values");
    if (R.seen != at)
      return group_err(g, MPC_E_INVAL, "rewrite accounting: member " + std::to_string(i) + " (" + algorithm_name(g->m[i]->algorithm) + ") is at line " +
                                           std::to_string(R.seen) + ", member 0 at line " + std::to_string(at) +
                                           ": a member was fed outside the group, its positions no longer line up with the others' (reset the members to start over)");
  }
  return MPC_OK;
}

int group_launch_accounted(mpc_group *g, const void *d_lines, u64 n, uint16_t *const *d_sizes, int8_t *const *d_sel, const uint8_t *d_classes,
                           const uint64_t *d_addrs, hipStream_t s)
{
  bool images = false;
  for (size_t i = 0; i < g->m.size(); i++) {
    mpc_handle *h = g->m[i];
    if (!h->img.on && !h->rw.on) continue;   // (a member without the accountings ignores the group's addresses)
    images = true;
    if (const int irc = image_refusal(h, n, d_addrs)) return group_err(g, irc, "member " + std::to_string(i) + " (" + algorithm_name(h->algorithm) + "): " + h->error);
  }
  if (d_addrs && !images) return group_err(g, MPC_E_INVAL, "image accounting is not switched on for any member of this group: the call must not bring addresses");
  int rc = group_launch(g, d_lines, n, d_sizes, d_sel, s);
  if (rc != MPC_OK || n == 0) return rc;
  bool any = false, sizes = false;
  for (int i = 0; i < (int)g->m.size(); i++) {
    if (!group_accounts(g, i)) continue;
    if (!d_sizes || !d_sizes[i]) return group_err(g, MPC_E_INVAL, "size accounting: the chunk has no sizes array for member " + std::to_string(i));
    any = true;
    sizes = sizes || accounts(g->m[(size_t)i]) || in_best(g, i);
  }
  if (!any) return MPC_OK;
  if (sizes) rc = group_account(g, d_sizes, n, s);
  if (rc == MPC_OK) rc = group_class_account(g, d_sizes, d_sel, d_classes, n, s);
  if (rc == MPC_OK) rc = group_pack_account(g, d_sizes, n, s);
  for (size_t i = 0; rc == MPC_OK && images && i < g->m.size(); i++)
    if (g->m[i]->img.on) rc = image_pass(sink_of(g), g->m[i], d_sizes[i], d_addrs, n, s);
  if (rc != MPC_OK || !images) return rc;
  // the members with rewrite accounting on: one sort of the chunk's keys, applied to each member's map
  std::vector<mpc_handle *> hs;
  std::vector<const uint16_t *> arr;
  for (size_t i = 0; i < g->m.size(); i++)
    if (g->m[i]->rw.on) {
      if (!hs.empty() && (g->m[i]->rw.seen != hs[0]->rw.seen || g->m[i]->rw.batch != hs[0]->rw.batch))
        return group_err(g, MPC_E_INVAL, "rewrite accounting: member " + std::to_string(i) + " is not at the line of the members before it (reset the members to start over)");
      hs.push_back(g->m[i]);
      arr.push_back(d_sizes[i]);
    }
  return hs.empty() ? rc : rewrite_pass(sink_of(g), hs.data(), arr.data(), (int)hs.size(), d_addrs, n, s);
}

// VPC: the size histogram is the sum over the clusters of the histogram in the raw statistics, clipped into MPC_SIZE_BINS bins
void vpc_size_hist(const mpc_handle *h, const std::vector<u64> &raw, std::vector<u64> &bins)
{
  const int K = h->cfg.M + 1, B = h->cfg.hist_bins;
  bins.assign(MPC_SIZE_BINS, 0);
  for (int k = 0; k < K; k++)
    for (int s = 0; s < B; s++) bins[(size_t)std::min(s, MPC_SIZE_BINS - 1)] += raw[2 * K + (u64)k * B + s];
}

// the line sizes an algorithm of the table takes (the refusal lands in mpc_last_error(NULL))
int check_line_size(Algo a, unsigned line_size)
{
  const AlgoFacts &f = facts(a);
  if (line_size >= f.min_line && line_size <= f.max_line && line_size % f.multiple == 0) return MPC_OK;
  return set_err(nullptr, MPC_E_INVAL, std::string(f.label) + " line size must be a multiple of " + std::to_string(f.multiple) + " in " +
                                           std::to_string(f.min_line) + ".." + std::to_string(f.max_line) + " bytes");
}

// A handle of an algorithm whose lengths are in the table: BDI, FPC and BPC are done with it, SC2 and Pattern add their
// own allocations.  *out is the handle or null.
int create_fixed(Algo a, unsigned line_size, int device, mpc_handle **out)
{
  if (!out) return MPC_E_INVAL;
  *out = nullptr;
  int rc = check_line_size(a, line_size);
  if (rc != MPC_OK) return rc;
  mpc_handle *h = new (std::nothrow) mpc_handle();
  if (!h) return MPC_E_NOMEM;
  h->algorithm = a;
  h->L = (int)line_size;
  h->raw_len = facts(a).raw_len;
  h->stats_len = facts(a).stats_len;
  rc = pick_device(device, &h->device, &h->num_cus);
  if (rc == MPC_OK) rc = finish_create(h);
  if (rc != MPC_OK) {
    mpc_destroy(h);
    return rc;
  }
  *out = h;
  return MPC_OK;
}

// (for SC2 and Pattern) the algorithm's own allocations failed: no handle
int create_failed(int rc, mpc_handle **out)
{
  mpc_destroy(*out);
  *out = nullptr;
  return rc;
}

// The two Fit analyses.  base == nullptr: the pair table.  The refusals come before any device is touched.
int create_fit(unsigned line_size, const uint8_t *base, int device, mpc_handle **out)
{
  if (!out) return MPC_E_INVAL;
  *out = nullptr;
  if (line_size != 32 && line_size != 64 && line_size != 128)
    return set_err(nullptr, MPC_E_INVAL, "Fit: line size " + std::to_string(line_size) + " is not one of 32, 64 and 128 bytes");
  for (unsigned i = 0; base && i < line_size; i++)
    if (base[i] >= line_size)
      return set_err(nullptr, MPC_E_INVAL, "Fit: base_table[" + std::to_string(i) + "] = " + std::to_string(base[i]) + " is not a byte of a " +
                                               std::to_string(line_size) + "-byte line");
  mpc_handle *h = new (std::nothrow) mpc_handle();
  if (!h) return MPC_E_NOMEM;
  h->algorithm = Algo::Fit;
  h->L = (int)line_size;
  h->fit.residues = base != nullptr;
  h->raw_len = base ? mpc_fit_residues_raw_len(line_size) : mpc_fit_pairs_raw_len(line_size);
  h->stats_len = base ? mpc_fit_residues_stats_len(line_size) : mpc_fit_pairs_stats_len(line_size);
  int rc = pick_device(device, &h->device, &h->num_cus);
  if (rc == MPC_OK && base) {
    h->fit.base.assign(base, base + line_size);
    if (hipMalloc((void **)&h->d_gtab, line_size) != hipSuccess) {
      h->d_gtab = nullptr;
      rc = set_err(nullptr, MPC_E_NOMEM, "Fit: hipMalloc of the base table failed");
    } else if (hipMemcpy(h->d_gtab, base, line_size, hipMemcpyHostToDevice) != hipSuccess) {
      rc = set_err(nullptr, MPC_E_NODEVICE, "Fit: hipMemcpy of the base table failed");
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

// the class table of the per-line minimum exists while the group's class accounting and its best-of are both on
int group_class_best_ensure(mpc_group *g)
{
  if (!g->cls.on || !g->best.on || g->cls.d_best) return MPC_OK;
  HIPCHK(g, hipSetDevice(g->stage.device));
  if (hipMalloc((void **)&g->cls.d_best, MPC_CLASS_TABLE_LEN * sizeof(u64)) != hipSuccess) {
    g->cls.d_best = nullptr;
    return group_err(g, MPC_E_NOMEM, "hipMalloc(class table of the best-of) failed");
  }
  HIPCHK(g, hipMemset(g->cls.d_best, 0, MPC_CLASS_TABLE_LEN * sizeof(u64)));
  HIPCHK(g, hipDeviceSynchronize());   // (the kernels run on non-blocking streams)
  return MPC_OK;
}

const char *const kClassesOff = "class accounting is not switched on for this handle (mpc_class_stats_enable)";
const char *const kGroupClassesOff = "class accounting is not switched on for this group (mpc_group_class_stats_enable)";
const char *const kClassTableLen = "a class table has MPC_CLASS_TABLE_LEN (256 x 10 = 2560) entries";

bool class_log_field_ok(int field) { return field >= MPC_CLASS_LOG_NONE && field <= MPC_CLASS_LOG_MFTYPE; }

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

int mpc_create_bdi(unsigned line_size, int device, mpc_handle **out) { return create_fixed(Algo::BDI, line_size, device, out); }
int mpc_create_fpc(unsigned line_size, int device, mpc_handle **out) { return create_fixed(Algo::FPC, line_size, device, out); }
int mpc_create_bpc(unsigned line_size, int device, mpc_handle **out) { return create_fixed(Algo::BPC, line_size, device, out); }

int mpc_create_cpack(unsigned line_size, int dictionary_scope, int device, mpc_handle **out)
{
  if (!out) return MPC_E_INVAL;
  *out = nullptr;
  if (dictionary_scope == MPC_CPACK_DICT_CARRIED)
    return set_err(nullptr, MPC_E_INVAL, "C-Pack: the reference's dictionary carried from line to line (MPC_CPACK_DICT_CARRIED) is not offered: "
                                         "it is sequential state and does not shard (DESIGN.md 8); MPC_CPACK_DICT_PER_LINE starts every line from a fresh dictionary");
  if (dictionary_scope != MPC_CPACK_DICT_PER_LINE)
    return set_err(nullptr, MPC_E_INVAL, "C-Pack: dictionary_scope " + std::to_string(dictionary_scope) + " is not one of MPC_CPACK_DICT_CARRIED (0), MPC_CPACK_DICT_PER_LINE (1)");
  return create_fixed(Algo::CPack, line_size, device, out);
}

int mpc_create_cpack_blocks(unsigned line_size, uint64_t block_lines, int device, mpc_handle **out)
{
  if (!out) return MPC_E_INVAL;
  *out = nullptr;
  // (the refusals before a device is touched: the line size, then the block length)
  int rc = check_line_size(Algo::CPack, line_size);
  if (rc != MPC_OK) return rc;
  if (block_lines < 1 || block_lines > 0xffffffffull)
    return set_err(nullptr, MPC_E_INVAL, "C-Pack: block_lines " + std::to_string(block_lines) + " is not in 1..4294967295 (2^32 - 1) lines; a block "
                                         "longer than the trace is the dictionary carried over all of it");
  rc = create_fixed(Algo::CPack, line_size, device, out);
  if (rc != MPC_OK) return rc;
  mpc_handle *h = *out;
  h->cpk.N = block_lines;
  h->cpk.form = "one lane per block of " + std::to_string(block_lines) + (block_lines == 1 ? " line" : " lines");
  if (hipMalloc((void **)&h->cpk.d_state, 2 * MPC_CPACK_STATE_WORDS * sizeof(uint32_t)) != hipSuccess) {
    h->cpk.d_state = nullptr;
    g_create_error = "C-Pack: hipMalloc of the open block's dictionary failed";
    return create_failed(MPC_E_NOMEM, out);
  }
  if (hipMemset(h->cpk.d_state, 0, 2 * MPC_CPACK_STATE_WORDS * sizeof(uint32_t)) != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
      hipEventCreateWithFlags(&h->cpk.done, hipEventDisableTiming) != hipSuccess) {
    g_create_error = "C-Pack: initialising the open block's dictionary failed";
    return create_failed(MPC_E_NODEVICE, out);
  }
  return MPC_OK;
}

int mpc_create_fit_pairs(unsigned line_size, int device, mpc_handle **out) { return create_fit(line_size, nullptr, device, out); }

int mpc_create_fit_residues(unsigned line_size, const uint8_t *base_table, int device, mpc_handle **out)
{
  if (!out) return MPC_E_INVAL;
  *out = nullptr;
  if (!base_table) return set_err(nullptr, MPC_E_INVAL, "Fit: base_table is NULL");
  return create_fit(line_size, base_table, device, out);
}

int mpc_fit_base_table(const mpc_handle *h, uint8_t *out, size_t n)
{
  if (!h || !out || h->algorithm != Algo::Fit || !h->fit.residues || n < (size_t)h->L) return MPC_E_INVAL;
  std::memcpy(out, h->fit.base.data(), (size_t)h->L);
  return MPC_OK;
}

int mpc_cpack_blocks_restart(mpc_handle *h)
{
  if (!h) return MPC_E_INVAL;
  if (h->algorithm != Algo::CPack || !h->cpk.N) return set_err(h, MPC_E_INVAL, "C-Pack: not a handle of mpc_create_cpack_blocks");
  h->cpk.pos = 0;      // (the dictionary on the device is only read by a launch that begins inside a block)
  return MPC_OK;
}

int mpc_cpack_block_lines(const mpc_handle *h, uint64_t *n)
{
  if (!h || !n || h->algorithm != Algo::CPack || !h->cpk.N) return MPC_E_INVAL;
  *n = h->cpk.N;
  return MPC_OK;
}

int mpc_create_pattern(unsigned line_size, int device, mpc_handle **out)
{
  int rc = create_fixed(Algo::Pattern, line_size, device, out);
  if (rc != MPC_OK) return rc;
  mpc_handle *h = *out;
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
    return create_failed(MPC_E_NOMEM, out);
  }
  if (hipMemset(S.tags, 0, slots * sizeof(u64)) != hipSuccess || hipMemset(S.ctl, 0, MPC_PSET_WORDS * sizeof(u64)) != hipSuccess ||
      hipDeviceSynchronize() != hipSuccess ||          // (the kernels run on non-blocking streams)
      hipEventCreateWithFlags(&h->pat.done, hipEventDisableTiming) != hipSuccess) {
    g_create_error = "initialising the Pattern line set failed";
    return create_failed(MPC_E_NODEVICE, out);
  }
  return MPC_OK;
}

int mpc_create_pattern_evicting(unsigned line_size, uint64_t capacity, int device, mpc_handle **out)
{
  if (!out) return MPC_E_INVAL;
  *out = nullptr;
  // (the refusals before a device is touched: the line size, then the capacity)
  int rc = check_line_size(Algo::Pattern, line_size);
  if (rc != MPC_OK) return rc;
  if (capacity > MPC_PATTERN_CAPACITY)
    return set_err(nullptr, MPC_E_INVAL, "Pattern: a capacity of " + std::to_string(capacity) + " lines is more than the reference's 16777215 (2^24 - 1); 0 stands for that");
  rc = create_fixed(Algo::Pattern, line_size, device, out);
  if (rc != MPC_OK) return rc;
  mpc_handle *h = *out;
  h->pat.evicting = true;
  MpcEvictSet &S = h->pat.evict;
  S.capacity = capacity ? capacity : MPC_PATTERN_CAPACITY;
  S.launch_max = (uint32_t)std::min<u64>(S.capacity, MPC_PATTERN_CHUNK);
  // the newer table holds at most C lines brought along and C - 1 + launch_max insertions (mpc_pattern.h)
  u64 slots = 8;
  while (2 * slots < 3 * (2 * S.capacity + S.launch_max)) slots <<= 1;
  S.slot_mask = (uint32_t)(slots - 1);
  S.tag_mask = ~0ull;
#if MPC_TESTING
  if (const char *e = getenv("MPC_TEST_PATTERN_TAG_BITS")) {      // as mpc_create_pattern
    const long bits = atol(e);
    if (bits >= 1 && bits < 64) S.tag_mask = (1ull << bits) - 1ull;
  }
#endif
  const size_t m = S.launch_max, blocks = (m + 255) / 256;
  bool ok = true;
  auto take = [&](auto **p, size_t bytes, int fill) {      // fill < 0: left as it comes
    ok = ok && hipMalloc((void **)p, bytes) == hipSuccess && (fill < 0 || hipMemset(*p, fill, bytes) == hipSuccess);
  };
  for (MpcEvictTable &T : S.tab) {
    take(&T.tags, slots * sizeof(u64), 0);
    take(&T.stamps, slots * sizeof(u64), 0xff);
    take(&T.first, slots * sizeof(u64), 0xff);        // (above every key a launch writes)
    take(&T.store, slots * (size_t)line_size, -1);
  }
  take(&S.ctl, MPC_ESET_WORDS * sizeof(u64), 0);
  take(&S.pend_a, m * sizeof(uint2), 0);
  take(&S.pend_b, m * sizeof(uint2), 0);
  take(&S.ent, m * sizeof(uint32_t), 0);
  take(&S.gone_before, m * sizeof(uint32_t), 0);
  take(&S.risk_before, m * sizeof(uint32_t), 0);
  take(&S.risk, m * sizeof(uint32_t), 0);
  take(&S.risk_missed, (m + 1) * sizeof(uint32_t), 0);
  take(&S.kind, m, 0);
  take(&S.block_sums, blocks * sizeof(uint2), 0);
  if (!ok) {
    g_create_error = "hipMalloc of the evicting Pattern line set (" + std::to_string(2 * slots * (3 * sizeof(u64) + line_size)) + " bytes) failed";
    return create_failed(MPC_E_NOMEM, out);
  }
  if (hipDeviceSynchronize() != hipSuccess ||          // (the kernels run on non-blocking streams)
      hipEventCreateWithFlags(&h->pat.done, hipEventDisableTiming) != hipSuccess) {
    g_create_error = "initialising the evicting Pattern line set failed";
    return create_failed(MPC_E_NODEVICE, out);
  }
  return MPC_OK;
}

int mpc_pattern_distinct_lines(mpc_handle *h, uint64_t *n)
{
  if (!h || !n || h->algorithm != Algo::Pattern) return MPC_E_INVAL;
  HIPCHK(h, hipSetDevice(h->device));
  int rc = sync_all(h);
  if (rc != MPC_OK) return rc;
  HIPCHK(h, hipDeviceSynchronize());   // callers may have used their own streams
  rc = pattern_status(h);
  if (rc != MPC_OK) return rc;
  u64 v = 0;
  HIPCHK(h, hipMemcpy(&v, h->pat.evicting ? h->pat.evict.ctl + MPC_ESET_INSERTIONS : h->pat.set.ctl + MPC_PSET_DISTINCT, sizeof(v), hipMemcpyDeviceToHost));
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
  // (the refusals in the order they have always come in: the line size, then the sample, and only then the device)
  int rc = check_line_size(Algo::SC2, line_size);
  if (rc != MPC_OK) return rc;
  if (sampling_lines == 0) {
    g_create_error = "SC2 needs at least one warm-up line (the reference builds its table from an empty map otherwise)";
    return MPC_E_INVAL;
  }
  const u64 words = sampling_lines * (u64)(line_size / 4);
  if (sampling_lines > (1ull << 28) || words > (1ull << 28)) {
    g_create_error = "SC2 warm-up sample of more than 2^28 words (its frequency table would exceed 4 GiB)";
    return MPC_E_INVAL;
  }
  rc = create_fixed(Algo::SC2, line_size, device, out);
  if (rc != MPC_OK) return rc;
  mpc_handle *h = *out;
  h->sc2.S = sampling_lines;
  u64 slots = 2;
  while (slots < 2 * words) slots <<= 1;
  h->sc2.hash_mask = slots - 1;
  if (hipMalloc((void **)&h->sc2.d_hash, slots * sizeof(u64)) != hipSuccess ||
      hipMalloc((void **)&h->sc2.d_buckets, MPC_SC2_MAX_BUCKETS * sizeof(uint4)) != hipSuccess ||
      hipMemset(h->sc2.d_hash, 0, slots * sizeof(u64)) != hipSuccess ||
      hipDeviceSynchronize() != hipSuccess) {        // (the kernels run on non-blocking streams)
    g_create_error = "hipMalloc of the SC2 frequency table (" + std::to_string(slots * sizeof(u64)) + " bytes) failed";
    return create_failed(MPC_E_NOMEM, out);
  }
  return MPC_OK;
}

int mpc_sc2_table(mpc_handle *h, uint32_t *symbols, uint16_t *lengths, size_t cap, size_t *n)
{
  if (!h || !n || h->algorithm != Algo::SC2) return MPC_E_INVAL;
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
  // (the handle's own stream first: an in-place call that failed half way may have left work that reads the stager's buffer)
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  mpcstage::destroy(h->stage);
  if (h->stream) (void)hipStreamDestroy(h->stream);
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
  {
    const MpcEvictSet &E = h->pat.evict;
    for (const MpcEvictTable &T : E.tab)
      for (void *p : {(void *)T.tags, (void *)T.stamps, (void *)T.first, (void *)T.store})
        if (p) (void)hipFree(p);
    for (void *p : {(void *)E.ctl, (void *)E.pend_a, (void *)E.pend_b, (void *)E.ent, (void *)E.gone_before, (void *)E.risk_before, (void *)E.risk,
                    (void *)E.risk_missed, (void *)E.kind, (void *)E.block_sums})
      if (p) (void)hipFree(p);
  }
  if (h->pat.done) (void)hipEventDestroy(h->pat.done);
  if (h->cpk.d_state) (void)hipFree(h->cpk.d_state);
  if (h->cpk.done) (void)hipEventDestroy(h->cpk.done);
  if (h->acct.d_hist) (void)hipFree(h->acct.d_hist);
  if (h->acct.d_scratch) (void)hipFree(h->acct.d_scratch);
  if (h->acct.scratch_done) (void)hipEventDestroy(h->acct.scratch_done);
  if (h->cls.d_tab) (void)hipFree(h->cls.d_tab);
  if (h->pack.d_tab) (void)hipFree(h->pack.d_tab);
  if (h->pack.d_carry) (void)hipFree(h->pack.d_carry);
  if (h->pack.done) (void)hipEventDestroy(h->pack.done);
  if (h->img.d_keys) (void)hipFree(h->img.d_keys);
  if (h->img.d_ctl) (void)hipFree(h->img.d_ctl);
  if (h->rw.d_keys) (void)hipFree(h->rw.d_keys);
  if (h->rw.d_dev) (void)hipFree(h->rw.d_dev);
  if (h->rw.d_scratch) (void)hipFree(h->rw.d_scratch);
  if (h->rw.done) (void)hipEventDestroy(h->rw.done);
  delete h;
}

int mpc_get_info(const mpc_handle *h, mpc_info *info)
{
  if (!h || !info) return MPC_E_INVAL;
  info->abi_version = MPC_ABI_VERSION;
  const bool vpc = h->algorithm == Algo::VPC;
  info->algorithm = (int)h->algorithm;
  info->line_size = h->L;
  info->num_modules = vpc ? h->cfg.M : 0;
  info->num_clusters = vpc ? h->cfg.M + 1 : h->fit.residues ? 256 : facts(h->algorithm).clusters;
  info->hist_bins = vpc ? h->cfg.hist_bins : 0;
  info->kernel_path = vpc && h->route.kernel == VpcKernel::Generic ? MPC_PATH_VPC_GENERIC : h->pat.evicting ? MPC_PATH_PATTERN_EVICTING
                      : h->cpk.N ? MPC_PATH_CPACK_BLOCKS : h->fit.residues ? MPC_PATH_FIT_RESIDUES : facts(h->algorithm).path;
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
  if (h->algorithm == Algo::SC2) return h->sc2.built ? "table sizing" : "warm-up counting";
  if (h->algorithm == Algo::Pattern && h->pat.evicting)
    return (h->L == 32 || h->L == 64 || h->L == 128) ? "unrolled, then the evicting set passes" : "run-time loop, then the evicting set passes";
  if (h->algorithm == Algo::Pattern) return (h->L == 32 || h->L == 64 || h->L == 128) ? "unrolled, then the set passes" : "run-time loop, then the set passes";
  if (h->algorithm == Algo::CPack && h->cpk.N) return h->cpk.form.c_str();
  if (h->algorithm == Algo::CPack) return (h->L == 32 || h->L == 64 || h->L == 128) ? "unrolled" : "run-time loop";
  if (h->algorithm == Algo::Fit) return h->fit.residues ? "one lane per byte" : "one lane per byte pair";
  if (h->algorithm != Algo::VPC) return "unrolled";
  if (h->route.kernel == VpcKernel::AtCreation && h->jit.from_cache) return "unrolled, compiled at creation (from the cache)";
  static const char *const form[] = {"unrolled", "unrolled, general layout", "unrolled, compiled at creation", "run-time loop", "generic"};
  return form[(int)h->route.kernel];      // (VpcKernel order)
}

const char *mpc_path_reason(const mpc_handle *h)
{
  return (h && h->algorithm == Algo::VPC) ? h->route.why_generic.c_str() : "";
}

// mpc_compress_batch_device, its classed twin (d_classes: null for class 0) and its addressed twin (d_addrs: null for none)
static int batch_device(mpc_handle *h, const void *d_lines, uint64_t n, const uint8_t *d_classes, const uint64_t *d_addrs, uint16_t *d_sizes, int8_t *d_sel,
                        void *hip_stream)
{
  if (!h || (!d_lines && n)) return MPC_E_INVAL;
  if (((uintptr_t)d_lines) & 15u) return set_err(h, MPC_E_INVAL, "device line buffer must be 16-byte aligned");
  if (h->algorithm == Algo::Fit && (d_sizes || d_sel)) return set_err(h, MPC_E_INVAL, kFitNoPerLine);
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t s = (hipStream_t)hip_stream;
  if (!needs_sizes(h) || d_sizes) return launch_accounted(h, d_lines, n, d_sizes, d_sel, d_classes, d_addrs, s);
  if (const int irc = image_refusal(h, n, d_addrs)) return irc;      // (before the scratch array is made)
  // accounting without a sizes array of the caller's: pieces of kAccountLines lines over the handle's scratch array
  if (!h->acct.d_scratch) {
    HIPCHK(h, hipMalloc((void **)&h->acct.d_scratch, kAccountLines * sizeof(uint16_t)));
    HIPCHK(h, hipEventCreateWithFlags(&h->acct.scratch_done, hipEventDisableTiming));
  }
  if (h->acct.recorded) HIPCHK(h, hipStreamWaitEvent(s, h->acct.scratch_done, 0));
  for (u64 at = 0; at < n; at += kAccountLines) {
    const u64 take = std::min<u64>(n - at, kAccountLines);
    const int rc = launch_accounted(h, static_cast<const uint8_t *>(d_lines) + at * (u64)h->L, take, h->acct.d_scratch, d_sel ? d_sel + at : nullptr,
                                    d_classes ? d_classes + at : nullptr, d_addrs ? d_addrs + at : nullptr, s);
    if (rc != MPC_OK) return rc;
  }
  HIPCHK(h, hipEventRecord(h->acct.scratch_done, s));
  h->acct.recorded = true;
  return MPC_OK;
}

int mpc_compress_batch_device(mpc_handle *h, const void *d_lines, uint64_t n, uint16_t *d_sizes, int8_t *d_sel,
                              void *hip_stream)
{
  return batch_device(h, d_lines, n, nullptr, nullptr, d_sizes, d_sel, hip_stream);
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
  if (h->algorithm == Algo::Fit && (sizes || sel)) return set_err(h, MPC_E_INVAL, kFitNoPerLine);
  if (n == 0) return MPC_OK;
  return mpcstage::compress_batch(h->stage, sink_of(h), h->stream, lines, n, nullptr, nullptr, &sizes, &sel);   // (a group of one)
}

int mpc_npy_shape(const char *path, uint64_t *rows, uint64_t *cols)
{
  if (!path || !rows || !cols) return MPC_E_INVAL;
  FILE *f = fopen(path, "rb");
  if (!f) { g_create_error = std::string("cannot open ") + path; return MPC_E_NOENT; }
  u64 r, c, off;
  std::string err;
  int rc = mpctrace::parse_npy_header(f, &r, &c, &off, err);
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
  return mpcstage::compress_npy(h->stage, sink_of(h), h->stream, path, first_row, n_rows, skip_last_row, rows_done);
}

int mpc_gpgpusim_log_line_size(const char *log_path, uint32_t *line_size)
{
  if (!log_path || !line_size) return MPC_E_INVAL;
  *line_size = 0;
  FILE *f = nullptr;
  std::string err;
  int rc = mpctrace::log_open(log_path, &f, err);
  if (rc != MPC_OK) return set_err(nullptr, rc, err);
  uint32_t t = 0, sz = 0;
  if (mpctrace::log_next(f, &t, &sz)) *line_size = sz;
  fclose(f);
  return MPC_OK;
}

int mpc_compress_gpgpusim_log(mpc_handle *h, const char *log_path, uint64_t *requests_read, uint64_t *lines_done)
{
  if (!h || !log_path) return MPC_E_INVAL;
  return mpcstage::compress_gpgpusim_log(h->stage, sink_of(h), h->stream, log_path, requests_read, lines_done);
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
    if (members[i]->algorithm == Algo::Fit)
      return group_err(nullptr, MPC_E_INVAL, "Fit: member " + std::to_string(i) + " is an analysis handle, which a group does not take");
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
  mpcstage::init(g->stage, members[0]->device, members[0]->L, n);
  group_route(g);
  // the streams and events now, not at the first staged call: the members wait for them in sc2_build
  bool ok = hipSetDevice(g->stage.device) == hipSuccess;
  for (mpcstage::Slot &s : g->stage.slots)
    ok = ok && hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking) == hipSuccess &&
         hipEventCreateWithFlags(&s.done, hipEventDisableTiming) == hipSuccess;
  if (!ok) {
    mpc_group_destroy(g);
    return group_err(nullptr, MPC_E_HIP, "hipStreamCreate / hipEventCreate failed for the group's slots");
  }
  for (mpc_handle *h : g->m) h->fed_by.push_back(&g->stage);
  *out = g;
  return MPC_OK;
}

void mpc_group_destroy(mpc_group *g)
{
  if (!g) return;
  (void)hipSetDevice(g->stage.device);
  for (mpc_handle *h : g->m) h->fed_by.erase(std::remove(h->fed_by.begin(), h->fed_by.end(), &g->stage), h->fed_by.end());
  mpcstage::destroy(g->stage);
  if (g->best.d_acc) (void)hipFree(g->best.d_acc);
  if (g->cls.d_best) (void)hipFree(g->cls.d_best);
  if (g->cls.d_scratch_sel) (void)hipFree(g->cls.d_scratch_sel);
  if (g->pack.d_best) (void)hipFree(g->pack.d_best);
  if (g->pack.d_carry) (void)hipFree(g->pack.d_carry);
  if (g->pack.done) (void)hipEventDestroy(g->pack.done);
  for (uint16_t *p : g->d_scratch) if (p) (void)hipFree(p);
  if (g->scratch_done) (void)hipEventDestroy(g->scratch_done);
  delete g;
}

const char *mpc_group_last_error(const mpc_group *g) { return g ? g->error.c_str() : g_create_error.c_str(); }

const char *mpc_group_form(const mpc_group *g) { return g ? g->form.c_str() : ""; }

int mpc_group_compress_batch(mpc_group *g, const uint8_t *lines, uint64_t n, uint16_t *const *sizes, int8_t *const *sel)
{
  if (!g || (!lines && n)) return MPC_E_INVAL;
  if (n == 0) return MPC_OK;
  group_refresh(g);
  if (const int prc = group_pack_check(g)) return prc;
  if (const int irc = group_image_check(g)) return irc;
  if (const int wrc = group_rewrite_check(g)) return wrc;
  return mpcstage::compress_batch(g->stage, sink_of(g), nullptr, lines, n, nullptr, nullptr, sizes, sel);
}

// mpc_group_compress_batch_device, its classed twin (d_classes: null for class 0, or the classes come from a member) and its
// addressed twin (d_addrs: null for none)
static int group_batch_device(mpc_group *g, const void *d_lines, uint64_t n, const uint8_t *d_classes, const uint64_t *d_addrs, uint16_t *const *d_sizes,
                              int8_t *const *d_sel, void *hip_stream)
{
  if (!g || (!d_lines && n)) return MPC_E_INVAL;
  if (((uintptr_t)d_lines) & 15u) return group_err(g, MPC_E_INVAL, "device line buffer must be 16-byte aligned");
  HIPCHK(g, hipSetDevice(g->stage.device));
  hipStream_t s = (hipStream_t)hip_stream;
  if (const int prc = group_pack_check(g)) return prc;
  if (const int irc = group_image_check(g)) return irc;
  if (const int wrc = group_rewrite_check(g)) return wrc;
  const size_t nm = g->m.size();
  bool any = false, scratch = false;
  for (size_t i = 0; i < nm; i++) {
    if (!group_accounts(g, (int)i)) continue;
    any = true;
    scratch = scratch || !(d_sizes && d_sizes[i]);
  }
  const int fm = g->cls.from_member;       // its selected values are needed on the device, asked for or not
  const bool sel_scratch = fm >= 0 && !(d_sel && d_sel[fm]);
  if (!any && !d_addrs) return group_launch(g, d_lines, n, d_sizes, d_sel, s);
  if (!scratch && !sel_scratch) return group_launch_accounted(g, d_lines, n, d_sizes, d_sel, d_classes, d_addrs, s);
  // accounting of a member without a sizes array of the caller's: pieces of kAccountLines lines, that member's sizes in a scratch array
  g->d_scratch.resize(nm, nullptr);
  g->piece_sizes.assign(nm, nullptr);
  g->piece_sel.assign(nm, nullptr);
  for (size_t i = 0; i < nm; i++)
    if (group_accounts(g, (int)i) && !(d_sizes && d_sizes[i]) && !g->d_scratch[i])
      HIPCHK(g, hipMalloc((void **)&g->d_scratch[i], kAccountLines * sizeof(uint16_t)));
  if (sel_scratch && !g->cls.d_scratch_sel) HIPCHK(g, hipMalloc((void **)&g->cls.d_scratch_sel, kAccountLines));
  if (!g->scratch_done) HIPCHK(g, hipEventCreateWithFlags(&g->scratch_done, hipEventDisableTiming));
  if (g->recorded) HIPCHK(g, hipStreamWaitEvent(s, g->scratch_done, 0));
  for (u64 at = 0; at < n; at += kAccountLines) {
    const u64 take = std::min<u64>(n - at, kAccountLines);
    for (size_t i = 0; i < nm; i++) {
      g->piece_sizes[i] = (d_sizes && d_sizes[i]) ? d_sizes[i] + at : group_accounts(g, (int)i) ? g->d_scratch[i] : nullptr;
      g->piece_sel[i] = (d_sel && d_sel[i]) ? d_sel[i] + at : (sel_scratch && (int)i == fm) ? g->cls.d_scratch_sel : nullptr;
    }
    const int rc = group_launch_accounted(g, static_cast<const uint8_t *>(d_lines) + at * (u64)g->stage.L, take, g->piece_sizes.data(), g->piece_sel.data(),
                                          d_classes ? d_classes + at : nullptr, d_addrs ? d_addrs + at : nullptr, s);
    if (rc != MPC_OK) return rc;
  }
  HIPCHK(g, hipEventRecord(g->scratch_done, s));
  g->recorded = true;
  return MPC_OK;
}

int mpc_group_compress_batch_device(mpc_group *g, const void *d_lines, uint64_t n, uint16_t *const *d_sizes, int8_t *const *d_sel,
                                    void *hip_stream)
{
  return group_batch_device(g, d_lines, n, nullptr, nullptr, d_sizes, d_sel, hip_stream);
}

int mpc_group_compress_npy(mpc_group *g, const char *path, uint64_t first_row, uint64_t n_rows, int skip_last_row, uint64_t *rows_done)
{
  if (!g || !path) return MPC_E_INVAL;
  group_refresh(g);
  if (const int prc = group_pack_check(g)) return prc;
  if (const int irc = group_image_check(g)) return irc;
  if (const int wrc = group_rewrite_check(g)) return wrc;
  return mpcstage::compress_npy(g->stage, sink_of(g), nullptr, path, first_row, n_rows, skip_last_row, rows_done);
}

int mpc_group_compress_gpgpusim_log(mpc_group *g, const char *log_path, uint64_t *requests_read, uint64_t *lines_done)
{
  if (!g || !log_path) return MPC_E_INVAL;
  group_refresh(g);
  if (const int prc = group_pack_check(g)) return prc;
  if (const int irc = group_image_check(g)) return irc;
  if (const int wrc = group_rewrite_check(g)) return wrc;
  return mpcstage::compress_gpgpusim_log(g->stage, sink_of(g), nullptr, log_path, requests_read, lines_done);
}

int mpc_group_sync(mpc_group *g)
{
  if (!g) return MPC_E_INVAL;
  HIPCHK(g, hipSetDevice(g->stage.device));
  const int rc = mpcstage::finish(g->stage, sink_of(g), nullptr);
  if (rc != MPC_OK) return rc;
  HIPCHK(g, hipDeviceSynchronize());   // batches may have been queued on caller streams
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
  HIPCHK(h, hipMemset(h->d_raw, 0, (h->raw_len + kTestWords) * sizeof(u64)));
  if (h->acct.d_hist) HIPCHK(h, hipMemset(h->acct.d_hist, 0, MPC_SIZE_BINS * sizeof(u64)));
  if (h->acct.on) h->acct.vpc_base.assign(h->acct.vpc_base.size(), 0);
  if (h->cls.d_tab) HIPCHK(h, hipMemset(h->cls.d_tab, 0, MPC_CLASS_TABLE_LEN * sizeof(u64)));
  h->cls.extra.assign(h->cls.extra.size(), 0);
  if (h->pack.d_tab) HIPCHK(h, hipMemset(h->pack.d_tab, 0, MPC_PACK_DEV_LEN * sizeof(u64)));
  h->pack.extra.assign(h->pack.extra.size(), 0);
  h->pack.seen = 0;                   // (the open block goes with the position: its carry is read only behind a launch that wrote it)
  if (h->img.on) {                    // the image, the position and the table (a handle that ran into its capacity never gets here, as a Pattern one)
    HIPCHK(h, hipMemset(h->img.d_keys, 0xff, h->img.slots * sizeof(u64)));
    HIPCHK(h, hipMemset(h->img.d_vals, 0, h->img.slots * sizeof(u64)));
    HIPCHK(h, hipMemset(h->img.d_ctl, 0, MPC_IMAGE_CTL_LEN * sizeof(u64)));
    h->img.seen = 0;
  }
  if (h->rw.on) {                     // the map, the position and the table
    HIPCHK(h, hipMemset(h->rw.d_keys, 0xff, h->rw.slots * sizeof(u64)));
    HIPCHK(h, hipMemset(h->rw.d_vals, 0, h->rw.slots * sizeof(u64)));
    HIPCHK(h, hipMemset(h->rw.d_dev, 0, MPC_REWRITE_DEV_LEN * sizeof(u64)));
    h->rw.seen = 0;
  }
  h->extra.assign(h->stats_len, 0);
  h->sc2.lines = h->sc2.warm = 0;     // SC2: the table and the line counter stay (C-Pack in blocks: the open block and the position in it)
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

// ---- size accounting (include/mpc_hip_sizes.h) ----------------------------------
int mpc_size_hist_enable(mpc_handle *h)
{
  if (!h) return MPC_E_INVAL;
  if (h->acct.on) return MPC_OK;
  if (h->algorithm == Algo::Fit) return set_err(h, MPC_E_INVAL, "Fit: an analysis has no per-line sizes to account");
  HIPCHK(h, hipSetDevice(h->device));
  if (h->algorithm == Algo::VPC) {
    // nothing to allocate: remember the statistics' histogram of the lines before this point
    int rc = sync_all(h);
    if (rc != MPC_OK) return rc;
    HIPCHK(h, hipDeviceSynchronize());
    std::vector<u64> raw(h->raw_len);
    HIPCHK(h, hipMemcpy(raw.data(), h->d_raw, h->raw_len * sizeof(u64), hipMemcpyDeviceToHost));
    vpc_size_hist(h, raw, h->acct.vpc_base);
  } else {
    if (hipMalloc((void **)&h->acct.d_hist, MPC_SIZE_BINS * sizeof(u64)) != hipSuccess) {
      h->acct.d_hist = nullptr;
      return set_err(h, MPC_E_NOMEM, "hipMalloc(size histogram) failed");
    }
    HIPCHK(h, hipMemset(h->acct.d_hist, 0, MPC_SIZE_BINS * sizeof(u64)));
    HIPCHK(h, hipDeviceSynchronize());   // (the kernels run on non-blocking streams)
    h->stage.account[0] = 1;
  }
  h->acct.on = true;
  return MPC_OK;
}

int mpc_size_hist_get(mpc_handle *h, uint64_t *bins, size_t n)
{
  if (!h) return MPC_E_INVAL;
  if (!h->acct.on) return set_err(h, MPC_E_INVAL, "size accounting is not switched on for this handle (mpc_size_hist_enable)");
  if (!bins || n != MPC_SIZE_BINS) return set_err(h, MPC_E_INVAL, "a size histogram has MPC_SIZE_BINS (4096) bins");
  HIPCHK(h, hipSetDevice(h->device));
  int rc = sync_all(h);
  if (rc != MPC_OK) return rc;
  HIPCHK(h, hipDeviceSynchronize());   // callers may have used their own streams
  rc = pattern_status(h);
  if (rc != MPC_OK) return rc;
  if (h->algorithm != Algo::VPC) {
    HIPCHK(h, hipMemcpy(bins, h->acct.d_hist, MPC_SIZE_BINS * sizeof(u64), hipMemcpyDeviceToHost));
    return MPC_OK;
  }
  std::vector<u64> raw(h->raw_len), now;
  HIPCHK(h, hipMemcpy(raw.data(), h->d_raw, h->raw_len * sizeof(u64), hipMemcpyDeviceToHost));
  vpc_size_hist(h, raw, now);
  for (size_t b = 0; b < MPC_SIZE_BINS; b++) bins[b] = now[b] - h->acct.vpc_base[b];
  return MPC_OK;
}

int mpc_group_best_enable(mpc_group *g)
{
  if (!g) return MPC_E_INVAL;
  if (g->best.on) return MPC_OK;
  std::vector<int> set;
  for (int i = 0; i < (int)g->m.size(); i++)
    if (g->m[(size_t)i]->algorithm != Algo::Pattern) set.push_back(i);
  if (set.size() < 2)
    return group_err(g, MPC_E_INVAL, "best-of needs at least two members that take part, this group has " + std::to_string(set.size()) +
                                         " (a Pattern member is an analyser and does not)");
  if (set.size() > MPC_SIZES_MAX)
    return group_err(g, MPC_E_INVAL, "best-of takes at most " + std::to_string(MPC_SIZES_MAX) + " members, this group has " + std::to_string(set.size()));
  HIPCHK(g, hipSetDevice(g->stage.device));
  if (hipMalloc((void **)&g->best.d_acc, MPC_SIZES_BEST_LEN * sizeof(u64)) != hipSuccess) {
    g->best.d_acc = nullptr;
    return group_err(g, MPC_E_NOMEM, "hipMalloc(best-of accumulators) failed");
  }
  HIPCHK(g, hipMemset(g->best.d_acc, 0, MPC_SIZES_BEST_LEN * sizeof(u64)));
  HIPCHK(g, hipDeviceSynchronize());   // (the kernels run on non-blocking streams)
  g->best.set = std::move(set);
  g->best.on = true;
  return group_class_best_ensure(g);
}

int mpc_group_best_get(mpc_group *g, uint64_t *bins, size_t n, uint64_t *wins, size_t n_members, uint64_t *best_bits, uint64_t *lines)
{
  if (!g) return MPC_E_INVAL;
  if (!g->best.on) return group_err(g, MPC_E_INVAL, "best-of is not switched on for this group (mpc_group_best_enable)");
  if ((bins && n != MPC_SIZE_BINS) || (wins && n_members != g->m.size()))
    return group_err(g, MPC_E_INVAL, "best-of: bins has MPC_SIZE_BINS (4096) entries, wins one per group member");
  int rc = mpc_group_sync(g);
  if (rc != MPC_OK) return rc;
  std::vector<u64> acc(MPC_SIZES_BEST_LEN);
  HIPCHK(g, hipMemcpy(acc.data(), g->best.d_acc, acc.size() * sizeof(u64), hipMemcpyDeviceToHost));
  u64 total = 0;
  for (size_t b = 0; b < MPC_SIZE_BINS; b++) total += acc[b];
  if (bins) std::memcpy(bins, acc.data(), MPC_SIZE_BINS * sizeof(u64));
  if (wins) {
    std::fill(wins, wins + n_members, 0);
    for (size_t k = 0; k < g->best.set.size(); k++) wins[g->best.set[k]] = acc[MPC_SIZES_WINS + k];
  }
  if (best_bits) *best_bits = acc[MPC_SIZES_BITS];
  if (lines) *lines = total;
  return MPC_OK;
}

int mpc_group_best_reset(mpc_group *g)
{
  if (!g) return MPC_E_INVAL;
  if (!g->best.on) return group_err(g, MPC_E_INVAL, "best-of is not switched on for this group (mpc_group_best_enable)");
  const int rc = mpc_group_sync(g);
  if (rc != MPC_OK) return rc;
  HIPCHK(g, hipMemset(g->best.d_acc, 0, MPC_SIZES_BEST_LEN * sizeof(u64)));
  if (g->cls.d_best) HIPCHK(g, hipMemset(g->cls.d_best, 0, MPC_CLASS_TABLE_LEN * sizeof(u64)));
  if (g->pack.d_best) HIPCHK(g, hipMemset(g->pack.d_best, 0, MPC_PACK_DEV_LEN * sizeof(u64)));
  g->pack.best_seen = 0;
  return MPC_OK;
}

int mpc_size_sectors(const uint64_t *bins, size_t n, unsigned line_size, unsigned sector_bytes, uint64_t *classes, size_t n_classes,
                     uint64_t *total_sectors, double *ratio)
{
  if (!bins || n != MPC_SIZE_BINS || sector_bytes == 0 || sector_bytes > line_size) return MPC_E_INVAL;
  const u64 most = ((u64)line_size + sector_bytes - 1) / sector_bytes, sector_bits = 8ull * sector_bytes;
  if (classes && n_classes != most) return MPC_E_INVAL;
  std::vector<u64> cls(most, 0);
  u64 lines = 0, sectors = 0;
  for (u64 s = 0; s < MPC_SIZE_BINS; s++) {
    const u64 c = std::min(std::max<u64>(1, (s + sector_bits - 1) / sector_bits), most);
    cls[c - 1] += bins[s];
    lines += bins[s];
    sectors += bins[s] * c;
  }
  if (classes) std::memcpy(classes, cls.data(), most * sizeof(u64));
  if (total_sectors) *total_sectors = sectors;
  if (ratio) *ratio = sectors ? (double)(lines * most) / (double)sectors : 0.0;
  return MPC_OK;
}


// ---- pack accounting (include/mpc_hip_pack.h) ------------------------------------
namespace {
const char *const kPackOff = "pack accounting is not switched on for this handle (mpc_pack_stats_enable)";
const char *const kGroupPackOff = "pack accounting is not switched on for this group (mpc_group_pack_stats_enable)";
const char *const kPackTableLen = "a pack table has MPC_PACK_TABLE_LEN (8 + 1024 = 1032) entries";

u64 pack_sectors_of(u64 bits, u64 sector_bytes, u64 cap)
{
  return std::min(std::max<u64>(1, (bits + 8 * sector_bytes - 1) / (8 * sector_bytes)), cap);
}
}  // namespace

int mpc_pack_check_values(unsigned line_size, uint64_t block_lines, unsigned sector_bytes, unsigned header_bits)
{
  const std::string why = line_size == 0 ? std::string("pack accounting: line_size must be at least 1") : pack_refusal(line_size, block_lines, sector_bytes, header_bits);
  return why.empty() ? MPC_OK : set_err(nullptr, MPC_E_INVAL, why);
}

int mpc_pack_stats_enable(mpc_handle *h, uint64_t block_lines, unsigned sector_bytes, unsigned header_bits)
{
  if (!h) return MPC_E_INVAL;
  if (h->algorithm == Algo::Fit) return set_err(h, MPC_E_INVAL, "Fit: an analysis has no per-line sizes to account");
  const std::string why = pack_refusal((unsigned)h->L, block_lines, sector_bytes, header_bits);
  if (!why.empty()) return set_err(h, MPC_E_INVAL, why);
  auto &P = h->pack;
  if (P.on) {
    if (P.N == block_lines && P.sector_bytes == sector_bytes && P.header_bits == header_bits) return MPC_OK;
    return set_err(h, MPC_E_INVAL, "pack accounting is already on with " + pack_values(P.N, P.sector_bytes, P.header_bits));
  }
  HIPCHK(h, hipSetDevice(h->device));
  if (hipMalloc((void **)&P.d_tab, MPC_PACK_DEV_LEN * sizeof(u64)) != hipSuccess) {
    P.d_tab = nullptr;
    return set_err(h, MPC_E_NOMEM, "hipMalloc(pack table) failed");
  }
  if (!P.d_carry && hipMalloc((void **)&P.d_carry, 2 * sizeof(uint32_t)) != hipSuccess) {
    P.d_carry = nullptr;
    (void)hipFree(P.d_tab);
    P.d_tab = nullptr;
    return set_err(h, MPC_E_NOMEM, "hipMalloc(pack carry) failed");
  }
  HIPCHK(h, hipMemset(P.d_tab, 0, MPC_PACK_DEV_LEN * sizeof(u64)));
  HIPCHK(h, hipMemset(P.d_carry, 0, 2 * sizeof(uint32_t)));
  if (!P.done) HIPCHK(h, hipEventCreateWithFlags(&P.done, hipEventDisableTiming));
  HIPCHK(h, hipDeviceSynchronize());   // (the kernels run on non-blocking streams)
  P.extra.assign(MPC_PACK_DEV_LEN, 0);
  P.N = block_lines;
  P.sector_bytes = sector_bytes;
  P.header_bits = header_bits;
  P.seen = 0;
  P.cur = 0;
  P.recorded = false;
  h->stage.account[0] = 1;
  P.on = true;
  return MPC_OK;
}

int mpc_pack_stats_get(mpc_handle *h, uint64_t *table, size_t n)
{
  if (!h) return MPC_E_INVAL;
  if (!h->pack.on) return set_err(h, MPC_E_INVAL, kPackOff);
  if (!table || n != MPC_PACK_TABLE_LEN) return set_err(h, MPC_E_INVAL, kPackTableLen);
  HIPCHK(h, hipSetDevice(h->device));
  int rc = sync_all(h);
  if (rc != MPC_OK) return rc;
  HIPCHK(h, hipDeviceSynchronize());   // callers may have used their own streams
  rc = pattern_status(h);
  if (rc != MPC_OK) return rc;
  const auto &P = h->pack;
  std::vector<u64> dev(MPC_PACK_DEV_LEN);
  HIPCHK(h, hipMemcpy(dev.data(), P.d_tab, MPC_PACK_DEV_LEN * sizeof(u64), hipMemcpyDeviceToHost));
  for (size_t i = 0; i < dev.size(); i++) dev[i] += P.extra[i];
  uint32_t open_bits = 0;
  if (P.seen % P.N) HIPCHK(h, hipMemcpy(&open_bits, P.d_carry + P.cur, sizeof(open_bits), hipMemcpyDeviceToHost));
  pack_table_out(dev, P.N, (unsigned)h->L, P.sector_bytes, P.header_bits, P.seen % P.N, open_bits, table);
  return MPC_OK;
}

int mpc_pack_stats_merge(mpc_handle *h, const uint64_t *table, size_t n)
{
  if (!h) return MPC_E_INVAL;
  auto &P = h->pack;
  if (!P.on) return set_err(h, MPC_E_INVAL, kPackOff);
  if (!table || n != MPC_PACK_TABLE_LEN) return set_err(h, MPC_E_INVAL, kPackTableLen);
  if (table[5] != P.N || table[6] != P.sector_bytes || table[7] != P.header_bits)
    return set_err(h, MPC_E_INVAL, "pack accounting: the table counts with other values than this handle (" + pack_values(P.N, P.sector_bytes, P.header_bits) + ")");
  if (table[3] >= P.N || table[4] > 0xffffffffull) return set_err(h, MPC_E_INVAL, "pack accounting: the table's open block is not one of this block size");
  if (table[3] && P.seen % P.N)
    return set_err(h, MPC_E_INVAL, "pack accounting: both sides have an open block (" + std::to_string(P.seen % P.N) + " and " + std::to_string(table[3]) +
                                       " lines); cut shards at multiples of block_lines, so that only the last has a tail");
  if (table[3]) {       // take the shard's open block over: the next line continues it
    HIPCHK(h, hipSetDevice(h->device));
    const int rc = sync_all(h);
    if (rc != MPC_OK) return rc;
    HIPCHK(h, hipDeviceSynchronize());
    const uint32_t bits = (uint32_t)table[4];
    HIPCHK(h, hipMemcpy(P.d_carry + P.cur, &bits, sizeof(bits), hipMemcpyHostToDevice));
    P.seen += table[3];
  }
  P.extra[0] += table[1];
  for (size_t k = 1; k <= MPC_PACK_MAX_SECTORS; k++) P.extra[k] += table[8 + k - 1];
  return MPC_OK;
}

int mpc_pack_sectors_of_tail(const uint64_t *table, size_t n, unsigned line_size, uint64_t *tail_sectors, uint64_t *tail_cap)
{
  if (!table || n != MPC_PACK_TABLE_LEN || line_size == 0 || table[6] == 0 || table[5] == 0 || table[3] >= table[5]) return MPC_E_INVAL;
  u64 sectors = 0, cap = 0;
  if (table[3]) {
    cap = (table[3] * (u64)line_size + table[6] - 1) / table[6];
    sectors = pack_sectors_of(table[4] + table[7], table[6], cap);
  }
  if (tail_sectors) *tail_sectors = sectors;
  if (tail_cap) *tail_cap = cap;
  return MPC_OK;
}

int mpc_group_pack_stats_enable(mpc_group *g, uint64_t block_lines, unsigned sector_bytes, unsigned header_bits)
{
  if (!g) return MPC_E_INVAL;
  const std::string why = pack_refusal((unsigned)g->stage.L, block_lines, sector_bytes, header_bits);
  if (!why.empty()) return group_err(g, MPC_E_INVAL, why);
  auto &G = g->pack;
  if (G.on) {
    if (G.N == block_lines && G.sector_bytes == sector_bytes && G.header_bits == header_bits) return MPC_OK;
    return group_err(g, MPC_E_INVAL, "pack accounting is already on with " + pack_values(G.N, G.sector_bytes, G.header_bits));
  }
  // every member fresh (it starts at line 0), or on with the same values; then all at one line
  bool first = true;
  u64 at = 0;
  for (size_t i = 0; i < g->m.size(); i++) {
    const auto &P = g->m[i]->pack;
    if (g->m[i]->algorithm == Algo::Fit) return group_err(g, MPC_E_INVAL, "Fit: an analysis has no per-line sizes to account");
    if (P.on && (P.N != block_lines || P.sector_bytes != sector_bytes || P.header_bits != header_bits))
      return group_err(g, MPC_E_INVAL, "pack accounting: member " + std::to_string(i) + " already counts with " + pack_values(P.N, P.sector_bytes, P.header_bits));
    const u64 seen = P.on ? P.seen : 0;
    if (!first && seen != at)
      return group_err(g, MPC_E_INVAL, "pack accounting: member " + std::to_string(i) + " is at line " + std::to_string(seen) + ", the members before it at line " +
                                           std::to_string(at) + " (reset the members first)");
    at = seen;
    first = false;
  }
  if (g->best.on && at % block_lines)
    return group_err(g, MPC_E_INVAL, "pack accounting: the members are " + std::to_string(at % block_lines) +
                                         " lines into a block, where the table of the best-of cannot begin (reset the members first)");
  for (size_t i = 0; i < g->m.size(); i++) {
    const int rc = mpc_pack_stats_enable(g->m[i], block_lines, sector_bytes, header_bits);
    if (rc != MPC_OK) return group_err(g, rc, "member " + std::to_string(i) + " (" + algorithm_name(g->m[i]->algorithm) + "): " + g->m[i]->error);
  }
  if (g->best.on) {
    unsigned tag_bits = 0;
    while ((1u << tag_bits) < g->best.set.size()) tag_bits++;
    HIPCHK(g, hipSetDevice(g->stage.device));
    if (hipMalloc((void **)&G.d_best, MPC_PACK_DEV_LEN * sizeof(u64)) != hipSuccess) {
      G.d_best = nullptr;
      return group_err(g, MPC_E_NOMEM, "hipMalloc(pack table of the best-of) failed");
    }
    if (!G.d_carry) HIPCHK(g, hipMalloc((void **)&G.d_carry, 2 * sizeof(uint32_t)));
    HIPCHK(g, hipMemset(G.d_best, 0, MPC_PACK_DEV_LEN * sizeof(u64)));
    HIPCHK(g, hipMemset(G.d_carry, 0, 2 * sizeof(uint32_t)));
    if (!G.done) HIPCHK(g, hipEventCreateWithFlags(&G.done, hipEventDisableTiming));
    HIPCHK(g, hipDeviceSynchronize());   // (the kernels run on non-blocking streams)
    G.best_header_bits = header_bits + (unsigned)block_lines * tag_bits;
    G.best_seen = at;
    G.cur = 0;
    G.recorded = false;
  }
  G.N = block_lines;
  G.sector_bytes = sector_bytes;
  G.header_bits = header_bits;
  G.on = true;
  return MPC_OK;
}

int mpc_group_pack_stats_get(mpc_group *g, int member, uint64_t *table, size_t n)
{
  if (!g) return MPC_E_INVAL;
  auto &G = g->pack;
  if (!G.on) return group_err(g, MPC_E_INVAL, kGroupPackOff);
  if (!table || n != MPC_PACK_TABLE_LEN) return group_err(g, MPC_E_INVAL, kPackTableLen);
  if (member != MPC_PACK_BEST && (member < 0 || member >= (int)g->m.size()))
    return group_err(g, MPC_E_INVAL, "pack accounting: member " + std::to_string(member) + " is not a member of the group or MPC_PACK_BEST");
  if (member == MPC_PACK_BEST && !G.d_best)
    return group_err(g, MPC_E_INVAL, "pack accounting: the best-of was not on when the group's pack accounting was switched on (mpc_group_best_enable first)");
  int rc = mpc_group_sync(g);
  if (rc != MPC_OK) return rc;
  if (member == MPC_PACK_BEST) {
    std::vector<u64> dev(MPC_PACK_DEV_LEN);
    HIPCHK(g, hipMemcpy(dev.data(), G.d_best, MPC_PACK_DEV_LEN * sizeof(u64), hipMemcpyDeviceToHost));
    uint32_t open_bits = 0;
    if (G.best_seen % G.N) HIPCHK(g, hipMemcpy(&open_bits, G.d_carry + G.cur, sizeof(open_bits), hipMemcpyDeviceToHost));
    pack_table_out(dev, G.N, (unsigned)g->stage.L, G.sector_bytes, G.best_header_bits, G.best_seen % G.N, open_bits, table);
    return MPC_OK;
  }
  mpc_handle *h = g->m[(size_t)member];
  rc = mpc_pack_stats_get(h, table, n);
  return rc == MPC_OK ? rc : group_err(g, rc, "member " + std::to_string(member) + " (" + algorithm_name(h->algorithm) + "): " + h->error);
}

// ---- image accounting (include/mpc_hip_image.h) ----------------------------------
namespace {
const char *const kImageOff = "image accounting is not switched on for this handle (mpc_image_stats_enable)";
const char *const kGroupImageOff = "image accounting is not switched on for this group (mpc_group_image_stats_enable)";
const char *const kImageTableLen = "an image table has MPC_IMAGE_TABLE_LEN (16 + 1024 = 1040) entries";

}  // namespace

uint64_t mpc_image_hash(uint64_t key) { return mpc_image_mix(key); }

int mpc_image_check_values(unsigned line_size, uint64_t capacity_lines, uint64_t block_lines, unsigned sector_bytes, unsigned header_bits)
{
  const std::string why = line_size == 0 ? std::string("image accounting: line_size must be at least 1")
                                         : image_refusal_of(line_size, capacity_lines, block_lines, sector_bytes, header_bits);
  return why.empty() ? MPC_OK : set_err(nullptr, MPC_E_INVAL, why);
}

int mpc_image_stats_enable(mpc_handle *h, uint64_t capacity_lines, uint64_t block_lines, unsigned sector_bytes, unsigned header_bits)
{
  if (!h) return MPC_E_INVAL;
  if (h->algorithm == Algo::Fit) return set_err(h, MPC_E_INVAL, "Fit: an analysis has no per-line sizes to account");
  const std::string why = image_refusal_of((unsigned)h->L, capacity_lines, block_lines, sector_bytes, header_bits);
  if (!why.empty()) return set_err(h, MPC_E_INVAL, why);
  auto &I = h->img;
  if (I.on) {
    if (I.capacity == capacity_lines && I.N == block_lines && I.sector_bytes == sector_bytes && I.header_bits == header_bits) return MPC_OK;
    return set_err(h, MPC_E_INVAL, "image accounting is already on with " + image_values(I.capacity, I.N, I.sector_bytes, I.header_bits));
  }
  HIPCHK(h, hipSetDevice(h->device));
  const u64 slots = image_slots(capacity_lines);
  if (hipMalloc((void **)&I.d_keys, 2 * slots * sizeof(u64)) != hipSuccess) {        // keys | vals
    I.d_keys = nullptr;
    return set_err(h, MPC_E_NOMEM, "hipMalloc(image table, " + std::to_string(2 * slots * sizeof(u64)) + " bytes) failed");
  }
  // (the counters, then the 8 KiB table of a get's pass, which a handle that is polled then does not allocate per get)
  if (!I.d_ctl && hipMalloc((void **)&I.d_ctl, (MPC_IMAGE_CTL_LEN + MPC_IMAGE_OUT_LEN) * sizeof(u64)) != hipSuccess) {
    I.d_ctl = nullptr;
    (void)hipFree(I.d_keys);
    I.d_keys = nullptr;
    return set_err(h, MPC_E_NOMEM, "hipMalloc(image counters) failed");
  }
  I.d_vals = I.d_keys + slots;
  hipError_t e = hipMemset(I.d_keys, 0xff, slots * sizeof(u64));
  if (e == hipSuccess) e = hipMemset(I.d_vals, 0, slots * sizeof(u64));
  if (e == hipSuccess) e = hipMemset(I.d_ctl, 0, MPC_IMAGE_CTL_LEN * sizeof(u64));
  if (e == hipSuccess) e = hipDeviceSynchronize();   // (the kernels run on non-blocking streams)
  if (e != hipSuccess) {               // the table does not stay behind a failed enable (mpc_destroy frees the counters)
    (void)hipFree(I.d_keys);
    I.d_keys = I.d_vals = nullptr;
    return set_err(h, MPC_E_HIP, std::string("image accounting: clearing the table: ") + hipGetErrorString(e));
  }
  I.hash_mask = ~0ull;
#if MPC_TESTING
  // chains through most of the table at any capacity: keep only the low bits of the hash
  if (const char *e = getenv("MPC_TEST_IMAGE_HASH_BITS")) {
    const long bits = atol(e);
    if (bits >= 0 && bits < 64) I.hash_mask = (1ull << bits) - 1ull;
  }
#endif
  I.capacity = capacity_lines;
  I.N = block_lines;
  I.sector_bytes = sector_bytes;
  I.header_bits = header_bits;
  I.slots = slots;
  I.seen = 0;
  I.over = false;
  h->stage.account[0] = 1;
  h->stage.log_addrs = true;
  I.on = true;
  return MPC_OK;
}

int mpc_image_stats_get(mpc_handle *h, uint64_t *table, size_t n)
{
  if (!h) return MPC_E_INVAL;
  if (!h->img.on) return set_err(h, MPC_E_INVAL, kImageOff);
  if (!table || n != MPC_IMAGE_TABLE_LEN) return set_err(h, MPC_E_INVAL, kImageTableLen);
  HIPCHK(h, hipSetDevice(h->device));
  int rc = sync_all(h);
  if (rc != MPC_OK) return rc;
  HIPCHK(h, hipDeviceSynchronize());   // callers may have used their own streams
  rc = pattern_status(h);
  if (rc != MPC_OK) return rc;
  const auto &I = h->img;
  const u64 *ctl = I.ctl;              // (image_status has just read the counters, with the work complete)
  std::vector<u64> out(MPC_IMAGE_OUT_LEN, 0);
  const u64 D = ctl[MPC_IMAGE_CTL_KEYS];
  const u64 S = (I.N * (u64)h->L + I.sector_bytes - 1) / I.sector_bytes;
  if (D) {
    // the block map lives for this get only: at most D blocks are touched
    const u64 bslots = image_slots(D);
    u64 *d_map = nullptr, *d_out = I.d_ctl + MPC_IMAGE_CTL_LEN;
    if (hipMalloc((void **)&d_map, 2 * bslots * sizeof(u64)) != hipSuccess)
      return set_err(h, MPC_E_NOMEM, "hipMalloc(image block map, " + std::to_string(2 * bslots * sizeof(u64)) + " bytes) failed");
    MpcImageGetArgs A{};
    A.keys = I.d_keys;
    A.vals = I.d_vals;
    A.slots = I.slots;
    A.bkeys = d_map;
    A.bvals = d_map + bslots;
    A.bmask = bslots - 1;
    A.hash_mask = I.hash_mask;
    A.block_lines = I.N;
    A.out = d_out;
    A.line_size = (unsigned)h->L;
    A.sector_bytes = I.sector_bytes;
    A.header_bits = I.header_bits;
    A.max_sectors = (unsigned)S;
    hipError_t e = hipMemsetAsync(A.bkeys, 0xff, bslots * sizeof(u64), h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(A.bvals, 0, bslots * sizeof(u64), h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(d_out, 0, MPC_IMAGE_OUT_LEN * sizeof(u64), h->stream);
    if (e == hipSuccess) e = mpc_launch_image_get(&A, grid_for(h, I.slots, 256, 8), h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(out.data(), d_out, MPC_IMAGE_OUT_LEN * sizeof(u64), hipMemcpyDeviceToHost, h->stream);
    const hipError_t e2 = hipStreamSynchronize(h->stream);
    (void)hipFree(d_map);
    if (e != hipSuccess || e2 != hipSuccess)
      return set_err(h, MPC_E_HIP, std::string("image accounting, get pass: ") + hipGetErrorString(e != hipSuccess ? e : e2));
    if (out[MPC_IMAGE_OUT_FULL]) return set_err(h, MPC_E_HIP, "image accounting: the block map of a get is full (internal error)");
  }
  std::fill(table, table + MPC_IMAGE_TABLE_LEN, 0);
  table[0] = ctl[MPC_IMAGE_CTL_LINES];
  table[1] = ctl[MPC_IMAGE_CTL_BITS];
  table[2] = D;
  table[3] = out[MPC_IMAGE_OUT_LATEST];
  table[6] = out[MPC_IMAGE_OUT_CAPS];
  table[7] = ctl[MPC_IMAGE_CTL_MISALIGNED];
  table[8] = I.N;
  table[9] = I.sector_bytes;
  table[10] = I.header_bits;
  table[11] = I.capacity;
  for (u64 k = 1; k <= S; k++) {
    const u64 v = out[MPC_IMAGE_OUT_HIST + k - 1];
    table[16 + k - 1] = v;
    table[4] += v;
    table[5] += v * k;
  }
  return MPC_OK;
}

int mpc_compress_batch_addressed(mpc_handle *h, const uint8_t *lines, uint64_t n, const uint64_t *addresses, uint16_t *sizes, int8_t *sel)
{
  if (!h || (!lines && n) || (!addresses && n)) return MPC_E_INVAL;
  if (!h->img.on && !h->rw.on) return set_err(h, MPC_E_INVAL, kImageOff);
  if (n == 0) return MPC_OK;
  return mpcstage::compress_batch(h->stage, sink_of(h), h->stream, lines, n, nullptr, addresses, &sizes, &sel);
}

int mpc_compress_batch_device_addressed(mpc_handle *h, const void *d_lines, uint64_t n, const uint64_t *d_addresses, uint16_t *d_sizes, int8_t *d_sel,
                                        void *hip_stream)
{
  if (!h || (!d_addresses && n)) return MPC_E_INVAL;
  if (!h->img.on && !h->rw.on) return set_err(h, MPC_E_INVAL, kImageOff);
  if (((uintptr_t)d_addresses) & 7u) return set_err(h, MPC_E_INVAL, "device address buffer must be 8-byte aligned");
  return batch_device(h, d_lines, n, nullptr, d_addresses, d_sizes, d_sel, hip_stream);
}

int mpc_group_image_stats_enable(mpc_group *g, uint64_t capacity_lines, uint64_t block_lines, unsigned sector_bytes, unsigned header_bits)
{
  if (!g) return MPC_E_INVAL;
  const std::string why = image_refusal_of((unsigned)g->stage.L, capacity_lines, block_lines, sector_bytes, header_bits);
  if (!why.empty()) return group_err(g, MPC_E_INVAL, why);
  auto &G = g->img;
  if (G.on) {
    if (G.capacity == capacity_lines && G.N == block_lines && G.sector_bytes == sector_bytes && G.header_bits == header_bits) return MPC_OK;
    return group_err(g, MPC_E_INVAL, "image accounting is already on with " + image_values(G.capacity, G.N, G.sector_bytes, G.header_bits));
  }
  // every member fresh (it starts at line 0), or on with the same values; then all at one line
  bool first = true;
  u64 at = 0;
  for (size_t i = 0; i < g->m.size(); i++) {
    const auto &I = g->m[i]->img;
    if (g->m[i]->algorithm == Algo::Fit) return group_err(g, MPC_E_INVAL, "Fit: an analysis has no per-line sizes to account");
    if (I.on && (I.capacity != capacity_lines || I.N != block_lines || I.sector_bytes != sector_bytes || I.header_bits != header_bits))
      return group_err(g, MPC_E_INVAL, "image accounting: member " + std::to_string(i) + " already counts with " + image_values(I.capacity, I.N, I.sector_bytes, I.header_bits));
    const u64 seen = I.on ? I.seen : 0;
    if (!first && seen != at)
      return group_err(g, MPC_E_INVAL, "image accounting: member " + std::to_string(i) + " is at line " + std::to_string(seen) + ", the members before it at line " +
                                           std::to_string(at) + " (reset the members first)");
    at = seen;
    first = false;
  }
  for (size_t i = 0; i < g->m.size(); i++) {
    const int rc = mpc_image_stats_enable(g->m[i], capacity_lines, block_lines, sector_bytes, header_bits);
    if (rc != MPC_OK) return group_err(g, rc, "member " + std::to_string(i) + " (" + algorithm_name(g->m[i]->algorithm) + "): " + g->m[i]->error);
  }
  G.capacity = capacity_lines;
  G.N = block_lines;
  G.sector_bytes = sector_bytes;
  G.header_bits = header_bits;
  G.on = true;
  return MPC_OK;
}

int mpc_group_image_stats_get(mpc_group *g, int member, uint64_t *table, size_t n)
{
  if (!g) return MPC_E_INVAL;
  if (!g->img.on) return group_err(g, MPC_E_INVAL, kGroupImageOff);
  if (!table || n != MPC_IMAGE_TABLE_LEN) return group_err(g, MPC_E_INVAL, kImageTableLen);
  if (member < 0 || member >= (int)g->m.size())
    return group_err(g, MPC_E_INVAL, "image accounting: member " + std::to_string(member) + " is not a member of the group");
  int rc = mpc_group_sync(g);
  if (rc != MPC_OK) return rc;
  mpc_handle *h = g->m[(size_t)member];
  rc = mpc_image_stats_get(h, table, n);
  return rc == MPC_OK ? rc : group_err(g, rc, "member " + std::to_string(member) + " (" + algorithm_name(h->algorithm) + "): " + h->error);
}

int mpc_group_compress_batch_addressed(mpc_group *g, const uint8_t *lines, uint64_t n, const uint64_t *addresses, uint16_t *const *sizes,
                                       int8_t *const *sel)
{
  if (!g || (!lines && n) || (!addresses && n)) return MPC_E_INVAL;
  if (!g->img.on && !g->rw.on) return group_err(g, MPC_E_INVAL, kGroupImageOff);
  if (n == 0) return MPC_OK;
  group_refresh(g);
  if (const int prc = group_pack_check(g)) return prc;
  if (const int irc = group_image_check(g)) return irc;
  if (const int wrc = group_rewrite_check(g)) return wrc;
  return mpcstage::compress_batch(g->stage, sink_of(g), nullptr, lines, n, nullptr, addresses, sizes, sel);
}

int mpc_group_compress_batch_device_addressed(mpc_group *g, const void *d_lines, uint64_t n, const uint64_t *d_addresses, uint16_t *const *d_sizes,
                                              int8_t *const *d_sel, void *hip_stream)
{
  if (!g || (!d_addresses && n)) return MPC_E_INVAL;
  if (!g->img.on && !g->rw.on) return group_err(g, MPC_E_INVAL, kGroupImageOff);
  if (((uintptr_t)d_addresses) & 7u) return group_err(g, MPC_E_INVAL, "device address buffer must be 8-byte aligned");
  group_refresh(g);
  return group_batch_device(g, d_lines, n, nullptr, d_addresses, d_sizes, d_sel, hip_stream);
}

// ---- rewrite accounting (include/mpc_hip_rewrite.h) --------------------------------
namespace {
const char *const kRewriteOff = "rewrite accounting is not switched on for this handle (mpc_rewrite_stats_enable)";
const char *const kGroupRewriteOff = "rewrite accounting is not switched on for this group (mpc_group_rewrite_stats_enable)";
const char *const kRewriteTableLen = "a rewrite table has MPC_REWRITE_TABLE_LEN (144 + 32 x 32 = 1168) entries";

}  // namespace

int mpc_rewrite_check_values(unsigned line_size, uint64_t capacity_lines, unsigned granule_bytes)
{
  const std::string why = line_size == 0 ? std::string("rewrite accounting: line_size must be at least 1") : rewrite_refusal_of(line_size, capacity_lines, granule_bytes);
  return why.empty() ? MPC_OK : set_err(nullptr, MPC_E_INVAL, why);
}

int mpc_rewrite_stats_enable(mpc_handle *h, uint64_t capacity_lines, unsigned granule_bytes)
{
  if (!h) return MPC_E_INVAL;
  if (h->algorithm == Algo::Fit) return set_err(h, MPC_E_INVAL, "Fit: an analysis has no per-line sizes to account");
  const std::string why = rewrite_refusal_of((unsigned)h->L, capacity_lines, granule_bytes);
  if (!why.empty()) return set_err(h, MPC_E_INVAL, why);
  auto &R = h->rw;
  if (R.on) {
    if (R.capacity == capacity_lines && R.granule == granule_bytes) return MPC_OK;
    return set_err(h, MPC_E_INVAL, "rewrite accounting is already on with " + rewrite_values(R.capacity, R.granule));
  }
  HIPCHK(h, hipSetDevice(h->device));
  u64 batch = MPC_REWRITE_BATCH;
  R.hash_mask = ~0ull;
#if MPC_TESTING
  // chains through most of the table at any capacity: keep only the low bits of the hash; sub-batch seams inside small calls
  if (const char *e = getenv("MPC_TEST_REWRITE_HASH_BITS")) {
    const long bits = atol(e);
    if (bits >= 0 && bits < 64) R.hash_mask = (1ull << bits) - 1ull;
  }
  if (const char *e = getenv("MPC_TEST_REWRITE_BATCH")) {
    const long long v = atoll(e);
    if (v >= 1 && (u64)v <= MPC_REWRITE_BATCH) batch = (u64)v;
  }
#endif
  const u64 slots = image_slots(capacity_lines);
  size_t scratch_bytes = 0;
  hipError_t e = mpc_rewrite_scratch_bytes(batch, &scratch_bytes);
  if (e != hipSuccess) return set_err(h, MPC_E_HIP, std::string("rewrite accounting: sizing the scratch of a sub-batch: ") + hipGetErrorString(e));
  auto give_up = [&](int code, const std::string &msg) {       // nothing stays behind a failed enable
    if (R.d_keys) (void)hipFree(R.d_keys);
    if (R.d_dev) (void)hipFree(R.d_dev);
    if (R.d_scratch) (void)hipFree(R.d_scratch);
    if (R.done) (void)hipEventDestroy(R.done);
    R.d_keys = R.d_vals = R.d_dev = nullptr;
    R.d_scratch = nullptr;
    R.done = nullptr;
    return set_err(h, code, msg);
  };
  if (hipMalloc((void **)&R.d_keys, 2 * slots * sizeof(u64)) != hipSuccess) {        // keys | vals
    R.d_keys = nullptr;
    return give_up(MPC_E_NOMEM, "hipMalloc(rewrite map, " + std::to_string(2 * slots * sizeof(u64)) + " bytes) failed");
  }
  if (hipMalloc((void **)&R.d_dev, MPC_REWRITE_DEV_LEN * sizeof(u64)) != hipSuccess) {
    R.d_dev = nullptr;
    return give_up(MPC_E_NOMEM, "hipMalloc(rewrite counters) failed");
  }
  if (hipMalloc(&R.d_scratch, scratch_bytes) != hipSuccess) {
    R.d_scratch = nullptr;
    return give_up(MPC_E_NOMEM, "hipMalloc(rewrite scratch, " + std::to_string(scratch_bytes) + " bytes) failed");
  }
  R.d_vals = R.d_keys + slots;
  e = mpc_rewrite_scratch_carve(R.d_scratch, batch, &R.scratch);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&R.done, hipEventDisableTiming);
  if (e == hipSuccess) e = hipMemset(R.d_keys, 0xff, slots * sizeof(u64));
  if (e == hipSuccess) e = hipMemset(R.d_vals, 0, slots * sizeof(u64));
  if (e == hipSuccess) e = hipMemset(R.d_dev, 0, MPC_REWRITE_DEV_LEN * sizeof(u64));
  if (e == hipSuccess) e = hipDeviceSynchronize();   // (the kernels run on non-blocking streams)
  if (e != hipSuccess) return give_up(MPC_E_HIP, std::string("rewrite accounting: clearing the map: ") + hipGetErrorString(e));
  R.capacity = capacity_lines;
  R.granule = granule_bytes;
  R.G = ((unsigned)h->L + granule_bytes - 1) / granule_bytes;
  R.slots = slots;
  R.batch = batch;
  R.seen = 0;
  R.over = false;
  R.recorded = false;
  h->stage.account[0] = 1;
  h->stage.log_addrs = true;
  R.on = true;
  return MPC_OK;
}

int mpc_rewrite_stats_get(mpc_handle *h, uint64_t *table, size_t n)
{
  if (!h) return MPC_E_INVAL;
  if (!h->rw.on) return set_err(h, MPC_E_INVAL, kRewriteOff);
  if (!table || n != MPC_REWRITE_TABLE_LEN) return set_err(h, MPC_E_INVAL, kRewriteTableLen);
  HIPCHK(h, hipSetDevice(h->device));
  int rc = sync_all(h);
  if (rc != MPC_OK) return rc;
  HIPCHK(h, hipDeviceSynchronize());   // callers may have used their own streams
  rc = pattern_status(h);
  if (rc != MPC_OK) return rc;
  const auto &R = h->rw;
  std::vector<u64> dev(MPC_REWRITE_DEV_LEN, 0);
  {
    const MpcRewriteMap M = rewrite_map(h);
    hipError_t e = hipMemsetAsync(R.d_dev + MPC_REWRITE_DEV_OUT, 0, MPC_REWRITE_OUT_LEN * sizeof(u64), h->stream);
    if (e == hipSuccess) e = mpc_launch_rewrite_get(&M, grid_for(h, R.slots, 256, 8), h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(dev.data(), R.d_dev, MPC_REWRITE_DEV_LEN * sizeof(u64), hipMemcpyDeviceToHost, h->stream);
    const hipError_t e2 = hipStreamSynchronize(h->stream);
    if (e != hipSuccess || e2 != hipSuccess)
      return set_err(h, MPC_E_HIP, std::string("rewrite accounting, get pass: ") + hipGetErrorString(e != hipSuccess ? e : e2));
  }
  const u64 *out = dev.data() + MPC_REWRITE_DEV_OUT;
  std::fill(table, table + MPC_REWRITE_TABLE_LEN, 0);
  table[0] = dev[MPC_REWRITE_CTL_LINES];
  table[1] = dev[MPC_REWRITE_CTL_BITS];
  table[2] = dev[MPC_REWRITE_CTL_KEYS];
  table[3] = dev[MPC_REWRITE_CTL_MISALIGNED];
  table[7] = dev[MPC_REWRITE_CTL_EQUAL];
  table[8] = out[MPC_REWRITE_OUT_LATEST_CLASSES];
  table[9] = out[MPC_REWRITE_OUT_PEAK_CLASSES];
  table[10] = out[MPC_REWRITE_OUT_LATEST_BITS];
  table[11] = out[MPC_REWRITE_OUT_PEAK_BITS];
  table[12] = R.granule;
  table[13] = R.capacity;
  table[14] = R.G;
  for (unsigned c = 0; c < MPC_REWRITE_MAX_CLASSES; c++) {
    table[16 + c] = dev[MPC_REWRITE_DEV_FIRST + c];
    table[48 + c] = out[MPC_REWRITE_OUT_HIST_LATEST + c];
    table[80 + c] = out[MPC_REWRITE_OUT_HIST_PEAK + c];
    table[112 + c] = out[MPC_REWRITE_OUT_HIST_COUNT + c];
    for (unsigned d = 0; d < MPC_REWRITE_MAX_CLASSES; d++) {
      const u64 v = dev[MPC_REWRITE_DEV_TRANS + c * MPC_REWRITE_MAX_CLASSES + d];
      table[144 + c * MPC_REWRITE_MAX_CLASSES + d] = v;
      table[4] += v;
      if (d > c) table[5] += v;
      if (d < c) table[6] += v;
    }
  }
  return MPC_OK;
}

int mpc_group_rewrite_stats_enable(mpc_group *g, uint64_t capacity_lines, unsigned granule_bytes)
{
  if (!g) return MPC_E_INVAL;
  const std::string why = rewrite_refusal_of((unsigned)g->stage.L, capacity_lines, granule_bytes);
  if (!why.empty()) return group_err(g, MPC_E_INVAL, why);
  auto &G = g->rw;
  if (G.on) {
    if (G.capacity == capacity_lines && G.granule == granule_bytes) return MPC_OK;
    return group_err(g, MPC_E_INVAL, "rewrite accounting is already on with " + rewrite_values(G.capacity, G.granule));
  }
  // every member fresh (it starts at line 0), or on with the same values; then all at one line
  bool first = true;
  u64 at = 0;
  for (size_t i = 0; i < g->m.size(); i++) {
    const auto &R = g->m[i]->rw;
    if (g->m[i]->algorithm == Algo::Fit) return group_err(g, MPC_E_INVAL, "Fit: an analysis has no per-line sizes to account");
    if (R.on && (R.capacity != capacity_lines || R.granule != granule_bytes))
      return group_err(g, MPC_E_INVAL, "rewrite accounting: member " + std::to_string(i) + " already counts with " + rewrite_values(R.capacity, R.granule));
    const u64 seen = R.on ? R.seen : 0;
    if (!first && seen != at)
      return group_err(g, MPC_E_INVAL, "rewrite accounting: member " + std::to_string(i) + " is at line " + std::to_string(seen) + ", the members before it at line " +
                                           std::to_string(at) + " (reset the members first)");
    at = seen;
    first = false;
  }
  for (size_t i = 0; i < g->m.size(); i++) {
    const int rc = mpc_rewrite_stats_enable(g->m[i], capacity_lines, granule_bytes);
    if (rc != MPC_OK) return group_err(g, rc, "member " + std::to_string(i) + " (" + algorithm_name(g->m[i]->algorithm) + "): " + g->m[i]->error);
  }
  G.capacity = capacity_lines;
  G.granule = granule_bytes;
  G.on = true;
  return MPC_OK;
}

int mpc_group_rewrite_stats_get(mpc_group *g, int member, uint64_t *table, size_t n)
{
  if (!g) return MPC_E_INVAL;
  if (!g->rw.on) return group_err(g, MPC_E_INVAL, kGroupRewriteOff);
  if (!table || n != MPC_REWRITE_TABLE_LEN) return group_err(g, MPC_E_INVAL, kRewriteTableLen);
  if (member < 0 || member >= (int)g->m.size())
    return group_err(g, MPC_E_INVAL, "rewrite accounting: member " + std::to_string(member) + " is not a member of the group");
  int rc = mpc_group_sync(g);
  if (rc != MPC_OK) return rc;
  mpc_handle *h = g->m[(size_t)member];
  rc = mpc_rewrite_stats_get(h, table, n);
  return rc == MPC_OK ? rc : group_err(g, rc, "member " + std::to_string(member) + " (" + algorithm_name(h->algorithm) + "): " + h->error);
}

// ---- per-class accounting (include/mpc_hip_classes.h) ----------------------------
int mpc_class_stats_enable(mpc_handle *h, unsigned sector_bytes)
{
  if (!h) return MPC_E_INVAL;
  if (h->algorithm == Algo::Fit) return set_err(h, MPC_E_INVAL, "Fit: an analysis has no per-line sizes to account");
  if (const char *why = class_sector_refusal((unsigned)h->L, sector_bytes)) return set_err(h, MPC_E_INVAL, why);
  if (h->cls.on) {
    if (h->cls.sector_bytes == sector_bytes) return MPC_OK;
    return set_err(h, MPC_E_INVAL, "class accounting is already on with sector_bytes " + std::to_string(h->cls.sector_bytes));
  }
  HIPCHK(h, hipSetDevice(h->device));
  if (hipMalloc((void **)&h->cls.d_tab, MPC_CLASS_TABLE_LEN * sizeof(u64)) != hipSuccess) {
    h->cls.d_tab = nullptr;
    return set_err(h, MPC_E_NOMEM, "hipMalloc(class table) failed");
  }
  HIPCHK(h, hipMemset(h->cls.d_tab, 0, MPC_CLASS_TABLE_LEN * sizeof(u64)));
  HIPCHK(h, hipDeviceSynchronize());   // (the kernels run on non-blocking streams)
  h->cls.extra.assign(MPC_CLASS_TABLE_LEN, 0);
  h->cls.sector_bytes = sector_bytes;
  h->stage.account[0] = 1;
  h->cls.on = true;
  return MPC_OK;
}

int mpc_class_stats_get(mpc_handle *h, uint64_t *table, size_t n)
{
  if (!h) return MPC_E_INVAL;
  if (!h->cls.on) return set_err(h, MPC_E_INVAL, kClassesOff);
  if (!table || n != MPC_CLASS_TABLE_LEN) return set_err(h, MPC_E_INVAL, kClassTableLen);
  HIPCHK(h, hipSetDevice(h->device));
  int rc = sync_all(h);
  if (rc != MPC_OK) return rc;
  HIPCHK(h, hipDeviceSynchronize());   // callers may have used their own streams
  rc = pattern_status(h);
  if (rc != MPC_OK) return rc;
  HIPCHK(h, hipMemcpy(table, h->cls.d_tab, MPC_CLASS_TABLE_LEN * sizeof(u64), hipMemcpyDeviceToHost));
  for (size_t i = 0; i < n; i++) table[i] += h->cls.extra[i];
  return MPC_OK;
}

int mpc_class_stats_merge(mpc_handle *h, const uint64_t *table, size_t n)
{
  if (!h) return MPC_E_INVAL;
  if (!h->cls.on) return set_err(h, MPC_E_INVAL, kClassesOff);
  if (!table || n != MPC_CLASS_TABLE_LEN) return set_err(h, MPC_E_INVAL, kClassTableLen);
  for (size_t i = 0; i < n; i++) h->cls.extra[i] += table[i];
  return MPC_OK;
}

int mpc_class_sector_bytes(const mpc_handle *h, unsigned *sector_bytes)
{
  if (!h || !sector_bytes || !h->cls.on) return MPC_E_INVAL;
  *sector_bytes = h->cls.sector_bytes;
  return MPC_OK;
}

int mpc_compress_batch_classed(mpc_handle *h, const uint8_t *lines, uint64_t n, const uint8_t *classes, uint16_t *sizes, int8_t *sel)
{
  if (!h || (!lines && n)) return MPC_E_INVAL;
  if (!h->cls.on) return set_err(h, MPC_E_INVAL, kClassesOff);
  if (n == 0) return MPC_OK;
  return mpcstage::compress_batch(h->stage, sink_of(h), h->stream, lines, n, classes, nullptr, &sizes, &sel);
}

int mpc_compress_batch_device_classed(mpc_handle *h, const void *d_lines, uint64_t n, const uint8_t *d_classes, uint16_t *d_sizes, int8_t *d_sel,
                                      void *hip_stream)
{
  if (!h) return MPC_E_INVAL;
  if (!h->cls.on) return set_err(h, MPC_E_INVAL, kClassesOff);
  return batch_device(h, d_lines, n, d_classes, nullptr, d_sizes, d_sel, hip_stream);
}

int mpc_class_log_field(mpc_handle *h, int field)
{
  if (!h) return MPC_E_INVAL;
  if (!class_log_field_ok(field)) return set_err(h, MPC_E_INVAL, "class accounting: the .log field is one of MPC_CLASS_LOG_NONE, _KERNEL, _RW, _MFTYPE (0 .. 3)");
  if (!h->cls.on) return set_err(h, MPC_E_INVAL, kClassesOff);
  h->stage.log_field = field;
  return MPC_OK;
}

int mpc_group_class_stats_enable(mpc_group *g, unsigned sector_bytes)
{
  if (!g) return MPC_E_INVAL;
  if (const char *why = class_sector_refusal((unsigned)g->stage.L, sector_bytes)) return group_err(g, MPC_E_INVAL, why);
  // (nothing is switched on unless every member can be)
  for (size_t i = 0; i < g->m.size(); i++)
    if (g->m[i]->cls.on && g->m[i]->cls.sector_bytes != sector_bytes)
      return group_err(g, MPC_E_INVAL, "class accounting: member " + std::to_string(i) + " already counts with sector_bytes " +
                                           std::to_string(g->m[i]->cls.sector_bytes));
  for (size_t i = 0; i < g->m.size(); i++) {
    const int rc = mpc_class_stats_enable(g->m[i], sector_bytes);
    if (rc != MPC_OK) return group_err(g, rc, "member " + std::to_string(i) + " (" + algorithm_name(g->m[i]->algorithm) + "): " + g->m[i]->error);
  }
  g->cls.sector_bytes = sector_bytes;
  g->cls.on = true;
  return group_class_best_ensure(g);
}

int mpc_group_class_stats_get(mpc_group *g, int member, uint64_t *table, size_t n)
{
  if (!g) return MPC_E_INVAL;
  if (!g->cls.on) return group_err(g, MPC_E_INVAL, kGroupClassesOff);
  if (!table || n != MPC_CLASS_TABLE_LEN) return group_err(g, MPC_E_INVAL, kClassTableLen);
  if (member != MPC_CLASS_BEST && (member < 0 || member >= (int)g->m.size()))
    return group_err(g, MPC_E_INVAL, "class accounting: member " + std::to_string(member) + " is not a member of the group or MPC_CLASS_BEST");
  if (member == MPC_CLASS_BEST && !g->cls.d_best) return group_err(g, MPC_E_INVAL, "best-of is not switched on for this group (mpc_group_best_enable)");
  int rc = mpc_group_sync(g);
  if (rc != MPC_OK) return rc;
  if (member == MPC_CLASS_BEST) {
    HIPCHK(g, hipMemcpy(table, g->cls.d_best, MPC_CLASS_TABLE_LEN * sizeof(u64), hipMemcpyDeviceToHost));
    return MPC_OK;
  }
  mpc_handle *h = g->m[(size_t)member];
  rc = mpc_class_stats_get(h, table, n);
  return rc == MPC_OK ? rc : group_err(g, rc, "member " + std::to_string(member) + " (" + algorithm_name(h->algorithm) + "): " + h->error);
}

int mpc_group_compress_batch_classed(mpc_group *g, const uint8_t *lines, uint64_t n, const uint8_t *classes, uint16_t *const *sizes,
                                     int8_t *const *sel)
{
  if (!g || (!lines && n)) return MPC_E_INVAL;
  if (!g->cls.on) return group_err(g, MPC_E_INVAL, kGroupClassesOff);
  if (classes && g->cls.from_member >= 0)
    return group_err(g, MPC_E_INVAL, "class accounting: the classes come from member " + std::to_string(g->cls.from_member) + ", the call must not bring its own");
  if (n == 0) return MPC_OK;
  group_refresh(g);
  if (const int prc = group_pack_check(g)) return prc;
  if (const int irc = group_image_check(g)) return irc;
  if (const int wrc = group_rewrite_check(g)) return wrc;
  return mpcstage::compress_batch(g->stage, sink_of(g), nullptr, lines, n, classes, nullptr, sizes, sel);
}

int mpc_group_compress_batch_device_classed(mpc_group *g, const void *d_lines, uint64_t n, const uint8_t *d_classes, uint16_t *const *d_sizes,
                                            int8_t *const *d_sel, void *hip_stream)
{
  if (!g) return MPC_E_INVAL;
  if (!g->cls.on) return group_err(g, MPC_E_INVAL, kGroupClassesOff);
  if (d_classes && g->cls.from_member >= 0)
    return group_err(g, MPC_E_INVAL, "class accounting: the classes come from member " + std::to_string(g->cls.from_member) + ", the call must not bring its own");
  return group_batch_device(g, d_lines, n, d_classes, nullptr, d_sizes, d_sel, hip_stream);
}

int mpc_group_class_log_field(mpc_group *g, int field)
{
  if (!g) return MPC_E_INVAL;
  if (!class_log_field_ok(field)) return group_err(g, MPC_E_INVAL, "class accounting: the .log field is one of MPC_CLASS_LOG_NONE, _KERNEL, _RW, _MFTYPE (0 .. 3)");
  if (!g->cls.on) return group_err(g, MPC_E_INVAL, kGroupClassesOff);
  g->cls.log_field = field;
  return MPC_OK;
}

int mpc_group_class_from_member(mpc_group *g, int member)
{
  if (!g) return MPC_E_INVAL;
  if (!g->cls.on) return group_err(g, MPC_E_INVAL, kGroupClassesOff);
  if (member < -1 || member >= (int)g->m.size())
    return group_err(g, MPC_E_INVAL, "class accounting: member " + std::to_string(member) + " is not a member of the group");
  if (member >= 0) {
    const Algo a = g->m[(size_t)member]->algorithm;
    if (a == Algo::FPC || a == Algo::BPC || a == Algo::CPack)
      return group_err(g, MPC_E_INVAL, std::string("class accounting: member ") + std::to_string(member) + " (" + algorithm_name(a) +
                                           ") has no selected output to take classes from (it is always 0)");
  }
  g->cls.from_member = member;
  return MPC_OK;
}

// ---- snapshots (include/mpc_hip_snapshot.h): the two calls that need a handle's or a group's insides; the snapshot object
// and its kernels are mpc_snapshot.hip ----
namespace {

// the emitted lines of (L, partial), piece by piece through the snapshot's scratch buffer into `feed`, on the snapshot's stream
typedef std::function<int(const void *, u64, const uint64_t *, const uint8_t *, void *)> SnapshotFeed;
int snapshot_pieces(mpc_snapshot *s, unsigned L, int partial, const SnapshotFeed &feed)
{
  uint64_t plan[MPC_SNAPSHOT_TABLE_LEN];
  if (const int rc = mpc_snapshot_plan(s, L, partial, plan)) return rc;
  const u64 n_out = plan[5], piece = (u64)mpc_snapshot_piece_lines();
  for (u64 at = 0; at < n_out; at += piece) {
    const u64 take = std::min<u64>(n_out - at, piece);
    const void *d_lines;
    const uint64_t *d_addrs;
    const uint8_t *d_presence;
    void *stream;
    if (const int rc = mpc_snapshot_piece(s, L, partial, at, take, &d_lines, &d_addrs, &d_presence, &stream)) return rc;
    if (const int rc = feed(d_lines, take, d_addrs, d_presence, stream)) return rc;
  }
  return MPC_OK;
}

}  // namespace

int mpc_snapshot_evaluate(mpc_snapshot *s, mpc_handle *h, unsigned line_size, int partial, int by_presence)
{
  if (!s || !h) return MPC_E_INVAL;
  if ((unsigned)h->L != line_size)
    return mpc_snapshot_fail(s, MPC_E_INVAL, ("snapshot: the evaluator's line size " + std::to_string(h->L) + " differs from the snapshot's lines of " +
                                              std::to_string(line_size) + " bytes").c_str());
  if (h->device != mpc_snapshot_device_of(s)) return mpc_snapshot_fail(s, MPC_E_INVAL, "snapshot: the evaluator is on another device");
  const bool classed = by_presence && h->cls.on;
  int rc = snapshot_pieces(s, line_size, partial, [&](const void *d, u64 n, const uint64_t *da, const uint8_t *dp, void *stream) {
    const int frc = batch_device(h, d, n, classed ? dp : nullptr, (h->img.on || h->rw.on) ? da : nullptr, nullptr, nullptr, stream);
    return frc == MPC_OK ? frc : mpc_snapshot_fail(s, frc, h->error.c_str());
  });
  if (rc != MPC_OK) return rc;
  rc = mpc_sync(h);
  return rc == MPC_OK ? rc : mpc_snapshot_fail(s, rc, h->error.c_str());
}

int mpc_snapshot_evaluate_group(mpc_snapshot *s, mpc_group *g, unsigned line_size, int partial, int by_presence)
{
  if (!s || !g) return MPC_E_INVAL;
  if ((unsigned)g->stage.L != line_size)
    return mpc_snapshot_fail(s, MPC_E_INVAL, ("snapshot: the group's line size " + std::to_string(g->stage.L) + " differs from the snapshot's lines of " +
                                              std::to_string(line_size) + " bytes").c_str());
  if (g->stage.device != mpc_snapshot_device_of(s)) return mpc_snapshot_fail(s, MPC_E_INVAL, "snapshot: the group is on another device");
  const bool classed = by_presence && g->cls.on;
  if (classed && g->cls.from_member >= 0)
    return mpc_snapshot_fail(s, MPC_E_INVAL, ("class accounting: the classes come from member " + std::to_string(g->cls.from_member) + ", by_presence cannot bring its own").c_str());
  group_refresh(g);
  int rc = snapshot_pieces(s, line_size, partial, [&](const void *d, u64 n, const uint64_t *da, const uint8_t *dp, void *stream) {
    const int frc = group_batch_device(g, d, n, classed ? dp : nullptr, (g->img.on || g->rw.on) ? da : nullptr, nullptr, nullptr, stream);
    return frc == MPC_OK ? frc : mpc_snapshot_fail(s, frc, g->error.c_str());
  });
  if (rc != MPC_OK) return rc;
  rc = mpc_group_sync(g);
  return rc == MPC_OK ? rc : mpc_snapshot_fail(s, rc, g->error.c_str());
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
         "\", \"needs\": [";
    // the plan itself: the layouts a kernel compiled at creation is asked for, and per prediction module what the planned
    // lane kernel reads and does for every byte (mpc::read_back_vpc_module; a fast plan only, whichever kernel the route picks)
    static const char *const need_names[] = {"BM", "ANYROOT", "PLANES", "GATHER", "WSHIFT"};
    bool first_need = true;
    for (int b = 0; b < 5; b++)
      if (plan.jit_needs & (1u << b)) {
        s += std::string(first_need ? "\"" : ", \"") + need_names[b] + "\"";
        first_need = false;
      }
    s += "], \"runtime_only\": " + std::to_string(plan.fast ? plan.params.runtime_only : 0) + ", \"modules\": [";
    auto ints = [](const std::vector<int> &v) {
      std::string a = "[";
      for (size_t j = 0; j < v.size(); j++) a += (j ? "," : "") + std::to_string(v[j]);
      return a + "]";
    };
    for (int i = 0; i < cfg.M; i++) {
      const mpc::Module &m = cfg.modules[(size_t)i];
      s += (i ? ", " : "");
      s += "{\"kind\": " + std::to_string(m.kind) + ", \"pred_kind\": " + std::to_string(m.pred_kind) + ", \"root\": " + std::to_string(m.root) +
           ", \"cx\": " + (m.consecutive_xor ? "1" : "0") + ", \"table_size\": " + std::to_string(m.table_size) + ", \"shifts\": [";
      for (size_t j = 0; j < m.weight.size(); j++)
        s += (j ? "," : "") + std::to_string(m.pred_kind == mpc::PRED_WEIGHT && (int)j != m.root ? mpc::weight_shift(m.weight[j]) : 0);
      s += "]";
      if (plan.fast && i >= cfg.start) {
        mpc::VpcModuleRead rb;
        mpc::read_back_vpc_module(plan, i - cfg.start, rb);
        s += ", \"kernel_base\": " + ints(rb.base);
        if (!rb.shift.empty()) s += ", \"kernel_shift\": " + ints(rb.shift);
        if (!rb.diff.empty()) s += ", \"kernel_diff\": " + ints(rb.diff);
        if (*rb.base_form) s += ", \"base_form\": \"" + std::string(rb.base_form) + "\"";
      }
      s += "}";
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

// test library only: what the evicting Pattern set's launches did since the handle was created -- out[0..6) = launches,
// rotations, first occurrences of gone lines, at-risk occurrences, at-risk misses, entries put on list B (the
// MPC_ESET_T_* words of mpc_pattern.h, which only the test library's kernels count in); out[i] = 0 beyond
int mpc_test_evict_counters(mpc_handle *h, uint64_t *out, size_t n)
{
  if (!h || !out || h->algorithm != Algo::Pattern || !h->pat.evicting) return MPC_E_INVAL;
  if (hipSetDevice(h->device) != hipSuccess) return MPC_E_HIP;
  HIPCHK(h, hipDeviceSynchronize());
  uint64_t ctl[MPC_ESET_WORDS];
  HIPCHK(h, hipMemcpy(ctl, h->pat.evict.ctl, sizeof(ctl), hipMemcpyDeviceToHost));
  const uint64_t v[6] = {ctl[MPC_ESET_SEQ], ctl[MPC_ESET_T_ROTATIONS], ctl[MPC_ESET_T_GONE], ctl[MPC_ESET_T_RISK], ctl[MPC_ESET_T_RISK_MISS],
                         ctl[MPC_ESET_T_LIST_B]};
  for (size_t i = 0; i < n; i++) out[i] = i < 6 ? v[i] : 0;
  return MPC_OK;
}

// test library only: the MPC_ELINE_* kind of the first n lines of the evicting set's most recent launch
int mpc_test_evict_kinds(mpc_handle *h, uint8_t *out, size_t n)
{
  if (!h || !out || h->algorithm != Algo::Pattern || !h->pat.evicting || n > (size_t)h->pat.evict.launch_max) return MPC_E_INVAL;
  if (hipSetDevice(h->device) != hipSuccess) return MPC_E_HIP;
  HIPCHK(h, hipDeviceSynchronize());
  if (n) HIPCHK(h, hipMemcpy(out, h->pat.evict.kind, n, hipMemcpyDeviceToHost));
  return MPC_OK;
}
#endif

#if MPC_STAMPS
// test library and -DMPC_STAMPS=1 builds: the workgroup stamps of the handle's last lane-kernel launch (mpc_device.h: MPC_STAMP_WORDS words)
int mpc_test_stamps(mpc_handle *h, uint64_t *out, size_t n)
{
  if (!h || !out || n > (size_t)MPC_STAMP_WORDS) return MPC_E_INVAL;
  if (hipSetDevice(h->device) != hipSuccess) return MPC_E_HIP;
  HIPCHK(h, hipDeviceSynchronize());
  HIPCHK(h, hipMemcpy(out, h->d_raw + h->raw_len + kRouteWords, n * sizeof(uint64_t), hipMemcpyDeviceToHost));
  return MPC_OK;
}
#endif

}  // extern "C"
