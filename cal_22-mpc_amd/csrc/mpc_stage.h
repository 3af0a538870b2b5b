// mpc_stage.h -- the host -> device staging pipeline (host side, used by mpc_capi.hip): ONE stager for a single handle
// and for a group of handles.
//
// A stager owns two slots, each a 64 MiB pinned host buffer, a device buffer, a stream and an event.  Chunk i+1 is
// filled (from the caller's buffer, a .npy file or a .log file) and copied while chunk i is being evaluated; per-line
// results come back through pinned buffers that exist per member and slot once a call has asked for that member's
// output.  Calls of up to kMiniLines lines skip the slots: one pinned, device-visible buffer that the kernels read the
// lines from and write the results to.  A member whose sizes are accounted on the device (Stager::account, mpc_sizes.h)
// gets its device array of sizes whether or not the caller asked; the copy back and the pinned mirror stay tied to
// "the caller asked".  The same holds for a member whose `selected` gives the classes of the lines (Stager::need_sel).
// With per-class accounting on (mpc_classes.h) a chunk may carry one class byte per line: a pinned buffer per slot
// beside the lines, with a device twin, both allocated when the first such chunk arrives.  With image accounting on
// (mpc_image.h) a chunk carries one 64-bit address per line in the same way: a pinned buffer per slot with a device twin,
// which exist only once a chunk has carried addresses.
//
// A handle is a group of one: the only difference between the two is "one output pointer" against "one output pointer
// per member", so every function here takes arrays of `members` pointers.  What a stager feeds is told by a Sink:
// what is launched on a stream for a chunk, where an error message goes, and what is checked once the work is
// complete.  mpc_capi.hip has two of them, sink_of(mpc_handle *) and sink_of(mpc_group *); a member of a group sees
// every line exactly as if it had been called alone because both run the code below.
#pragma once
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "../../include/mpc_hip.h"
#include "mpc_trace_files.h"

namespace mpcstage {
namespace {   // (one translation unit includes this: nothing here is exported)

typedef unsigned long long u64;

constexpr size_t kStageBytes = 64ull << 20;   // per slot
constexpr size_t kMiniLines = 512;            // batches up to this many lines are evaluated in place

struct Sink {
  void *ctx;
  // every member over the same device-visible lines on stream s; d_sizes / d_sel: one pointer per member (null: not asked for);
  // d_classes: one device-visible class byte per line, or null (class 0); d_addrs: one device-visible address per line, or null
  int (*launch)(void *ctx, const void *d_lines, u64 n, uint16_t *const *d_sizes, int8_t *const *d_sel, const uint8_t *d_classes, const uint64_t *d_addrs,
                hipStream_t s);
  int (*fail)(void *ctx, int code, const std::string &msg);   // keeps the message, returns the code
  int (*status)(void *ctx);                                   // at a point where the work is complete (Pattern's capacity)
};
inline const Sink &sink_of(const Sink &k) { return k; }

// the one error check of the host side: `to` is a Sink or whatever has a sink_of() (a handle, a group)
#define HIPCHK(to, call)                                                                        \
  do {                                                                                          \
    hipError_t e_ = (call);                                                                     \
    if (e_ != hipSuccess) {                                                                     \
      const mpcstage::Sink k_ = sink_of(to);                                                    \
      return k_.fail(k_.ctx, MPC_E_HIP, std::string(#call) + ": " + hipGetErrorString(e_));     \
    }                                                                                           \
  } while (0)

struct Slot {
  hipStream_t stream = nullptr;
  hipEvent_t done = nullptr;
  uint8_t *h_in = nullptr;       // pinned
  uint8_t *d_in = nullptr;
  uint8_t *h_cls = nullptr;      // pinned, [stage_lines] class bytes; null until a chunk carries classes
  uint8_t *d_cls = nullptr;
  uint64_t *h_adr = nullptr;     // pinned, [stage_lines] line addresses; null until a chunk carries addresses
  uint64_t *d_adr = nullptr;
  // per member; the buffers are allocated when a call first asks for that member's per-line output
  std::vector<uint16_t *> d_sizes, h_sizes, user_sizes;   // user_*: where the pending results go
  std::vector<int8_t *> d_sel, h_sel, user_sel;
  u64 pending_lines = 0;
  bool busy = false;
};

struct Stager {
  int device = 0;
  int L = 0;
  size_t members = 0;
  Slot slots[2];
  size_t stage_lines = 0;
  uint8_t *mini = nullptr;       // [kMiniLines * L] lines | per member [kMiniLines] uint16 sizes | per member [kMiniLines] int8 clusters
  bool slots_ready = false;
  std::vector<uint16_t *> ask_sizes;   // the launch in the making: per member the device buffer, null where the caller
  std::vector<int8_t *> ask_sel;       // did not ask (kept here so that no call allocates)
  std::vector<char> account;           // per member: its sizes are wanted on the device whether or not the caller asked (size
                                       // accounting, mpc_sizes.h); all 0 unless the owner switched accounting on
  std::vector<char> need_sel;          // per member: the same for its `selected` (it gives the lines' classes)
  uint8_t *mini_cls = nullptr;         // [kMiniLines] pinned class bytes of an in-place call; null until one carries classes
  int log_field = 0;                   // MPC_CLASS_LOG_*: the class of a .log record's line (the owner keeps it 0 while accounting is off)
  uint64_t *mini_adr = nullptr;        // [kMiniLines] pinned addresses of an in-place call; null until one carries addresses
  bool log_addrs = false;              // a .log record's line carries its mem_addr (the owner keeps it false while image accounting is off)
};

inline void init(Stager &st, int device, int L, size_t members)
{
  st.device = device;
  st.L = L;
  st.members = members;
  st.stage_lines = kStageBytes / (size_t)L;
  for (Slot &s : st.slots) {
    s.d_sizes.assign(members, nullptr); s.h_sizes.assign(members, nullptr); s.user_sizes.assign(members, nullptr);
    s.d_sel.assign(members, nullptr); s.h_sel.assign(members, nullptr); s.user_sel.assign(members, nullptr);
  }
  st.ask_sizes.assign(members, nullptr);
  st.ask_sel.assign(members, nullptr);
  st.account.assign(members, 0);
  st.need_sel.assign(members, 0);
}

// Creates what a staged call needs and is still missing.  When that is differs on purpose: a handle has nothing before
// its first staged call (one used only per line or through mpc_compress_batch_device never pays for 2 x 64 MiB), a
// group has had its streams and events since mpc_group_create (its members register them for sc2_build).
inline int ensure(Stager &st, const Sink &k)
{
  if (st.slots_ready) return MPC_OK;
  for (Slot &s : st.slots) {
    if (!s.stream) HIPCHK(k, hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking));
    if (!s.done) HIPCHK(k, hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
    if (!s.h_in) HIPCHK(k, hipHostMalloc((void **)&s.h_in, kStageBytes, hipHostMallocDefault));
    if (!s.d_in) HIPCHK(k, hipMalloc((void **)&s.d_in, kStageBytes));
  }
  st.slots_ready = true;
  return MPC_OK;
}

// the per-line output buffers of member i in a slot, when a call asks for them for the first time.  The device array of
// sizes also exists for a member whose sizes are accounted; its pinned mirror only once the caller asked.
inline int ensure_outputs(Stager &st, const Sink &k, Slot &s, size_t i, bool sizes, bool sel)
{
  if ((sizes || st.account[i]) && !s.d_sizes[i]) HIPCHK(k, hipMalloc((void **)&s.d_sizes[i], st.stage_lines * sizeof(uint16_t)));
  if (sizes && !s.h_sizes[i]) HIPCHK(k, hipHostMalloc((void **)&s.h_sizes[i], st.stage_lines * sizeof(uint16_t), hipHostMallocDefault));
  if ((sel || st.need_sel[i]) && !s.d_sel[i]) HIPCHK(k, hipMalloc((void **)&s.d_sel[i], st.stage_lines));
  if (sel && !s.h_sel[i]) HIPCHK(k, hipHostMalloc((void **)&s.h_sel[i], st.stage_lines, hipHostMallocDefault));
  return MPC_OK;
}

// the class buffers of a slot, when a walk carries classes for the first time
inline int ensure_classes(Stager &st, const Sink &k, Slot &s)
{
  if (!s.h_cls) HIPCHK(k, hipHostMalloc((void **)&s.h_cls, st.stage_lines, hipHostMallocDefault));
  if (!s.d_cls) HIPCHK(k, hipMalloc((void **)&s.d_cls, st.stage_lines));
  return MPC_OK;
}

// the address buffers of a slot, when a walk carries addresses for the first time
inline int ensure_addrs(Stager &st, const Sink &k, Slot &s)
{
  if (!s.h_adr) HIPCHK(k, hipHostMalloc((void **)&s.h_adr, st.stage_lines * sizeof(uint64_t), hipHostMallocDefault));
  if (!s.d_adr) HIPCHK(k, hipMalloc((void **)&s.d_adr, st.stage_lines * sizeof(uint64_t)));
  return MPC_OK;
}

// wait for a slot's in-flight chunk and hand its per-line results to the caller
inline int retire(Stager &st, const Sink &k, Slot &s)
{
  if (!s.busy) return MPC_OK;
  HIPCHK(k, hipEventSynchronize(s.done));
  for (size_t i = 0; i < st.members; i++) {
    if (s.user_sizes[i]) std::memcpy(s.user_sizes[i], s.h_sizes[i], s.pending_lines * sizeof(uint16_t));
    if (s.user_sel[i]) std::memcpy(s.user_sel[i], s.h_sel[i], s.pending_lines);
  }
  s.busy = false;
  return MPC_OK;
}

// submit the chunk already sitting in s.h_in (with_classes: and its class bytes in s.h_cls; with_addrs: and its
// addresses in s.h_adr): one copy, then the sink's
// launch on the slot's stream.
// sizes / sel: the caller's arrays of per-member pointers (or null), `first` the chunk's first line in them.
inline int submit(Stager &st, const Sink &k, Slot &s, u64 lines, uint16_t *const *sizes, int8_t *const *sel, u64 first, bool with_classes,
                  bool with_addrs)
{
  for (size_t i = 0; i < st.members; i++) {
    s.user_sizes[i] = (sizes && sizes[i]) ? sizes[i] + first : nullptr;
    s.user_sel[i] = (sel && sel[i]) ? sel[i] + first : nullptr;
    const int rc = ensure_outputs(st, k, s, i, s.user_sizes[i] != nullptr, s.user_sel[i] != nullptr);
    if (rc != MPC_OK) return rc;
    st.ask_sizes[i] = (s.user_sizes[i] || st.account[i]) ? s.d_sizes[i] : nullptr;
    st.ask_sel[i] = (s.user_sel[i] || st.need_sel[i]) ? s.d_sel[i] : nullptr;
  }
  HIPCHK(k, hipMemcpyAsync(s.d_in, s.h_in, lines * (u64)st.L, hipMemcpyHostToDevice, s.stream));
  if (with_classes) HIPCHK(k, hipMemcpyAsync(s.d_cls, s.h_cls, lines, hipMemcpyHostToDevice, s.stream));
  if (with_addrs) HIPCHK(k, hipMemcpyAsync(s.d_adr, s.h_adr, lines * sizeof(uint64_t), hipMemcpyHostToDevice, s.stream));
  const int rc = k.launch(k.ctx, s.d_in, lines, st.ask_sizes.data(), st.ask_sel.data(), with_classes ? s.d_cls : nullptr, with_addrs ? s.d_adr : nullptr,
                          s.stream);
  if (rc != MPC_OK) return rc;
  for (size_t i = 0; i < st.members; i++) {
    if (s.user_sizes[i]) HIPCHK(k, hipMemcpyAsync(s.h_sizes[i], s.d_sizes[i], lines * sizeof(uint16_t), hipMemcpyDeviceToHost, s.stream));
    if (s.user_sel[i]) HIPCHK(k, hipMemcpyAsync(s.h_sel[i], s.d_sel[i], lines, hipMemcpyDeviceToHost, s.stream));
  }
  HIPCHK(k, hipEventRecord(s.done, s.stream));
  s.pending_lines = lines;
  s.busy = true;
  return MPC_OK;
}

// After an error: nothing of the failed call may be delivered later.  Wait for both slots' streams
// and forget their pending results (the caller's output pointers may be gone by the next call).
inline void abandon(Stager &st)
{
  for (Slot &s : st.slots) {
    if (s.stream) (void)hipStreamSynchronize(s.stream);
    s.busy = false;
    s.pending_lines = 0;
    std::fill(s.user_sizes.begin(), s.user_sizes.end(), nullptr);
    std::fill(s.user_sel.begin(), s.user_sel.end(), nullptr);
  }
}

// the slot streams that exist (sc2_build: a warm-up chunk may still be counting on any of them)
inline int sync_slots(Stager &st, const Sink &k)
{
  for (Slot &s : st.slots)
    if (s.stream) HIPCHK(k, hipStreamSynchronize(s.stream));
  return MPC_OK;
}

// Both slots retired, the owner's streams idle, the sink's check.  Which streams are drained differs on purpose and is
// kept as it was: `own` is a handle's own stream (its in-place calls and its table build run there; its slot streams
// were waited for by retire); a group has none (own == null) and drains its two slot streams, which always exist.
inline int finish(Stager &st, const Sink &k, hipStream_t own)
{
  for (Slot &s : st.slots) {
    const int rc = retire(st, k, s);
    if (rc != MPC_OK) return rc;
  }
  if (own) HIPCHK(k, hipStreamSynchronize(own));
  else {
    const int rc = sync_slots(st, k);
    if (rc != MPC_OK) return rc;
  }
  return k.status(k.ctx);
}

// n <= kMiniLines lines, evaluated in place from pinned host memory: the sink's launch on stream s, one synchronisation
// (polling hipStreamQuery instead was slower: 46 k vs 58 k lines/s).  The stream is the caller's choice and differs on
// purpose: a handle's own stream, a group's first slot stream (idle: every group call ends synchronised).
inline int in_place(Stager &st, const Sink &k, hipStream_t s, const uint8_t *lines, u64 n, const uint8_t *classes, const uint64_t *addrs,
                    uint16_t *const *sizes, int8_t *const *sel)
{
  const size_t nm = st.members;
  if (!st.mini) HIPCHK(k, hipHostMalloc((void **)&st.mini, kMiniLines * ((size_t)st.L + nm * (sizeof(uint16_t) + 1)), hipHostMallocDefault));
  uint16_t *out_sizes = reinterpret_cast<uint16_t *>(st.mini + kMiniLines * (size_t)st.L);
  int8_t *out_sel = reinterpret_cast<int8_t *>(out_sizes + nm * kMiniLines);
  for (size_t i = 0; i < nm; i++) {
    st.ask_sizes[i] = ((sizes && sizes[i]) || st.account[i]) ? out_sizes + i * kMiniLines : nullptr;
    st.ask_sel[i] = ((sel && sel[i]) || st.need_sel[i]) ? out_sel + i * kMiniLines : nullptr;
  }
  std::memcpy(st.mini, lines, (size_t)(n * (u64)st.L));
  if (classes) {
    if (!st.mini_cls) HIPCHK(k, hipHostMalloc((void **)&st.mini_cls, kMiniLines, hipHostMallocDefault));
    std::memcpy(st.mini_cls, classes, (size_t)n);
  }
  if (addrs) {
    if (!st.mini_adr) HIPCHK(k, hipHostMalloc((void **)&st.mini_adr, kMiniLines * sizeof(uint64_t), hipHostMallocDefault));
    std::memcpy(st.mini_adr, addrs, (size_t)n * sizeof(uint64_t));
  }
  const int rc = k.launch(k.ctx, st.mini, n, st.ask_sizes.data(), st.ask_sel.data(), classes ? st.mini_cls : nullptr, addrs ? st.mini_adr : nullptr, s);
  if (rc != MPC_OK) { (void)hipStreamSynchronize(s); return rc; }   // (what was enqueued before the failure reads st.mini)
  HIPCHK(k, hipStreamSynchronize(s));
  for (size_t i = 0; i < nm; i++) {
    if (sizes && sizes[i]) std::memcpy(sizes[i], st.ask_sizes[i], (size_t)n * sizeof(uint16_t));
    if (sel && sel[i]) std::memcpy(sel[i], st.ask_sel[i], (size_t)n);
  }
  return k.status(k.ctx);
}

// A walk over a trace: retire a slot, let `fill` put up to `room` lines into its pinned buffer (with_classes: and their
// class bytes into the slot's class buffer, with_addrs: and their addresses into the slot's address buffer, else that
// argument is null), submit them, take the other slot; until fill
// returns 0 lines or fails (< 0: the code, already reported).  Then finish, or abandon after a failure.
template <class Fill>
inline int pump(Stager &st, const Sink &k, hipStream_t own, uint16_t *const *sizes, int8_t *const *sel, u64 *lines_done, bool with_classes,
                bool with_addrs, Fill fill)
{
  int rc = ensure(st, k);
  u64 done = 0;
  int which = 0;
  while (rc == MPC_OK) {
    Slot &s = st.slots[which];
    rc = retire(st, k, s);   // the slot's previous chunk (overlapped with the other slot's work)
    if (rc == MPC_OK && with_classes) rc = ensure_classes(st, k, s);
    if (rc == MPC_OK && with_addrs) rc = ensure_addrs(st, k, s);
    if (rc != MPC_OK) break;
    const long long got = fill(s.h_in, with_classes ? s.h_cls : nullptr, with_addrs ? s.h_adr : nullptr, (u64)st.stage_lines, done);
    if (got < 0) rc = (int)got;
    if (got <= 0) break;
    rc = submit(st, k, s, (u64)got, sizes, sel, done, with_classes, with_addrs);
    if (rc != MPC_OK) break;
    done += (u64)got;
    which ^= 1;
  }
  if (rc == MPC_OK) rc = finish(st, k, own);
  if (rc != MPC_OK) abandon(st);
  if (rc == MPC_OK && lines_done) *lines_done = done;
  return rc;
}

// n lines in the caller's memory.  sizes / sel: arrays of one pointer per member (the array or any entry may be null).
// classes: one class byte per line in the caller's memory, or null; addrs: one address per line in the caller's memory, or null.
inline int compress_batch(Stager &st, const Sink &k, hipStream_t own, const uint8_t *lines, u64 n, const uint8_t *classes, const uint64_t *addrs,
                          uint16_t *const *sizes, int8_t *const *sel)
{
  HIPCHK(k, hipSetDevice(st.device));
  if (n <= kMiniLines) return in_place(st, k, own ? own : st.slots[0].stream, lines, n, classes, addrs, sizes, sel);
  return pump(st, k, own, sizes, sel, nullptr, classes != nullptr, addrs != nullptr, [&](uint8_t *buf, uint8_t *cls, uint64_t *adr, u64 room, u64 done) -> long long {
    const u64 take = (n - done) < room ? (n - done) : room;
    mpctrace::parallel_copy(buf, lines + done * (u64)st.L, (size_t)(take * (u64)st.L));
    if (cls) std::memcpy(cls, classes + done, (size_t)take);
    if (adr) std::memcpy(adr, addrs + done, (size_t)take * sizeof(uint64_t));
    return (long long)take;
  });
}

// rows [first_row, first_row + n_rows) of a 2-D uint8 .npy file, statistics only
inline int compress_npy(Stager &st, const Sink &k, hipStream_t own, const char *path, uint64_t first_row, uint64_t n_rows, int skip_last_row,
                        uint64_t *rows_done)
{
  if (rows_done) *rows_done = 0;
  FILE *f = fopen(path, "rb");
  if (!f) return k.fail(k.ctx, MPC_E_NOENT, std::string("cannot open ") + path);
  u64 rows, cols, off;
  std::string err;
  int rc = mpctrace::parse_npy_header(f, &rows, &cols, &off, err);
  if (rc != MPC_OK) { fclose(f); return k.fail(k.ctx, rc, err); }
  if (cols != (u64)st.L) {
    fclose(f);
    return k.fail(k.ctx, MPC_E_INVAL, "trace line size " + std::to_string(cols) + " differs from the evaluator's " + std::to_string(st.L));
  }
  // the reference driver drops the final row (LoaderNPY.cpp:28-32 + main.cpp:240)
  const u64 usable = (skip_last_row && rows > 0) ? rows - 1 : rows;
  const u64 begin = first_row < usable ? first_row : usable;
  const u64 end = (n_rows > usable - begin) ? usable : begin + n_rows;
  if (hipSetDevice(st.device) != hipSuccess) { fclose(f); return k.fail(k.ctx, MPC_E_HIP, "hipSetDevice failed"); }
  const int fd = fileno(f);
  u64 done_rows = 0;
  rc = pump(st, k, own, nullptr, nullptr, &done_rows, false, false, [&](uint8_t *buf, uint8_t *, uint64_t *, u64 room, u64 done) -> long long {
    const u64 take = (end - begin - done) < room ? (end - begin - done) : room;
    if (take && !mpctrace::parallel_pread(fd, buf, (size_t)(take * cols), off + (begin + done) * cols))
      return k.fail(k.ctx, MPC_E_PARSE, "short read: .npy file is truncated");
    return (long long)take;
  });
  fclose(f);
  if (rc == MPC_OK && rows_done) *rows_done = done_rows;
  return rc;
}

// the global-memory requests of a GPGPU-Sim .log file, statistics only
inline int compress_gpgpusim_log(Stager &st, const Sink &k, hipStream_t own, const char *log_path, uint64_t *requests_read, uint64_t *lines_done)
{
  if (requests_read) *requests_read = 0;
  if (lines_done) *lines_done = 0;
  mpctrace::LogMap log;
  std::string err;
  int rc = log.open(log_path, err);
  if (rc != MPC_OK) return k.fail(k.ctx, rc, err);
  if (hipSetDevice(st.device) != hipSuccess) return k.fail(k.ctx, MPC_E_HIP, "hipSetDevice failed");
  const u64 L = (u64)st.L;
  u64 requests = 0, lines = 0;
  bool first = true, ended = false;
  const int field = st.log_field;       // the class of a record's line: a byte of the record's header (mpc_hip_classes.h)
  rc = pump(st, k, own, nullptr, nullptr, &lines, field != MPC_CLASS_LOG_NONE, st.log_addrs, [&](uint8_t *buf, uint8_t *cls, uint64_t *adr, u64 room, u64) -> long long {
    u64 fill = 0;
    uint32_t req_type, req_size;
    const unsigned char *payload;
    while (!ended && fill < room) {
      if (!log.next(&req_type, &req_size, &payload)) { ended = true; break; }
      if (first && req_size != L)
        return k.fail(k.ctx, MPC_E_INVAL, "trace line size " + std::to_string(req_size) + " differs from the evaluator's " + std::to_string(L));
      first = false;
      if (!payload) { ended = true; break; }                     // incomplete trailing request
      if (req_type == 0u || req_type == 4u) {                      // GLOBAL_ACC_R, GLOBAL_ACC_W
        if (req_size != L)
          return k.fail(k.ctx, MPC_E_INVAL, "the GPGPU-sim trace mixes request sizes (" + std::to_string(req_size) + " after " + std::to_string(L) + " bytes)");
        std::memcpy(buf + fill * L, payload, (size_t)L);
        if (cls) {
          const unsigned char *rec = payload - mpctrace::kLogRecordHeader;
          cls[fill] = field == MPC_CLASS_LOG_KERNEL ? rec[0] : field == MPC_CLASS_LOG_MFTYPE ? rec[1] : (req_type == 4u ? 1 : 0);
        }
        if (adr) std::memcpy(&adr[fill], payload - mpctrace::kLogRecordHeader + mpctrace::kLogRecordAddr, sizeof(uint64_t));   // mem_addr
        fill++;
      }
      requests++;
    }
    return (long long)fill;
  });
  if (rc == MPC_OK) {
    if (requests_read) *requests_read = requests;
    if (lines_done) *lines_done = lines;
  }
  return rc;
}

// teardown: the streams are waited for before their buffers go
inline void destroy(Stager &st)
{
  for (Slot &s : st.slots) {
    if (s.stream) (void)hipStreamSynchronize(s.stream);
    if (s.h_in) (void)hipHostFree(s.h_in);
    if (s.d_in) (void)hipFree(s.d_in);
    if (s.h_cls) (void)hipHostFree(s.h_cls);
    if (s.d_cls) (void)hipFree(s.d_cls);
    if (s.h_adr) (void)hipHostFree(s.h_adr);
    if (s.d_adr) (void)hipFree(s.d_adr);
    for (uint16_t *p : s.d_sizes) if (p) (void)hipFree(p);
    for (uint16_t *p : s.h_sizes) if (p) (void)hipHostFree(p);
    for (int8_t *p : s.d_sel) if (p) (void)hipFree(p);
    for (int8_t *p : s.h_sel) if (p) (void)hipHostFree(p);
    if (s.done) (void)hipEventDestroy(s.done);
    if (s.stream) (void)hipStreamDestroy(s.stream);
    s = Slot();
  }
  if (st.mini) (void)hipHostFree(st.mini);
  st.mini = nullptr;
  if (st.mini_cls) (void)hipHostFree(st.mini_cls);
  st.mini_cls = nullptr;
  if (st.mini_adr) (void)hipHostFree(st.mini_adr);
  st.mini_adr = nullptr;
  st.slots_ready = false;
}

}  // namespace
}  // namespace mpcstage
