// mpc_trace_files.h -- the trace files the library reads, without any HIP: the .npy header, the GPGPU-Sim .log
// records, and the threaded copies that fill a staging buffer.  Used by the stager's file walkers (mpc_stage.h) and by
// mpc_npy_shape / mpc_gpgpusim_log_line_size (mpc_capi.hip).  Functions return MPC_OK or an MPC_E_* code with the
// message in `err`; where a message lands is the caller's business.
#pragma once
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <system_error>
#include <thread>
#include <vector>

#include "../../include/mpc_hip.h"

namespace mpctrace {
namespace {   // (one translation unit includes this: nothing here is exported)

typedef unsigned long long u64;

// ---- .npy header (format spec: magic, version, header length, python dict) ----
inline int parse_npy_header(FILE *f, u64 *rows, u64 *cols, u64 *data_off, std::string &err)
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

// ---- GPGPU-Sim .log: a file header of 1 + 7 * 17 bytes, then records of a 62-byte header (request type at 38, payload
// size at 58) and the payload (LoaderGPGPU.cpp:9-119) ----
constexpr int kLogKeys = 17, kLogRecordHeader = 62;
constexpr int kLogRecordAddr = 30;      // mem_addr, a u64 (LoaderGPGPU.cpp)
constexpr u64 kLogFileHeader = 1 + 7 * kLogKeys;

// validates the file header of a GPGPU-Sim trace (LoaderGPGPU.cpp:93-119)
inline int log_open(const char *path, FILE **out, std::string &err)
{
  FILE *f = fopen(path, "rb");
  if (!f) { err = std::string("Failed to open a file. Check the path of the file: ") + path; return MPC_E_NOENT; }
  unsigned char hdr[kLogFileHeader];
  if (fread(hdr, 1, sizeof(hdr), f) != sizeof(hdr) || hdr[0] != kLogKeys) {
    fclose(f);
    err = "The header of the GPGPU-sim trace file is not valid.";
    return MPC_E_PARSE;
  }
  *out = f;
  return MPC_OK;
}

// one request header; false at the end of the file (or inside an incomplete header)
inline bool log_next(FILE *f, uint32_t *req_type, uint32_t *req_size)
{
  unsigned char h[kLogRecordHeader];
  if (fread(h, 1, sizeof(h), f) != sizeof(h)) return false;
  std::memcpy(req_type, h + 38, 4);
  std::memcpy(req_size, h + 58, 4);
  return true;
}

// The same records from a whole file, which is mapped and walked in memory (per-request stdio calls cap the rate at
// ~35 M requests/s).
struct LogMap {
  const unsigned char *base = nullptr;
  u64 size = 0, pos = kLogFileHeader;
  LogMap() = default;
  LogMap(const LogMap &) = delete;
  LogMap &operator=(const LogMap &) = delete;
  ~LogMap() { if (base) munmap(const_cast<unsigned char *>(base), (size_t)size); }

  int open(const char *path, std::string &err)
  {
    const int fd = ::open(path, O_RDONLY);
    if (fd < 0) { err = std::string("Failed to open a file. Check the path of the file: ") + path; return MPC_E_NOENT; }
    struct stat st;
    if (fstat(fd, &st) != 0) { close(fd); err = std::string("cannot stat ") + path; return MPC_E_NOENT; }
    size = (u64)st.st_size;
    if (size > 0) {
      void *m = mmap(nullptr, (size_t)size, PROT_READ, MAP_PRIVATE, fd, 0);
      if (m == MAP_FAILED) { close(fd); err = std::string("cannot map ") + path; return MPC_E_NOMEM; }
      base = static_cast<const unsigned char *>(m);
      (void)madvise(m, (size_t)size, MADV_SEQUENTIAL);
    }
    close(fd);
    if (size < kLogFileHeader || base[0] != kLogKeys) { err = "The header of the GPGPU-sim trace file is not valid."; return MPC_E_PARSE; }
    return MPC_OK;
  }

  // The next record: its type, its payload size and the payload.  False at the end of the file (or inside an incomplete
  // header); *payload is null for the incomplete trailing request, whose header is still reported.
  bool next(uint32_t *req_type, uint32_t *req_size, const unsigned char **payload)
  {
    if (pos + kLogRecordHeader > size) return false;
    std::memcpy(req_type, base + pos + 38, 4);
    std::memcpy(req_size, base + pos + 58, 4);
    const u64 end = pos + kLogRecordHeader + (u64)*req_size;
    *payload = end > size ? nullptr : base + pos + kLogRecordHeader;
    if (end <= size) pos = end;
    return true;
  }
};

// ---- Staging copies (caller's buffer -> pinned slot) are memory-bandwidth work on the host: one
// thread moves ~12-24 GB/s, less than the PCIe link takes, so large copies are split over a
// few threads.
constexpr size_t kCopySlice = 8u << 20;
constexpr unsigned kCopyThreads = 4;

inline void parallel_copy(void *dst, const void *src, size_t bytes)
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
inline bool parallel_pread(int fd, void *dst, size_t bytes, u64 file_off)
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

}  // namespace
}  // namespace mpctrace
