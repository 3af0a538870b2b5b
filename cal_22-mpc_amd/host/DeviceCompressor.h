// DeviceCompressor.h -- ADDITIVE, no counterpart in the reference: what the seven GPU evaluators (VPC, BDI, FPC, BPC,
// SC2, Pattern, CPACK) share over one libmpc_hip handle (include/mpc_hip.h), size accounting (SizeReport.h) included.  A derived class keeps its constructor (the
// create call, its result object, its name), LoadResult() and whatever the reference's class of that name has of its own.
#ifndef MPC_HOST_DEVICECOMPRESSOR_H
#define MPC_HOST_DEVICECOMPRESSOR_H

#include <string>

#include "Compressor.h"
#include "ClassReport.h"
#include "ImageReport.h"
#include "PackReport.h"
#include "RewriteReport.h"
#include "SizeReport.h"

namespace comp
{

// Prints "<what> (<rc>): <msg>" to stdout and exits with 1, as every failure of a library call does here.
[[noreturn]] void fail(const std::string &what, int rc, const char *msg);

class DeviceCompressor : public Compressor
{
public:
  virtual ~DeviceCompressor();
  virtual unsigned CompressLine(std::vector<uint8_t> &dataLine);
  // the statistics vector of the handle through LoadResult() into m_Stat
  virtual CompResult *GetResult();
  virtual void CompressBatch(const uint8_t *lines, unsigned long long n);
  // a .npy file or a GPGPU-Sim .log file, streamed by the library
  virtual unsigned long long CompressFile(const std::string &tracePath);
  virtual unsigned GetLineSize() { return m_LineSize; }
  // (a handle that has been handed out counts as fed: whoever holds it may have sent lines through it)
  virtual mpc_handle *DeviceHandle() { FlushLines(); m_Fed = true; return m_Handle; }
  // ADDITIVE: count, from now on, how many lines compress to how many bits (mpc_size_hist_enable); off by default
  void EnableSizeHistogram();
  // ... that histogram (mpc_size_hist_get), buffered lines evaluated first; a failure (not enabled) exits like every other
  SizeReport GetSizeHistogram(unsigned sectorBytes = ACCESS_GRAN);
  // ADDITIVE: sum, from now on, lines, bits and sector counts per class of a line (mpc_class_stats_enable); off by default.
  // Lines count in class 0 unless they come from a .log file after SetLogClassField.
  void EnableClassStats(unsigned sectorBytes = ACCESS_GRAN);
  // ... those sums (mpc_class_stats_get), buffered lines evaluated first; a failure (not enabled) exits like every other
  ClassReport GetClassStats();
  // which field of a .log record is the class of its line: MPC_CLASS_LOG_NONE / _KERNEL / _RW / _MFTYPE (mpc_class_log_field)
  void SetLogClassField(int field);
  // ADDITIVE: count, from now on, the sectors that blocks of blockLines consecutive lines occupy when they are packed and
  // rounded up once, headerBits added per block (mpc_pack_stats_enable); off by default
  void EnablePackStats(unsigned long long blockLines, unsigned sectorBytes = ACCESS_GRAN, unsigned headerBits = 0);
  // ... that table (mpc_pack_stats_get), buffered lines evaluated first; a failure (not enabled) exits like every other
  PackReport GetPackStats();
  // ADDITIVE: keep, from now on, the size of the latest line per line address (a .log's mem_addr) for up to capacityLines
  // distinct lines, and report the sectors of address-aligned blocks of blockLines lines (mpc_image_stats_enable); off by default
  void EnableImageStats(unsigned long long blockLines, unsigned sectorBytes = ACCESS_GRAN, unsigned headerBits = 0,
                        unsigned long long capacityLines = 1ull << 24);
  // ... that table (mpc_image_stats_get; not destructive), buffered lines evaluated first; a failure exits like every other
  ImageReport GetImageStats();
  // ADDITIVE: follow, from now on, the sequence of sizes per line address (a .log's mem_addr) for up to capacityLines
  // distinct lines, in size classes of granuleBytes bytes (mpc_rewrite_stats_enable); off by default
  void EnableRewriteStats(unsigned granuleBytes = ACCESS_GRAN, unsigned long long capacityLines = 1ull << 24);
  // ... that table (mpc_rewrite_stats_get; not destructive), buffered lines evaluated first; a failure exits like every other
  RewriteReport GetRewriteStats();
  // whether EnableRewriteStats takes these values for lines of lineSize bytes (mpc_rewrite_check_values; no device); why: the refusal
  static bool CheckRewriteValues(unsigned lineSize, unsigned granuleBytes, unsigned long long capacityLines, std::string &why);

protected:
  // tag: the short name in front of this class's messages ("BDI", "VPC", ...)
  DeviceCompressor(const char *tag, unsigned lineSize = 0) : m_Handle(nullptr), m_LineSize(lineSize), m_Tag(tag) {}
  // after the create call of a constructor: "<tag>: cannot create the evaluator (rc): ..." unless it succeeded
  void CheckCreated(int rc);
  // "<what> (rc): <the handle's last error>", exit(1)
  [[noreturn]] void Fail(const std::string &what, int rc);
  // m_Stat from the statistics vector (layout per algorithm in include/mpc_hip.h)
  virtual void LoadResult(const uint64_t *v) = 0;
  // a line of the wrong length: message and exit(1)
  virtual void RefuseLine(size_t bytes);
  // whether a line has arrived by any route, buffered lines flushed first
  bool Fed() { FlushLines(); return m_Fed; }

  mpc_handle *m_Handle;
  unsigned m_LineSize;

private:
  std::string m_Tag;
  bool m_Fed = false;
};

}  // namespace comp

#endif
