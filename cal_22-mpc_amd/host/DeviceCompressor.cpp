#include "DeviceCompressor.h"

#include <cstdio>
#include <cstdlib>

#include "TraceFile.h"
#include "mpc_hip.h"

namespace comp
{

void fail(const std::string &what, int rc, const char *msg)
{
  printf("%s (%d): %s\n", what.c_str(), rc, msg ? msg : "");
  exit(1);
}

void DeviceCompressor::Fail(const std::string &what, int rc) { fail(what, rc, mpc_last_error(m_Handle)); }

// (a failed create call leaves m_Handle null: the message is the library's creation error)
void DeviceCompressor::CheckCreated(int rc)
{
  if (rc != MPC_OK) Fail(m_Tag + ": cannot create the evaluator", rc);
}

DeviceCompressor::~DeviceCompressor() { mpc_destroy(m_Handle); }

void DeviceCompressor::RefuseLine(size_t bytes)
{
  printf("%s: line of %zu bytes, expected %u.\n", m_Tag.c_str(), bytes, m_LineSize);
  exit(1);
}

unsigned DeviceCompressor::CompressLine(std::vector<uint8_t> &dataLine)
{
  if (dataLine.size() != m_LineSize) RefuseLine(dataLine.size());
  if (LineBuffering()) {
    BufferLine(dataLine);
    return 0;
  }
  uint16_t bits = 0;
  int rc = mpc_compress_batch(DeviceHandle(), dataLine.data(), 1, &bits, nullptr);
  if (rc != MPC_OK) Fail(m_Tag + "::CompressLine", rc);
  return bits;
}

void DeviceCompressor::CompressBatch(const uint8_t *lines, unsigned long long n)
{
  FlushLines();
  m_Fed = m_Fed || n > 0;
  int rc = mpc_compress_batch(m_Handle, lines, n, nullptr, nullptr);
  if (rc != MPC_OK) Fail(m_Tag + "::CompressBatch", rc);
}

unsigned long long DeviceCompressor::CompressFile(const std::string &tracePath)
{
  mpc_handle *h = DeviceHandle();
  uint64_t done = 0;
  int rc = trace::IsGpgpuSimLog(tracePath) ? mpc_compress_gpgpusim_log(h, tracePath.c_str(), nullptr, &done)
                                           : mpc_compress_npy(h, tracePath.c_str(), 0, ~0ull, 1, &done);
  if (rc != MPC_OK) Fail(m_Tag + "::CompressFile", rc);
  return done;
}

void DeviceCompressor::EnableSizeHistogram()
{
  FlushLines();
  int rc = mpc_size_hist_enable(m_Handle);
  if (rc != MPC_OK) Fail(m_Tag + "::EnableSizeHistogram", rc);
}

SizeReport DeviceCompressor::GetSizeHistogram(unsigned sectorBytes)
{
  FlushLines();
  SizeReport report(m_LineSize, sectorBytes);
  report.Bins.assign(MPC_SIZE_BINS, 0);
  int rc = mpc_size_hist_get(m_Handle, report.Bins.data(), report.Bins.size());
  if (rc != MPC_OK) Fail(m_Tag + "::GetSizeHistogram", rc);
  return report;
}

void DeviceCompressor::EnableClassStats(unsigned sectorBytes)
{
  FlushLines();
  int rc = mpc_class_stats_enable(m_Handle, sectorBytes);
  if (rc != MPC_OK) Fail(m_Tag + "::EnableClassStats", rc);
}

ClassReport DeviceCompressor::GetClassStats()
{
  FlushLines();
  unsigned sectorBytes = 0;
  int rc = mpc_class_sector_bytes(m_Handle, &sectorBytes);
  ClassReport report(m_LineSize, sectorBytes);
  report.Table.assign(MPC_CLASS_TABLE_LEN, 0);
  // (accounting off: the get call refuses and leaves the message)
  rc = mpc_class_stats_get(m_Handle, report.Table.data(), report.Table.size());
  if (rc != MPC_OK) Fail(m_Tag + "::GetClassStats", rc);
  return report;
}

void DeviceCompressor::EnablePackStats(unsigned long long blockLines, unsigned sectorBytes, unsigned headerBits)
{
  FlushLines();
  int rc = mpc_pack_stats_enable(m_Handle, blockLines, sectorBytes, headerBits);
  if (rc != MPC_OK) Fail(m_Tag + "::EnablePackStats", rc);
}

PackReport DeviceCompressor::GetPackStats()
{
  FlushLines();
  PackReport report(m_LineSize);
  int rc = mpc_pack_stats_get(m_Handle, report.Table.data(), report.Table.size());
  if (rc != MPC_OK) Fail(m_Tag + "::GetPackStats", rc);
  return report;
}

void DeviceCompressor::EnableImageStats(unsigned long long blockLines, unsigned sectorBytes, unsigned headerBits, unsigned long long capacityLines)
{
  FlushLines();
  int rc = mpc_image_stats_enable(m_Handle, capacityLines, blockLines, sectorBytes, headerBits);
  if (rc != MPC_OK) Fail(m_Tag + "::EnableImageStats", rc);
}

ImageReport DeviceCompressor::GetImageStats()
{
  FlushLines();
  ImageReport report(m_LineSize);
  int rc = mpc_image_stats_get(m_Handle, report.Table.data(), report.Table.size());
  if (rc != MPC_OK) Fail(m_Tag + "::GetImageStats", rc);
  return report;
}

void DeviceCompressor::EnableRewriteStats(unsigned granuleBytes, unsigned long long capacityLines)
{
  FlushLines();
  int rc = mpc_rewrite_stats_enable(m_Handle, capacityLines, granuleBytes);
  if (rc != MPC_OK) Fail(m_Tag + "::EnableRewriteStats", rc);
}

bool DeviceCompressor::CheckRewriteValues(unsigned lineSize, unsigned granuleBytes, unsigned long long capacityLines, std::string &why)
{
  if (mpc_rewrite_check_values(lineSize, capacityLines, granuleBytes) == MPC_OK) return true;
  why = mpc_last_error(nullptr);
  return false;
}

RewriteReport DeviceCompressor::GetRewriteStats()
{
  FlushLines();
  RewriteReport report(m_LineSize);
  int rc = mpc_rewrite_stats_get(m_Handle, report.Table.data(), report.Table.size());
  if (rc != MPC_OK) Fail(m_Tag + "::GetRewriteStats", rc);
  return report;
}

void DeviceCompressor::SetLogClassField(int field)
{
  int rc = mpc_class_log_field(m_Handle, field);
  if (rc != MPC_OK) Fail(m_Tag + "::SetLogClassField", rc);
}

CompResult *DeviceCompressor::GetResult()
{
  FlushLines();
  uint64_t len = 0;
  mpc_stats_len(m_Handle, &len);
  std::vector<uint64_t> v(len);
  int rc = mpc_stats_get(m_Handle, v.data(), v.size());
  if (rc != MPC_OK) Fail(m_Tag + "::GetResult", rc);
  LoadResult(v.data());
  return m_Stat;
}

}  // namespace comp
