// RewriteReport.h -- ADDITIVE, no counterpart in the reference: how the size of a line changes when its address is
// evaluated again -- per distinct line address the sequence of sizes in trace order, as transitions between size classes
// of granule_bytes bytes, first touches, and the latest and peak size per address (DeviceCompressor::GetRewriteStats,
// CompressorSet::GetRewriteStats).  Next to ImageReport.h, which keeps only the latest size.
#ifndef MPC_HOST_REWRITEREPORT_H
#define MPC_HOST_REWRITEREPORT_H

#include <cstdint>
#include <string>
#include <vector>

#include "Loader.h"

namespace comp
{

struct RewriteReport {
  static constexpr size_t MaxClasses = 32, TableLen = 144 + MaxClasses * MaxClasses;      // MPC_REWRITE_MAX_CLASSES, MPC_REWRITE_TABLE_LEN (include/mpc_hip_rewrite.h)

  explicit RewriteReport(unsigned lineSize) : Table(TableLen, 0), LineSize(lineSize) {}

  // Appends one row to filePath (stdout for ""), the header first when the file does not exist yet, as the result
  // classes' Print does:
  //   Workload,Line Size,Granule Bytes,Lines,Distinct Lines,Rewrites,Grows,Shrinks,Equal Bits,Latest Granules,Peak Granules,Image Granule Ratio,Peak Granule Ratio,Transitions,
  // the two ratios formatted like CompRatio; Transitions: "old>new:count" for every non-zero entry, old 0 for a first
  // touch, first touches first, then ascending by old and new, joined by ';'.
  void Print(std::string workloadName = "", std::string filePath = "");

  uint64_t Lines() const { return Table[0]; }
  uint64_t Bits() const { return Table[1]; }
  uint64_t DistinctLines() const { return Table[2]; }
  uint64_t Misaligned() const { return Table[3]; }
  uint64_t Rewrites() const { return Table[4]; }
  uint64_t Grows() const { return Table[5]; }
  uint64_t Shrinks() const { return Table[6]; }
  uint64_t EqualBits() const { return Table[7]; }
  uint64_t LatestGranules() const { return Table[8]; }
  uint64_t PeakGranules() const { return Table[9]; }
  uint64_t LatestBits() const { return Table[10]; }
  uint64_t PeakBits() const { return Table[11]; }
  unsigned GranuleBytes() const { return (unsigned)Table[12]; }
  uint64_t Capacity() const { return Table[13]; }
  // G: the classes of a line, ceil(L / granule_bytes)
  size_t Classes() const { return (size_t)Table[14] <= MaxClasses ? (size_t)Table[14] : MaxClasses; }
  // first touches in class c; keys whose latest / peak class is c; c = 1 .. Classes()
  uint64_t First(size_t c) const { return Table[16 + c - 1]; }
  uint64_t LatestIn(size_t c) const { return Table[48 + c - 1]; }
  uint64_t PeakIn(size_t c) const { return Table[80 + c - 1]; }
  // keys observed 2^b .. 2^(b + 1) - 1 times, b = 0 .. 31
  uint64_t CountLog2(size_t b) const { return Table[112 + b]; }
  // rewrites from class cOld to class cNew
  uint64_t Transitions(size_t cOld, size_t cNew) const { return Table[144 + (cOld - 1) * MaxClasses + (cNew - 1)]; }
  // Grows / Rewrites, DistinctLines x G / LatestGranules, DistinctLines x G / PeakGranules, Lines x 8 L / Bits; each 0
  // where its divisor is 0
  double OverflowRate() const { return Rewrites() ? (double)Grows() / (double)Rewrites() : 0.0; }
  double ImageGranuleRatio() const { return LatestGranules() ? (double)(DistinctLines() * Table[14]) / (double)LatestGranules() : 0.0; }
  double PeakGranuleRatio() const { return PeakGranules() ? (double)(DistinctLines() * Table[14]) / (double)PeakGranules() : 0.0; }
  double TrafficRatio() const { return Bits() ? (double)(Lines() * 8 * LineSize) / (double)Bits() : 0.0; }

  std::vector<uint64_t> Table;     // the layout of mpc_rewrite_stats_get
  unsigned LineSize;
};

}  // namespace comp

#endif
