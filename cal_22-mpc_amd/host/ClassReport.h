// ClassReport.h -- ADDITIVE, no counterpart in the reference: one evaluator's lines, compressed bits and sector counts
// broken down by a per-line class (DeviceCompressor::GetClassStats, CompressorSet::GetClassStats): the reads and the
// writes of a trace, its kernels, or the lines that each VPC cluster takes.  Next to SizeReport.h, which has the
// distribution for the whole trace.
#ifndef MPC_HOST_CLASSREPORT_H
#define MPC_HOST_CLASSREPORT_H

#include <cstdint>
#include <string>
#include <vector>

#include "Loader.h"

namespace comp
{

struct ClassReport {
  static constexpr size_t Classes = 256, Row = 10;      // MPC_CLASS_COUNT, MPC_CLASS_ROW (include/mpc_hip_classes.h)

  explicit ClassReport(unsigned lineSize, unsigned sectorBytes = ACCESS_GRAN) : LineSize(lineSize), SectorBytes(sectorBytes) {}

  // Appends one row per class that has lines to filePath (stdout for ""), in ascending class order, the header first
  // when the file does not exist yet, as the result classes' Print does:
  //   Workload,Class,Lines,Original Bits,Compressed Bits,Ratio,Sector Ratio,
  // Original Bits: Lines x 8 x LineSize; Ratio: Original Bits / Compressed Bits (0 without compressed bits); Sector
  // Ratio: uncompressed sectors / occupied sectors; both formatted like CompRatio.
  void Print(std::string workloadName = "", std::string filePath = "");

  uint64_t Lines(size_t c) const { return Table.empty() ? 0 : Table[c * Row]; }
  uint64_t Bits(size_t c) const { return Table.empty() ? 0 : Table[c * Row + 1]; }
  // lines of class c that occupy k sectors, k = 1 .. ceil(LineSize / SectorBytes)
  uint64_t Sectors(size_t c, size_t k) const { return Table.empty() ? 0 : Table[c * Row + 1 + k]; }

  std::vector<uint64_t> Table;     // Classes x Row entries, the layout of mpc_class_stats_get (empty: no lines)
  unsigned LineSize;
  unsigned SectorBytes;
};

}  // namespace comp

#endif
