// SizeReport.h -- ADDITIVE, no counterpart in the reference: the distribution of the per-line compressed sizes of one
// evaluator (DeviceCompressor::GetSizeHistogram) or of the per-line best of a set (CompressorSet::GetBest), and what it
// means for a memory system that moves lines in sectors of SectorBytes bytes (ACCESS_GRAN in the reference).  The
// reference writes a size histogram for VPC only (VPCResult::PrintDetail); this one is the same for all evaluators.
#ifndef MPC_HOST_SIZEREPORT_H
#define MPC_HOST_SIZEREPORT_H

#include <cstdint>
#include <string>
#include <vector>

#include "Loader.h"

namespace comp
{

struct SizeReport {
  explicit SizeReport(unsigned lineSize, unsigned sectorBytes = ACCESS_GRAN) : LineSize(lineSize), SectorBytes(sectorBytes) {}

  // Appends one row to filePath (stdout for ""), the header first when the file does not exist yet, as the result
  // classes' Print does:
  //   Workload,Line Size,Lines,Sector Bytes,Sector Ratio,Sector Classes,Histogram,
  // Sector Classes: lines that occupy 1, 2, ... ceil(LineSize / SectorBytes) sectors, joined by ';' (mpc_size_sectors,
  // include/mpc_hip_sizes.h); Sector Ratio: uncompressed sectors / occupied sectors, formatted like CompRatio;
  // Histogram: the non-empty bins as size:count in ascending size, joined by ';'.
  void Print(std::string workloadName = "", std::string filePath = "");

  std::vector<uint64_t> Bins;      // MPC_SIZE_BINS entries: lines per size in bits (empty: no lines)
  unsigned LineSize;
  unsigned SectorBytes;
};

// best-of of a CompressorSet: the histogram of the per-line smallest size and who won
struct BestReport {
  explicit BestReport(unsigned lineSize) : Sizes(lineSize) {}
  // original bits / (BestBits + Lines x TagBits); 0 without lines
  double CompRatio() const
  {
    const double comp = (double)(BestBits + Lines * TagBits);
    return comp > 0 ? (double)(Lines * 8ull * Sizes.LineSize) / comp : 0.0;
  }
  SizeReport Sizes;                // sizes without tag bits
  std::vector<uint64_t> Wins;      // per member of the set; 0 for a member that does not take part (Pattern)
  uint64_t BestBits = 0, Lines = 0;
  unsigned TagBits = 0;            // ceil(log2(members taking part)): what a hybrid stores per line to name the winner
};

}  // namespace comp

#endif
