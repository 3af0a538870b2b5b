// ImageReport.h -- ADDITIVE, no counterpart in the reference: the compressed image of the memory a trace touches, by line
// address -- per distinct line the size of the latest line evaluated there, and the sectors that address-aligned blocks
// of N lines of it occupy when packed and rounded up once (DeviceCompressor::GetImageStats,
// CompressorSet::GetImageStats).  Next to PackReport.h, whose blocks are consecutive requests of the traffic.
#ifndef MPC_HOST_IMAGEREPORT_H
#define MPC_HOST_IMAGEREPORT_H

#include <cstdint>
#include <string>
#include <vector>

#include "Loader.h"

namespace comp
{

struct ImageReport {
  static constexpr size_t MaxSectors = 1024, TableLen = 16 + MaxSectors;      // MPC_IMAGE_MAX_SECTORS, MPC_IMAGE_TABLE_LEN (include/mpc_hip_image.h)

  explicit ImageReport(unsigned lineSize) : Table(TableLen, 0), LineSize(lineSize) {}

  // Appends one row to filePath (stdout for ""), the header first when the file does not exist yet, as the result
  // classes' Print does:
  //   Workload,Line Size,Block Lines,Sector Bytes,Header Bits,Lines,Distinct Lines,Blocks,Traffic Ratio,Image Ratio,Image Sector Ratio,Histogram,
  // the three ratios formatted like CompRatio; Histogram: "k:blocks" for every number of sectors k that touched blocks
  // occupy, ascending, joined by ';'.
  void Print(std::string workloadName = "", std::string filePath = "");

  uint64_t Lines() const { return Table[0]; }
  uint64_t Bits() const { return Table[1]; }
  uint64_t DistinctLines() const { return Table[2]; }
  uint64_t ImageBits() const { return Table[3]; }
  uint64_t Blocks() const { return Table[4]; }
  uint64_t Sectors() const { return Table[5]; }
  uint64_t Caps() const { return Table[6]; }
  uint64_t Misaligned() const { return Table[7]; }
  uint64_t BlockLines() const { return Table[8]; }
  unsigned SectorBytes() const { return (unsigned)Table[9]; }
  unsigned HeaderBits() const { return (unsigned)Table[10]; }
  uint64_t Capacity() const { return Table[11]; }
  // S_B: the sectors of an uncompressed, fully touched block
  uint64_t BlockSectors() const { return SectorBytes() ? (BlockLines() * LineSize + SectorBytes() - 1) / SectorBytes() : 0; }
  // touched blocks that occupy k sectors, k = 1 .. BlockSectors()
  uint64_t BlocksOf(size_t k) const { return Table[16 + k - 1]; }
  // Lines x 8 L / Bits, DistinctLines x 8 L / ImageBits, Caps / Sectors; each 0 where its divisor is 0
  double TrafficRatio() const { return Bits() ? (double)(Lines() * 8 * LineSize) / (double)Bits() : 0.0; }
  double ImageRatio() const { return ImageBits() ? (double)(DistinctLines() * 8 * LineSize) / (double)ImageBits() : 0.0; }
  double ImageSectorRatio() const { return Sectors() ? (double)Caps() / (double)Sectors() : 0.0; }

  std::vector<uint64_t> Table;     // the layout of mpc_image_stats_get
  unsigned LineSize;
};

}  // namespace comp

#endif
