// PackReport.h -- ADDITIVE, no counterpart in the reference: the sectors that blocks of N consecutive lines occupy when
// their compressed lines are packed and the block is rounded up to whole sectors once (DeviceCompressor::GetPackStats,
// CompressorSet::GetPackStats).  Next to SizeReport.h and ClassReport.h, which round every line on its own.
#ifndef MPC_HOST_PACKREPORT_H
#define MPC_HOST_PACKREPORT_H

#include <cstdint>
#include <string>
#include <vector>

#include "Loader.h"

namespace comp
{

struct PackReport {
  static constexpr size_t MaxSectors = 1024, TableLen = 8 + MaxSectors;      // MPC_PACK_MAX_SECTORS, MPC_PACK_TABLE_LEN (include/mpc_hip_pack.h)

  explicit PackReport(unsigned lineSize) : Table(TableLen, 0), LineSize(lineSize) {}

  // Appends one row to filePath (stdout for ""), the header first when the file does not exist yet, as the result
  // classes' Print does:
  //   Workload,Line Size,Block Lines,Sector Bytes,Header Bits,Blocks,Tail Lines,Sector Ratio,Histogram,
  // Blocks: the closed blocks; Tail Lines: the lines behind the last of them; Sector Ratio: SectorRatio(), the tail
  // included, formatted like CompRatio; Histogram: "k:blocks" for every number of sectors k that closed blocks occupy,
  // ascending, joined by ';'.
  void Print(std::string workloadName = "", std::string filePath = "");

  uint64_t Blocks() const { return Table[0]; }
  uint64_t PayloadBits() const { return Table[1]; }
  uint64_t Sectors() const { return Table[2]; }
  uint64_t TailLines() const { return Table[3]; }
  uint64_t TailBits() const { return Table[4]; }
  uint64_t BlockLines() const { return Table[5]; }
  unsigned SectorBytes() const { return (unsigned)Table[6]; }
  unsigned HeaderBits() const { return (unsigned)Table[7]; }
  // S_B: the sectors of an uncompressed block
  uint64_t BlockSectors() const { return SectorBytes() ? (BlockLines() * LineSize + SectorBytes() - 1) / SectorBytes() : 0; }
  // closed blocks that occupy k sectors, k = 1 .. BlockSectors()
  uint64_t BlocksOf(size_t k) const { return Table[8 + k - 1]; }
  // the tail closed as a short block (mpc_pack_sectors_of_tail): its sectors, and those of its lines uncompressed; 0 without a tail
  uint64_t TailSectors() const;
  uint64_t TailCap() const;
  // (Blocks x S_B + TailCap) / (Sectors + TailSectors); 0 without sectors
  double SectorRatio() const;

  std::vector<uint64_t> Table;     // the layout of mpc_pack_stats_get
  unsigned LineSize;
};

}  // namespace comp

#endif
