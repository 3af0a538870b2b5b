#include "PackReport.h"

#include <algorithm>
#include <fstream>
#include <iostream>

#include "CompResult.h"

namespace comp
{

uint64_t PackReport::TailCap() const
{
  return (TailLines() && SectorBytes()) ? (TailLines() * LineSize + SectorBytes() - 1) / SectorBytes() : 0;
}

uint64_t PackReport::TailSectors() const
{
  const uint64_t cap = TailCap();
  if (!cap) return 0;
  const uint64_t sectorBits = 8ull * SectorBytes();
  return std::min(std::max<uint64_t>(1, (TailBits() + HeaderBits() + sectorBits - 1) / sectorBits), cap);
}

double PackReport::SectorRatio() const
{
  const uint64_t occupied = Sectors() + TailSectors();
  return occupied ? (double)(Blocks() * BlockSectors() + TailCap()) / (double)occupied : 0.0;
}

void PackReport::Print(std::string workloadName, std::string filePath)
{
  std::ofstream file;
  if (filePath != "")
    CompResult::openForAppend(file, filePath, "Workload,Line Size,Block Lines,Sector Bytes,Header Bits,Blocks,Tail Lines,Sector Ratio,Histogram,\n");
  std::ostream &stream = (filePath == "") ? std::cout : file;
  stream << workloadName << "," << LineSize << "," << BlockLines() << "," << SectorBytes() << "," << HeaderBits() << "," << Blocks() << ","
         << TailLines() << "," << mpctext::num(SectorRatio()) << ",";
  bool first = true;
  for (size_t k = 1; k <= (size_t)std::min<uint64_t>(BlockSectors(), MaxSectors); k++) {
    if (!BlocksOf(k)) continue;
    stream << (first ? "" : ";") << k << ":" << BlocksOf(k);
    first = false;
  }
  stream << "," << std::endl;
}

}  // namespace comp
