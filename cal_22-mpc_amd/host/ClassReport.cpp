#include "ClassReport.h"

#include <fstream>
#include <iostream>

#include "CompResult.h"

namespace comp
{

void ClassReport::Print(std::string workloadName, std::string filePath)
{
  const size_t most = SectorBytes ? ((size_t)LineSize + SectorBytes - 1) / SectorBytes : 0;
  if (most == 0 || most > Row - 2 || SectorBytes > LineSize) {
    std::cout << "ClassReport: sectors of " << SectorBytes << " bytes do not fit lines of " << LineSize << " bytes (1 to " << Row - 2
              << " sectors a line)." << std::endl;
    exit(1);
  }
  std::ofstream file;
  if (filePath != "") CompResult::openForAppend(file, filePath, "Workload,Class,Lines,Original Bits,Compressed Bits,Ratio,Sector Ratio,\n");
  std::ostream &stream = (filePath == "") ? std::cout : file;
  for (size_t c = 0; c < Classes; c++) {
    const uint64_t lines = Lines(c);
    if (!lines) continue;
    const uint64_t original = lines * 8ull * LineSize, compressed = Bits(c);
    uint64_t occupied = 0;
    for (size_t k = 1; k <= most; k++) occupied += k * Sectors(c, k);
    const double ratio = compressed ? (double)original / (double)compressed : 0.0;
    const double sectorRatio = occupied ? (double)(lines * most) / (double)occupied : 0.0;
    stream << workloadName << "," << c << "," << lines << "," << original << "," << compressed << "," << mpctext::num(ratio) << ","
           << mpctext::num(sectorRatio) << "," << std::endl;
  }
}

}  // namespace comp
