#include "ImageReport.h"

#include <algorithm>
#include <fstream>
#include <iostream>

#include "CompResult.h"

namespace comp
{

void ImageReport::Print(std::string workloadName, std::string filePath)
{
  std::ofstream file;
  if (filePath != "")
    CompResult::openForAppend(file, filePath,
                              "Workload,Line Size,Block Lines,Sector Bytes,Header Bits,Lines,Distinct Lines,Blocks,Traffic Ratio,Image Ratio,Image Sector Ratio,Histogram,\n");
  std::ostream &stream = (filePath == "") ? std::cout : file;
  stream << workloadName << "," << LineSize << "," << BlockLines() << "," << SectorBytes() << "," << HeaderBits() << "," << Lines() << ","
         << DistinctLines() << "," << Blocks() << "," << mpctext::num(TrafficRatio()) << "," << mpctext::num(ImageRatio()) << ","
         << mpctext::num(ImageSectorRatio()) << ",";
  bool first = true;
  for (size_t k = 1; k <= (size_t)std::min<uint64_t>(BlockSectors(), MaxSectors); k++) {
    if (!BlocksOf(k)) continue;
    stream << (first ? "" : ";") << k << ":" << BlocksOf(k);
    first = false;
  }
  stream << "," << std::endl;
}

}  // namespace comp
