#include "RewriteReport.h"

#include <fstream>
#include <iostream>

#include "CompResult.h"

namespace comp
{

void RewriteReport::Print(std::string workloadName, std::string filePath)
{
  std::ofstream file;
  if (filePath != "")
    CompResult::openForAppend(file, filePath,
                              "Workload,Line Size,Granule Bytes,Lines,Distinct Lines,Rewrites,Grows,Shrinks,Equal Bits,Latest Granules,Peak Granules,"
                              "Image Granule Ratio,Peak Granule Ratio,Transitions,\n");
  std::ostream &stream = (filePath == "") ? std::cout : file;
  stream << workloadName << "," << LineSize << "," << GranuleBytes() << "," << Lines() << "," << DistinctLines() << "," << Rewrites() << "," << Grows() << ","
         << Shrinks() << "," << EqualBits() << "," << LatestGranules() << "," << PeakGranules() << "," << mpctext::num(ImageGranuleRatio()) << ","
         << mpctext::num(PeakGranuleRatio()) << ",";
  bool first = true;
  for (size_t c = 1; c <= Classes(); c++) {
    if (!First(c)) continue;
    stream << (first ? "" : ";") << "0>" << c << ":" << First(c);
    first = false;
  }
  for (size_t o = 1; o <= Classes(); o++)
    for (size_t c = 1; c <= Classes(); c++) {
      if (!Transitions(o, c)) continue;
      stream << (first ? "" : ";") << o << ">" << c << ":" << Transitions(o, c);
      first = false;
    }
  stream << "," << std::endl;
}

}  // namespace comp
