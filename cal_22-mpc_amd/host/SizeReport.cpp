#include "SizeReport.h"

#include <fstream>
#include <iostream>

#include "CompResult.h"
#include "mpc_hip.h"

namespace comp
{

void SizeReport::Print(std::string workloadName, std::string filePath)
{
  std::vector<uint64_t> bins(Bins);
  bins.resize(MPC_SIZE_BINS, 0);
  const size_t nClasses = SectorBytes ? ((size_t)LineSize + SectorBytes - 1) / SectorBytes : 0;
  std::vector<uint64_t> classes(nClasses, 0);
  uint64_t sectors = 0, lines = 0;
  double ratio = 0;
  if (mpc_size_sectors(bins.data(), bins.size(), LineSize, SectorBytes, classes.data(), nClasses, &sectors, &ratio) != MPC_OK) {
    std::cout << "SizeReport: sectors of " << SectorBytes << " bytes do not divide lines of " << LineSize << " bytes." << std::endl;
    exit(1);
  }
  for (uint64_t c : classes) lines += c;

  std::ofstream file;
  if (filePath != "") CompResult::openForAppend(file, filePath, "Workload,Line Size,Lines,Sector Bytes,Sector Ratio,Sector Classes,Histogram,\n");
  std::ostream &stream = (filePath == "") ? std::cout : file;
  stream << workloadName << "," << LineSize << "," << lines << "," << SectorBytes << "," << mpctext::num(ratio) << ",";
  for (size_t c = 0; c < classes.size(); c++) stream << (c ? ";" : "") << classes[c];
  stream << ",";
  bool first = true;
  for (size_t s = 0; s < bins.size(); s++) {
    if (!bins[s]) continue;
    stream << (first ? "" : ";") << s << ":" << bins[s];
    first = false;
  }
  stream << "," << std::endl;
}

}  // namespace comp
