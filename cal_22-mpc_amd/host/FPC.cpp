#include "FPC.h"

#include <cstdio>
#include <cstdlib>

#include "mpc_hip.h"

namespace comp
{

// reference FPC.h:40-84
void FPCResult::Print(std::string workloadName, std::string filePath)
{
  std::ofstream file;
  if (filePath != "")
    openForAppend(file, filePath,
                  "Workload,Original Size,Compressed Size,Compression Ratio,Total Words,Prefix0,Prefix1,Prefix2,Prefix3,"
                  "Prefix4,Prefix5,Prefix6,Prefix7,\n");
  std::ostream &stream = (filePath == "") ? std::cout : file;
  stream << workloadName << "," << OriginalSize << "," << CompressedSize << "," << mpctext::num(CompRatio) << ",";
  stream << TotalWords << ",";
  for (int i = 0; i < NUM_FPC_PATTERN; i++) stream << Counts[(size_t)i] << ",";
  stream << std::endl;
}

void FPCResult::LoadVector(const uint64_t *v)
{
  OriginalSize = v[1];
  CompressedSize = v[2];
  CompRatio = v[0] ? (double)OriginalSize / (double)CompressedSize : 0.0;
  TotalWords = 0;
  for (int i = 0; i < NUM_FPC_PATTERN; i++) {
    Counts[(size_t)i] = v[3 + i];
    TotalWords += v[3 + i];
  }
}

FPC::FPC(unsigned lineSize) : DeviceCompressor("FPC", lineSize)
{
  CheckCreated(mpc_create_fpc(lineSize, -1, &m_Handle));
  m_Stat = new FPCResult(lineSize);
  m_Stat->CompressorName = "Frequent Pattern Compression";
}

}  // namespace comp
