#include "BPC.h"

#include <cstdio>
#include <cstdlib>

#include "mpc_hip.h"

namespace comp
{

// reference BPC.h:35-84
void BPCResult::Print(std::string workloadName, std::string filePath)
{
  std::ofstream file;
  if (filePath != "")
    openForAppend(file, filePath,
                  "Workload,Original Size,Compressed Size,Compression Ratio,Total Words,Pattern0,Pattern1,Pattern2,Pattern3,"
                  "Pattern4,Pattern5,Pattern6,\n");
  std::ostream &stream = (filePath == "") ? std::cout : file;
  stream << workloadName << "," << OriginalSize << "," << CompressedSize << "," << mpctext::num(CompRatio) << ",";
  stream << TotalWords << ",";
  for (int i = 0; i < NUM_BPC_PATTERN; i++) stream << Counts[(size_t)i] << ",";
  stream << std::endl;
}

void BPCResult::LoadVector(const uint64_t *v)
{
  OriginalSize = v[1];
  CompressedSize = v[2];
  CompRatio = v[0] ? (double)OriginalSize / (double)CompressedSize : 0.0;
  TotalWords = v[3];
  for (int i = 0; i < NUM_BPC_PATTERN; i++) Counts[(size_t)i] = v[4 + i];
}

BPC::BPC(unsigned lineSize) : DeviceCompressor("BPC", lineSize)
{
  CheckCreated(mpc_create_bpc(lineSize, -1, &m_Handle));
  m_Stat = new BPCResult(lineSize);
  m_Stat->CompressorName = "Bit-Plane Compression";
}

}  // namespace comp
