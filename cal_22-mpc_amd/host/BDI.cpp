#include "BDI.h"

#include <cstdio>
#include <cstdlib>

#include "mpc_hip.h"

namespace comp
{

void BDIResult::Print(std::string workloadName, std::string filePath)
{
  std::ofstream file;
  if (filePath != "")
    openForAppend(file, filePath,
                  "Workload,Original Size,Compressed Size,Compression Ratio,Zeros,Repeated,B8D1,B8D2,B8D4,B4D1,B4D2,"
                  "B2D1,Uncompressed,\n");
  std::ostream &stream = (filePath == "") ? std::cout : file;
  stream << workloadName << "," << OriginalSize << "," << CompressedSize << "," << mpctext::num(CompRatio) << ",";
  for (int i = 0; i < 9; i++) stream << Counts[(size_t)i] << ",";
  stream << std::endl;
}

void BDIResult::LoadVector(const uint64_t *v)
{
  OriginalSize = v[1];
  CompressedSize = v[2];
  CompRatio = v[0] ? (double)OriginalSize / (double)CompressedSize : 0.0;
  for (int i = 0; i < 9; i++) Counts[(size_t)i] = v[3 + i];
}

BDI::BDI(unsigned lineSize) : DeviceCompressor("BDI", lineSize)
{
  CheckCreated(mpc_create_bdi(lineSize, -1, &m_Handle));
  m_Stat = new BDIResult(lineSize);
  m_Stat->CompressorName = "Base-Delta Immediate";
}

}  // namespace comp
