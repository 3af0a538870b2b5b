#include "CPACK.h"

#include <cstdio>
#include <cstdlib>

#include "mpc_hip.h"

namespace comp
{

// reference CPACK.h:45-91
void CPACKResult::Print(std::string workloadName, std::string filePath)
{
  std::ofstream file;
  if (filePath != "")
    openForAppend(file, filePath,
                  "Workload,Original Size,Compressed Size,Compression Ratio,Total Words,Pattern0,Pattern1,Pattern2,Pattern3,"
                  "Pattern4,Pattern5,\n");
  std::ostream &stream = (filePath == "") ? std::cout : file;
  stream << workloadName << "," << OriginalSize << "," << CompressedSize << "," << mpctext::num(CompRatio) << ",";
  stream << TotalWords << ",";
  for (int i = 0; i < NUM_CPACK_PATTERN; i++) stream << Counts[(size_t)i] << ",";
  stream << std::endl;
}

void CPACKResult::LoadVector(const uint64_t *v)
{
  OriginalSize = v[1];
  CompressedSize = v[2];
  CompRatio = v[0] ? (double)OriginalSize / (double)CompressedSize : 0.0;
  TotalWords = v[3];
  for (int i = 0; i < NUM_CPACK_PATTERN; i++) Counts[(size_t)i] = v[4 + i];
}

CPACK::CPACK(unsigned lineSize, CPACKDictionary scope) : DeviceCompressor("CPACK", lineSize)
{
  CheckCreated(mpc_create_cpack(lineSize, (int)scope, -1, &m_Handle));
  m_Stat = new CPACKResult(lineSize);
  m_Stat->CompressorName = "C-Pack";
}

CPACK::CPACK(unsigned lineSize, CPACKDictionary scope, uint64_t blockLines) : DeviceCompressor("CPACK", lineSize), m_BlockLines(blockLines)
{
  if (scope != CPACKDictionary::PerBlock)
    fail("CPACK: cannot create the evaluator", MPC_E_INVAL, "C-Pack: a block length goes with CPACKDictionary::PerBlock only");
  CheckCreated(mpc_create_cpack_blocks(lineSize, blockLines, -1, &m_Handle));
  m_Stat = new CPACKResult(lineSize);
  m_Stat->CompressorName = "C-Pack";
}

void CPACK::Restart()
{
  FlushLines();
  int rc = mpc_cpack_blocks_restart(m_Handle);
  if (rc != MPC_OK) Fail("CPACK::Restart", rc);
}

}  // namespace comp
