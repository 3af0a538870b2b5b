#include "SC2.h"

#include <cstdio>
#include <cstdlib>

#include "mpc_hip.h"

namespace comp
{

SC2::SC2(unsigned lineSize, unsigned warmupCnt) : DeviceCompressor("SC2", lineSize)
{
  CheckCreated(mpc_create_sc2(lineSize, warmupCnt, -1, &m_Handle));
  m_Stat = new CompResult(lineSize);
  m_Stat->CompressorName = "SC2-Huffman";
}

void SC2::SetSamplingCnt(unsigned cnt)
{
  if (Fed()) {
    printf("SC2::SetSamplingCnt after the first line is not supported (the warm-up sample has begun).\n");
    exit(1);
  }
  mpc_destroy(m_Handle);
  m_Handle = nullptr;
  int rc = mpc_create_sc2(m_LineSize, cnt, -1, &m_Handle);
  if (rc != MPC_OK) Fail("SC2::SetSamplingCnt", rc);
}

void SC2::LoadResult(const uint64_t *v)
{
  m_Stat->OriginalSize = v[1];
  m_Stat->CompressedSize = v[2];
  m_Stat->CompRatio = v[0] ? (double)v[1] / (double)v[2] : 0.0;
}

}  // namespace comp
