#include "Pattern.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "mpc_hip.h"

namespace comp
{

double PatternResult::ComputeEntropy(std::map<uint8_t, uint64_t> &symbolCounts)
{
  uint64_t sum = 0;
  for (auto &kv : symbolCounts) sum += kv.second;
  double entropy = 0;
  for (auto &kv : symbolCounts) {
    const double probability = (double)kv.second / (double)sum;
    entropy += -probability * log2(probability);
  }
  return entropy;
}

void PatternResult::Print(std::string workloadName, std::string filePath)
{
  std::ofstream file;
  if (filePath != "")
    openForAppend(file, filePath,
                  "Workload,Entropy [b/B],Entropy except AllZeros AllWordSame [b/B],Zeros [B],Repeated Line [B],"
                  "Temporal Locality [B],B8D1-Implicit [B],B8D1-Explicit [B],B8D2-Implicit [B],B8D2-Explicit [B],"
                  "B8D4-Implicit [B],B8D4-Explicit [B],B4D1-Implicit [B],B4D1-Explicit [B],B4D2-Implicit [B],"
                  "B4D2-Explicit [B],B2D1-Implicit [B],B2D1-Explicit [B],Undefined [B],Total Size [B],\n");
  std::ostream &stream = (filePath == "") ? std::cout : file;
  stream << workloadName << "," << mpctext::num(ComputeEntropy(SymbolCounts)) << ","
         << mpctext::num(ComputeEntropy(SymbolCountsExceptAllZerosAllWordSame)) << ",";
  stream << Z << "," << R << "," << T << ",";
  for (int i = 0; i < 6; i++) stream << ImplicitCounts[(size_t)i] << "," << ExplicitCounts[(size_t)i] << ",";
  stream << U << "," << Total << "," << std::endl;
}

void PatternResult::LoadVector(const uint64_t *v)
{
  // CompResult::Update is never called by the reference's Pattern: the three CompResult numbers stay 0
  OriginalSize = 0;
  CompressedSize = 0;
  CompRatio = 0;
  Z = v[4];
  R = v[5];
  T = v[6];
  U = v[7];
  Total = v[8];
  for (int i = 0; i < 6; i++) {
    ImplicitCounts[(size_t)i] = v[9 + i];
    ExplicitCounts[(size_t)i] = v[15 + i];
  }
  SymbolCounts.clear();
  SymbolCountsExceptAllZerosAllWordSame.clear();
  for (int b = 0; b < 256; b++) {
    if (v[22 + b]) SymbolCounts[(uint8_t)b] = v[22 + b];
    if (v[278 + b]) SymbolCountsExceptAllZerosAllWordSame[(uint8_t)b] = v[278 + b];
  }
}

Pattern::Pattern(unsigned lineSize) : DeviceCompressor("Pattern", lineSize)
{
  CheckCreated(mpc_create_pattern(lineSize, -1, &m_Handle));
  m_Stat = new PatternResult(lineSize);
  m_Stat->CompressorName = "Pattern Checker";
}

Pattern::Pattern(unsigned lineSize, PatternOnFull onFull, unsigned long long capacity) : DeviceCompressor("Pattern", lineSize)
{
  if (onFull == PatternOnFull::Evict) {
    CheckCreated(mpc_create_pattern_evicting(lineSize, capacity, -1, &m_Handle));
  } else {
    if (capacity != 0 || onFull != PatternOnFull::Refuse) fail("Pattern: a capacity belongs to PatternOnFull::Evict, and there is no third mode", MPC_E_INVAL, "");
    CheckCreated(mpc_create_pattern(lineSize, -1, &m_Handle));
  }
  m_Stat = new PatternResult(lineSize);
  m_Stat->CompressorName = "Pattern Checker";
}

unsigned long long Pattern::DistinctLines()
{
  FlushLines();
  uint64_t n = 0;
  int rc = mpc_pattern_distinct_lines(m_Handle, &n);
  if (rc != MPC_OK) Fail("Pattern::DistinctLines", rc);
  return n;
}

}  // namespace comp
