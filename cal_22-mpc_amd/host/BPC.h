// BPC.h -- Bit-Plane Compression baseline behind the reference's class names
// (reference src/compressor/BPC.h); evaluation on the MI355X via libmpc_hip.so.
#ifndef MPC_HOST_BPC_H
#define MPC_HOST_BPC_H

#include "CompResult.h"
#include "DeviceCompressor.h"

#define NUM_BPC_PATTERN 7

namespace comp
{

enum class BPCPattern { Uncomp = 0, ZRLE = 1, Zero = 2, SingleOne = 3, ConsecTwoOnes = 4, ZeroDBP = 5, AllOnes = 6 };

struct BPCResult : public CompResult {
  BPCResult(unsigned lineSize) : CompResult(lineSize), Counts(NUM_BPC_PATTERN, 0), TotalWords(0) {}
  void UpdatePattern(unsigned numWords, int selected)
  {
    TotalWords += numWords;
    Counts[(size_t)selected]++;
  }
  virtual void Print(std::string workloadName = "", std::string filePath = "");
  void LoadVector(const uint64_t *vec);
  std::vector<uint64_t> Counts;
  uint64_t TotalWords;
};

class BPC : public DeviceCompressor
{
public:
  BPC(unsigned lineSize);

protected:
  virtual void LoadResult(const uint64_t *v) { static_cast<BPCResult *>(m_Stat)->LoadVector(v); }
};

}  // namespace comp

#endif
