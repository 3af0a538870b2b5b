// BDI.h -- Base-Delta-Immediate baseline behind the reference's class names
// (reference src/compressor/BDI.h); evaluation on the MI355X via libmpc_hip.so.
#ifndef MPC_HOST_BDI_H
#define MPC_HOST_BDI_H

#include "CompResult.h"
#include "DeviceCompressor.h"

namespace comp
{

enum class BDIState {
  Zeros = 0, Repeat = 1, Base8Delta1 = 2, Base8Delta2 = 3, Base8Delta4 = 4,
  Base4Delta1 = 5, Base4Delta2 = 6, Base2Delta1 = 7, Uncompressed = 8
};

struct BDIResult : public CompResult {
  BDIResult(unsigned lineSize) : CompResult(lineSize), Counts(9, 0) {}
  virtual void Update(unsigned uncompSize, unsigned compSize, int selected)
  {
    CompResult::Update(uncompSize, compSize);
    Counts[(size_t)selected]++;
  }
  virtual void Print(std::string workloadName = "", std::string filePath = "");
  void LoadVector(const uint64_t *vec);
  std::vector<uint64_t> Counts;
};

class BDI : public DeviceCompressor
{
public:
  BDI(unsigned lineSize);

protected:
  virtual void LoadResult(const uint64_t *v) { static_cast<BDIResult *>(m_Stat)->LoadVector(v); }
};

}  // namespace comp

#endif
