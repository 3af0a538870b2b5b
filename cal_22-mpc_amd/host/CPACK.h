// CPACK.h -- C-Pack behind the reference's class names (reference src/compressor/CPACK.h), evaluated on the MI355X via
// libmpc_hip.so WITH A PER-LINE DICTIONARY: the numbers of a fresh reference comp::CPACK per line.  The reference's own
// object carries its 16-entry dictionary from line to line (CPACK.h:107-113, CPACK.cpp:86-93); that scope is not offered
// (DESIGN.md 8), so the constructor takes the scope and gives it no default: `new comp::CPACK(lineSize)` written for the
// reference does not compile here rather than compile into other numbers.
#ifndef MPC_HOST_CPACK_H
#define MPC_HOST_CPACK_H

#include "CompResult.h"
#include "DeviceCompressor.h"

#define NUM_CPACK_PATTERN 6

namespace comp
{

enum class CPACKPattern { ZZZZ = 0, ZZZX = 1, MMMM = 2, MMMX = 3, MMXX = 4, XXXX = 5 };

// where the dictionary starts afresh; Carried (the reference's driver) is refused by the library with a message
enum class CPACKDictionary { Carried = 0, PerLine = 1 };

struct CPACKResult : public CompResult {
  CPACKResult(unsigned lineSize) : CompResult(lineSize), Counts(NUM_CPACK_PATTERN, 0), TotalWords(0) {}
  void UpdatePattern(int selected)
  {
    TotalWords++;
    Counts[(size_t)selected]++;
  }
  virtual void Print(std::string workloadName = "", std::string filePath = "");
  void LoadVector(const uint64_t *vec);
  std::vector<uint64_t> Counts;
  uint64_t TotalWords;
};

class CPACK : public DeviceCompressor
{
public:
  CPACK(unsigned lineSize, CPACKDictionary scope);

protected:
  virtual void LoadResult(const uint64_t *v) { static_cast<CPACKResult *>(m_Stat)->LoadVector(v); }
};

}  // namespace comp

#endif
