// CPACK.h -- C-Pack behind the reference's class names (reference src/compressor/CPACK.h), evaluated on the MI355X via
// libmpc_hip.so WITH A PER-LINE DICTIONARY: the numbers of a fresh reference comp::CPACK per line.  The reference's own
// object carries its 16-entry dictionary from line to line (CPACK.h:107-113, CPACK.cpp:86-93); that scope is not offered
// (DESIGN.md 8), so the constructor takes the scope and gives it no default: `new comp::CPACK(lineSize)` written for the
// reference does not compile here rather than compile into other numbers.
// ADDITIVE: CPACK(lineSize, CPACKDictionary::PerBlock, blockLines) -- one dictionary per block of blockLines lines, the
// numbers of a fresh reference comp::CPACK every blockLines lines (mpc_create_cpack_blocks in include/mpc_hip.h: the
// result depends on where blocks begin, a block is one lane's sequential work, blockLines beyond the trace is the
// reference's own run on a single lane).
#ifndef MPC_HOST_CPACK_H
#define MPC_HOST_CPACK_H

#include "CompResult.h"
#include "DeviceCompressor.h"

#define NUM_CPACK_PATTERN 6

namespace comp
{

enum class CPACKPattern { ZZZZ = 0, ZZZX = 1, MMMM = 2, MMMX = 3, MMXX = 4, XXXX = 5 };

// where the dictionary starts afresh; Carried (the reference's driver) is refused by the library with a message
// PerBlock goes with the three-argument constructor only
enum class CPACKDictionary { Carried = 0, PerLine = 1, PerBlock = 2 };

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
  // scope: PerBlock (anything else: a message and exit(1)); blockLines: 1 .. 2^32 - 1
  CPACK(unsigned lineSize, CPACKDictionary scope, uint64_t blockLines);
  // PerBlock: the next line starts a block (a second trace through the same object); buffered lines are evaluated first
  void Restart();
  uint64_t GetBlockLines() const { return m_BlockLines; }      // 0: per-line dictionary

protected:
  virtual void LoadResult(const uint64_t *v) { static_cast<CPACKResult *>(m_Stat)->LoadVector(v); }

private:
  uint64_t m_BlockLines = 0;
};

}  // namespace comp

#endif
