// Pattern.h -- the dataset analyser behind the reference's class names (reference src/compressor/Pattern.h):
// zero / repeated / already-seen / base-delta bytes and the byte entropy of a trace; evaluation on the MI355X via
// libmpc_hip.so (mpc_create_pattern).  The counts come from the device, the two entropies are computed here from the
// count maps, as the reference's Print does.  The reference's public m_DataCache member (its LRU of lines) has no
// counterpart: the set of lines lives in device memory (DistinctLines() is its size).  ADDITIVE: PatternOnFull::Evict
// models the reference's eviction beyond 2^24 - 1 lines (mpc_create_pattern_evicting); the default refuses such a trace.
#ifndef MPC_HOST_PATTERN_H
#define MPC_HOST_PATTERN_H

#include <map>

#include "CompResult.h"
#include "DeviceCompressor.h"

namespace comp
{

enum class PatternState {
  Base8Delta1 = 0, Base8Delta2 = 1, Base8Delta4 = 2, Base4Delta1 = 3, Base4Delta2 = 4, Base2Delta1 = 5,
  Zeros = 6, Repeat = 7, TemporalLocality = 8, NotDefined = 9,
};

struct PatternResult : public CompResult {
  PatternResult(unsigned lineSize) : CompResult(lineSize), ImplicitCounts(6, 0), ExplicitCounts(6, 0), Z(0), R(0), T(0), U(0), Total(0) {}
  // entropy = sum(-p * log2(p)) over the symbols of the map, ascending (Pattern.h:124-154)
  double ComputeEntropy(std::map<uint8_t, uint64_t> &symbolCounts);
  // the 22-column row (Pattern.h:156-217)
  virtual void Print(std::string workloadName = "", std::string filePath = "");
  // the statistics vector of a Pattern handle (mpc_hip.h); a symbol that never occurred has no map entry
  void LoadVector(const uint64_t *vec);

  std::vector<uint64_t> ImplicitCounts;
  std::vector<uint64_t> ExplicitCounts;
  std::map<uint8_t, uint64_t> SymbolCounts;
  std::map<uint8_t, uint64_t> SymbolCountsExceptAllZerosAllWordSame;
  uint64_t Z, R, T, U;   // Zeros, Repeated, TemporalLocality, NotDefined
  uint64_t Total;
};

// What the set of lines does when the 2^24-th distinct line arrives: stop with an error (the default), or evict as the
// reference's cache does -- a FIFO over insertions (include/mpc_hip.h: mpc_create_pattern_evicting).
enum class PatternOnFull { Refuse = 0, Evict = 1 };

class Pattern : public DeviceCompressor
{
public:
  Pattern(unsigned lineSize);
  // ADDITIVE.  capacity (Evict only): 0 for the reference's 2^24 - 1, or 1 .. 2^24 - 1 lines
  Pattern(unsigned lineSize, PatternOnFull onFull, unsigned long long capacity = 0);
  // lines that joined the set.  Refuse: its distinct lines (at most 2^24 - 1: the reference evicts beyond that, this evaluator
  // stops with an error).  Evict: its insertions (a line that was evicted and comes back is inserted again)
  unsigned long long DistinctLines();

protected:
  virtual void LoadResult(const uint64_t *v) { static_cast<PatternResult *>(m_Stat)->LoadVector(v); }
};

}  // namespace comp

#endif
