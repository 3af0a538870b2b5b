// comp::PatternResult (cal_22-mpc_amd/host/Pattern.h) without a device:
//   pattern_probe <stats.bin> <workload> <csv>
// loads a statistics vector of 534 uint64 (the layout of include/mpc_hip.h) into a PatternResult, as Pattern::GetResult
// does, prints "entropy <%a> <%a>" and "counts Z R T U Total", and lets Print append its row to <csv>.
#include <cstdio>
#include <vector>

#include "Pattern.h"

int main(int argc, char **argv)
{
  if (argc != 4) return 2;
  std::vector<uint64_t> v(534);
  FILE *f = fopen(argv[1], "rb");
  if (!f || fread(v.data(), sizeof(uint64_t), v.size(), f) != v.size()) return 3;
  fclose(f);
  comp::PatternResult r(64);
  r.LoadVector(v.data());
  printf("entropy %a %a\n", r.ComputeEntropy(r.SymbolCounts), r.ComputeEntropy(r.SymbolCountsExceptAllZerosAllWordSame));
  printf("counts %llu %llu %llu %llu %llu\n", (unsigned long long)r.Z, (unsigned long long)r.R, (unsigned long long)r.T,
         (unsigned long long)r.U, (unsigned long long)r.Total);
  printf("maps %zu %zu\n", r.SymbolCounts.size(), r.SymbolCountsExceptAllZerosAllWordSame.size());
  printf("result %llu %llu %a\n", (unsigned long long)r.OriginalSize, (unsigned long long)r.CompressedSize, r.CompRatio);
  r.Print(argv[2], argv[3]);
  return 0;
}
