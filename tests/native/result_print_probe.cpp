// result_print_probe.cpp -- CPU test driver: the CSV text of the host result classes (BDIResult / FPCResult /
// BPCResult::Print, cal_22-mpc_amd/host) for a given statistics vector (mpc_stats_get layout):
//   result_print_probe <BDI|FPC|BPC> <L> <workload> <csv path> <v0> <v1> ...
// appends to the csv file (header first when the file is new), like one run of the command line.
#include <cstdint>
#include <cstdlib>
#include <string>
#include <vector>

#include "BDI.h"
#include "BPC.h"
#include "FPC.h"

int main(int argc, char **argv)
{
  if (argc < 6) return 2;
  const std::string algo = argv[1];
  const unsigned L = (unsigned)std::atoi(argv[2]);
  std::vector<uint64_t> v;
  for (int i = 5; i < argc; i++) v.push_back(std::strtoull(argv[i], nullptr, 10));
  v.resize(16, 0);
  if (algo == "BDI") {
    comp::BDIResult r(L);
    r.LoadVector(v.data());
    r.Print(argv[3], argv[4]);
  } else if (algo == "FPC") {
    comp::FPCResult r(L);
    r.LoadVector(v.data());
    r.Print(argv[3], argv[4]);
  } else if (algo == "BPC") {
    comp::BPCResult r(L);
    r.LoadVector(v.data());
    r.Print(argv[3], argv[4]);
  } else {
    return 2;
  }
  return 0;
}
