// result_print_probe.cpp -- CPU test driver: the CSV text of the host result classes (BDIResult / FPCResult /
// BPCResult::Print, VPCResult::Print / PrintDetail, cal_22-mpc_amd/host) for a given statistics vector (mpc_stats_get
// layout):
//   result_print_probe <BDI|FPC|BPC> <L> <workload> <csv path> <v0> <v1> ...
//   result_print_probe VPC <L> <workload> <csv path> <detail csv path> <modules> <histogram bins> <v0> <v1> ...
// appends to the csv file(s) (header first when a file is new), like one run of the command line.
#include <cstdint>
#include <cstdlib>
#include <string>
#include <vector>

#include "BDI.h"
#include "BPC.h"
#include "FPC.h"
#include "VPC.h"

int main(int argc, char **argv)
{
  if (argc < 6) return 2;
  const std::string algo = argv[1];
  const unsigned L = (unsigned)std::atoi(argv[2]);
  if (algo == "VPC") {
    if (argc < 9) return 2;
    const int M = std::atoi(argv[6]), bins = std::atoi(argv[7]);
    std::vector<uint64_t> vv;
    for (int i = 8; i < argc; i++) vv.push_back(std::strtoull(argv[i], nullptr, 10));
    if (M < 1 || bins < 1 || vv.size() != 3 + (size_t)(M + 1) * (6 + (size_t)bins)) return 3;
    comp::VPCResult r(L, M);
    r.LoadVector(vv.data(), M, bins);
    r.Print(argv[3], argv[4]);
    r.PrintDetail(argv[3], argv[5]);
    return 0;
  }
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
