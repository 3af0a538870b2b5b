// comp::SizeReport (cal_22-mpc_amd/host/SizeReport.h) without a device:
//   size_report_probe <csv> <line size> <sector bytes> <workload> [size:count ...]
// fills a report's histogram from the size:count pairs (none: a report without lines; the bins are then left empty) and lets
// Print append its row to <csv>.  Built with the address and undefined-behaviour sanitizers by tests/test_size_hist_cpu.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "SizeReport.h"
#include "mpc_hip.h"

int main(int argc, char **argv)
{
  if (argc < 5) return 2;
  comp::SizeReport report((unsigned)atoi(argv[2]), (unsigned)atoi(argv[3]));
  for (int i = 5; i < argc; i++) {
    const char *colon = strchr(argv[i], ':');
    if (!colon) return 3;
    const unsigned long long size = strtoull(argv[i], nullptr, 10), count = strtoull(colon + 1, nullptr, 10);
    if (size >= MPC_SIZE_BINS) return 4;
    if (report.Bins.empty()) report.Bins.assign(MPC_SIZE_BINS, 0);
    report.Bins[size] += count;
  }
  report.Print(argv[4], argv[1]);
  return 0;
}
