// comp::PackReport (cal_22-mpc_amd/host/PackReport.h) without a device:
//   pack_report_probe <csv> <line size> <workload> <table entry 0> ... <table entry 7> [k:blocks ...]
// fills a report's table from the arguments -- the eight leading entries of a pack table, then the closed blocks that
// occupy k sectors -- and lets Print append its row to <csv>.  Built with the address and undefined-behaviour
// sanitizers by tests/test_pack_cpu.py.
#include <cstdio>
#include <cstdlib>

#include "PackReport.h"

int main(int argc, char **argv)
{
  if (argc < 12) return 2;
  comp::PackReport report((unsigned)atoi(argv[2]));
  for (int i = 0; i < 8; i++) report.Table[(size_t)i] = strtoull(argv[4 + i], nullptr, 10);
  for (int i = 12; i < argc; i++) {
    char *p = nullptr;
    const unsigned long long k = strtoull(argv[i], &p, 10);
    if (*p != ':' || k < 1 || k > comp::PackReport::MaxSectors) return 3;
    report.Table[8 + k - 1] = strtoull(p + 1, nullptr, 10);
  }
  report.Print(argv[3], argv[1]);
  return 0;
}
