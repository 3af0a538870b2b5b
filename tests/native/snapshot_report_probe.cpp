// comp::SnapshotReport (cal_22-mpc_amd/host/SnapshotReport.h) without a device:
//   snapshot_report_probe <csv> <line size> <skip|zero> <workload> <stats entry 0> ... <stats entry 4> <plan entry 0> ... <plan entry 5>
// fills a report from the arguments -- the five leading entries of a snapshot's stats vector, the six of a plan -- and
// lets Print append its row to <csv>.  Built with the address and undefined-behaviour sanitizers by
// tests/test_snapshot_cpu.py.
#include <cstdlib>
#include <cstring>

#include "SnapshotReport.h"

int main(int argc, char **argv)
{
  if (argc != 16) return 2;
  if (strcmp(argv[3], "skip") != 0 && strcmp(argv[3], "zero") != 0) return 3;
  comp::SnapshotReport report((unsigned)atoi(argv[2]), strcmp(argv[3], "zero") == 0);
  for (int i = 0; i < 5; i++) report.Stats[(size_t)i] = strtoull(argv[5 + i], nullptr, 10);
  for (int i = 0; i < 6; i++) report.Plan[(size_t)i] = strtoull(argv[10 + i], nullptr, 10);
  report.Print(argv[4], argv[1]);
  return 0;
}
