// comp::ClassReport (cal_22-mpc_amd/host/ClassReport.h) without a device:
//   class_report_probe <csv> <line size> <sector bytes> <workload> [class:bits:s1;s2;... ...]
// fills a report's table from the arguments -- s_k: lines of the class that occupy k sectors, their sum the class's lines
// -- (none: a report without lines; the table is then left empty) and lets Print append its rows to <csv>.  Built with the
// address and undefined-behaviour sanitizers by tests/test_classes_cpu.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "ClassReport.h"

int main(int argc, char **argv)
{
  if (argc < 5) return 2;
  comp::ClassReport report((unsigned)atoi(argv[2]), (unsigned)atoi(argv[3]));
  for (int i = 5; i < argc; i++) {
    char *p = nullptr;
    const unsigned long long cls = strtoull(argv[i], &p, 10);
    if (*p != ':' || cls >= comp::ClassReport::Classes) return 3;
    const unsigned long long bits = strtoull(p + 1, &p, 10);
    if (*p != ':') return 3;
    if (report.Table.empty()) report.Table.assign(comp::ClassReport::Classes * comp::ClassReport::Row, 0);
    uint64_t *row = report.Table.data() + cls * comp::ClassReport::Row;
    row[1] += bits;
    for (size_t k = 1; *p && k <= comp::ClassReport::Row - 2; k++) {
      const unsigned long long lines = strtoull(p + 1, &p, 10);
      row[1 + k] += lines;
      row[0] += lines;
    }
  }
  report.Print(argv[4], argv[1]);
  return 0;
}
