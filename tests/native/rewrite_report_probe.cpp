// comp::RewriteReport (cal_22-mpc_amd/host/RewriteReport.h) without a device:
//   rewrite_report_probe <csv> <line size> <workload> <table entry 0> ... <table entry 14> [old>new:count ...]
// fills a report's table from the arguments -- the fifteen leading entries of a rewrite table, then first touches (old 0)
// and transitions -- and lets Print append its row to <csv>.  Built with the address and undefined-behaviour sanitizers
// by tests/test_rewrite_cpu.py.
#include <cstdio>
#include <cstdlib>

#include "RewriteReport.h"

int main(int argc, char **argv)
{
  if (argc < 19) return 2;
  comp::RewriteReport report((unsigned)atoi(argv[2]));
  for (int i = 0; i < 15; i++) report.Table[(size_t)i] = strtoull(argv[4 + i], nullptr, 10);
  for (int i = 19; i < argc; i++) {
    char *p = nullptr, *q = nullptr;
    const unsigned long long o = strtoull(argv[i], &p, 10);
    if (*p != '>') return 3;
    const unsigned long long c = strtoull(p + 1, &q, 10);
    if (*q != ':' || o > comp::RewriteReport::MaxClasses || c < 1 || c > comp::RewriteReport::MaxClasses) return 3;
    const unsigned long long v = strtoull(q + 1, nullptr, 10);
    if (o == 0) report.Table[16 + c - 1] = v;
    else report.Table[144 + (o - 1) * comp::RewriteReport::MaxClasses + (c - 1)] = v;
  }
  report.Print(argv[3], argv[1]);
  return 0;
}
