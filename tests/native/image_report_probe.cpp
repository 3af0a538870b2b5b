// comp::ImageReport (cal_22-mpc_amd/host/ImageReport.h) without a device:
//   image_report_probe <csv> <line size> <workload> <table entry 0> ... <table entry 11> [k:blocks ...]
// fills a report's table from the arguments -- the twelve leading entries of an image table, then the touched blocks
// that occupy k sectors -- and lets Print append its row to <csv>.  Built with the address and undefined-behaviour
// sanitizers by tests/test_image_cpu.py.
#include <cstdio>
#include <cstdlib>

#include "ImageReport.h"

int main(int argc, char **argv)
{
  if (argc < 16) return 2;
  comp::ImageReport report((unsigned)atoi(argv[2]));
  for (int i = 0; i < 12; i++) report.Table[(size_t)i] = strtoull(argv[4 + i], nullptr, 10);
  for (int i = 16; i < argc; i++) {
    char *p = nullptr;
    const unsigned long long k = strtoull(argv[i], &p, 10);
    if (*p != ':' || k < 1 || k > comp::ImageReport::MaxSectors) return 3;
    report.Table[16 + k - 1] = strtoull(p + 1, nullptr, 10);
  }
  report.Print(argv[3], argv[1]);
  return 0;
}
