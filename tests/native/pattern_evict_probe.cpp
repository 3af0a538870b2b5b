// comp::Pattern in evicting mode (cal_22-mpc_amd/host/Pattern.h: PatternOnFull::Evict).  Test infrastructure
// (tests/test_pattern_evict_gpu.py), not product code.
//
//   pattern_evict_probe refuse <L> <capacity>                     (no device: the library refuses before it looks for one)
//     constructs comp::Pattern(L, Evict, capacity); the message and exit(1), or "not refused" and 0
//   pattern_evict_probe run <LINES.bin> <L> <capacity>            (needs the GPU)
//     all lines of the file, per route R "R <lines> <T> <Total> <insertions>":
//       a  CompressLine per line
//       c  CompressBatch of the first 113 lines, then of the rest
//       f  member of a CompressorSet of BDI and Pattern, fed like c
//     and "form <the set's form>"
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "BDI.h"
#include "CompressorSet.h"
#include "Pattern.h"

static void report(char route, comp::CompResult *r, unsigned long long insertions, size_t n)
{
  comp::PatternResult *p = static_cast<comp::PatternResult *>(r);
  std::printf("%c %llu %llu %llu %llu\n", route, (unsigned long long)n, (unsigned long long)p->T, (unsigned long long)p->Total, insertions);
}

template <class Sink>
static void twoBatches(Sink *c, const std::vector<uint8_t> &all, unsigned L)
{
  const size_t n = all.size() / L, first = n < 113 ? n : 113;
  c->CompressBatch(all.data(), first);
  c->CompressBatch(all.data() + first * L, n - first);
}

static int run(const std::string &path, unsigned L, unsigned long long capacity)
{
  FILE *f = std::fopen(path.c_str(), "rb");
  if (!f) return 3;
  std::vector<uint8_t> all;
  std::vector<uint8_t> line(L);
  while (std::fread(line.data(), 1, L, f) == L) all.insert(all.end(), line.begin(), line.end());
  std::fclose(f);
  const size_t n = all.size() / L;
  {
    comp::Pattern c(L, comp::PatternOnFull::Evict, capacity);
    for (size_t i = 0; i < n; i++) {
      line.assign(all.begin() + (long)(i * L), all.begin() + (long)((i + 1) * L));
      c.CompressLine(line);
    }
    report('a', c.GetResult(), c.DistinctLines(), n);
  }
  {
    comp::Pattern c(L, comp::PatternOnFull::Evict, capacity);
    twoBatches(&c, all, L);
    report('c', c.GetResult(), c.DistinctLines(), n);
  }
  {
    comp::BDI bdi(L);
    comp::Pattern c(L, comp::PatternOnFull::Evict, capacity);
    std::vector<comp::Compressor *> members = {&bdi, &c};
    comp::CompressorSet set(members);
    twoBatches(&set, all, L);
    report('f', set.GetResult(1), c.DistinctLines(), n);
    std::printf("form %s\n", set.GetForm().c_str());
  }
  return 0;
}

int main(int argc, char **argv)
{
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "refuse" && argc == 4) {
    comp::Pattern c((unsigned)std::atoi(argv[2]), comp::PatternOnFull::Evict, std::strtoull(argv[3], nullptr, 10));
    std::printf("not refused\n");
    return 0;
  }
  if (mode == "run" && argc == 5) return run(argv[2], (unsigned)std::atoi(argv[3]), std::strtoull(argv[4], nullptr, 10));
  std::fprintf(stderr, "usage: pattern_evict_probe refuse L CAPACITY | run LINES.bin L CAPACITY\n");
  return 2;
}
