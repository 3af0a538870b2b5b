// comp::CPACK(lineSize, CPACKDictionary::PerBlock, blockLines) (cal_22-mpc_amd/host/CPACK.h).  Test infrastructure
// (tests/test_cpack_blocks_cpu.py, tests/test_cpack_blocks_gpu.py), not product code.
//
//   cpack_blocks_probe refuse <scope> <L> <N>                     (no device: refused before one is looked for)
//     constructs comp::CPACK(L, scope, N); the message and exit(1), or "not refused" and 0
//   cpack_blocks_probe print <L> <workload> <csv> <v0> ... <v9>   (no device)
//     a statistics vector (the C-Pack layout of include/mpc_hip.h) into a CPACKResult, as CPACK::GetResult does:
//     "result <OriginalSize> <CompressedSize> <CompRatio %a> <TotalWords>", and Print appends its row to <csv>
//   cpack_blocks_probe run <TRACE.npy> <N>                        (needs the GPU)
//     every row of the file but the last through CompressFile, per route "R <lines> <OriginalSize> <CompressedSize>
//     <CompRatio %a> <TotalWords> <Counts x 6>":
//       d  comp::CPACK(L, PerBlock, N) alone
//       e  the same object after Restart(), the file once more (totals of both passes)
//       f  member of a CompressorSet of BDI, FPC, BPC, CPACK(L, PerLine) and CPACK(L, PerBlock, N)
//     then "form <the set's form>" and "blocks <GetBlockLines()>"
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "BDI.h"
#include "BPC.h"
#include "CPACK.h"
#include "CompressorSet.h"
#include "FPC.h"
#include "LoaderNPY.h"

static void row(char route, unsigned long long n, comp::CompResult *res)
{
  comp::CPACKResult *r = static_cast<comp::CPACKResult *>(res);
  std::printf("%c %llu %llu %llu %a %llu", route, n, (unsigned long long)r->OriginalSize, (unsigned long long)r->CompressedSize, r->CompRatio,
              (unsigned long long)r->TotalWords);
  for (uint64_t c : r->Counts) std::printf(" %llu", (unsigned long long)c);
  std::printf("\n");
}

static int run(const std::string &npy, uint64_t N)
{
  unsigned L = 0;
  {
    trace::LoaderNPY loader(npy);
    L = loader.GetCachelineSize();
  }
  {
    comp::CPACK c(L, comp::CPACKDictionary::PerBlock, N);
    row('d', c.CompressFile(npy), c.GetResult());
    c.Restart();
    row('e', c.CompressFile(npy), c.GetResult());
    std::printf("blocks %llu\n", (unsigned long long)c.GetBlockLines());
  }
  {
    comp::BDI bdi(L);
    comp::FPC fpc(L);
    comp::BPC bpc(L);
    comp::CPACK line(L, comp::CPACKDictionary::PerLine);
    comp::CPACK c(L, comp::CPACKDictionary::PerBlock, N);
    std::vector<comp::Compressor *> members = {&bdi, &fpc, &bpc, &line, &c};
    comp::CompressorSet set(members);
    row('f', set.CompressFile(npy), set.GetResult(4));
    std::printf("form %s\n", set.GetForm().c_str());
  }
  return 0;
}

int main(int argc, char **argv)
{
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "refuse" && argc == 5) {
    comp::CPACK c((unsigned)std::atoi(argv[3]), (comp::CPACKDictionary)std::atoi(argv[2]), std::strtoull(argv[4], nullptr, 10));
    std::printf("not refused\n");
    return 0;
  }
  if (mode == "print" && argc == 15) {
    std::vector<uint64_t> v;
    for (int i = 5; i < argc; i++) v.push_back(std::strtoull(argv[i], nullptr, 10));
    comp::CPACKResult r((unsigned)std::atoi(argv[2]));
    r.LoadVector(v.data());
    std::printf("result %llu %llu %a %llu\n", (unsigned long long)r.OriginalSize, (unsigned long long)r.CompressedSize, r.CompRatio,
                (unsigned long long)r.TotalWords);
    r.Print(argv[3], argv[4]);
    return 0;
  }
  if (mode == "run" && argc == 4) return run(argv[2], std::strtoull(argv[3], nullptr, 10));
  std::fprintf(stderr, "usage: cpack_blocks_probe refuse SCOPE L N | print L WORKLOAD CSV V0..V9 | run TRACE.npy N\n");
  return 2;
}
