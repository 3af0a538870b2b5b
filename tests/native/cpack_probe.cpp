// comp::CPACK / comp::CPACKResult (cal_22-mpc_amd/host/CPACK.h).  Test infrastructure (tests/test_cpack_cpu.py,
// tests/test_cpack_gpu.py), not product code.
//
//   cpack_probe print <L> <workload> <csv> <v0> ... <v9>        (no device)
//     loads a statistics vector (the C-Pack layout of include/mpc_hip.h) into a CPACKResult, as CPACK::GetResult does,
//     prints "result <OriginalSize> <CompressedSize> <CompRatio %a> <TotalWords>" and lets Print append its row to <csv>
//   cpack_probe refuse <scope> <L>                               (no device: the library refuses before it looks for one)
//     constructs comp::CPACK(L, scope); the message and exit(1), or "not refused" and 0
//   cpack_probe run <TRACE.npy> <OUTDIR>                         (needs the GPU)
//     every row of the file but the last, per route R into OUTDIR/R.csv (Print, workload "probe_trace"):
//       a  CompressLine per line, the returned sizes as uint16 in OUTDIR/a.sizes
//       c  CompressBatch of the first 113 lines, then of the rest
//       d  CompressFile(TRACE.npy)
//       f  member of a CompressorSet of BDI, FPC, BPC and CPACK, fed like c
//     stdout: "R <lines>" per route and "form <the set's form>"
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

static void report(const std::string &out, char route, unsigned long long n, comp::CompResult *r)
{
  r->Print("probe_trace", out + "/" + route + ".csv");
  std::printf("%c %llu\n", route, n);
}

template <class Sink>
static void twoBatches(Sink *c, const std::vector<uint8_t> &all, unsigned L)
{
  const size_t n = all.size() / L, first = n < 113 ? n : 113;
  c->CompressBatch(all.data(), first);
  c->CompressBatch(all.data() + first * L, n - first);
}

static int run(const std::string &npy, const std::string &out)
{
  trace::LoaderNPY loader(npy);
  const unsigned L = loader.GetCachelineSize();
  std::vector<uint8_t> all((size_t)loader.GetNumLines() * L);
  const unsigned long long n = loader.GetBatch(all.data(), loader.GetNumLines());
  all.resize((size_t)n * L);
  {
    comp::CPACK c(L, comp::CPACKDictionary::PerLine);
    std::vector<uint16_t> sizes;
    std::vector<uint8_t> line(L);
    for (size_t i = 0; i < n; i++) {
      line.assign(all.begin() + (long)(i * L), all.begin() + (long)((i + 1) * L));
      sizes.push_back((uint16_t)c.CompressLine(line));
    }
    FILE *f = std::fopen((out + "/a.sizes").c_str(), "wb");
    if (!f) return 3;
    std::fwrite(sizes.data(), sizeof(uint16_t), sizes.size(), f);
    std::fclose(f);
    report(out, 'a', n, c.GetResult());
  }
  {
    comp::CPACK c(L, comp::CPACKDictionary::PerLine);
    twoBatches(&c, all, L);
    report(out, 'c', n, c.GetResult());
  }
  {
    comp::CPACK c(L, comp::CPACKDictionary::PerLine);
    report(out, 'd', c.CompressFile(npy), c.GetResult());
  }
  {
    comp::BDI bdi(L);
    comp::FPC fpc(L);
    comp::BPC bpc(L);
    comp::CPACK c(L, comp::CPACKDictionary::PerLine);
    std::vector<comp::Compressor *> members = {&bdi, &fpc, &bpc, &c};
    comp::CompressorSet set(members);
    twoBatches(&set, all, L);
    report(out, 'f', n, set.GetResult(3));
    std::printf("form %s\n", set.GetForm().c_str());
  }
  return 0;
}

int main(int argc, char **argv)
{
  const std::string mode = argc > 1 ? argv[1] : "";
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
  if (mode == "refuse" && argc == 4) {
    comp::CPACK c((unsigned)std::atoi(argv[3]), (comp::CPACKDictionary)std::atoi(argv[2]));
    std::printf("not refused\n");
    return 0;
  }
  if (mode == "run" && argc == 4) return run(argv[2], argv[3]);
  std::fprintf(stderr, "usage: cpack_probe print L WORKLOAD CSV V0..V9 | refuse SCOPE L | run TRACE.npy OUTDIR\n");
  return 2;
}
