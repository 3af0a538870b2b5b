// evaluator_probe.cpp -- every route into each of the six GPU evaluators of cal_22-mpc_amd/host (comp::VPC, BDI, FPC,
// BPC, SC2, Pattern: one comp::DeviceCompressor underneath), a fresh evaluator per route.  Test infrastructure
// (tests/test_host_evaluators_gpu.py), not product code.
//
//   evaluator_probe run CONFIG.json TRACE.npy TRACE.log KEPT.npy OUTDIR
//     per class TAG and route R, OUTDIR/TAG.R.csv (Print) and OUTDIR/TAG.R.detail.csv (PrintDetail):
//       a  CompressLine per line, the returned sizes as uint16 in OUTDIR/TAG.a.sizes
//       b  the same after SetLineBuffering(7), sizes in OUTDIR/TAG.b.sizes
//       c  CompressBatch of the first 113 lines, then of the rest
//       d  CompressFile(TRACE.npy)          e  CompressFile(TRACE.log)
//       f  member of a CompressorSet of all six, fed like c
//       k  like c, over the lines of KEPT.npy
//     stdout: "TAG R <lines>" per route
//   evaluator_probe refuse sc2-line|sc2-handle|bdi-short|vpc-short CONFIG.json
//     what an evaluator refuses with a message and exit(1); 0 if it did not
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "BDI.h"
#include "BPC.h"
#include "CompressorSet.h"
#include "FPC.h"
#include "LoaderNPY.h"
#include "Pattern.h"
#include "SC2.h"
#include "VPC.h"

static const char *kTags[6] = {"VPC", "BDI", "FPC", "BPC", "SC2", "Pattern"};
static const unsigned kWarmup = 100;

static comp::Compressor *make(const std::string &tag, const std::string &config, unsigned L)
{
  if (tag == "VPC") return new comp::VPC(config);
  if (tag == "BDI") return new comp::BDI(L);
  if (tag == "FPC") return new comp::FPC(L);
  if (tag == "BPC") return new comp::BPC(L);
  if (tag == "SC2") return new comp::SC2(L, kWarmup);
  return new comp::Pattern(L);
}

// every row but the last, as the reference driver sees a .npy file
static std::vector<uint8_t> readLines(const std::string &npy, unsigned &L)
{
  trace::LoaderNPY loader(npy);
  L = loader.GetCachelineSize();
  std::vector<uint8_t> all((size_t)loader.GetNumLines() * L);
  const unsigned long long n = loader.GetBatch(all.data(), loader.GetNumLines());
  all.resize((size_t)n * L);
  return all;
}

static void report(const std::string &out, const std::string &tag, char route, unsigned long long n, comp::CompResult *r)
{
  const std::string stem = out + "/" + tag + "." + route;
  r->Print("probe_trace", stem + ".csv");
  r->PrintDetail("probe_trace", stem + ".detail.csv");
  std::printf("%s %c %llu\n", tag.c_str(), route, n);
}

static void perLine(comp::Compressor *c, const std::vector<uint8_t> &all, unsigned L, const std::string &sizesPath)
{
  std::vector<uint16_t> sizes;
  std::vector<uint8_t> line(L);
  for (size_t i = 0; i < all.size() / L; i++) {
    line.assign(all.begin() + (long)(i * L), all.begin() + (long)((i + 1) * L));
    sizes.push_back((uint16_t)c->CompressLine(line));
  }
  FILE *f = std::fopen(sizesPath.c_str(), "wb");
  if (!f) std::exit(3);
  std::fwrite(sizes.data(), sizeof(uint16_t), sizes.size(), f);
  std::fclose(f);
}

template <class Sink>
static void twoBatches(Sink *c, const std::vector<uint8_t> &all, unsigned L)
{
  const size_t n = all.size() / L, first = n < 113 ? n : 113;
  c->CompressBatch(all.data(), first);
  c->CompressBatch(all.data() + first * L, n - first);
}

static int run(const std::string &config, const std::string &npy, const std::string &log, const std::string &keptNpy,
               const std::string &out)
{
  unsigned L = 0, keptL = 0;
  const std::vector<uint8_t> all = readLines(npy, L), kept = readLines(keptNpy, keptL);
  if (keptL != L) return 4;
  const unsigned long long n = all.size() / L;
  for (const char *t : kTags) {
    const std::string tag = t;
    for (char route : std::string("abcdek")) {
      comp::Compressor *c = make(tag, config, L);
      unsigned long long done = n;
      if (route == 'a') perLine(c, all, L, out + "/" + tag + ".a.sizes");
      if (route == 'b') {
        c->SetLineBuffering(7);
        perLine(c, all, L, out + "/" + tag + ".b.sizes");
      }
      if (route == 'c') twoBatches(c, all, L);
      if (route == 'd') done = c->CompressFile(npy);
      if (route == 'e') done = c->CompressFile(log);
      if (route == 'k') {
        twoBatches(c, kept, L);
        done = kept.size() / L;
      }
      report(out, tag, route, done, c->GetResult());
      delete c;
    }
  }
  std::vector<comp::Compressor *> members;
  for (const char *t : kTags) members.push_back(make(t, config, L));
  {
    comp::CompressorSet set(members);
    twoBatches(&set, all, L);
    for (size_t i = 0; i < members.size(); i++) report(out, kTags[i], 'f', n, set.GetResult(i));
  }
  for (comp::Compressor *c : members) delete c;
  return 0;
}

static int refuse(const std::string &what, const std::string &config)
{
  std::vector<uint8_t> line(64, 0), half(32, 0);
  if (what == "sc2-line" || what == "sc2-handle") {
    comp::SC2 c(64, kWarmup);
    if (what == "sc2-line") c.CompressLine(line);
    else (void)c.DeviceHandle();
    c.SetSamplingCnt(50);
  } else if (what == "bdi-short") {
    comp::BDI c(64);
    c.CompressLine(half);
  } else if (what == "vpc-short") {
    comp::VPC c(config);
    c.CompressLine(half);
  } else {
    return 2;
  }
  std::printf("not refused\n");
  return 0;
}

int main(int argc, char **argv)
{
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "run" && argc == 7) return run(argv[2], argv[3], argv[4], argv[5], argv[6]);
  if (mode == "refuse" && argc == 4) return refuse(argv[2], argv[3]);
  std::fprintf(stderr, "usage: evaluator_probe run CONFIG TRACE.npy TRACE.log KEPT.npy OUTDIR | refuse CASE CONFIG\n");
  return 2;
}
