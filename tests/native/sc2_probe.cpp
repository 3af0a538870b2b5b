// The reference driver's use of comp::SC2 against cal_22-mpc_amd/host/SC2.h (libmpc_hip.so underneath):
//   sc2_probe <lines.bin> <trace.npy> <L> <S>
// prints "<mode> <OriginalSize> <CompressedSize> <name>" for three fresh compressors: CompressLine per line (the
// reference loop), CompressBatch in chunks of 1000 lines, CompressFile of the .npy (all rows but the last).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "SC2.h"

static void report(const char *mode, comp::Compressor *c)
{
  comp::CompResult *r = c->GetResult();
  printf("%s %llu %llu %s\n", mode, (unsigned long long)r->OriginalSize, (unsigned long long)r->CompressedSize,
         c->GetCompressorName().c_str());
}

int main(int argc, char **argv)
{
  if (argc != 5) return 2;
  const unsigned L = (unsigned)atoi(argv[3]);
  const unsigned S = (unsigned)strtoul(argv[4], nullptr, 10);
  std::vector<uint8_t> all;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 3;
  std::vector<uint8_t> line(L);
  while (fread(line.data(), 1, L, f) == L) all.insert(all.end(), line.begin(), line.end());
  fclose(f);
  const size_t n = all.size() / L;
  {
    comp::SC2 c(L, S);
    for (size_t i = 0; i < n; i++) {
      line.assign(all.begin() + (long)(i * L), all.begin() + (long)((i + 1) * L));
      c.CompressLine(line);
    }
    report("line", &c);
  }
  {
    comp::SC2 c(L, 1);
    c.SetSamplingCnt(S);
    for (size_t i = 0; i < n; i += 1000) c.CompressBatch(all.data() + i * L, (n - i) < 1000 ? (n - i) : 1000);
    report("batch", &c);
  }
  {
    comp::SC2 c(L, S);
    c.CompressFile(argv[2]);
    report("file", &c);
  }
  return 0;
}
