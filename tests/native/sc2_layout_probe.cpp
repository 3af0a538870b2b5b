// sc2_layout_probe -- mpcsc2::layout (csrc/mpc_sc2.h) on the host, and the sizing kernel's lookup restated over its image.
//
//   usage: sc2_layout_probe FILE
//   FILE:  "n q", then n lines "key length" (keys ascending, as sc2_build passes them), then q query words
//   out:   "layout mask seed1 seed2"            (or "layout failed")
//          "image w w w ..."                    the nb x 4 dwords of the bucket image
//          "query word length|miss"             one per query, by sc2_word_bits' rule: the second bucket is read only
//                                               for a word whose first bucket is full
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "mpc_sc2.h"

namespace {

struct Bucket { uint32_t x, y, z, w; };

// sc2_probe (mpc_sc2.hip)
uint32_t probe(Bucket b, uint32_t k, bool &hit)
{
  const uint32_t c = b.w >> 30;
  hit = true;
  if (c > 0u && b.x == k) return b.w & 1023u;
  if (c > 1u && b.y == k) return (b.w >> 10) & 1023u;
  if (c > 2u && b.z == k) return (b.w >> 20) & 1023u;
  hit = false;
  return MPC_SC2_MISS_BITS;
}

// sc2_word_bits (mpc_sc2.hip)
uint32_t word_bits(const std::vector<uint32_t> &image, const MpcSc2Table &T, uint32_t k, bool &hit)
{
  auto bucket = [&](uint32_t i) { return Bucket{image[4 * (size_t)i], image[4 * (size_t)i + 1], image[4 * (size_t)i + 2], image[4 * (size_t)i + 3]}; };
  const Bucket b = bucket(mpc_sc2_hash(k, T.seed1) & T.mask);
  uint32_t len = probe(b, k, hit);
  if (!hit && (b.w >> 30) == 3u) len = probe(bucket(mpc_sc2_hash(k, T.seed2) & T.mask), k, hit);
  return len;
}

}  // namespace

int main(int argc, char **argv)
{
  if (argc != 2) return 2;
  FILE *f = std::fopen(argv[1], "r");
  if (!f) return 2;
  size_t n = 0, q = 0;
  if (std::fscanf(f, "%zu %zu", &n, &q) != 2 || n > MPC_SC2_ENTRIES) return 2;
  std::vector<uint32_t> keys(n), queries(q);
  std::vector<uint16_t> lens(n);
  for (size_t i = 0; i < n; i++) {
    unsigned len = 0;
    if (std::fscanf(f, "%" SCNu32 " %u", &keys[i], &len) != 2) return 2;
    lens[i] = (uint16_t)len;
  }
  for (size_t i = 0; i < q; i++)
    if (std::fscanf(f, "%" SCNu32, &queries[i]) != 1) return 2;
  std::fclose(f);
  std::vector<uint32_t> image;
  MpcSc2Table T{};
  if (!mpcsc2::layout(keys, lens, image, T)) {
    std::printf("layout failed\n");
    return 1;
  }
  std::printf("layout %" PRIu32 " %" PRIu32 " %" PRIu32 "\n", T.mask, T.seed1, T.seed2);
  std::printf("image");
  for (uint32_t w : image) std::printf(" %" PRIu32, w);
  std::printf("\n");
  for (uint32_t k : queries) {
    bool hit = false;
    const uint32_t len = word_bits(image, T, k, hit);
    if (hit) std::printf("query %" PRIu32 " %" PRIu32 "\n", k, len);
    else std::printf("query %" PRIu32 " miss\n", k);
  }
  return 0;
}
