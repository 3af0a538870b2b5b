// mpc_sc2.h -- SC2 (reference src/compressor/SC2.cpp): the host side of the code table, shared by the C ABI
// (mpc_capi.hip: sc2_build, launch_sc2) and the kernels (mpc_sc2.hip; their launchers: mpc_launch.h).
//
//   code_lengths()   the reference's table build, step for step: eviction to the 1024 largest (freq, symbol) pairs
//                    (SC2.cpp:292-308), MinHeap over the kept symbols in ascending symbol order (:24-37), the Huffman
//                    loop with its ExtractMin / AddNode (:92-148), code length = leaf depth (:150-161).  Any optimal
//                    code has the same total size on the sample, but not the same per-symbol lengths where frequencies
//                    tie, so the heap is replayed exactly.  No HIP call: mpc_sc2_code_lengths exposes it for CPU tests.
//   layout()         the table as the sizing kernel reads it from LDS: nb buckets of 16 B, three keys and one dword of
//                    three 10-bit code lengths plus a 2-bit entry count.  A key sits in bucket h(k, seed1) or, only when
//                    that bucket is full, in h(k, seed2); the host tries seeds in a fixed order until every key fits, so
//                    a lookup is one 16-B probe, two only for words that hash to a full bucket.
#pragma once

#include <stdint.h>

#define MPC_SC2_ENTRIES 1024          /* HEAP_CAPACITY = SC2_ENTRIES (SC2.h:15, SC2.cpp:6) */
#define MPC_SC2_MAX_BUCKETS 2048      /* 2 x entries: 32 KiB of LDS */
#define MPC_SC2_RAW_LEN 2             /* [0] compressed_bits  [1] words found in the table */
#define MPC_SC2_MISS_BITS 33          /* a word not in the table: 32 bits + 1 tag bit (SC2.cpp:323-327) */
#define MPC_SC2_EVICTED 0xffffu       /* mpc_sc2_code_lengths: the symbol did not make the 1024 */

struct MpcSc2Table {
  const void *buckets;   /* device: nb x uint4 {key0, key1, key2, len0 | len1 << 10 | len2 << 20 | count << 30} */
  uint32_t mask;         /* nb - 1 (nb a power of two, 2 .. MPC_SC2_MAX_BUCKETS) */
  uint32_t seed1, seed2;
};

// bucket hash of a 32-bit word (both sides)
#ifdef __HIPCC__
__host__ __device__
#endif
static inline uint32_t mpc_sc2_hash(uint32_t k, uint32_t seed)
{
  uint32_t h = (k ^ seed) * 0x9E3779B1u;
  h ^= h >> 15;
  h *= 0x2C1B3C6Du;
  h ^= h >> 12;
  return h;
}

#include <algorithm>
#include <utility>
#include <vector>

namespace mpcsc2 {

// Code lengths of n distinct symbols with their warm-up frequencies, in input order; MPC_SC2_EVICTED for a symbol
// outside the 1024 kept ones.  Returns 0, or -22 for n == 0 (the reference builds from an empty map: undefined).
inline int code_lengths(const uint32_t *sym, const uint64_t *freq, size_t n, uint16_t *out)
{
  if (n == 0 || !sym || !freq || !out) return -22;
  std::vector<size_t> order(n);
  for (size_t i = 0; i < n; i++) order[i] = i;
  for (size_t i = 0; i < n; i++) out[i] = MPC_SC2_EVICTED;
  // erase from the front of the (freq asc, symbol asc) order until 1024 remain (huffman::cmp, SC2.cpp:257)
  if (n > MPC_SC2_ENTRIES) {
    std::sort(order.begin(), order.end(), [&](size_t a, size_t b) {
      return freq[a] == freq[b] ? sym[a] < sym[b] : freq[a] < freq[b];
    });
    order.erase(order.begin(), order.begin() + (std::ptrdiff_t)(n - MPC_SC2_ENTRIES));
  }
  // MinHeap(std::map): leaves in ascending symbol order
  std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return sym[a] < sym[b]; });
  const size_t m = order.size();
  struct Node { uint64_t freq; int left, right; };
  std::vector<Node> nodes;
  nodes.reserve(2 * m);
  for (size_t i = 0; i < m; i++) nodes.push_back(Node{freq[order[i]], -1, -1});
  std::vector<int> heap(m);
  for (size_t i = 0; i < m; i++) heap[i] = (int)i;
  int size = (int)m;
  auto f = [&](int i) { return nodes[(size_t)heap[(size_t)i]].freq; };
  auto heapify = [&](int i) {      // MinHeap::minHeapify (tail recursion as a loop)
    for (;;) {
      int mi = i;
      const int l = 2 * i + 1, r = 2 * i + 2;
      if (l <= size - 1 && f(l) < f(mi)) mi = l;
      if (r <= size - 1 && f(r) < f(mi)) mi = r;
      if (mi == i) return;
      std::swap(heap[(size_t)i], heap[(size_t)mi]);
      i = mi;
    }
  };
  for (int i = size / 2 - 1; i >= 0; i--) heapify(i);     // buildHeap
  auto extract = [&]() {                                  // ExtractMin: swap root and last, shrink, sift down
    const int top = heap[0];
    std::swap(heap[0], heap[(size_t)size - 1]);
    size--;
    heapify(0);
    return top;
  };
  while (size > 1) {                                      // BuildHuffmanTree
    const int a = extract(), b = extract();
    nodes.push_back(Node{nodes[(size_t)a].freq + nodes[(size_t)b].freq, a, b});
    heap[(size_t)size++] = (int)nodes.size() - 1;         // AddNode: sift up while parent > child, GetParent = ceil(i/2)-1
    for (int i = size - 1; i > 0 && f((i - 1) / 2) > f(i);) {
      std::swap(heap[(size_t)i], heap[(size_t)(i - 1) / 2]);
      i = (i - 1) / 2;
    }
  }
  // GetHuffmanCode: a leaf's code is its path from the root (one symbol: the empty code)
  std::vector<std::pair<int, int>> stack{{heap[0], 0}};
  while (!stack.empty()) {
    const std::pair<int, int> t = stack.back();
    stack.pop_back();
    const Node &nd = nodes[(size_t)t.first];
    if (nd.left < 0 && nd.right < 0) {
      out[order[(size_t)t.first]] = (uint16_t)t.second;
    } else {
      stack.push_back({nd.left, t.second + 1});
      stack.push_back({nd.right, t.second + 1});
    }
  }
  return 0;
}

// The bucket image for n <= MPC_SC2_ENTRIES distinct keys (lengths < 1024).  words receives nb x 4 dwords.
inline bool layout(const std::vector<uint32_t> &keys, const std::vector<uint16_t> &lens, std::vector<uint32_t> &words,
                   MpcSc2Table &t)
{
  uint32_t nb = 2;
  while (nb < 2 * keys.size() && nb < MPC_SC2_MAX_BUCKETS) nb <<= 1;
  const uint32_t mask = nb - 1;
  uint64_t state = 0x5C2ull;
  auto next = [&]() {             // splitmix64: the seeds in a fixed order
    uint64_t z = (state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (uint32_t)(z ^ (z >> 31));
  };
  for (int attempt = 0; attempt < 4096; attempt++) {
    const uint32_t s1 = next(), s2 = next();
    words.assign((size_t)nb * 4, 0u);
    bool ok = true;
    for (size_t i = 0; i < keys.size() && ok; i++) {
      const uint32_t b1 = mpc_sc2_hash(keys[i], s1) & mask, b2 = mpc_sc2_hash(keys[i], s2) & mask;
      uint32_t b = b1;
      if ((words[4 * (size_t)b1 + 3] >> 30) == 3u) b = b2;                // second bucket only when the first is full
      uint32_t &meta = words[4 * (size_t)b + 3];
      const uint32_t c = meta >> 30;
      if (c == 3u || lens[i] > 1023u) { ok = false; break; }
      words[4 * (size_t)b + c] = keys[i];
      meta = (meta & 0x3fffffffu) | ((uint32_t)lens[i] << (10 * c)) | ((c + 1) << 30);
    }
    if (ok) {
      t.mask = mask;
      t.seed1 = s1;
      t.seed2 = s2;
      return true;
    }
  }
  return false;
}

}  // namespace mpcsc2
