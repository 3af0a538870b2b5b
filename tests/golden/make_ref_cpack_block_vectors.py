#!/usr/bin/env python3
"""Generate tests/golden/ref_cpack_block_vectors.npz: what the REFERENCE's own C-Pack (src/compressor/CPACK.cpp and
src/utils.cpp, compiled unmodified with g++) reports for the cases of tests/cpack_blocks_ref.py:CASES when a FRESH
comp::CPACK object is constructed every N lines -- the dictionary shared by blocks of N lines that mpc_create_cpack_blocks
evaluates -- for every N of cpack_blocks_ref.BLOCKS.  Per case and N ("<name>.N<N>.<key>" arrays):

    sizes   CompressLine's return value per line (uint16); line i went to object number i / N
    stats   OriginalSize, CompressedSize, TotalWords, Counts[6] summed over the objects' own results (uint64)
    ratio   CompRatio of one reference CPACKResult that was given every line's Update(8 L, size) (float64, exact)

"meta" (a JSON string) holds the case specs with their line counts and input digests, and the block lengths.

The driver program is this generator's own; it and a stand-in for the strutil.h header are written, with the builds,
into a temporary directory that is removed afterwards.  As in make_ref_cpack_vectors.py the driver replaces the global
operator new / delete (every allocation and a 64-byte tail after it are filled with a non-zero sentinel), every case runs
under two sentinels and under an -O0 and an -O3 build, and the four runs must agree.

Run where the reference sources are (REF, as in oracle/Makefile):
    REF=/path/to/reference python tests/golden/make_ref_cpack_block_vectors.py [--check]
--check regenerates everything in memory and compares it with the committed file instead of writing it.
"""
import io
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import cpack_blocks_ref  # noqa: E402
import cpack_ref  # noqa: E402
from make_ref_sc2_vectors import STRUTIL  # noqa: E402

OUT = os.path.join(HERE, "ref_cpack_block_vectors.npz")
SENTINELS = (0xA5, 0x3C)
OPT = ("-O3", "-O0")                     # the reference builds with -O3 (Makefile:4)

DRIVER = r"""
#include <cassert>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <fstream>
#include <iostream>
#include <map>
#include <new>
#include <sstream>
#include <string>
#include <vector>
#include <fmt/core.h>
#include "CPACK.h"

// Every allocation and 64 bytes after it hold a non-zero sentinel (set from the command line before any input is read).
static unsigned char g_sentinel = 0xA5;
static void *fill_alloc(size_t n)
{
  void *p = std::malloc(n + 64);
  if (!p) std::abort();
  std::memset(p, g_sentinel, n + 64);
  return p;
}
void *operator new(size_t n) { return fill_alloc(n); }
void *operator new[](size_t n) { return fill_alloc(n); }
void operator delete(void *p) noexcept { std::free(p); }
void operator delete[](void *p) noexcept { std::free(p); }
void operator delete(void *p, size_t) noexcept { std::free(p); }
void operator delete[](void *p, size_t) noexcept { std::free(p); }

// usage: driver <sentinel> <L> <N> <lines.bin>
//   -> "s <size>" per line, then "t <orig> <comp> <words> <6 counts>" (the objects' own results, summed) and
//      "r <ratio %a>" (one result that was given every line)
int main(int argc, char **argv)
{
  if (argc != 5) return 2;
  g_sentinel = (unsigned char)std::strtoul(argv[1], nullptr, 0);
  const unsigned L = (unsigned)std::atoi(argv[2]);
  const unsigned long long N = std::strtoull(argv[3], nullptr, 10);
  FILE *f = std::fopen(argv[4], "rb");
  if (!f || !N) return 3;
  comp::CPACKResult total(L);
  unsigned long long sum[3 + NUM_CPACK_PATTERN] = {0};
  comp::CPACK *block = nullptr;
  auto close_block = [&]() {
    if (!block) return;
    comp::CPACKResult *r = static_cast<comp::CPACKResult *>(block->GetResult());
    sum[0] += r->OriginalSize;
    sum[1] += r->CompressedSize;
    sum[2] += r->TotalWords;
    for (int k = 0; k < NUM_CPACK_PATTERN; k++) sum[3 + k] += r->Counts[k];
    delete r;
    delete block;
    block = nullptr;
  };
  std::vector<uint8_t> line(L);
  unsigned long long i = 0;
  while (std::fread(line.data(), 1, L, f) == L) {
    if (i % N == 0) {
      close_block();
      block = new comp::CPACK(L);                             // a dictionary of its own, all zero
    }
    const unsigned size = block->CompressLine(line);
    total.Update(8 * L, size);
    std::printf("s %u\n", size);
    i++;
  }
  close_block();
  std::fclose(f);
  std::printf("t");
  for (unsigned long long v : sum) std::printf(" %llu", v);
  std::printf("\nr %a\n", total.CompRatio);
  if (total.OriginalSize != sum[0] || total.CompressedSize != sum[1]) return 5;
  return 0;
}
"""


def _run(exe, *args) -> str:
    r = subprocess.run([exe, *[str(a) for a in args]], capture_output=True, text=True, check=True)
    return r.stdout


def _parse(out: str):
    sizes, stats, ratio = [], None, None
    for ln in out.split("\n"):
        p = ln.split()
        if not p:
            continue
        if p[0] == "s":
            sizes.append(int(p[1]))
        elif p[0] == "t":
            stats = [int(x) for x in p[1:]]
        elif p[0] == "r":
            ratio = float.fromhex(p[1])
    return np.array(sizes, dtype=np.uint16), np.array(stats, dtype=np.uint64), np.array([ratio], dtype=np.float64)


def generate(ref: str) -> dict:
    src = os.path.join(ref, "src")
    import torch
    fmt_inc = os.path.join(os.path.dirname(torch.__file__), "include")
    tmp = tempfile.mkdtemp(prefix="ref_cpack_blocks_")
    arrays, meta = {}, {"source": "reference src/compressor/CPACK.cpp, compiled unmodified; a fresh comp::CPACK every N lines",
                        "sentinels": list(SENTINELS), "builds": list(OPT), "blocks": list(cpack_blocks_ref.BLOCKS), "cases": []}
    try:
        with open(os.path.join(tmp, "strutil.h"), "w") as f:
            f.write(STRUTIL)
        with open(os.path.join(tmp, "driver.cpp"), "w") as f:
            f.write(DRIVER)
        exes = []
        for opt in OPT:
            exe = os.path.join(tmp, "driver" + opt)
            subprocess.run(["g++", opt, "-std=c++17", "-DFMT_HEADER_ONLY", "-w", "-I", tmp, "-I", fmt_inc,
                            "-I", os.path.join(src, "compressor"), "-I", src, os.path.join(tmp, "driver.cpp"),
                            os.path.join(src, "compressor", "CPACK.cpp"), os.path.join(src, "utils.cpp"), "-o", exe], check=True)
            exes.append(exe)
        runs = [(exe, s) for exe in exes for s in SENTINELS]
        path = os.path.join(tmp, "lines.bin")
        for spec in cpack_blocks_ref.CASES:
            lines = cpack_blocks_ref.case_lines(spec)
            lines.tofile(path)
            name, L = spec["name"], spec["L"]
            for N in cpack_blocks_ref.BLOCKS:
                outs = {_run(exe, s, L, N, path) for exe, s in runs}
                assert len(outs) == 1, f"{name}, N = {N}: the reference's numbers depend on the sentinel or the build"
                sizes, stats, ratio = _parse(outs.pop())
                assert len(sizes) == len(lines) and int(stats[2]) == len(lines) * (L // 4) == int(stats[3:].sum())
                arrays[f"{name}.N{N}.sizes"] = sizes
                arrays[f"{name}.N{N}.stats"] = stats
                arrays[f"{name}.N{N}.ratio"] = ratio
            meta["cases"].append(dict(spec, n=len(lines), sha256=cpack_ref.digest(lines)))
            print(f"{name}: {len(lines)} lines, compressed bits " +
                  ", ".join(f"{int(arrays[f'{name}.N{N}.stats'][1])} (N = {N})" for N in cpack_blocks_ref.BLOCKS))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    arrays["meta"] = np.array(json.dumps(meta, sort_keys=True))
    return arrays


def main():
    ref = os.environ.get("REF")
    if not ref:
        sys.exit("set REF to the root of the reference sources (as for oracle/Makefile)")
    arrays = generate(ref)
    if "--check" in sys.argv:
        with np.load(OUT) as old:
            keys = set(old.files)
            diff = sorted(keys ^ set(arrays))
            for k in sorted(keys & set(arrays)):
                a, b = old[k], arrays[k]
                if a.dtype != b.dtype or a.shape != b.shape or not (a == b).all():
                    diff.append(k)
        if diff:
            sys.exit(f"differs from {OUT}: {diff}")
        print(f"{OUT}: no difference ({len(arrays)} arrays)")
        return
    buf = io.BytesIO()
    np.savez_compressed(buf, **arrays)
    with open(OUT, "wb") as f:
        f.write(buf.getvalue())
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
