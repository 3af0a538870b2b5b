#!/usr/bin/env python3
"""Generate tests/golden/ref_cpack_vectors.npz: what the REFERENCE's own C-Pack (src/compressor/CPACK.cpp and
src/utils.cpp, compiled unmodified with g++) reports for the seeded cases of tests/cpack_ref.py:CASES when a FRESH
comp::CPACK object is constructed for every line -- the per-line dictionary the library evaluates.  Per case
("<name>.<key>" arrays):

    sizes          CompressLine's return value per line, each from its own fresh object (uint16)
    counts         that object's Counts after its one line, CPACKPattern order (uint8 [n, 6])
    stats          OriginalSize, CompressedSize, TotalWords, Counts[6] of one reference CPACKResult that was given every
                   line's Update(8 L, size) and UpdatePattern calls (uint64)
    ratio          that result's CompRatio (float64, exact)
    carried        for the same lines in the same order, the sizes of ONE object fed the whole case: the dictionary carried
                   from line to line, as the reference's driver runs it (uint16).  Not what the library evaluates; recorded
                   to pin the other mode of the restatement and to show that the two differ.
    carried_stats  OriginalSize, CompressedSize, TotalWords, Counts[6] of that one object (uint64)

"meta" (a JSON string) holds the case specs with their line counts and input digests, and the header and row that
CPACKResult::Print(workload, path) writes into a new file for two cases, over all lines but the last (what a driver does
with <dir>/<name>.npy: the loader drops the last row), workload "<dir>_<name>".

Our own driver program and a stand-in for the strutil.h header are written, with the builds, into a temporary
directory that is removed afterwards.  The driver replaces the global operator new / delete: every allocation and a
64-byte tail after it are filled with a non-zero sentinel (the dictionary entries are allocations of 4 bytes).  Every
case runs under two sentinels and under an -O0 and an -O3 build, and the four runs must agree.

Run where the reference sources are (REF, as in oracle/Makefile):
    REF=/path/to/reference python tests/golden/make_ref_cpack_vectors.py [--check]
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
import cpack_ref  # noqa: E402
from make_ref_sc2_vectors import STRUTIL  # noqa: E402

OUT = os.path.join(HERE, "ref_cpack_vectors.npz")
SENTINELS = (0xA5, 0x3C)
OPT = ("-O3", "-O0")                     # the reference builds with -O3 (Makefile:4)
PRINT_DIR = "refbench"

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

static void row(const char *tag, comp::CPACKResult *r)
{
  std::printf("%s %llu %llu %a %llu", tag, (unsigned long long)r->OriginalSize, (unsigned long long)r->CompressedSize, r->CompRatio,
              (unsigned long long)r->TotalWords);
  for (uint64_t k : r->Counts) std::printf(" %llu", (unsigned long long)k);
  std::printf("\n");
}

// usage:
//   driver <sentinel> run <L> <lines.bin>                     -> "s <size> <6 counts> <carried size>" per line, then
//                                                                "r <orig> <comp> <ratio %a> <words> <counts...>" (fresh
//                                                                objects) and "k ..." (the one carried object)
//   driver <sentinel> print <L> <lines.bin> <workload> <csv>  -> Print(workload, csv) of the fresh objects' totals
int main(int argc, char **argv)
{
  g_sentinel = (unsigned char)std::strtoul(argv[1], nullptr, 0);
  const std::string mode = argv[2];
  const unsigned L = (unsigned)std::atoi(argv[3]);
  FILE *f = std::fopen(argv[4], "rb");
  if (!f) return 3;
  comp::CPACKResult total(L);
  comp::CPACK carried(L);
  std::vector<uint8_t> line(L);
  while (std::fread(line.data(), 1, L, f) == L) {
    comp::CPACK *fresh = new comp::CPACK(L);                  // a dictionary of its own, all zero
    const unsigned size = fresh->CompressLine(line);
    comp::CPACKResult *r = static_cast<comp::CPACKResult *>(fresh->GetResult());
    if (r->CompressedSize != size || r->OriginalSize != 8ull * L) return 5;
    total.Update(8 * L, size);
    for (int k = 0; k < NUM_CPACK_PATTERN; k++)
      for (uint64_t c = 0; c < r->Counts[k]; c++) total.UpdatePattern(k);
    const unsigned csize = carried.CompressLine(line);
    if (mode == "run") {
      std::printf("s %u", size);
      for (uint64_t k : r->Counts) std::printf(" %llu", (unsigned long long)k);
      std::printf(" %u\n", csize);
    }
    delete r;
    delete fresh;
  }
  std::fclose(f);
  if (mode == "print") {
    total.Print(argv[5], argv[6]);
    return 0;
  }
  row("r", &total);
  row("k", static_cast<comp::CPACKResult *>(carried.GetResult()));
  return 0;
}
"""


def _run(exe, *args) -> str:
    r = subprocess.run([exe, *[str(a) for a in args]], capture_output=True, text=True, check=True)
    return r.stdout


def _parse_run(out: str):
    sizes, counts, carried, stats, ratio, cstats = [], [], [], None, None, None
    for ln in out.split("\n"):
        p = ln.split()
        if not p:
            continue
        if p[0] == "s":
            sizes.append(int(p[1]))
            counts.append([int(x) for x in p[2:8]])
            carried.append(int(p[8]))
        elif p[0] in "rk":
            row = [int(p[1]), int(p[2]), int(p[4])] + [int(x) for x in p[5:]]
            if p[0] == "r":
                stats, ratio = row, float.fromhex(p[3])
            else:
                cstats = row
    return (np.array(sizes, dtype=np.uint16), np.array(counts, dtype=np.uint8).reshape(-1, 6), np.array(carried, dtype=np.uint16),
            np.array(stats, dtype=np.uint64), np.array([ratio], dtype=np.float64), np.array(cstats, dtype=np.uint64))


def generate(ref: str) -> dict:
    src = os.path.join(ref, "src")
    import torch
    fmt_inc = os.path.join(os.path.dirname(torch.__file__), "include")
    tmp = tempfile.mkdtemp(prefix="ref_cpack_")
    arrays, meta = {}, {"source": "reference src/compressor/CPACK.cpp, compiled unmodified; a fresh comp::CPACK per line",
                        "sentinels": list(SENTINELS), "builds": list(OPT), "cases": [], "print": []}
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
        for spec in cpack_ref.CASES:
            lines = cpack_ref.case_lines(spec)
            lines.tofile(path)
            outs = {_run(exe, s, "run", spec["L"], path) for exe, s in runs}
            assert len(outs) == 1, f"{spec['name']}: the reference's numbers depend on the sentinel or the build"
            sizes, counts, carried, stats, ratio, cstats = _parse_run(outs.pop())
            assert len(sizes) == len(lines) and (counts.sum(axis=1) == spec["L"] // 4).all()
            name = spec["name"]
            arrays[f"{name}.sizes"] = sizes
            arrays[f"{name}.counts"] = counts
            arrays[f"{name}.stats"] = stats
            arrays[f"{name}.ratio"] = ratio
            arrays[f"{name}.carried"] = carried
            arrays[f"{name}.carried_stats"] = cstats
            meta["cases"].append(dict(spec, n=len(lines), sha256=cpack_ref.digest(lines)))
            if name in cpack_ref.PRINT_CASES:
                lines[:-1].tofile(path)
                texts = set()
                for k, (exe, s) in enumerate(runs):
                    csv = os.path.join(tmp, f"out{k}.csv")
                    _run(exe, s, "print", spec["L"], path, f"{PRINT_DIR}_{name}", csv)
                    with open(csv) as f:
                        texts.add(f.read())
                    os.remove(csv)
                assert len(texts) == 1
                meta["print"].append({"case": name, "npy": f"{PRINT_DIR}/{name}.npy", "text": texts.pop()})
            print(f"{name}: {len(lines)} lines, ratio {ratio[0]!r}, {int((sizes != carried).sum())} sizes differ from the carried dictionary's")
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
