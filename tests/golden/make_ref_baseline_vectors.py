#!/usr/bin/env python3
"""Generate tests/golden/ref_baseline_vectors.npz: what the REFERENCE's own BDI, FPC and BPC (src/compressor/BDI.cpp,
FPC.cpp, BPC.cpp and src/utils.cpp, compiled unmodified with g++) report for the seeded cases of
tests/baseline_ref.py:CASES.  Per case ("<name>.<key>" arrays):

    sizes     CompressLine's return value per line (uint16)
    states    BDI only: the BDIState of each line, the Counts entry that CompressLine incremented (int8)
    stats     OriginalSize, CompressedSize, TotalWords (FPC / BPC; 0 for BDI), Counts[...] at the end (uint64)
    ratio     CompRatio at the end (float64, exact)

and stage pins of BDI:  reduce_sign_in / reduce_sign_out (BDI::reduceSign on edge values), check_<case> (BDI::checkBDI
for the six (base, delta) combinations, [lines, 6], on the first CHECK_LINES lines of a few cases).  "meta" (a JSON
string) holds the case specs with their line counts and input digests, and the text that Result::Print(workload, path)
writes into a new file for one case per compressor at 64 and 128 bytes, over all lines but the last (what the command
line does with <dir>/<name>.npy: the loader drops the last row), workload "<dir>_<name>".

Our own driver program and a stand-in for the strutil.h header are written, with the builds, into a temporary
directory that is removed afterwards.  The driver replaces the global operator new / delete: every allocation and a
64-byte tail after it are filled with a non-zero sentinel.  FPC's zero-run loop (FPC.cpp:26) reads the word after the
line's last one; with the sentinel there, a run ends at the end of the line.  Every case runs under two sentinels and
under an -O0 and an -O3 build, and the four runs must agree: the recorded numbers depend neither on what lies past the
FPC word vector nor on the uninitialised upper half of BPC's int64_t words (BPC.cpp:42-44; it is the same for every
word of a line, so it cancels in the deltas).

Run where the reference sources are (REF, as in oracle/Makefile):
    REF=/path/to/reference python tests/golden/make_ref_baseline_vectors.py [--check]
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
import baseline_ref  # noqa: E402
from make_ref_sc2_vectors import STRUTIL  # noqa: E402

OUT = os.path.join(HERE, "ref_baseline_vectors.npz")
SENTINELS = (0xA5, 0x3C)
OPT = ("-O3", "-O0")                     # the reference builds with -O3 (Makefile:4)
CHECK_CASES = ("bdi_L24", "bdi_L64", "bdi_L136")
CHECK_LINES = 120
PRINT_CASES = ("bdi_L64", "bdi_L128", "fpc_L64", "fpc_L128", "bpc_L64", "bpc_L128")
PRINT_DIR = "refbench"

DRIVER = r"""
#include <cassert>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <map>
#include <new>
#include <set>
#include <sstream>
#include <string>
#include <unordered_map>
#include <vector>
#include <fmt/core.h>
#define private public      // (BDI::reduceSign, BDI::checkBDI: the stage pins)
#include "BDI.h"
#include "FPC.h"
#include "BPC.h"
#undef private

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

static std::vector<std::vector<uint8_t>> read_lines(const char *path, unsigned L)
{
  std::vector<std::vector<uint8_t>> out;
  FILE *f = std::fopen(path, "rb");
  if (!f) std::exit(3);
  std::vector<uint8_t> line(L);
  while (std::fread(line.data(), 1, L, f) == L) out.push_back(line);
  std::fclose(f);
  return out;
}

static comp::Compressor *make(const std::string &algo, unsigned L)
{
  if (algo == "BDI") return new comp::BDI(L);
  if (algo == "FPC") return new comp::FPC(L);
  if (algo == "BPC") return new comp::BPC(L);
  std::exit(4);
}

static std::vector<uint64_t> *counts_of(const std::string &algo, comp::CompResult *r, uint64_t *total_words)
{
  *total_words = 0;
  if (algo == "BDI") return &static_cast<comp::BDIResult *>(r)->Counts;
  if (algo == "FPC") { *total_words = static_cast<comp::FPCResult *>(r)->TotalWords; return &static_cast<comp::FPCResult *>(r)->Counts; }
  *total_words = static_cast<comp::BPCResult *>(r)->TotalWords;
  return &static_cast<comp::BPCResult *>(r)->Counts;
}

// usage:
//   driver <sentinel> run <algo> <L> <lines.bin>      -> "s <size> <state>" per line, then "r <orig> <comp> <ratio %a> <words> <counts...>"
//   driver <sentinel> print <algo> <L> <lines.bin> <workload> <csv>   -> Print(workload, csv) after the last line
//   driver <sentinel> check <L> <lines.bin>           -> "c <6 x checkBDI>" per line
//   driver <sentinel> reduce <values.bin>             -> "u <reduceSign>" per uint64
int main(int argc, char **argv)
{
  g_sentinel = (unsigned char)std::strtoul(argv[1], nullptr, 0);
  const std::string mode = argv[2];
  if (mode == "run" || mode == "print") {
    const std::string algo = argv[3];
    const unsigned L = (unsigned)std::atoi(argv[4]);
    auto lines = read_lines(argv[5], L);
    comp::Compressor *c = make(algo, L);
    uint64_t words = 0;
    for (auto &line : lines) {
      std::vector<uint64_t> before = *counts_of(algo, c->GetResult(), &words);
      const unsigned size = c->CompressLine(line);
      int state = 0;
      if (algo == "BDI") {
        const std::vector<uint64_t> &after = *counts_of(algo, c->GetResult(), &words);
        state = -1;
        for (size_t k = 0; k < after.size(); k++)
          if (after[k] != before[k]) { if (state != -1 || after[k] != before[k] + 1) std::exit(5); state = (int)k; }
      }
      if (mode == "run") std::printf("s %u %d\n", size, state);
    }
    comp::CompResult *r = c->GetResult();
    if (mode == "print") {
      if (algo == "BDI") static_cast<comp::BDIResult *>(r)->Print(argv[6], argv[7]);
      else if (algo == "FPC") static_cast<comp::FPCResult *>(r)->Print(argv[6], argv[7]);
      else static_cast<comp::BPCResult *>(r)->Print(argv[6], argv[7]);
      return 0;
    }
    const std::vector<uint64_t> &counts = *counts_of(algo, r, &words);
    std::printf("r %llu %llu %a %llu", (unsigned long long)r->OriginalSize, (unsigned long long)r->CompressedSize,
                r->CompRatio, (unsigned long long)words);
    for (uint64_t k : counts) std::printf(" %llu", (unsigned long long)k);
    std::printf("\n");
    return 0;
  }
  if (mode == "check") {
    const unsigned L = (unsigned)std::atoi(argv[3]);
    auto lines = read_lines(argv[4], L);
    comp::BDI bdi(L);
    const unsigned combos[6][2] = {{8, 1}, {8, 2}, {8, 4}, {4, 1}, {4, 2}, {2, 1}};
    for (auto &line : lines) {
      std::printf("c");
      for (auto &bd : combos) std::printf(" %u", bdi.checkBDI(line, bd[0], bd[1]));
      std::printf("\n");
    }
    return 0;
  }
  if (mode == "reduce") {
    comp::BDI bdi(8);
    FILE *f = std::fopen(argv[3], "rb");
    uint64_t x;
    while (std::fread(&x, 8, 1, f) == 1) std::printf("u %llu\n", (unsigned long long)bdi.reduceSign(x));
    std::fclose(f);
    return 0;
  }
  return 2;
}
"""


def reduce_sign_inputs() -> np.ndarray:
    """Edge values of BDI::reduceSign: around 0, the delta limits of 1 / 2 / 4 bytes on both signs, the sign bit."""
    v = [0, 1, 2, 0x7F, 0x80, 0xFF, 0x100, 0x7FFF, 0x8000, 0xFFFF, 0x10000, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF,
         0x100000000, (1 << 63) - 1, 1 << 63, (1 << 63) + 1, 0xC000000000000000, 0xBFFFFFFFFFFFFFFF]
    for D in (1, 2, 4):
        h = 1 << (8 * D - 1)
        for d in (-h - 2, -h - 1, -h, -h + 1, -2, -1, 2 * h - 1, 2 * h):
            v.append(d & ((1 << 64) - 1))
    v += [(-(1 << k)) & ((1 << 64) - 1) for k in range(0, 64, 5)]
    v += [((-(1 << k)) - 1) & ((1 << 64) - 1) for k in (7, 8, 15, 16, 31, 32)]
    v += [(1 << k) - 1 for k in range(2, 64, 4)]
    return np.array(sorted(set(v)), dtype=np.uint64)


def _run(exe, *args) -> str:
    r = subprocess.run([exe, *[str(a) for a in args]], capture_output=True, text=True, check=True)
    return r.stdout


def _parse_run(out: str, comp: str):
    sizes, states, stats, ratio = [], [], None, None
    for ln in out.split("\n"):
        p = ln.split()
        if not p:
            continue
        if p[0] == "s":
            sizes.append(int(p[1]))
            states.append(int(p[2]))
        elif p[0] == "r":
            ratio = float.fromhex(p[3])
            stats = [int(p[1]), int(p[2]), int(p[4])] + [int(x) for x in p[5:]]
    return (np.array(sizes, dtype=np.uint16), np.array(states, dtype=np.int8), np.array(stats, dtype=np.uint64),
            np.array([ratio], dtype=np.float64))


def generate(ref: str) -> dict:
    src = os.path.join(ref, "src")
    import torch
    fmt_inc = os.path.join(os.path.dirname(torch.__file__), "include")
    tmp = tempfile.mkdtemp(prefix="ref_baseline_")
    arrays, meta = {}, {"source": "reference src/compressor/{BDI,FPC,BPC}.cpp, compiled unmodified",
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
                            "-I", os.path.join(src, "compressor"), "-I", src, os.path.join(tmp, "driver.cpp")]
                           + [os.path.join(src, "compressor", f"{c}.cpp") for c in ("BDI", "FPC", "BPC")]
                           + [os.path.join(src, "utils.cpp"), "-o", exe], check=True)
            exes.append(exe)
        runs = [(exe, s) for exe in exes for s in SENTINELS]
        path = os.path.join(tmp, "lines.bin")
        for spec in baseline_ref.CASES:
            lines = baseline_ref.case_lines(spec)
            lines.tofile(path)
            outs = {_run(exe, s, "run", spec["comp"], spec["L"], path) for exe, s in runs}
            assert len(outs) == 1, f"{spec['name']}: the reference's numbers depend on the sentinel or the build"
            sizes, states, stats, ratio = _parse_run(outs.pop(), spec["comp"])
            assert len(sizes) == len(lines)
            name = spec["name"]
            arrays[f"{name}.sizes"] = sizes
            if spec["comp"] == "BDI":
                assert (states >= 0).all()
                arrays[f"{name}.states"] = states
            arrays[f"{name}.stats"] = stats
            arrays[f"{name}.ratio"] = ratio
            meta["cases"].append(dict(spec, n=len(lines), sha256=baseline_ref.digest(lines)))
            if name in CHECK_CASES:
                lines[:CHECK_LINES].tofile(path)
                outs = {_run(exe, s, "check", spec["L"], path) for exe, s in runs}
                assert len(outs) == 1
                arrays[f"check_{name}"] = np.array([[int(x) for x in ln.split()[1:]] for ln in outs.pop().strip().split("\n")],
                                                   dtype=np.uint32)
            if name in PRINT_CASES:
                lines[:-1].tofile(path)
                texts = set()
                for k, (exe, s) in enumerate(runs):
                    csv = os.path.join(tmp, f"out{k}.csv")
                    _run(exe, s, "print", spec["comp"], spec["L"], path, f"{PRINT_DIR}_{name}", csv)
                    with open(csv) as f:
                        texts.add(f.read())
                    os.remove(csv)
                assert len(texts) == 1
                meta["print"].append({"case": name, "comp": spec["comp"], "npy": f"{PRINT_DIR}/{name}.npy",
                                      "text": texts.pop()})
            print(f"{name}: {len(lines)} lines, ratio {ratio[0]!r}")
        rs = reduce_sign_inputs()
        rs.tofile(path)
        outs = {_run(exe, s, "reduce", path) for exe, s in runs}
        assert len(outs) == 1
        arrays["reduce_sign_in"] = rs
        arrays["reduce_sign_out"] = np.array([int(ln.split()[1]) for ln in outs.pop().strip().split("\n")], dtype=np.uint64)
        meta["check"] = {"cases": list(CHECK_CASES), "lines": CHECK_LINES}
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
