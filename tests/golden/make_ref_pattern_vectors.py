#!/usr/bin/env python3
"""Generate tests/golden/ref_pattern_vectors.npz: what the REFERENCE's own Pattern analyser (src/compressor/Pattern.cpp
and src/utils.cpp, compiled unmodified with g++) reports for the seeded cases of tests/pattern_ref.py:CASES --

    <case>/sizes     CompressLine's return value per line
    <case>/sel       the PatternState the line was counted under (0..5, 9 = NotDefined), read off the counters: which of
                     U / ImplicitCounts[k] / ExplicitCounts[k] the line moved
    <case>/stats     the library's statistics vector (include/mpc_hip.h) assembled from the reference's counters and
                     both symbol maps after the last line; [21] = lines - T / L
    <case>/entropy   ComputeEntropy of both maps (the doubles, bit for bit)
    meta             JSON: per case its seed, an input digest and the row Print wrote

Our own driver program and stand-ins for two headers the build has no copy of -- strutil.h and
boost/functional/hash.hpp (boost::hash_range; the hash reaches no result) -- are written, with the builds, into a
temporary directory that is removed afterwards.  The driver replaces the global operator new / delete: every
allocation and a 64-byte tail after it are filled with a non-zero sentinel.  Every case runs under two sentinels and
under an -O0 and an -O3 build, and the four runs must agree.

Run where the reference sources are (REF, as in oracle/Makefile):
    REF=/path/to/reference python tests/golden/make_ref_pattern_vectors.py
"""
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import pattern_ref  # noqa: E402

OUT = os.path.join(HERE, "ref_pattern_vectors.npz")
SENTINELS = (0xA5, 0x3C)
OPT = ("-O3", "-O0")                     # the reference builds with -O3 (Makefile:4)

STRUTIL = r"""
#pragma once
#include <string>
#include <vector>
namespace strutil {
inline std::vector<std::string> split(const std::string &s, const std::string &d)
{
  std::vector<std::string> out;
  size_t a = 0, b;
  while ((b = s.find(d, a)) != std::string::npos) { out.push_back(s.substr(a, b - a)); a = b + d.size(); }
  out.push_back(s.substr(a));
  return out;
}
inline bool replace_all(std::string &s, const std::string &from, const std::string &to)
{
  bool any = false;
  size_t p = 0;
  while (!from.empty() && (p = s.find(from, p)) != std::string::npos) { s.replace(p, from.size(), to); p += to.size(); any = true; }
  return any;
}
inline bool ends_with(const std::string &s, const std::string &e)
{
  return s.size() >= e.size() && s.compare(s.size() - e.size(), e.size(), e) == 0;
}
}
"""

BOOST_HASH = r"""
#pragma once
#include <cstddef>
namespace boost { template <class It> std::size_t hash_range(It a, It b) { std::size_t h = 0; for (; a != b; ++a) h = h * 1099511628211ull + (std::size_t)*a; return h; } }
"""

DRIVER = r"""
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <map>
#include <new>
#include <sstream>
#include <string>
#include <vector>
#include <fmt/core.h>
#include "Pattern.h"

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

// usage: driver <sentinel> <L> <lines.bin> <workload> <csv>
//   "s <size> <state>" per line, "r Z R T U Total", "i <6 implicit>", "e <6 explicit>", "m <symbol> <count>" and
//   "x <symbol> <count>" per map entry, "h <entropy %a> <entropy except %a>"; Print(workload, csv) after the last line
int main(int argc, char **argv)
{
  g_sentinel = (unsigned char)std::strtoul(argv[1], nullptr, 0);
  const unsigned L = (unsigned)atoi(argv[2]);
  FILE *f = fopen(argv[3], "rb");
  if (!f) return 3;
  comp::Pattern pat(L);
  comp::PatternResult *r = static_cast<comp::PatternResult *>(pat.GetResult());
  std::vector<uint8_t> line(L);
  while (fread(line.data(), 1, L, f) == L) {
    const uint64_t u = r->U;
    std::vector<uint64_t> imp = r->ImplicitCounts, exp = r->ExplicitCounts;
    const unsigned size = pat.CompressLine(line);
    int state = -1;
    if (r->U != u) state = 9;
    for (int k = 0; k < 6; k++)
      if (r->ImplicitCounts[k] != imp[k] || r->ExplicitCounts[k] != exp[k]) state = state == -1 ? k : 100;
    printf("s %u %d\n", size, state);
  }
  fclose(f);
  printf("r %llu %llu %llu %llu %llu\n", (unsigned long long)r->Z, (unsigned long long)r->R, (unsigned long long)r->T,
         (unsigned long long)r->U, (unsigned long long)r->Total);
  printf("i");
  for (int k = 0; k < 6; k++) printf(" %llu", (unsigned long long)r->ImplicitCounts[k]);
  printf("\ne");
  for (int k = 0; k < 6; k++) printf(" %llu", (unsigned long long)r->ExplicitCounts[k]);
  printf("\n");
  for (auto &kv : r->SymbolCounts) printf("m %u %llu\n", (unsigned)kv.first, (unsigned long long)kv.second);
  for (auto &kv : r->SymbolCountsExceptAllZerosAllWordSame) printf("x %u %llu\n", (unsigned)kv.first, (unsigned long long)kv.second);
  printf("h %a %a\n", r->ComputeEntropy(r->SymbolCounts), r->ComputeEntropy(r->SymbolCountsExceptAllZerosAllWordSame));
  printf("c %llu %llu %a %s\n", (unsigned long long)r->OriginalSize, (unsigned long long)r->CompressedSize, r->CompRatio,
         pat.GetCompressorName().c_str());
  fflush(stdout);
  r->Print(argv[4], argv[5]);
  return 0;
}
"""


def _parse(text, n, L):
    sizes, sel = [], []
    v = np.zeros(pattern_ref.STATS_LEN, dtype=np.uint64)
    ent, comp = None, None
    for ln in text.split("\n"):
        p = ln.split()
        if not p:
            continue
        if p[0] == "s":
            sizes.append(int(p[1]))
            sel.append(int(p[2]))
        elif p[0] == "r":
            v[4:9] = [int(x) for x in p[1:6]]
        elif p[0] == "i":
            v[9:15] = [int(x) for x in p[1:7]]
        elif p[0] == "e":
            v[15:21] = [int(x) for x in p[1:7]]
        elif p[0] == "m":
            v[22 + int(p[1])] = int(p[2])
        elif p[0] == "x":
            v[278 + int(p[1])] = int(p[2])
        elif p[0] == "h":
            ent = [float.fromhex(p[1]), float.fromhex(p[2])]
        elif p[0] == "c":
            comp = (int(p[1]), int(p[2]), float.fromhex(p[3]), " ".join(p[4:]))
    assert len(sizes) == n and all(s in (0, 1, 2, 3, 4, 5, 9) for s in sel), "a line moved no counter or several"
    assert comp == (0, 0, 0.0, "Pattern Checker"), comp
    v[0] = n
    v[3] = sum(sizes)
    assert int(v[6]) % L == 0
    v[21] = n - int(v[6]) // L
    return np.array(sizes, np.uint16), np.array(sel, np.int8), v, np.array(ent, np.float64)


def main():
    ref = os.environ.get("REF")
    if not ref:
        sys.exit("set REF to the root of the reference sources (as for oracle/Makefile)")
    src = os.path.join(ref, "src")
    import torch
    fmt_inc = os.path.join(os.path.dirname(torch.__file__), "include")
    tmp = tempfile.mkdtemp(prefix="ref_pattern_")
    arrays, meta = {}, {"source": "reference src/compressor/Pattern.cpp, compiled unmodified", "sentinels": list(SENTINELS),
                        "builds": list(OPT), "cases": []}
    try:
        os.makedirs(os.path.join(tmp, "boost", "functional"))
        for name, text in (("strutil.h", STRUTIL), ("driver.cpp", DRIVER), (os.path.join("boost", "functional", "hash.hpp"), BOOST_HASH)):
            with open(os.path.join(tmp, name), "w") as f:
                f.write(text)
        exes = []
        for opt in OPT:
            exe = os.path.join(tmp, "driver" + opt)
            subprocess.run(["g++", opt, "-std=c++17", "-DFMT_HEADER_ONLY", "-w", "-I", tmp, "-I", fmt_inc,
                            "-I", os.path.join(src, "compressor"), "-I", src, os.path.join(tmp, "driver.cpp"),
                            os.path.join(src, "compressor", "Pattern.cpp"), os.path.join(src, "utils.cpp"), "-o", exe], check=True)
            exes.append(exe)
        for spec in pattern_ref.CASES:
            lines = pattern_ref.case_input(spec)
            path = os.path.join(tmp, "lines.bin")
            lines.tofile(path)
            outs = set()
            for exe in exes:
                for s in SENTINELS:
                    csv = os.path.join(tmp, "out.csv")
                    if os.path.exists(csv):
                        os.remove(csv)
                    r = subprocess.run([exe, str(s), str(spec["L"]), path, spec["name"], csv], capture_output=True, text=True, check=True)
                    with open(csv) as f:
                        rows = f.read().split("\n")
                    outs.add((r.stdout, rows[0], rows[1] + "\n"))
            assert len(outs) == 1, f"{spec['name']}: the reference's numbers depend on the sentinel or the build"
            text, header, row = outs.pop()
            sizes, sel, v, ent = _parse(text, len(lines), spec["L"])
            arrays[spec["name"] + "/sizes"] = sizes
            arrays[spec["name"] + "/sel"] = sel
            arrays[spec["name"] + "/stats"] = v
            arrays[spec["name"] + "/entropy"] = ent
            case = dict(spec)
            case.update({"n": len(lines), "sha256": pattern_ref.digest(lines), "print": row, "header": header})
            meta["cases"].append(case)
            print(f"{spec['name']}: {len(lines)} lines, selected {np.bincount(sel, minlength=10).tolist()}, T {int(v[6])}, "
                  f"entropy {ent[0]:.4f} / {ent[1]:.4f}")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    arrays["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    np.savez_compressed(OUT, **arrays)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
