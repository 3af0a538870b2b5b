#!/usr/bin/env python3
"""Generate tests/golden/ref_sc2_vectors.json: what the REFERENCE's own SC2 (src/compressor/SC2.cpp and
src/utils.cpp, compiled unmodified with g++) reports for the seeded cases of tests/sc2_ref.py:CASES --

    table       [[symbol, code length], ...] of its Huffman table (m_huffmanCodes), ascending symbol order
    sizes       CompressLine's return value for lines sizes_from .. n-1 (the earlier ones are warm-up lines)
    original / compressed   its CompResult at the end

Each case passes its warm-up count to the reference constructor, SC2(lineSize, S).  Our own driver program and a
stand-in for the strutil.h header are written, with the build, into a temporary directory outside the repository that
is removed afterwards; the output holds seeds, an input digest and the reference's outputs only.

Run where the reference sources are (REF, as in oracle/Makefile):
    REF=/path/to/reference python tests/golden/make_ref_sc2_vectors.py [--check]
--check regenerates everything in memory and compares it with the committed file instead of writing it.
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
import sc2_ref  # noqa: E402

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

DRIVER = r"""
#include <cassert>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <map>
#include <set>
#include <sstream>
#include <string>
#include <unordered_map>
#include <vector>
#include <fmt/core.h>
#define private public      // (m_huffmanCodes: the table the driver prints)
#include "SC2.h"
#undef private
// usage: driver lines.bin L S  -> "size <bits>" per line, "table <symbol> <length>" per entry, "result <orig> <comp>"
int main(int argc, char **argv)
{
  FILE *f = fopen(argv[1], "rb");
  const unsigned L = (unsigned)atoi(argv[2]);
  comp::SC2 sc2(L, (unsigned)strtoul(argv[3], nullptr, 10));
  std::vector<uint8_t> line(L);
  while (fread(line.data(), 1, L, f) == L) printf("size %u\n", sc2.CompressLine(line));
  fclose(f);
  for (auto &kv : sc2.m_huffmanCodes) printf("table %lld %zu\n", (long long)kv.first, kv.second.size());
  comp::CompResult *r = sc2.GetResult();
  printf("result %llu %llu\n", (unsigned long long)r->OriginalSize, (unsigned long long)r->CompressedSize);
  return 0;
}
"""


OUT = os.path.join(HERE, "ref_sc2_vectors.json")


def generate(ref):
    src = os.path.join(ref, "src")
    import torch
    fmt_inc = os.path.join(os.path.dirname(torch.__file__), "include")
    tmp = tempfile.mkdtemp(prefix="ref_sc2_")
    try:
        with open(os.path.join(tmp, "strutil.h"), "w") as f:
            f.write(STRUTIL)
        with open(os.path.join(tmp, "driver.cpp"), "w") as f:
            f.write(DRIVER)
        exe = os.path.join(tmp, "driver")
        subprocess.run(["g++", "-O2", "-std=c++17", "-DFMT_HEADER_ONLY", "-w", "-I", tmp, "-I", fmt_inc,
                        "-I", os.path.join(src, "compressor"), "-I", src, os.path.join(tmp, "driver.cpp"),
                        os.path.join(src, "compressor", "SC2.cpp"), os.path.join(src, "utils.cpp"), "-o", exe], check=True)
        out = []
        for spec in sc2_ref.CASES:
            lines = sc2_ref.case_input(spec)
            path = os.path.join(tmp, "lines.bin")
            lines.tofile(path)
            r = subprocess.run([exe, path, str(spec["L"]), str(spec["S"])], capture_output=True, text=True, check=True)
            sizes, table, res = [], [], None
            for ln in r.stdout.split("\n"):
                p = ln.split()
                if not p:
                    continue
                if p[0] == "size":
                    sizes.append(int(p[1]))
                elif p[0] == "table":
                    table.append([int(p[1]), int(p[2])])
                elif p[0] == "result":
                    res = (int(p[1]), int(p[2]))
            n = len(lines)
            assert len(sizes) == n
            frm = max(0, min(spec["S"], n) - 4)
            assert all(s == 33 * spec["L"] // 4 for s in sizes[:frm])
            case = dict(spec)
            case.update({"n": n, "sha256": sc2_ref.digest(lines), "table": table, "sizes_from": frm, "sizes": sizes[frm:],
                         "original": res[0], "compressed": res[1]})
            out.append(case)
            print(f"{spec['name']}: {n} lines, {len(table)} symbols, max length {max([t[1] for t in table], default=0)}, "
                  f"ratio {res[0] / res[1]:.4f}")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return {"source": "reference src/compressor/SC2.cpp, compiled unmodified", "cases": out}


def main():
    ref = os.environ.get("REF")
    if not ref:
        sys.exit("set REF to the root of the reference sources (as for oracle/Makefile)")
    doc = generate(ref)
    if "--check" in sys.argv:
        with open(OUT) as f:
            old = json.load(f)
        new = json.loads(json.dumps(doc))
        names = [c["name"] for c in new["cases"]]
        diff = sorted(set(names) ^ {c["name"] for c in old["cases"]})
        diff += [c["name"] for c in new["cases"] for o in old["cases"] if o["name"] == c["name"] and o != c]
        if diff or old["source"] != new["source"] or [c["name"] for c in old["cases"]] != names:
            sys.exit(f"differs from {OUT}: {diff or 'order or source'}")
        print(f"{OUT}: no difference ({len(names)} cases)")
        return
    with open(OUT, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
