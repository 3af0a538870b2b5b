#!/usr/bin/env python3
"""Generate tests/golden/ref_pattern_evict_vectors.npz: what the REFERENCE's own line cache answers once it evicts.

Small capacities -- src/compressor/LRU.h, compiled unmodified: LRUCache<std::vector<uint8_t>, int, std::vector<uint8_t>>
(the type Pattern.h:250 declares) of capacity C, driven as Pattern::isExistedBefore drives it (exist, on a miss put(line, 0)),
over the seeded cases of tests/pattern_evict_ref.py:CASES --

    <case>/existed      the per-line answer, packed bits (numpy.packbits)
    <case>/insertions   the number of put calls

The real capacity -- src/compressor/Pattern.cpp and src/utils.cpp, compiled unmodified: comp::Pattern(8) over the five
parts of pattern_evict_ref.REAL_PARTS (8-byte lines v[i] = i * 0x9E3779B97F4A7C15) --

    real/totals         [5, 18] uint64: after every part, the fields pattern_evict_ref.REAL_FIELDS of PatternResult
    real/insertions     [5] uint64: lines - T / 8 after every part

    meta                JSON: per case its parameters and an input digest

Our own two driver programs and stand-ins for two headers the build has no copy of -- strutil.h and
boost/functional/hash.hpp (boost::hash_range; the hash reaches no result) -- are written, with the builds, into a
temporary directory that is removed afterwards.  An -O0 and an -O3 build run everything and must agree.  The real-capacity
run needs about 4 GB of memory per build.

Run where the reference sources are (REF, as in oracle/Makefile):
    REF=/path/to/reference python tests/golden/make_ref_pattern_evict_vectors.py [--check]
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
import pattern_evict_ref as per  # noqa: E402
from make_ref_pattern_vectors import BOOST_HASH, STRUTIL  # noqa: E402  (the same stand-ins)

OUT = os.path.join(HERE, "ref_pattern_evict_vectors.npz")
OPT = ("-O3", "-O0")                     # the reference builds with -O3 (Makefile:4)

# usage: lru_driver <L> <C> <lines.bin>  ->  one character per line ('1' existed, '0' not), then " <put calls>"
LRU_DRIVER = r"""
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "LRU.h"

int main(int argc, char **argv)
{
  const unsigned L = (unsigned)atoi(argv[1]);
  LRUCache<std::vector<uint8_t>, int, std::vector<uint8_t>> cache(atoi(argv[2]));
  FILE *f = fopen(argv[3], "rb");
  if (!f) return 3;
  std::vector<uint8_t> line(L);
  std::string out;
  unsigned long long puts = 0;
  while (fread(line.data(), 1, L, f) == L) {
    if (cache.exist(line)) {
      out.push_back('1');
    } else {
      cache.put(line, 0);
      puts++;
      out.push_back('0');
    }
  }
  fclose(f);
  printf("%s %llu\n", out.c_str(), puts);
  return 0;
}
"""

# usage: pattern_driver <mult> <a0> <b0> <a1> <b1> ...  ->  per part "p <lines> Z R T U Total <6 implicit> <6 explicit>"
PATTERN_DRIVER = r"""
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <fmt/core.h>
#include "Pattern.h"

int main(int argc, char **argv)
{
  const uint64_t mult = strtoull(argv[1], nullptr, 0);
  comp::Pattern pat(8);
  comp::PatternResult *r = static_cast<comp::PatternResult *>(pat.GetResult());
  std::vector<uint8_t> line(8);
  unsigned long long lines = 0;
  for (int k = 2; k + 1 < argc; k += 2) {
    const uint64_t a = strtoull(argv[k], nullptr, 0), b = strtoull(argv[k + 1], nullptr, 0);
    for (uint64_t i = a; i < b; i++) {
      const uint64_t v = i * mult;
      memcpy(line.data(), &v, 8);
      pat.CompressLine(line);
      lines++;
    }
    printf("p %llu %llu %llu %llu %llu %llu", lines, (unsigned long long)r->Z, (unsigned long long)r->R, (unsigned long long)r->T,
           (unsigned long long)r->U, (unsigned long long)r->Total);
    for (int j = 0; j < 6; j++) printf(" %llu", (unsigned long long)r->ImplicitCounts[j]);
    for (int j = 0; j < 6; j++) printf(" %llu", (unsigned long long)r->ExplicitCounts[j]);
    printf("\n");
    fflush(stdout);
  }
  return 0;
}
"""


def generate(ref: str) -> dict:
    src = os.path.join(ref, "src")
    import torch
    fmt_inc = os.path.join(os.path.dirname(torch.__file__), "include")
    tmp = tempfile.mkdtemp(prefix="ref_pattern_evict_")
    arrays, meta = {}, {"source": "reference src/compressor/LRU.h and Pattern.cpp, compiled unmodified", "builds": list(OPT), "cases": [],
                        "real_parts": [list(p) for p in per.REAL_PARTS], "real_fields": list(per.REAL_FIELDS)}
    try:
        os.makedirs(os.path.join(tmp, "boost", "functional"))
        for name, text in (("strutil.h", STRUTIL), ("lru_driver.cpp", LRU_DRIVER), ("pattern_driver.cpp", PATTERN_DRIVER),
                           (os.path.join("boost", "functional", "hash.hpp"), BOOST_HASH)):
            with open(os.path.join(tmp, name), "w") as f:
                f.write(text)
        inc = ["-I", tmp, "-I", fmt_inc, "-I", os.path.join(src, "compressor"), "-I", src]
        lru, pat = [], []
        for opt in OPT:
            lru.append(os.path.join(tmp, "lru" + opt))
            subprocess.run(["g++", opt, "-std=c++17", "-w", *inc, os.path.join(tmp, "lru_driver.cpp"), "-o", lru[-1]], check=True)
            pat.append(os.path.join(tmp, "pattern" + opt))
            subprocess.run(["g++", opt, "-std=c++17", "-DFMT_HEADER_ONLY", "-w", *inc, os.path.join(tmp, "pattern_driver.cpp"),
                            os.path.join(src, "compressor", "Pattern.cpp"), os.path.join(src, "utils.cpp"), "-o", pat[-1]], check=True)
        # the real capacity: both builds side by side (minutes), the small cases meanwhile
        args = [hex(per.GOLDEN)] + [str(x) for p in per.REAL_PARTS for x in p]
        real = [subprocess.Popen([exe, *args], stdout=subprocess.PIPE, text=True) for exe in pat]
        path = os.path.join(tmp, "lines.bin")
        for spec in per.CASES:
            lines = per.case_input(spec)
            lines.tofile(path)
            outs = {subprocess.run([exe, str(spec["L"]), str(spec["C"]), path], capture_output=True, text=True, check=True).stdout for exe in lru}
            assert len(outs) == 1, f"{spec['name']}: the reference's answers depend on the build"
            bits, puts = outs.pop().split()
            flags = np.frombuffer(bits.encode(), dtype=np.uint8) == ord("1")
            assert len(flags) == len(lines) and int(puts) == int((~flags).sum())
            arrays[spec["name"] + "/existed"] = np.packbits(flags)
            arrays[spec["name"] + "/insertions"] = np.array(int(puts), dtype=np.uint64)
            meta["cases"].append(dict(spec, sha256=per.digest(lines), hits=int(flags.sum())))
        print(f"{len(per.CASES)} small-capacity cases")
        texts = set()
        for p in real:
            out, _ = p.communicate()
            assert p.returncode == 0
            texts.add(out)
        assert len(texts) == 1, "the real-capacity run depends on the build"
        rows = [[int(x) for x in ln.split()[1:]] for ln in texts.pop().split("\n") if ln.startswith("p ")]
        totals = np.array(rows, dtype=np.uint64)
        assert totals.shape == (len(per.REAL_PARTS), len(per.REAL_FIELDS)) and not (totals[:, 3] % 8).any()
        arrays["real/totals"] = totals
        arrays["real/insertions"] = totals[:, 0] - totals[:, 3] // 8
        print("real capacity: lines", totals[:, 0].tolist(), "T", totals[:, 3].tolist(), "insertions", arrays["real/insertions"].tolist())
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    arrays["meta"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), dtype=np.uint8)
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
