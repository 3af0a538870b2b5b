#!/usr/bin/env python3
"""Generate tests/golden/ref_loader_vectors.json: what the REFERENCE's own trace loaders (src/loader/LoaderGPGPU.cpp --
trace::gpgpusim::LoaderGPGPU for GPGPU-Sim .log files and trace::apsim::LoaderGPGPU for APSim .txt files -- and
src/loader/LoaderNPY.cpp, compiled unmodified with g++) deliver for the seeded trace files of tests/loader_ref.py:CASES.

Our own driver restates only the loop of the reference's compressLines (src/main.cpp:213-248): GetCacheline, isEnd tested
before the request is used, and for .log the GLOBAL_ACC_R / GLOBAL_ACC_W filter.  Per case the output holds the case's
recipe, the sha256 of the input file and, under "ref":

    line_size, num_lines     GetCachelineSize() and GetNumLines()
    delivered, delivered_sha256, delivered_sizes
                             the requests the loop hands on: their number, the sha256 of their data bytes in order, and
                             how many of them had which data size
    req_sizes, rw            (.txt) how many delivered requests had which reqSize and which rw (0 READ, 1 WRITE, 2 NA)

For .txt, "ref" holds all of that per line size asked for (32, 64) and per order of calls: "fresh" (the loop on a loader
that was just constructed; GetNumLines() from a second fresh loader) and "after" (GetNumLines() first, then the loop on
the same loader -- the reference's Reset() does not empty its beat queues).

What this pins and what it does not: the third-party npy.hpp that LoaderNPY.cpp includes is not available, so
LoaderNPY.cpp is compiled against our own stand-in offering npy::LoadArrayFromNumpy(path, shape, fortran_order, data).
That pins LoaderNPY.cpp itself (the shape it reports, the dropped last row, GetNumLines counting that row), NOT the
parsing of the .npy header.  strutil.h is a stand-in of ours as well (split, contains).  The driver, both stand-ins and
the build live in a temporary directory outside the repository that is removed afterwards; the output holds recipes,
digests and recorded numbers only.

Run where the reference sources are (REF, as in oracle/Makefile):
    REF=/path/to/reference python tests/golden/make_ref_loader_vectors.py
"""
import json
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import conftest  # noqa: E402,F401  (puts the repository root on the path)
import loader_ref  # noqa: E402

STRUTIL = r"""
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
namespace strutil {
inline std::vector<std::string> split(const std::string &s, char d)
{
  std::vector<std::string> out;
  size_t a = 0, b;
  while ((b = s.find(d, a)) != std::string::npos) { out.push_back(s.substr(a, b - a)); a = b + 1; }
  out.push_back(s.substr(a));
  return out;
}
inline bool contains(const std::string &s, const std::string &what) { return s.find(what) != std::string::npos; }
}
"""

NPY = r"""
#pragma once
// stand-in for the third-party npy.hpp: reads a C-order uint8 .npy file of format version 1, 2 or 3
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>
namespace npy {
template <typename T, typename S>
inline void LoadArrayFromNumpy(const std::string &path, std::vector<S> &shape, bool &fortran_order, std::vector<T> &data)
{
  static_assert(sizeof(T) == 1, "uint8 only");
  std::ifstream f(path, std::ios::binary);
  if (!f) { printf("npy stand-in: cannot open %s\n", path.c_str()); exit(1); }
  unsigned char pre[12];
  f.read((char *)pre, 10);
  size_t hlen = pre[8] | (pre[9] << 8);
  if (pre[6] != 1) { f.read((char *)pre + 10, 2); hlen |= ((size_t)pre[10] << 16) | ((size_t)pre[11] << 24); }
  std::string h(hlen, '\0');
  f.read(&h[0], (std::streamsize)hlen);
  if (h.find("'|u1'") == std::string::npos) { printf("npy stand-in: not uint8\n"); exit(1); }
  fortran_order = h.find("'fortran_order': True") != std::string::npos;
  const size_t a = h.find('(', h.find("'shape'")), b = h.find(')', a);
  shape.clear();
  size_t total = 1;
  for (size_t i = a + 1; i < b;) {
    while (i < b && (h[i] < '0' || h[i] > '9')) i++;
    if (i >= b) break;
    S v = 0;
    while (i < b && h[i] >= '0' && h[i] <= '9') v = v * 10 + (S)(h[i++] - '0');
    shape.push_back(v);
    total *= (size_t)v;
  }
  data.resize(total);
  f.read((char *)data.data(), (std::streamsize)total);
  if ((size_t)f.gcount() != total) { printf("npy stand-in: short file\n"); exit(1); }
}
}
"""

DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include "LoaderGPGPU.h"
#include "LoaderNPY.h"
// usage: driver log|npy|txt FILE DUMP [line_size fresh|after]
static std::map<unsigned long long, unsigned long long> g_sizes, g_req, g_rw;
static unsigned long long g_delivered = 0;
static FILE *g_dump;
static void hand_on(trace::MemReq_t *r)
{
  g_delivered++;
  g_sizes[r->data.size()]++;
  g_req[r->reqSize]++;
  g_rw[(unsigned long long)r->rw]++;
  if (!r->data.empty()) fwrite(r->data.data(), 1, r->data.size(), g_dump);
}
static void show(const char *name, const std::map<unsigned long long, unsigned long long> &m)
{
  printf("%s", name);
  for (auto &kv : m) printf(" %llu:%llu", kv.first, kv.second);
  printf("\n");
}
int main(int argc, char **argv)
{
  const std::string kind = argv[1], path = argv[2];
  g_dump = fopen(argv[3], "wb");
  unsigned lineSize = 0;
  unsigned long long numLines = 0;
  if (kind == "log") {
    trace::Loader *loader = new trace::gpgpusim::LoaderGPGPU(path);
    lineSize = loader->GetCachelineSize();
    numLines = loader->GetNumLines();
    trace::MemReq_t *memReq = new trace::gpgpusim::MemReqGPU_t;
    while (1) {
      memReq = loader->GetCacheline(memReq);
      if (memReq->isEnd) break;
      const trace::gpgpusim::MemReqGPU_t *g = static_cast<trace::gpgpusim::MemReqGPU_t *>(memReq);
      if (!(g->reqType == trace::gpgpusim::GLOBAL_ACC_R || g->reqType == trace::gpgpusim::GLOBAL_ACC_W)) continue;
      hand_on(memReq);
    }
  } else if (kind == "npy") {
    trace::Loader *loader = new trace::LoaderNPY(path);
    lineSize = loader->GetCachelineSize();
    numLines = loader->GetNumLines();
    trace::MemReq_t *memReq = new trace::MemReq_t;
    while (1) {
      memReq = loader->GetCacheline(memReq);
      if (memReq->isEnd) break;
      hand_on(memReq);
    }
  } else {
    const unsigned asked = (unsigned)atoi(argv[4]);
    const bool after = !strcmp(argv[5], "after");
    trace::Loader *loader = new trace::apsim::LoaderGPGPU(path, asked);
    lineSize = loader->GetCachelineSize();
    if (after) numLines = loader->GetNumLines();
    trace::MemReq_t *memReq = new trace::apsim::MemReqGPU_t;
    while (1) {
      memReq = loader->GetCacheline(memReq);
      if (memReq->isEnd) break;
      hand_on(memReq);
    }
    if (!after) numLines = (new trace::apsim::LoaderGPGPU(path, asked))->GetNumLines();
  }
  fclose(g_dump);
  printf("line_size %u\nnum_lines %llu\ndelivered %llu\n", lineSize, numLines, g_delivered);
  show("sizes", g_sizes);
  show("req_sizes", g_req);
  show("rw", g_rw);
  return 0;
}
"""


def run_driver(exe, dump, args, txt):
    r = subprocess.run([exe] + args[:2] + [dump] + args[2:], capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit(f"driver {args}: exit {r.returncode}\n{r.stdout}\n{r.stderr}")
    out = {}
    for ln in r.stdout.strip().split("\n"):
        p = ln.split()
        if p[0] in ("line_size", "num_lines", "delivered"):
            out[p[0]] = int(p[1])
        else:
            out[{"sizes": "delivered_sizes"}.get(p[0], p[0])] = {kv.split(":")[0]: int(kv.split(":")[1]) for kv in p[1:]}
    with open(dump, "rb") as f:
        out["delivered_sha256"] = loader_ref.bytes_digest(f.read())
    if not txt:
        del out["req_sizes"], out["rw"]
    return out


def main():
    ref = os.environ.get("REF")
    if not ref:
        sys.exit("set REF to the root of the reference sources (as for oracle/Makefile)")
    src = os.path.join(ref, "src", "loader")
    import torch
    fmt_inc = os.path.join(os.path.dirname(torch.__file__), "include")
    tmp = tempfile.mkdtemp(prefix="ref_loader_")
    try:
        for name, text in (("strutil.h", STRUTIL), ("npy.hpp", NPY), ("driver.cpp", DRIVER)):
            with open(os.path.join(tmp, name), "w") as f:
                f.write(text)
        exe = os.path.join(tmp, "driver")
        subprocess.run(["g++", "-O1", "-std=c++17", "-DFMT_HEADER_ONLY", "-w", "-include", "cstdint", "-I", tmp, "-I", fmt_inc, "-I", src,
                        os.path.join(tmp, "driver.cpp"), os.path.join(src, "LoaderGPGPU.cpp"), os.path.join(src, "LoaderNPY.cpp"),
                        "-o", exe], check=True)
        dump = os.path.join(tmp, "delivered.bin")
        out = []
        for spec in loader_ref.CASES:
            path = loader_ref.build_input(spec, tmp, name="case")
            case = dict(spec)
            case["sha256"] = loader_ref.file_digest(path)
            if spec["fmt"] == "txt":
                case["ref"] = {str(L): {order: run_driver(exe, dump, ["txt", path, str(L), order], True) for order in ("fresh", "after")}
                               for L in spec["line_sizes"]}
                show = {L: (v["fresh"]["delivered"], v["after"]["delivered"]) for L, v in case["ref"].items()}
            else:
                case["ref"] = run_driver(exe, dump, [spec["fmt"], path], False)
                show = (case["ref"]["line_size"], case["ref"]["num_lines"], case["ref"]["delivered"], case["ref"]["delivered_sizes"])
            os.unlink(path)
            out.append(case)
            print(f"{spec['name']}: {show}")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    dst = os.path.join(HERE, "ref_loader_vectors.json")
    with open(dst, "w") as f:
        json.dump({"source": "reference src/loader/LoaderGPGPU.cpp and LoaderNPY.cpp, compiled unmodified", "cases": out}, f,
                  separators=(",", ":"))
    print(dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()
