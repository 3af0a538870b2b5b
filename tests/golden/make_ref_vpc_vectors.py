#!/usr/bin/env python3
"""Generate tests/golden/ref_vpc_vectors.npz: what the REFERENCE's own VPC (src/compressor/VPC.cpp, every
src/compressor/VPCmodules/*.cpp and src/utils.cpp, compiled unmodified with g++) reports for the seeded cases of
tests/vpc_ref.py.  Per case ("<name>.<key>" arrays):

    sizes     CompressLine's return value per line (uint16)
    clusters  the cluster of each line: the ClusterStat whose count CompressLine incremented (int8)
    totals    OriginalSize, CompressedSize, then per cluster -1 .. M-1: count, originalSize, compressedSize,
              m_NumLines (uint64)
    doubles   CompRatio, then per cluster: compRatio, m_SumMAE, m_MAE, m_SumMSE, m_MSE (float64, exact)
    hist      every non-zero compSizeHistogram entry as (cluster, size, count), sizes of 288 and above included (int64)

The long cases (vpc_ref.LONG) keep totals / doubles / hist and, in "meta", the SHA-256 of their per-line arrays only.
"meta" (a JSON string) holds the case specs with line counts, input and configuration digests and what the reference
parsed from each configuration (m_LineSize, m_NumModules, the whole m_EncodingBits map, the module classes in order,
the compressLine variant); and, for PRINT_CASES, the text VPCResult::Print / PrintDetail(workload, path) write into new
files over all lines but the last (what the command line does with <dir>/<name>.npy: the loader drops the last row),
workload "<dir>_<name>", with that run's totals / doubles / hist as "<name>.print.*" arrays.

Our own driver program and stand-ins for the strutil.h and json/json.h headers are written, with the builds, into a
temporary directory that is removed afterwards.  The json/json.h stand-in is a small JSON reader of its own covering
exactly what VPC::parseConfig uses; it shares nothing with the library's reader (csrc/mpc_json.h).  The driver prints
back what the reference parsed, and the generator compares that with the configuration.  The driver replaces the
global operator new / delete: every allocation and a 64-byte tail after it are filled with a non-zero sentinel.  Every
case runs under two sentinels and under an -O0 and an -O3 build, and the four runs must agree.

Run where the reference sources are (REF, as in oracle/Makefile):
    REF=/path/to/reference python tests/golden/make_ref_vpc_vectors.py [--check]
--check regenerates everything in memory and compares it with the committed file instead of writing it.
"""
import glob
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
import vpc_ref  # noqa: E402
from make_ref_sc2_vectors import STRUTIL  # noqa: E402

OUT = os.path.join(HERE, "ref_vpc_vectors.npz")
SENTINELS = (0xA5, 0x3C)
OPT = ("-O3", "-O0")                     # the reference builds with -O3 (Makefile:4)
PRINT_CASES = ("probe_L64", "mpc_L32", "bits_L32", "bits_L64", "root7_L32", "m1_L64", "L48")
PRINT_DIR = "refvpc"

JSON_H = r"""
#pragma once
// Stand-in for jsoncpp's <json/json.h>: a small JSON reader covering what VPC::parseConfig uses.  A member or index
// that is not there reads as null (asInt 0, asFloat 0, asBool false, asString ""); numbers are read with strtod into a
// double, asInt truncates it, asFloat rounds it to float.
#include <cstdlib>
#include <cstring>
#include <istream>
#include <iterator>
#include <map>
#include <string>
#include <utility>
#include <vector>
#define JSONCPP_STRING std::string
namespace Json {
struct Value {
  enum Kind { Null, Bool, Number, String, Array, Object };
  Kind kind = Null;
  double num = 0.0;
  std::string str;
  std::vector<Value> items;
  std::map<std::string, Value> members;
  std::map<int, Value> missing;        // the nulls handed out for indices past the end
  Value() {}
  Value(bool b) : kind(Bool), num(b ? 1.0 : 0.0) {}
  bool isNull() const { return kind == Null; }
  int asInt() const { return (kind == Number || kind == Bool) ? (int)num : 0; }
  float asFloat() const { return (kind == Number || kind == Bool) ? (float)num : 0.0f; }
  bool asBool() const { return (kind == Number || kind == Bool) && num != 0.0; }
  std::string asString() const { return kind == String ? str : std::string(); }
  unsigned size() const { return kind == Array ? (unsigned)items.size() : kind == Object ? (unsigned)members.size() : 0u; }
  Value &operator[](const std::string &key)
  {
    if (kind == Null) kind = Object;
    return members[key];
  }
  Value &operator[](int index)
  {
    if (kind == Array && index >= 0 && index < (int)items.size()) return items[(size_t)index];
    return missing[index];
  }
};

struct Reader {
  const char *p, *end;
  void ws() { while (p < end && (*p == ' ' || *p == '\t' || *p == '\n' || *p == '\r')) p++; }
  bool lit(const char *w)
  {
    const size_t n = std::strlen(w);
    if ((size_t)(end - p) < n || std::strncmp(p, w, n) != 0) return false;
    p += n;
    return true;
  }
  bool str(std::string &s)
  {
    if (p >= end || *p != '"') return false;
    for (p++; p < end && *p != '"'; p++) {
      if (*p == '\\') {
        if (++p >= end) return false;
        s += *p == 'n' ? '\n' : *p == 't' ? '\t' : *p == 'r' ? '\r' : *p;
      } else {
        s += *p;
      }
    }
    if (p >= end) return false;
    p++;
    return true;
  }
  bool value(Value &v)
  {
    ws();
    if (p >= end) return false;
    if (*p == '{') {
      p++;
      v.kind = Value::Object;
      ws();
      if (p < end && *p == '}') { p++; return true; }
      for (;;) {
        ws();
        std::string k;
        if (!str(k)) return false;
        ws();
        if (p >= end || *p != ':') return false;
        p++;
        Value m;
        if (!value(m)) return false;
        v.members[k] = std::move(m);
        ws();
        if (p < end && *p == ',') { p++; continue; }
        if (p < end && *p == '}') { p++; return true; }
        return false;
      }
    }
    if (*p == '[') {
      p++;
      v.kind = Value::Array;
      ws();
      if (p < end && *p == ']') { p++; return true; }
      for (;;) {
        Value e;
        if (!value(e)) return false;
        v.items.push_back(std::move(e));
        ws();
        if (p < end && *p == ',') { p++; continue; }
        if (p < end && *p == ']') { p++; return true; }
        return false;
      }
    }
    if (*p == '"') { v.kind = Value::String; return str(v.str); }
    if (lit("true")) { v = Value(true); return true; }
    if (lit("false")) { v = Value(false); return true; }
    if (lit("null")) { v = Value(); return true; }
    char *q = nullptr;
    const double d = std::strtod(p, &q);
    if (q == p) return false;
    v.kind = Value::Number;
    v.num = d;
    p = q;
    return true;
  }
};

class CharReaderBuilder {
public:
  Value &operator[](const std::string &key) { return settings_[key]; }
  Value settings_;
};

inline bool parseFromStream(const CharReaderBuilder &, std::istream &in, Value *root, JSONCPP_STRING *errs)
{
  const std::string text((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
  Reader r{text.c_str(), text.c_str() + text.size()};
  *root = Value();
  bool ok = r.value(*root);
  if (ok) { r.ws(); ok = r.p == r.end; }
  if (!ok && errs) *errs = "not a JSON document";
  return ok;
}
}  // namespace Json
"""

DRIVER = r"""
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <ios>
#include <iostream>
#include <map>
#include <new>
#include <set>
#include <sstream>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>
#include <fmt/core.h>
#define private public      // (the parsed configuration and the compressLine variant: the parse pins)
#include "VPC.h"
#include "VPCmodules/AllWordSameModule.h"
#include "VPCmodules/AllZeroModule.h"
#include "VPCmodules/PredCompModule.h"
#undef private

// Every allocation and 64 bytes after it hold a non-zero sentinel (set from the command line before anything is read).
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

static const char *module_kind(comp::CompressionModule *m)
{
  if (dynamic_cast<comp::AllZeroModule *>(m)) return "AllZero";
  if (dynamic_cast<comp::AllWordSameModule *>(m)) return "AllWordSame";
  if (dynamic_cast<comp::PredCompModule *>(m)) return "PredComp";
  return "?";
}

static void print_stats(comp::VPCResult *r, int M)
{
  std::printf("r %llu %llu %a\n", (unsigned long long)r->OriginalSize, (unsigned long long)r->CompressedSize, r->CompRatio);
  for (int i = -1; i < M; i++) {
    comp::ClusterStat &c = r->m_ClusterStats[i];
    std::printf("c %d %llu %llu %llu %a %llu %a %a %a %a\n", i, (unsigned long long)c.count, (unsigned long long)c.originalSize,
                (unsigned long long)c.compressedSize, c.compRatio, (unsigned long long)r->m_NumLines[i], r->m_SumMAE[i],
                r->m_MAE[i], r->m_SumMSE[i], r->m_MSE[i]);
  }
  for (int i = -1; i < M; i++)
    for (auto &kv : r->m_ClusterStats[i].compSizeHistogram)
      if (kv.second) std::printf("h %d %d %llu\n", i, kv.first, (unsigned long long)kv.second);
}

// usage:
//   driver <sentinel> parse <cfg.json>              -> "L", "M", "bits <cluster> <bits>" per m_EncodingBits entry,
//                                                      "mod <i> <class>" per module, "line <compressLine variant>"
//   driver <sentinel> run <cfg.json> <lines.bin>    -> "s <size> <cluster>" per line, then the statistics:
//        "r <orig> <comp> <ratio>", "c <cluster> <count> <orig> <comp> <ratio> <lines> <sumMAE> <MAE> <sumMSE> <MSE>",
//        "h <cluster> <size> <count>" per non-zero histogram entry (doubles as %a)
//   driver <sentinel> print <cfg.json> <lines.bin> <workload> <csv> <detail csv>  -> Print, PrintDetail, the statistics
int main(int argc, char **argv)
{
  if (argc < 4) return 2;
  g_sentinel = (unsigned char)std::strtoul(argv[1], nullptr, 0);
  const std::string mode = argv[2];
  comp::VPC vpc(argv[3]);
  const int M = vpc.m_NumModules;
  if (mode == "parse") {
    std::printf("L %d\nM %d\n", vpc.m_LineSize, M);
    for (auto &kv : vpc.m_EncodingBits) std::printf("bits %d %d\n", kv.first, kv.second);
    for (int i = 0; i < M; i++) std::printf("mod %d %s\n", i, module_kind(vpc.m_CompModules[(size_t)i]));
    std::printf("line %s\n", vpc.compressLine == &comp::VPC::compressLineAllWordSame ? "AllWordSame"
                             : vpc.compressLine == &comp::VPC::compressLineOnlyAllZero ? "OnlyAllZero" : "?");
    return 0;
  }
  if (argc < 5) return 2;
  auto lines = read_lines(argv[4], (unsigned)vpc.m_LineSize);
  comp::VPCResult *r = static_cast<comp::VPCResult *>(vpc.GetResult());
  std::vector<uint64_t> before((size_t)M + 1);
  for (auto &line : lines) {
    for (int i = -1; i < M; i++) before[(size_t)(i + 1)] = r->m_ClusterStats[i].count;
    const unsigned size = vpc.CompressLine(line);
    int k = -2;
    for (int i = -1; i < M; i++) {
      const uint64_t now = r->m_ClusterStats[i].count;
      if (now != before[(size_t)(i + 1)]) {
        if (k != -2 || now != before[(size_t)(i + 1)] + 1) std::exit(5);
        k = i;
      }
    }
    if (k == -2) std::exit(6);
    if (mode == "run") std::printf("s %u %d\n", size, k);
  }
  if (mode == "print") {
    if (argc < 8) return 2;
    r->Print(argv[5], argv[6]);
    r->PrintDetail(argv[5], argv[7]);
  }
  print_stats(r, M);
  return 0;
}
"""


def _run(exe, *args) -> str:
    r = subprocess.run([exe, *[str(a) for a in args]], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"{os.path.basename(exe)} {args[:3]}: exit {r.returncode}\n{r.stdout[-800:]}{r.stderr[-800:]}")
    return r.stdout


def _parse_pins(out: str) -> dict:
    d = {"bits": {}, "modules": []}
    for ln in out.split("\n"):
        p = ln.split()
        if not p:
            continue
        if p[0] in ("L", "M"):
            d[p[0]] = int(p[1])
        elif p[0] == "bits":
            d["bits"][p[1]] = int(p[2])
        elif p[0] == "mod":
            d["modules"].append(p[2])
        elif p[0] == "line":
            d["line"] = p[1]
    return d


def _expected_parse(cfg: dict) -> dict:
    """What parseConfig should have read from the configuration (VPC.cpp:97-330)."""
    ov = cfg["overview"]
    M = int(ov["num_modules"])
    bits = ov.get("encoding_bits") or [vpc_ref.default_bits(M)] * (M + 1)
    kinds = {"AllZero": "AllZero", "AllWordSame": "AllWordSame", "ByteplaneAllSame": "AllWordSame", "PredComp": "PredComp"}
    return {"L": int(ov["lineSize"]), "M": M, "bits": {str(k - 1): int(b) for k, b in enumerate(bits)},
            "modules": [kinds[cfg["modules"][str(i)]["name"]] for i in range(M)]}


def _parse_stats(out: str, M: int):
    sizes, clusters, hist, per = [], [], [], {}
    totals, dbl = None, None
    for ln in out.split("\n"):
        p = ln.split()
        if not p:
            continue
        if p[0] == "s":
            sizes.append(int(p[1]))
            clusters.append(int(p[2]))
        elif p[0] == "r":
            totals, dbl = [int(p[1]), int(p[2])], [float.fromhex(p[3])]
        elif p[0] == "c":
            per[int(p[1])] = p[2:]
        elif p[0] == "h":
            hist.append([int(p[1]), int(p[2]), int(p[3])])
    assert sorted(per) == list(range(-1, M)) and totals is not None
    for k in range(-1, M):
        f = per[k]
        totals += [int(f[0]), int(f[1]), int(f[2]), int(f[4])]
        dbl += [float.fromhex(x) for x in (f[3], f[5], f[6], f[7], f[8])]
    assert not sizes or max(sizes) < (1 << 16)
    return (np.array(sizes, np.uint16), np.array(clusters, np.int8), np.array(totals, np.uint64),
            np.array(dbl, np.float64), np.array(hist, np.int64).reshape(-1, 3))


def generate(ref: str) -> dict:
    src = os.path.join(ref, "src")
    comp_dir = os.path.join(src, "compressor")
    import torch
    fmt_inc = os.path.join(os.path.dirname(torch.__file__), "include")
    tmp = tempfile.mkdtemp(prefix="ref_vpc_")
    arrays = {}
    meta = {"source": "reference src/compressor/VPC.cpp, VPCmodules/*.cpp and src/utils.cpp, compiled unmodified",
            "sentinels": list(SENTINELS), "builds": list(OPT), "cases": [], "long": [], "print": []}
    try:
        os.makedirs(os.path.join(tmp, "json"))
        for rel, text in (("strutil.h", STRUTIL), ("json/json.h", JSON_H), ("driver.cpp", DRIVER)):
            with open(os.path.join(tmp, rel), "w") as f:
                f.write(text)
        modules = sorted(glob.glob(os.path.join(comp_dir, "VPCmodules", "*.cpp")))
        exes = []
        for opt in OPT:
            exe = os.path.join(tmp, "driver" + opt)
            subprocess.run(["g++", opt, "-std=c++17", "-DFMT_HEADER_ONLY", "-w", "-I", tmp, "-I", fmt_inc, "-I", comp_dir,
                            "-I", src, os.path.join(tmp, "driver.cpp"), os.path.join(comp_dir, "VPC.cpp"), *modules,
                            os.path.join(src, "utils.cpp"), "-o", exe], check=True)
            exes.append(exe)
        runs = [(exe, s) for exe in exes for s in SENTINELS]
        path = os.path.join(tmp, "lines.bin")
        for spec in vpc_ref.CASES + vpc_ref.LONG:
            name = spec["name"]
            cfg = vpc_ref.case_config(spec)
            cfg_path = vpc_ref.configs.write_config(cfg, os.path.join(tmp, name + ".json"))
            outs = {_run(exe, s, "parse", cfg_path) for exe, s in runs}
            assert len(outs) == 1, f"{name}: what the reference parsed depends on the sentinel or the build"
            parsed = _parse_pins(outs.pop())
            want = _expected_parse(cfg)
            assert {k: parsed[k] for k in want} == want, (name, parsed, want)
            M = parsed["M"]
            lines = vpc_ref.case_lines(spec)
            lines.tofile(path)
            outs = {_run(exe, s, "run", cfg_path, path) for exe, s in runs}
            assert len(outs) == 1, f"{name}: the reference's numbers depend on the sentinel or the build"
            sizes, clusters, totals, dbl, hist = _parse_stats(outs.pop(), M)
            assert len(sizes) == len(lines)
            rec = dict(spec, M=M, n=len(lines), sha256=vpc_ref.digest(lines), config_sha256=vpc_ref.config_digest(cfg),
                       parsed=parsed)
            arrays[f"{name}.totals"], arrays[f"{name}.doubles"], arrays[f"{name}.hist"] = totals, dbl, hist
            if spec.get("long"):
                rec["sizes_sha256"], rec["clusters_sha256"] = vpc_ref.digest(sizes), vpc_ref.digest(clusters)
                meta["long"].append(rec)
            else:
                arrays[f"{name}.sizes"], arrays[f"{name}.clusters"] = sizes, clusters
                meta["cases"].append(rec)
            if name in PRINT_CASES:
                lines[:-1].tofile(path)
                texts, stats = set(), set()
                for k, (exe, s) in enumerate(runs):
                    csv, det = os.path.join(tmp, f"r{k}.csv"), os.path.join(tmp, f"d{k}.csv")
                    stats.add(_run(exe, s, "print", cfg_path, path, f"{PRINT_DIR}_{name}", csv, det))
                    with open(csv) as f, open(det) as g:
                        texts.add((f.read(), g.read()))
                    os.remove(csv)
                    os.remove(det)
                assert len(texts) == 1 and len(stats) == 1, name
                results, detail = texts.pop()
                _, _, t, d, h = _parse_stats(stats.pop(), M)
                arrays[f"{name}.print.totals"], arrays[f"{name}.print.doubles"], arrays[f"{name}.print.hist"] = t, d, h
                meta["print"].append({"case": name, "npy": f"{PRINT_DIR}/{name}.npy", "results": results, "detail": detail})
            print(f"{name}: {len(lines)} lines, M {M}, ratio {dbl[0]!r}", flush=True)
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
        print(f"{OUT}: no difference ({len(arrays)} arrays; sentinels {SENTINELS}, builds {OPT})")
        return
    buf = io.BytesIO()
    np.savez_compressed(buf, **arrays)
    with open(OUT, "wb") as f:
        f.write(buf.getvalue())
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
