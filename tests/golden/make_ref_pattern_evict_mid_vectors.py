#!/usr/bin/env python3
"""Generate tests/golden/ref_pattern_evict_mid_vectors.npz: what the REFERENCE's own line cache answers at capacities of
65537 and 262145 lines and on the edge-driven trace (tests/pattern_evict_ref.py: MID_CASES, edge_index).

src/compressor/LRU.h, compiled unmodified: LRUCache<std::vector<uint8_t>, int, std::vector<uint8_t>> of capacity C, driven
as Pattern::isExistedBefore drives it, by the driver program of make_ref_pattern_evict_vectors.py --

    <case>/existed      the per-line answer, packed bits (numpy.packbits)
    <case>/insertions   the number of put calls

    meta                JSON: per case its parameters, its hits and an input digest

and, beside it, tests/golden/pattern_evict_coverage.json: what pattern_evict_ref.census counts on every case (in one call
and in the calls of pattern_evict_ref.mid_cuts), written only once the census has reproduced the reference's flags, with
the cumulative counters that the GPU tests compare the test library's read-outs against.

The driver and the two stand-in headers come from the existing makers; they are written, with the builds, into a temporary
directory that is removed afterwards.  An -O0 and an -O3 build run everything and must agree.  The real-capacity part of
make_ref_pattern_evict_vectors.py is not run again.

Run where the reference sources are (REF, as in oracle/Makefile):
    REF=/path/to/reference python tests/golden/make_ref_pattern_evict_mid_vectors.py [--check]
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
from make_ref_pattern_evict_vectors import LRU_DRIVER, OPT  # noqa: E402  (the same driver, the same two builds)
from make_ref_pattern_vectors import BOOST_HASH, STRUTIL  # noqa: E402  (the same stand-ins)

OUT = os.path.join(HERE, "ref_pattern_evict_mid_vectors.npz")
COVERAGE = os.path.join(HERE, "pattern_evict_coverage.json")


def generate(ref: str) -> dict:
    src = os.path.join(ref, "src")
    tmp = tempfile.mkdtemp(prefix="ref_pattern_evict_mid_")
    arrays, meta = {}, {"source": "reference src/compressor/LRU.h, compiled unmodified", "builds": list(OPT), "cases": [],
                        "motifs": [list(m) for m in per.MOTIFS], "edge_seed": per.EDGE_SEED}
    try:
        os.makedirs(os.path.join(tmp, "boost", "functional"))
        for name, text in (("strutil.h", STRUTIL), ("lru_driver.cpp", LRU_DRIVER), (os.path.join("boost", "functional", "hash.hpp"), BOOST_HASH)):
            with open(os.path.join(tmp, name), "w") as f:
                f.write(text)
        import torch
        inc = ["-I", tmp, "-I", os.path.join(os.path.dirname(torch.__file__), "include"), "-I", os.path.join(src, "compressor"), "-I", src]
        lru = []
        for opt in OPT:
            lru.append(os.path.join(tmp, "lru" + opt))
            subprocess.run(["g++", opt, "-std=c++17", "-w", *inc, os.path.join(tmp, "lru_driver.cpp"), "-o", lru[-1]], check=True)
        path = os.path.join(tmp, "lines.bin")
        for spec in per.MID_CASES:
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
            print(spec["name"], len(flags), "lines,", int(puts), "insertions")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    arrays["meta"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), dtype=np.uint8)
    return arrays


def coverage(arrays: dict) -> str:
    """The text of pattern_evict_coverage.json: per case what pattern_evict_ref.census counts, in one call and in the
    calls of mid_cuts, once its flags have been found equal to the reference's."""
    cases = {}
    for spec in per.MID_CASES:
        want = np.unpackbits(arrays[spec["name"] + "/existed"])[:spec["n"]].astype(bool)
        cases[spec["name"]], runs = per.coverage_of(spec)
        for how, z in runs.items():
            assert (z["flags"] == want).all() and z["insertions"] == int(arrays[spec["name"] + "/insertions"]), (spec["name"], how)
    doc = {"counters": list(per.COUNTERS), "cut_steps": list(per.CUT_STEPS), "launch_limit": per.LAUNCH_LIMIT, "cases": cases}
    return json.dumps(doc, sort_keys=True, indent=1) + "\n"


def main():
    ref = os.environ.get("REF")
    if not ref:
        sys.exit("set REF to the root of the reference sources (as for oracle/Makefile)")
    arrays = generate(ref)
    cov = coverage(arrays)
    if "--check" in sys.argv:
        with open(COVERAGE) as f:
            if f.read() != cov:
                sys.exit(f"differs from {COVERAGE}")
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
    assert len(buf.getvalue()) < (1 << 20), "a committed file stays below 1 MiB"
    with open(OUT, "wb") as f:
        f.write(buf.getvalue())
    with open(COVERAGE, "w") as f:
        f.write(cov)
    print(OUT, os.path.getsize(OUT), "bytes;", COVERAGE, len(cov), "bytes")


if __name__ == "__main__":
    main()
