#!/usr/bin/env python3
"""Generate tests/golden/ref_baseline_chosen_vectors.npz: what the REFERENCE's own BDI, FPC and BPC report for the chosen
cases of tests/baseline_chosen.py:CASES.  The recipe is that of make_ref_baseline_vectors.py, whose driver text, strutil.h
stand-in, sentinels and builds are imported: BDI.cpp, FPC.cpp, BPC.cpp and utils.cpp compiled unmodified with g++ at -O3
and -O0, every case run under both sentinels, and the four runs must agree.  Per case ("<name>.<key>" arrays):

    sizes     CompressLine's return value per line (uint16)
    states    BDI only: the BDIState of each line (int8)
    stats     OriginalSize, CompressedSize, TotalWords (0 for BDI), Counts[...] at the end (uint64)
    ratio     CompRatio at the end (float64, exact)
    check     BDI only: BDI::checkBDI of the six (base, delta) combinations per line ([lines, 6] uint16)

and, for the groups of tests/test_baseline_chosen_gpu.py, "group_L<L>.<comp>.<key>": each compressor on
baseline_chosen.group_lines(L), and "pool_L<L>.<key>": BDI on baseline_chosen.random_pool(L).  "meta" (a JSON string) holds
the case specs with their line counts and input digests.  Only recorded numbers are written; `apart` at 128 bytes is
recorded in full (every row pair of every plane: the file stays near 120 KiB).

    REF=/path/to/reference python tests/golden/make_ref_baseline_chosen_vectors.py [--check]
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
import baseline_chosen  # noqa: E402
from make_ref_baseline_vectors import DRIVER, OPT, SENTINELS, _parse_run, _run  # noqa: E402
from make_ref_sc2_vectors import STRUTIL  # noqa: E402

OUT = os.path.join(HERE, "ref_baseline_chosen_vectors.npz")


def generate(ref: str) -> dict:
    src = os.path.join(ref, "src")
    import torch
    fmt_inc = os.path.join(os.path.dirname(torch.__file__), "include")
    tmp = tempfile.mkdtemp(prefix="ref_baseline_chosen_")
    arrays, meta = {}, {"source": "reference src/compressor/{BDI,FPC,BPC}.cpp, compiled unmodified",
                        "sentinels": list(SENTINELS), "builds": list(OPT), "cases": []}
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
        extra = [{"name": f"group_L{L}.{comp}", "comp": comp, "L": L, "lines": "group"} for L in baseline_chosen.GROUP_SIZES
                 for comp in ("BDI", "FPC", "BPC")]
        extra += [{"name": f"pool_L{L}", "comp": "BDI", "L": L, "lines": "pool"} for L in baseline_chosen.BDI_SIZES]
        for spec in baseline_chosen.CASES + extra:
            name, comp, L = spec["name"], spec["comp"], spec["L"]
            if spec.get("lines") == "group":
                lines = baseline_chosen.group_lines(L)
            elif spec.get("lines") == "pool":
                lines = baseline_chosen.random_pool(L)
            else:
                lines, _ = baseline_chosen.build(name)
            lines.tofile(path)
            outs = {_run(exe, s, "run", comp, L, path) for exe, s in runs}
            assert len(outs) == 1, f"{name}: the reference's numbers depend on the sentinel or the build"
            sizes, states, stats, ratio = _parse_run(outs.pop(), comp)
            assert len(sizes) == len(lines)
            arrays[f"{name}.sizes"] = sizes
            if comp == "BDI":
                assert (states >= 0).all()
                arrays[f"{name}.states"] = states
            if comp == "BDI" and "lines" not in spec:
                outs = {_run(exe, s, "check", L, path) for exe, s in runs}
                assert len(outs) == 1
                check = np.array([[int(x) for x in ln.split()[1:]] for ln in outs.pop().strip().split("\n")])
                assert check.shape == (len(lines), 6) and check.max() < 65536
                arrays[f"{name}.check"] = check.astype(np.uint16)
            arrays[f"{name}.stats"] = stats
            arrays[f"{name}.ratio"] = ratio
            meta["cases"].append(dict(spec, n=len(lines), sha256=baseline_chosen.digest(lines)))
            print(f"{name}: {len(lines)} lines, ratio {ratio[0]!r}")
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
