#!/usr/bin/env python3
"""Timings of the two Fit analyses on the MI355X (tests/test_fit_gpu.py checks the numbers; this measures what they cost).
Device-resident traces of --gib GiB at 32-, 64- and 128-byte lines: random bytes (mpc_synth_fill) and the 16-byte record
trace of tests/fit_ref.py (a tile of 65 536 lines, repeated).  Per trace, taking turns for --rounds rounds after a warm-up
pass of each, HIP events on the launching stream around each launch: the pair table (FitPairs), the residue histogram
for base[i] = max(i - 4, 0) (FitResidues) and the stream alone (mpc_read_bandwidth_probe) on the same buffer.  Beside
them the numpy reference's rate on the first 4096 lines, on the host.  The pair kernel's cost is set by L^2 residues per
line, not by bytes: the table gives lines, pairs and bytes per second.
    python tools/time_fit.py [--gib G] [--rounds N] [--out FILE]"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import fit_ref  # noqa: E402

mpc = importlib.import_module("cal_22-mpc_amd")
TILE = 1 << 16


def _trace(L, kind, gib):
    n = (gib << 30) // L
    buf = torch.empty(n * L, dtype=torch.uint8, device="cuda:0")
    if kind == "records16":
        tile = torch.from_numpy(fit_ref.records16(TILE, L, 1).reshape(-1)).to("cuda:0")
        buf.view(n // TILE, TILE * L).copy_(tile[None, :].expand(n // TILE, TILE * L))
    else:
        mpc.synth_fill(buf.data_ptr(), n, L, kind)
    torch.cuda.synchronize()
    return buf, n


def _rounds(passes, st, rounds):
    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        fn()
        b.record(st)
        return a, b

    for fn in passes.values():
        fn()
    torch.cuda.synchronize()
    rec = [{name: timed(fn) for name, fn in passes.items()} for _ in range(rounds)]
    torch.cuda.synchronize()
    return {name: [r[name][0].elapsed_time(r[name][1]) for r in rec] for name in passes}


def case(L, kind, gib, rounds):
    buf, n = _trace(L, kind, gib)
    st = torch.cuda.Stream()
    base = [max(i - 4, 0) for i in range(L)]
    pairs, res = mpc.FitPairs(L, device=0), mpc.FitResidues(L, base, device=0)
    ms = _rounds({"pairs": lambda: pairs.compress_device(buf.data_ptr(), n, stream=st.cuda_stream),
                  "residues": lambda: res.compress_device(buf.data_ptr(), n, stream=st.cuda_stream),
                  "stream alone": lambda: mpc.read_bandwidth_probe(buf.data_ptr(), n * L, stream=st.cuda_stream)}, st, rounds)
    assert pairs.lines() == res.lines() == (rounds + 1) * n
    head = buf[:4096 * L].cpu().numpy().reshape(4096, L)
    t0 = time.perf_counter()
    fit_ref.pair_table(head)
    t1 = time.perf_counter()
    fit_ref.residue_table(head, base)
    t2 = time.perf_counter()
    out = {"L": L, "kind": kind, "bytes": n * L, "lines": n, "rounds": rounds}
    for name, v in ms.items():
        med = statistics.median(v)
        out[name] = {"median_ms": round(med, 3), "min_ms": round(min(v), 3), "GB_s": round(n * L / med / 1e6, 1), "Mlines_s": round(n / med / 1e3, 1)}
    out["pairs"]["Gpairs_s"] = round(n * L * L / out["pairs"]["median_ms"] / 1e6, 1)
    out["numpy"] = {"pairs_lines_s": round(4096 / (t1 - t0), 1), "residues_lines_s": round(4096 / (t2 - t1), 1)}
    pairs.close()
    res.close()
    del buf
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    res = []
    for L in (32, 64, 128):
        for kind in ("random_u32", "records16"):
            res.append(case(L, kind, a.gib, a.rounds))
            print(json.dumps(res[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
