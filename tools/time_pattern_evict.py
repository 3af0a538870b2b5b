#!/usr/bin/env python3
"""What the evicting mode of the Pattern analyser costs on the MI355X (device-resident traces of 64-byte lines, torch's
allocator for the buffers).  For the record only: nothing here is a pass threshold.

Below the capacity, per trace -- zeros, sine, mixed, structured, random, pointers -- of at most 2^23 lines: the default
handle (Pattern(L)) and the evicting handle (Pattern(L, on_full="evict")) take turns on the same buffer.  A round creates
both afresh, times each one's `first` pass (the new lines join the set) and its `again` pass (every line is found) with
events around the calls, and closes them; the medians of 7 rounds after a warm-up round and their ratio are reported.

Above the capacity, with the evicting handle alone:
  random     2^28 distinct random lines (16 GiB): one pass
  cyclic     2^24 distinct lines, one more than the capacity, swept three times: after the first sweep every line comes
             back just after its eviction (the at-risk walk throughout)
each beside the streaming-read probe over the same buffer.

    python tools/time_pattern_evict.py [--lines N] [--rounds R] [--big-lines N] [--skip-big] [--out FILE]
    python tools/time_pattern_evict.py --kernels [--lines N]      per kernel name, calls and total time of one first and one
                                                                  again pass of the evicting handle (rocprofv3 --kernel-trace --stats)"""
import argparse
import csv
import glob
import importlib
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from time_pattern import KINDS, L, timed, trace  # noqa: E402

CAPACITY = (1 << 24) - 1


def below(mpc, torch, st, kinds, lines, rounds):
    res = []
    for kind in kinds:
        buf = trace(mpc, torch, kind, lines)
        t = {"default_first": [], "default_again": [], "evict_first": [], "evict_again": []}
        distinct = None
        for rnd in range(rounds + 1):                       # round 0 warms up
            for name, make in (("default", lambda: mpc.Pattern(L, device=0)), ("evict", lambda: mpc.Pattern(L, device=0, on_full="evict"))):
                ev = make()
                call = lambda: ev.compress_device(buf.data_ptr(), lines, stream=st.cuda_stream)      # noqa: E731
                first, again = timed(torch, st, call, 1), timed(torch, st, call, 1)
                ev.sync()
                distinct = ev.distinct_lines()
                ev.close()
                if rnd:
                    t[name + "_first"].append(first)
                    t[name + "_again"].append(again)
        med = {k: round(statistics.median(v), 4) for k, v in t.items()}
        out = {"kind": kind, "L": L, "lines": lines, "distinct_lines": distinct, "rounds": rounds, **{k + "_ms": v for k, v in med.items()},
               "ratio_first": round(med["evict_first"] / med["default_first"], 3), "ratio_again": round(med["evict_again"] / med["default_again"], 3)}
        res.append(out)
        print(json.dumps(out), flush=True)
        del buf
        torch.cuda.empty_cache()
    return res


def above(mpc, torch, st, big_lines):
    res = []
    for name, n, sweeps in (("random", big_lines, 1), ("cyclic", CAPACITY + 1, 3)):
        buf = torch.empty(n * L, dtype=torch.uint8, device="cuda:0")
        mpc.synth_fill(buf.data_ptr(), n, L, "random_u32")
        torch.cuda.synchronize()
        mpc.read_bandwidth_probe(buf.data_ptr(), n * L, st.cuda_stream)
        torch.cuda.synchronize()
        read_ms = timed(torch, st, lambda: mpc.read_bandwidth_probe(buf.data_ptr(), n * L, st.cuda_stream), 3)
        ev = mpc.Pattern(L, device=0, on_full="evict")
        passes = []
        for _ in range(sweeps):
            passes.append(round(timed(torch, st, lambda: ev.compress_device(buf.data_ptr(), n, stream=st.cuda_stream), 1), 3))
        ev.sync()
        v = ev.stats_vector()
        out = {"trace": name, "L": L, "lines_per_pass": n, "bytes": n * L, "read_ms": round(read_ms, 3), "pass_ms": passes,
               "lines": int(v[0]), "hits": int(v[6]) // L, "insertions": int(v[21])}
        ev.close()
        res.append(out)
        print(json.dumps(out), flush=True)
        del buf
        torch.cuda.empty_cache()
    return res


def kernels(lines):
    tool = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    tmp = tempfile.mkdtemp(prefix="time_pattern_evict_")
    try:
        for kind in KINDS:
            out = os.path.join(tmp, kind)
            # (the program goes after `--`: the traced process is a fresh child)
            r = subprocess.run([tool, "--kernel-trace", "--stats", "-d", out, "-o", "run", "--output-format", "csv", "--",
                                sys.executable, os.path.abspath(__file__), "--child", kind, "--lines", str(lines)],
                               capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                print(json.dumps({"kind": kind, "error": (r.stdout + r.stderr)[-800:]}), flush=True)
                return 1
            rows = []
            for path in glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True):
                with open(path) as f:
                    for row in csv.DictReader(f):
                        if any(k in row["Name"] for k in ("pattern_", "evict_")):
                            rows.append({"kernel": row["Name"].split("(")[0], "calls": int(row["Calls"]),
                                         "total_ms": round(int(row["TotalDurationNs"]) / 1e6, 4)})
            print(json.dumps({"kind": kind, "lines": lines, "kernels": rows}), flush=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return 0


def child(kind, lines):
    import torch
    mpc = importlib.import_module("cal_22-mpc_amd")
    buf = trace(mpc, torch, kind, lines)
    ev = mpc.Pattern(L, device=0, on_full="evict")
    for _ in range(2):
        ev.compress_device(buf.data_ptr(), lines)
    ev.sync()
    ev.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=1 << 23)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--big-lines", type=int, default=1 << 28)
    ap.add_argument("--skip-big", action="store_true")
    ap.add_argument("--out", default="")
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--child", default="")
    a = ap.parse_args()
    if a.lines > (1 << 23):
        sys.exit("at most 2^23 lines below the capacity")
    if a.kernels:
        sys.exit(kernels(a.lines))
    if a.child:
        return child(a.child, a.lines)
    import torch
    mpc = importlib.import_module("cal_22-mpc_amd")
    st = torch.cuda.Stream()
    res = {"below": below(mpc, torch, st, KINDS, a.lines, a.rounds)}
    if not a.skip_big:
        res["above"] = above(mpc, torch, st, a.big_lines)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
