#!/usr/bin/env python3
"""SC2 timings on the MI355X (device-resident traces, torch's allocator for the buffers):

  sizing    the table-sizing kernel over a 16 GiB trace of synthetic kind 1-4 (mpc_synth_fill) at 64 and 128 B,
            the table built from that trace's first 10^6 lines; event time per pass, fraction of 8 TB/s
  warm-up   S = 10^6 lines of 64 B, all-zero and random: the counting kernel, then the table build (device
            selection + host heap + upload), host clock around synchronised calls

Kernel times for the report come from a separate `rocprofv3 --kernel-trace --stats` run of this script
(`--reps 1`); this script's own numbers include launch gaps.
    python tools/time_sc2.py [--reps N] [--gib G]"""
import argparse
import importlib
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

mpc = importlib.import_module("cal_22-mpc_amd")
PEAK = 8.0e12
S = 1_000_000


def sizing(L, kind, gib, reps):
    n = (gib << 30) // L
    buf = torch.empty(n * L, dtype=torch.uint8, device="cuda:0")
    mpc.synth_fill(buf.data_ptr(), n, L, kind)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    ev = mpc.SC2(L, S, device=0)
    ev.compress_device(buf.data_ptr(), S + 1, stream=st.cuda_stream)      # warm-up lines + the build at line S
    ev.sync()
    ev.compress_device(buf.data_ptr(), n, stream=st.cuda_stream)          # first full pass (not timed)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(st)
    for _ in range(reps):
        ev.compress_device(buf.data_ptr(), n, stream=st.cuda_stream)
    b.record(st)
    torch.cuda.synchronize()
    ms = a.elapsed_time(b) / reps
    r = ev.result()
    out = {"what": "sizing", "L": L, "kind": kind, "bytes": n * L, "ms": round(ms, 4),
           "TB_s": round(n * L / ms / 1e9, 3), "frac_8TBs": round(n * L / ms / 1e9 / 8.0, 4),
           "table_symbols": r["table_symbols"], "hit_rate": round(r["words_in_table"] / max(1, (r["lines"] - S) * L // 4), 4)}
    ev.close()
    del buf
    torch.cuda.empty_cache()
    return out


def warmup(kind):
    L = 64
    buf = torch.empty((S + 1) * L, dtype=torch.uint8, device="cuda:0")
    mpc.synth_fill(buf.data_ptr(), S + 1, L, kind)
    torch.cuda.synchronize()
    ev = mpc.SC2(L, S, device=0)
    st = torch.cuda.Stream()
    t0 = time.perf_counter()
    ev.compress_device(buf.data_ptr(), S, stream=st.cuda_stream)
    st.synchronize()
    t1 = time.perf_counter()
    ev.compress_device(buf.data_ptr() + S * L, 1, stream=st.cuda_stream)   # line S: select, build, upload, size it
    st.synchronize()
    t2 = time.perf_counter()
    out = {"what": "warmup", "L": L, "kind": kind, "S": S, "count_ms": round((t1 - t0) * 1e3, 3),
           "build_ms": round((t2 - t1) * 1e3, 3), "table_symbols": ev.result()["table_symbols"]}
    ev.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--gib", type=int, default=16)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    res = []
    for kind in ("zeros", "random_u32"):
        res.append(warmup(kind))
        print(json.dumps(res[-1]), flush=True)
    for L in (64, 128):
        for kind in ("random_u32", "sine_f32", "mixed", "pointers_u64"):
            res.append(sizing(L, kind, a.gib, a.reps))
            print(json.dumps(res[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
