#!/usr/bin/env python3
"""Pattern analyser timings on the MI355X (device-resident traces of 64-byte lines, torch's allocator for the buffers).
For the record only: nothing here is a pass threshold.

Per trace -- zeros, sine, mixed, structured, random, pointers -- from the same box and run:

  read        the streaming-read probe over the buffer (the HBM read ceiling)
  bdi         bdi_kernel over the same buffer
  pattern     a Pattern handle's whole call, twice: `first` on a fresh handle (the new lines join the set), `again` over
              the same lines (every line is found).  Event times around the calls, so launch gaps are in.

The split into the analysis kernel and the three set passes comes from the kernel trace:

    python tools/time_pattern.py --kernels [--lines N]

runs this script as a child of `rocprofv3 --kernel-trace --stats` (one pass per trace, no repetitions) and prints, per
kernel name, calls and total time from its summary.
    python tools/time_pattern.py [--lines N] [--reps R] [--out FILE]"""
import argparse
import csv
import glob
import importlib
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
L = 64
KINDS = ("zeros", "sine_f32", "mixed", "structured", "random_u32", "pointers_u64")


def trace(mpc, torch, kind, n):
    buf = torch.empty(n * L, dtype=torch.uint8, device="cuda:0")
    if kind == "structured":        # generated on the host (cal_22-mpc_amd/traces.py), 2^20 lines at a time with its own seed
        traces = importlib.import_module("cal_22-mpc_amd.traces")
        step = 1 << 20
        for at in range(0, n, step):
            part = traces.structured(min(step, n - at), L, seed=4242 + at)
            buf[at * L:(at + len(part)) * L] = torch.from_numpy(part.reshape(-1)).to("cuda:0")
    else:
        mpc.synth_fill(buf.data_ptr(), n, L, kind)
    torch.cuda.synchronize()
    return buf


def timed(torch, st, fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(st)
    for _ in range(reps):
        fn()
    b.record(st)
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def run(lines, reps, kinds):
    import torch
    mpc = importlib.import_module("cal_22-mpc_amd")
    st = torch.cuda.Stream()
    res = []
    for kind in kinds:
        buf = trace(mpc, torch, kind, lines)
        nbytes = lines * L
        mpc.read_bandwidth_probe(buf.data_ptr(), nbytes, st.cuda_stream)
        torch.cuda.synchronize()
        read_ms = timed(torch, st, lambda: mpc.read_bandwidth_probe(buf.data_ptr(), nbytes, st.cuda_stream), max(1, reps))
        bdi = mpc.BDI(L, device=0)
        bdi.compress_device(buf.data_ptr(), lines, stream=st.cuda_stream)
        torch.cuda.synchronize()
        bdi_ms = timed(torch, st, lambda: bdi.compress_device(buf.data_ptr(), lines, stream=st.cuda_stream), max(1, reps))
        bdi.close()
        pat = mpc.Pattern(L, device=0)
        first_ms = timed(torch, st, lambda: pat.compress_device(buf.data_ptr(), lines, stream=st.cuda_stream), 1)
        again_ms = timed(torch, st, lambda: pat.compress_device(buf.data_ptr(), lines, stream=st.cuda_stream), max(1, reps)) if reps else None
        pat.sync()
        r = pat.result()
        out = {"kind": kind, "L": L, "lines": lines, "bytes": nbytes, "read_ms": round(read_ms, 4), "bdi_ms": round(bdi_ms, 4),
               "pattern_first_ms": round(first_ms, 4), "pattern_again_ms": round(again_ms, 4) if again_ms is not None else None,
               "distinct_lines": pat.distinct_lines(), "entropy": r["entropy"], "entropy_except": r["entropy_except"],
               "Z": r["Z"], "R": r["R"], "U": r["U"]}
        pat.close()
        del buf
        torch.cuda.empty_cache()
        res.append(out)
        print(json.dumps(out), flush=True)
    return res


def kernels(lines):
    """One pass per trace under the kernel trace; the summary's rows for this project's kernels."""
    tool = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    tmp = tempfile.mkdtemp(prefix="time_pattern_")
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
                        if any(k in row["Name"] for k in ("pattern_", "bdi_kernel", "read_probe")):
                            rows.append({"kernel": row["Name"].split("(")[0], "calls": int(row["Calls"]),
                                         "total_ms": round(int(row["TotalDurationNs"]) / 1e6, 4)})
            print(json.dumps({"kind": kind, "lines": lines, "kernels": rows}), flush=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=1 << 23)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--child", default="")
    a = ap.parse_args()
    if a.lines > (1 << 23):
        sys.exit("at most 2^23 lines")
    if a.kernels:
        sys.exit(kernels(a.lines))
    res = run(a.lines, 0 if a.child else a.reps, (a.child,) if a.child else KINDS)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
