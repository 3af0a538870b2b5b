#!/usr/bin/env python3
"""C-Pack with a dictionary per block of N lines: timings on the MI355X (tests/test_cpack_blocks_gpu.py checks the numbers;
this measures what they cost).  Device-resident traces of --gib GiB from mpc_synth_fill, torch's allocator for the
buffers, one process.  Per trace (random, mixed and all-zero at 64 B, random at 32 B, pointers at 128 B) the evaluators
take turns on one buffer: the per-line cpack_kernel of the same build, cpack_block_kernel at N = 2, 4, 64 and 4096 (one
lane per block), and the stream alone (mpc_read_bandwidth_probe); --rounds rounds after a warm-up pass of each, HIP
events on the launching stream around each launch.  Per evaluator: median and minimum ms per pass, TB/s counted on the
trace read once, and the time relative to the per-line kernel.  A block handle that ends a pass inside a block is
restarted before the next, so every pass evaluates the same blocks.

Counters (fetched bytes per algorithmic byte) come from a `rocprofv3 --pmc` run of `--rounds 1` on its own.
    python tools/time_cpack_blocks.py [--gib G] [--rounds N] [--blocks 2,4,64,4096] [--out FILE]"""
import argparse
import importlib
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

mpc = importlib.import_module("cal_22-mpc_amd")
PEAK = 8.0e12
CASES = ((64, "random_u32"), (64, "mixed"), (64, "zeros"), (32, "random_u32"), (128, "pointers_u64"))


def _trace(L, kind, gib):
    n = int(gib * (1 << 30)) // L
    buf = torch.empty(n * L, dtype=torch.uint8, device="cuda:0")
    mpc.synth_fill(buf.data_ptr(), n, L, kind)
    torch.cuda.synchronize()
    return buf, n


def _rounds(passes, st, rounds):
    """passes: {name: callable that enqueues one pass on st}; -> {name: [ms per round]}, the passes taking turns."""
    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        fn()
        b.record(st)
        return a, b

    for fn in passes.values():                     # warm-up: code objects loaded, clocks up
        fn()
    torch.cuda.synchronize()
    rec = [{name: timed(fn) for name, fn in passes.items()} for _ in range(rounds)]
    torch.cuda.synchronize()
    return {name: [r[name][0].elapsed_time(r[name][1]) for r in rec] for name in passes}


def _row(ms, nbytes, base=None):
    med = statistics.median(ms)
    row = {"median_ms": round(med, 4), "min_ms": round(min(ms), 4), "TB_s": round(nbytes / med / 1e9, 3),
           "frac_8TBs": round(nbytes / med / 1e9 / (PEAK / 1e12), 4)}
    if base:
        row["x_per_line"] = round(med / base, 2)
    return row


def case(L, kind, gib, rounds, blocks):
    buf, n = _trace(L, kind, gib)
    st = torch.cuda.Stream()
    per_line = mpc.CPACK(L, device=0)
    evs = {f"N={N}": mpc.CPACK(L, dictionary="block", block_lines=N, device=0) for N in blocks}

    def block_pass(ev):
        ev.restart()
        ev.compress_device(buf.data_ptr(), n, stream=st.cuda_stream)

    passes = {"per line": lambda: per_line.compress_device(buf.data_ptr(), n, stream=st.cuda_stream)}
    passes.update({name: (lambda ev=ev: block_pass(ev)) for name, ev in evs.items()})
    passes["stream alone"] = lambda: mpc.read_bandwidth_probe(buf.data_ptr(), n * L, stream=st.cuda_stream)
    ms = _rounds(passes, st, rounds)
    base = statistics.median(ms["per line"])
    out = {"what": "cpack blocks", "L": L, "kind": kind, "bytes": n * L, "lines": n, "rounds": rounds,
           "ratio": {"per line": round(per_line.result()["comp_ratio"], 4), **{name: round(ev.result()["comp_ratio"], 4) for name, ev in evs.items()}},
           **{name: _row(v, n * L, None if name == "per line" else base) for name, v in ms.items()}}
    for ev in [per_line, *evs.values()]:
        ev.close()
    del buf
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=4.0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--blocks", default="2,4,64,4096")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    blocks = [int(x) for x in a.blocks.split(",")]
    res = []
    for L, kind in CASES:
        res.append(case(L, kind, a.gib, a.rounds, blocks))
        print(json.dumps(res[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
