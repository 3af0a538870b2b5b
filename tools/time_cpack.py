#!/usr/bin/env python3
"""C-Pack (per-line dictionary) timings on the MI355X (tests/test_cpack_gpu.py checks the numbers; this measures what they
cost).  Device-resident traces of --gib GiB from mpc_synth_fill, torch's allocator for the buffers, one process:

  solo     C-Pack at 64 B on random, sine, mixed and all-zero, at 128 B on pointers, at 32 B on random; on the same
           buffer the solo FPC and BPC kernels as the yardstick and the stream alone (mpc_read_bandwidth_probe).  The
           evaluators take turns, --rounds rounds after a warm-up pass of each; HIP events on the launching stream around
           each launch.  Per trace: median and minimum ms per pass, and the fraction of 8 TB/s counted on the trace read once.
  group    at 64 B on random and mixed: a [BDI, FPC, BPC] group against a [BDI, FPC, BPC, CPACK] group, alternating.

Counters come from a `rocprofv3 --pmc` run of `--only solo --rounds 1` on its own.
    python tools/time_cpack.py [--only solo|group] [--gib G] [--rounds N] [--out FILE]"""
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
SOLO = ((64, "random_u32"), (64, "sine_f32"), (64, "mixed"), (64, "zeros"), (128, "pointers_u64"), (32, "random_u32"))
GROUP = ((64, "random_u32"), (64, "mixed"))


def _trace(L, kind, gib):
    n = (gib << 30) // L
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


def _row(ms, nbytes):
    med = statistics.median(ms)
    return {"median_ms": round(med, 4), "min_ms": round(min(ms), 4), "TB_s": round(nbytes / med / 1e9, 3),
            "frac_8TBs": round(nbytes / med / 1e9 / (PEAK / 1e12), 4)}


def solo(L, kind, gib, rounds):
    buf, n = _trace(L, kind, gib)
    st = torch.cuda.Stream()
    evs = {"CPACK": mpc.CPACK(L, device=0), "FPC": mpc.FPC(L, device=0), "BPC": mpc.BPC(L, device=0)}
    passes = {name: (lambda ev=ev: ev.compress_device(buf.data_ptr(), n, stream=st.cuda_stream)) for name, ev in evs.items()}
    passes["stream alone"] = lambda: mpc.read_bandwidth_probe(buf.data_ptr(), n * L, stream=st.cuda_stream)
    ms = _rounds(passes, st, rounds)
    r = evs["CPACK"].result()
    out = {"what": "solo", "L": L, "kind": kind, "bytes": n * L, "rounds": rounds, "cpack_ratio": round(r["comp_ratio"], 4),
           "cpack_counts_per_word": [round(c / max(1, r["total_words"]), 4) for c in r["counts"]],
           **{name: _row(v, n * L) for name, v in ms.items()}}
    for ev in evs.values():
        ev.close()
    del buf
    torch.cuda.empty_cache()
    return out


def group(L, kind, gib, rounds):
    buf, n = _trace(L, kind, gib)
    st = torch.cuda.Stream()
    three = [mpc.BDI(L, device=0), mpc.FPC(L, device=0), mpc.BPC(L, device=0)]
    four = [mpc.BDI(L, device=0), mpc.FPC(L, device=0), mpc.BPC(L, device=0), mpc.CPACK(L, device=0)]
    g3, g4 = mpc.EvaluatorSet(three), mpc.EvaluatorSet(four)
    assert g3.form == "BDI+FPC+BPC: one kernel" and g4.form == "BDI+FPC+BPC: one kernel; CPACK: own kernel", (g3.form, g4.form)
    ms = _rounds({"BDI+FPC+BPC": lambda: g3.compress_device(buf.data_ptr(), n, stream=st.cuda_stream),
                  "BDI+FPC+BPC+CPACK": lambda: g4.compress_device(buf.data_ptr(), n, stream=st.cuda_stream)}, st, rounds)
    for a, b in zip(three, four):                  # the fourth member changed nothing for the other three
        assert (a.stats_vector() == b.stats_vector()).all()
    out = {"what": "group", "L": L, "kind": kind, "bytes": n * L, "rounds": rounds, **{name: _row(v, n * L) for name, v in ms.items()}}
    g3.close()
    g4.close()
    for ev in three + four:
        ev.close()
    del buf
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=("solo", "group"), default="")
    ap.add_argument("--gib", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    res = []
    for what, cases, fn in (("solo", SOLO, solo), ("group", GROUP, group)):
        if a.only and a.only != what:
            continue
        for L, kind in cases:
            res.append(fn(L, kind, a.gib, a.rounds))
            print(json.dumps(res[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
