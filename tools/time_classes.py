#!/usr/bin/env python3
"""What per-class accounting costs on the MI355X (tests/test_classes_gpu.py checks the numbers; this measures the time).

A device-resident trace of --gib GiB (mpc_synth_fill "mixed") at 32-, 64- and 128-byte lines, evaluated through
mpc_compress_batch_device without a sizes array of the caller's:

  BDI      one handle with accounting off; one with its size histogram on; one with its class table on, fed three class
           arrays: all 0, runs of 2^20 lines, random bytes
  group    BDI+FPC+BPC (one shared kernel) the same way: off; the three histograms and the best-of; the three class
           tables (no best-of, so that the number is the class pass alone) with the three class arrays

With accounting on a batch is evaluated in pieces of 4 Mi lines, each followed by the accounting pass.  Same process, the
variants alternating, --rounds rounds after a warm-up pass of each; HIP events on the launching stream around each call.
Per line size: the median of each, its round-to-round spread (max - min), and on / off for the histogram and for each
class array.  --off-only skips everything that needs the accounting entry points, so that this file, copied into the
tools/ of a checkout of an earlier commit, takes the same measurement there: the "off" numbers of two builds are
compared with their spreads.
    python tools/time_classes.py [--gib G] [--rounds N] [--off-only] [--out FILE]"""
import argparse
import importlib
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

mpc = importlib.import_module("cal_22-mpc_amd")
BASELINES = ("BDI", "FPC", "BPC")
SECTOR = {32: 16, 64: 32, 128: 32}


def measure(L, gib, rounds, off_only):
    n = (gib << 30) // L
    buf = torch.empty(n * L, dtype=torch.uint8, device="cuda:0")
    mpc.synth_fill(buf.data_ptr(), n, L, "mixed")
    torch.cuda.synchronize()
    st = torch.cuda.Stream()

    def make_group(mode):
        members = [getattr(mpc, c)(L, device=0) for c in BASELINES]
        group = mpc.EvaluatorSet(members)
        assert group.form == "BDI+FPC+BPC: one kernel", group.form
        if mode == "hist":
            for ev in members:
                ev.enable_size_histogram()
            group.enable_best()
        if mode == "classes":
            group.enable_class_stats(SECTOR[L])
        return group, members

    bdi = {"off": mpc.BDI(L, device=0)}
    groups = {"off": make_group("off")}
    arrays = {}
    if not off_only:
        bdi["hist"] = mpc.BDI(L, device=0)
        bdi["hist"].enable_size_histogram()
        bdi["classes"] = mpc.BDI(L, device=0)
        bdi["classes"].enable_class_stats(SECTOR[L])
        groups["hist"] = make_group("hist")
        groups["classes"] = make_group("classes")
        idx = torch.arange(n, device="cuda:0", dtype=torch.int32)
        arrays = {"zero": torch.zeros(n, dtype=torch.uint8, device="cuda:0"),
                  "runs": ((idx >> 20) & 255).to(torch.uint8),
                  "random": torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda:0")}
        del idx

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        fn()
        b.record(st)
        return a, b

    def one_pass():
        rec = {}
        for m in ("off", "hist"):
            if m in bdi:
                rec["bdi_" + m] = timed(lambda ev=bdi[m]: ev.compress_device(buf.data_ptr(), n, stream=st.cuda_stream))
                rec["group_" + m] = timed(lambda g=groups[m][0]: g.compress_device(buf.data_ptr(), n, stream=st.cuda_stream))
        for name, arr in arrays.items():
            rec["bdi_classes_" + name] = timed(lambda: bdi["classes"].compress_device(buf.data_ptr(), n, stream=st.cuda_stream, classes=arr.data_ptr()))
            rec["group_classes_" + name] = timed(lambda: groups["classes"][0].compress_device(buf.data_ptr(), n, stream=st.cuda_stream, classes=arr.data_ptr()))
        return rec

    one_pass()                                     # warm-up: code objects loaded, scratch arrays allocated, clocks up
    torch.cuda.synchronize()
    recs = [one_pass() for _ in range(rounds)]
    torch.cuda.synchronize()
    out = {"L": L, "kind": "mixed", "bytes": n * L, "lines": n, "rounds": rounds}
    for key in recs[0]:
        ms = [r[key][0].elapsed_time(r[key][1]) for r in recs]
        out[key + "_ms"] = round(statistics.median(ms), 4)
        out[key + "_spread_ms"] = round(max(ms) - min(ms), 4)
    if not off_only:
        for who in ("bdi", "group"):
            for key in ("hist", "classes_zero", "classes_runs", "classes_random"):
                out[f"{who}_{key}_over_off"] = round(out[f"{who}_{key}_ms"] / out[f"{who}_off_ms"], 4)
        # accounting changed nothing the handles compute, and it counted every line of every pass
        assert (bdi["classes"].stats_vector()[1:] == 3 * bdi["off"].stats_vector()[1:]).all()
        t = bdi["classes"].class_table()
        assert int(t[:, 0].sum()) == 3 * (rounds + 1) * n and int(t[:, 1].sum()) == int(bdi["classes"].stats_vector()[2])
        for i, (a, b) in enumerate(zip(groups["classes"][1], groups["off"][1])):
            assert (a.stats_vector()[1:] == 3 * b.stats_vector()[1:]).all()
            assert int(groups["classes"][0].class_table(i)[:, 0].sum()) == 3 * (rounds + 1) * n
    for group, members in groups.values():
        group.close()
        for ev in members:
            ev.close()
    for ev in bdi.values():
        ev.close()
    del buf, arrays
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--off-only", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    res = []
    for L in (32, 64, 128):
        res.append(measure(L, a.gib, a.rounds, a.off_only))
        print(json.dumps(res[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
