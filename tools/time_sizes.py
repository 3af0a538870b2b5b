#!/usr/bin/env python3
"""What size accounting costs on the MI355X (tests/test_size_hist_gpu.py checks the numbers; this measures the time).

A device-resident trace of --gib GiB (mpc_synth_fill: random and all-zero lines of 64 and 32 bytes), evaluated through
mpc_compress_batch_device without a sizes array of the caller's:

  BDI      one handle with accounting off against one with its size histogram on (evaluated in pieces of 4 Mi lines,
           each followed by the accounting pass)
  group    BDI+FPC+BPC (one shared kernel) with accounting off against the same group with the three histograms and the
           best-of on (one accounting pass over three arrays per piece)

Same process, alternating off / on, --rounds rounds after a warm-up pass of each; HIP events on the launching stream
around each call (the kernel time of a pass, as tools/time_group.py takes it).  Per trace: the mean of each, its
round-to-round spread (max - min), and on / off.  --off-only skips everything that needs the accounting entry points,
so that this file, copied into the tools/ of a checkout of an earlier commit, takes the same measurement there: the "off"
numbers of two builds are compared with their spreads.
    python tools/time_sizes.py [--gib G] [--rounds N] [--off-only] [--out FILE]"""
import argparse
import importlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

mpc = importlib.import_module("cal_22-mpc_amd")
BASELINES = ("BDI", "FPC", "BPC")


def measure(L, kind, gib, rounds, off_only):
    n = (gib << 30) // L
    buf = torch.empty(n * L, dtype=torch.uint8, device="cuda:0")
    mpc.synth_fill(buf.data_ptr(), n, L, kind)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()

    def make_group(on):
        members = [getattr(mpc, c)(L, device=0) for c in BASELINES]
        group = mpc.EvaluatorSet(members)
        assert group.form == "BDI+FPC+BPC: one kernel", group.form
        if on:
            for ev in members:
                ev.enable_size_histogram()
            group.enable_best()
        return group, members

    bdi = {"off": mpc.BDI(L, device=0)}
    groups = {"off": make_group(False)}
    if not off_only:
        bdi["on"] = mpc.BDI(L, device=0)
        bdi["on"].enable_size_histogram()
        groups["on"] = make_group(True)
    modes = list(bdi)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        fn()
        b.record(st)
        return a, b

    def one_pass():
        rec = {}
        for m in modes:
            rec["bdi_" + m] = timed(lambda ev=bdi[m]: ev.compress_device(buf.data_ptr(), n, stream=st.cuda_stream))
            rec["group_" + m] = timed(lambda g=groups[m][0]: g.compress_device(buf.data_ptr(), n, stream=st.cuda_stream))
        return rec

    one_pass()                                     # warm-up: code objects loaded, scratch arrays allocated, clocks up
    torch.cuda.synchronize()
    recs = [one_pass() for _ in range(rounds)]
    torch.cuda.synchronize()
    mean = lambda v: sum(v) / len(v)
    out = {"L": L, "kind": kind, "bytes": n * L, "lines": n, "rounds": rounds}
    for key in recs[0]:
        ms = [r[key][0].elapsed_time(r[key][1]) for r in recs]
        out[key + "_ms"] = round(mean(ms), 4)
        out[key + "_spread_ms"] = round(max(ms) - min(ms), 4)
        out[key + "_TB_s"] = round(n * L / mean(ms) / 1e9, 3)
    if not off_only:
        out["bdi_on_over_off"] = round(out["bdi_on_ms"] / out["bdi_off_ms"], 4)
        out["group_on_over_off"] = round(out["group_on_ms"] / out["group_off_ms"], 4)
        # accounting changed nothing the handles compute, and it counted every line of every pass
        assert (bdi["on"].stats_vector() == bdi["off"].stats_vector()).all()
        assert int(bdi["on"].size_histogram().sum()) == (rounds + 1) * n
        for a, b in zip(groups["on"][1], groups["off"][1]):
            assert (a.stats_vector() == b.stats_vector()).all()
        best = groups["on"][0].best()
        assert best["lines"] == (rounds + 1) * n and int(best["wins"].sum()) == best["lines"]
    for group, members in groups.values():
        group.close()
        for ev in members:
            ev.close()
    for ev in bdi.values():
        ev.close()
    del buf
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--off-only", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    res = []
    for L in (64, 32):
        for kind in ("random_u32", "zeros"):
            res.append(measure(L, kind, a.gib, a.rounds, a.off_only))
            print(json.dumps(res[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
