#!/usr/bin/env python3
"""What image accounting costs on the MI355X (tests/test_image_gpu.py checks the numbers; this measures the time).

A device-resident trace of --gib GiB (mpc_synth_fill "mixed") at 32-, 64- and 128-byte lines, evaluated through
mpc_compress_batch_device without a sizes array of the caller's:

  BDI      one handle with accounting off; one with its class table on (un-classed calls: class 0); one each with image
           accounting on (blocks of 4 lines, 32-byte sectors) for three address patterns
  group    BDI+FPC+BPC (one shared kernel) the same way; every member keeps its own image

The address patterns: "seq" every line at its own address p L (all distinct: every line claims a slot), "rand" uniform
random over 2^20 lines (the table stays small, the atomics go to random slots), "one" one address for all lines (a run:
the lanes of a wave combine).  Class accounting is the yardstick the earlier passes used: with any accounting on a
batch is evaluated in pieces of 4 Mi lines, each followed by the accounting passes.  A handle with image accounting on
is reset before every pass (outside the timed span), so that every pass builds its image from empty.  Same process, the
variants alternating, --rounds rounds after a warm-up pass of each; HIP events on the launching stream around each
call.  Per line size: the median of each, its round-to-round spread (max - min), on / off for each, and the wall time
of one image_stats() on the BDI handle of each pattern.  --off-only skips everything that needs the accounting entry
points, so that this file, copied into the tools/ of a checkout of an earlier commit, takes the same measurement there:
the "off" numbers of two builds are compared with their spreads.
    python tools/time_image.py [--gib G] [--rounds N] [--off-only] [--out FILE]"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

mpc = importlib.import_module("cal_22-mpc_amd")
BASELINES = ("BDI", "FPC", "BPC")
CLASS_SECTOR = {32: 16, 64: 32, 128: 32}
PATTERNS = ("seq", "rand", "one")
RAND_LINES = 1 << 20


def measure(L, gib, rounds, off_only):
    n = (gib << 30) // L
    buf = torch.empty(n * L, dtype=torch.uint8, device="cuda:0")
    mpc.synth_fill(buf.data_ptr(), n, L, "mixed")
    addresses, capacity = {}, {"seq": n, "rand": RAND_LINES, "one": 1}
    if not off_only:
        addresses["seq"] = torch.arange(n, dtype=torch.int64, device="cuda:0") * L
        addresses["rand"] = torch.randint(0, RAND_LINES, (n,), dtype=torch.int64, device="cuda:0", generator=torch.Generator("cuda:0").manual_seed(1)) * L
        addresses["one"] = torch.full((n,), 4096 * L, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    st = torch.cuda.Stream()

    def switch_on(ev, mode):
        if mode == "classes":
            ev.enable_class_stats(CLASS_SECTOR[L])
        elif mode != "off":
            ev.enable_image_stats(4, 32, 0, capacity[mode])

    def make_group(mode):
        members = [getattr(mpc, c)(L, device=0) for c in BASELINES]
        group = mpc.EvaluatorSet(members)
        assert group.form == "BDI+FPC+BPC: one kernel", group.form
        switch_on(group, mode)
        return group, members

    def make_bdi(mode):
        ev = mpc.BDI(L, device=0)
        switch_on(ev, mode)
        return ev

    modes = ["off"] if off_only else ["off", "classes", *PATTERNS]
    bdi = {m: make_bdi(m) for m in modes}
    groups = {m: make_group(m) for m in modes}

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        fn()
        b.record(st)
        return a, b

    def feed(ev, m):
        if m in PATTERNS:
            ev.compress_device(buf.data_ptr(), n, stream=st.cuda_stream, addresses=addresses[m].data_ptr())
        else:
            ev.compress_device(buf.data_ptr(), n, stream=st.cuda_stream)

    def one_pass():
        rec = {}
        for m in modes:
            if m in PATTERNS:                      # the image from empty, every pass (reset waits for the device)
                bdi[m].reset()
                for ev in groups[m][1]:
                    ev.reset()
            rec["bdi_" + m] = timed(lambda m=m: feed(bdi[m], m))
            rec["group_" + m] = timed(lambda m=m: feed(groups[m][0], m))
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
    for who in ("bdi", "group"):
        for m in modes[1:]:
            out[f"{who}_{m}_over_off"] = round(out[f"{who}_{m}_ms"] / out[f"{who}_off_ms"], 4)
    # accounting changed nothing the handles compute, and the image is that of one pass
    for m in modes[2:]:
        t0 = time.perf_counter()
        view = bdi[m].image_stats()
        out[f"bdi_{m}_get_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
        assert view["lines"] == n and view["distinct_lines"] == (n if m == "seq" else 1 if m == "one" else view["distinct_lines"])
        assert view["distinct_lines"] <= capacity[m] and view["bits"] == int(bdi[m].stats_vector()[2])
        out[f"bdi_{m}_distinct"] = view["distinct_lines"]
        out[f"bdi_{m}_image_ratio"] = round(view["image_ratio"], 4)
        for i in range(len(BASELINES)):
            assert int(groups[m][0].image_table(i)[0]) == n
    for group, members in groups.values():
        group.close()
        for ev in members:
            ev.close()
    for ev in bdi.values():
        ev.close()
    del buf, addresses
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
