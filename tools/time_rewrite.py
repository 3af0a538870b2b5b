#!/usr/bin/env python3
"""What rewrite accounting costs on the MI355X (tests/test_rewrite_gpu.py checks the numbers; this measures the time).

A device-resident trace of --gib GiB (mpc_synth_fill "mixed") at 32-, 64- and 128-byte lines, evaluated through
mpc_compress_batch_device without a sizes array of the caller's:

  BDI      one handle with accounting off; one each with image accounting on (blocks of 4 lines, 32-byte sectors) and one
           each with rewrite accounting on (32-byte granules), for three address patterns
  group    BDI+FPC+BPC (one shared kernel) the same way; every member keeps its own image or map

The address patterns: "seq" every line at its own address p L (all distinct: every line is a run of one and claims a
slot), "rand" uniform random over 2^20 lines (every sub-batch rewrites the same keys), "one" one address for all lines (a
sub-batch is one run of 4 Mi).  Image accounting's update on the same addresses is the yardstick, measured in the same
run; the plain evaluator pass is "off".  A handle with an accounting on is reset before every pass (outside the timed
span), so that every pass builds its map from empty.  Same process, the variants alternating, --rounds rounds after a
warm-up pass of each; HIP events on the launching stream around each call.  Per line size: the median of each, its
round-to-round spread (max - min), on / off for each, rewrite / image for each pattern, and the wall time of one
rewrite_stats() on the BDI handle of each pattern.  --off-only skips everything that needs the accounting entry points,
so that this file, copied into the tools/ of a checkout of an earlier commit, takes the same measurement there: the
"off" numbers of two builds are compared with their spreads.
    python tools/time_rewrite.py [--gib G] [--rounds N] [--off-only] [--out FILE]"""
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
        if mode.startswith("image_"):
            ev.enable_image_stats(4, 32, 0, capacity[mode[6:]])
        elif mode.startswith("rewrite_"):
            ev.enable_rewrite_stats(32, capacity[mode[8:]])

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

    modes = ["off"] if off_only else ["off"] + [f"{a}_{p}" for p in PATTERNS for a in ("image", "rewrite")]
    bdi = {m: make_bdi(m) for m in modes}
    groups = {m: make_group(m) for m in modes}

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        fn()
        b.record(st)
        return a, b

    def feed(ev, m):
        if m == "off":
            ev.compress_device(buf.data_ptr(), n, stream=st.cuda_stream)
        else:
            ev.compress_device(buf.data_ptr(), n, stream=st.cuda_stream, addresses=addresses[m.split("_")[1]].data_ptr())

    def one_pass():
        rec = {}
        for m in modes:
            if m != "off":                         # the map from empty, every pass (reset waits for the device)
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
        if not off_only:
            for p in PATTERNS:
                out[f"{who}_rewrite_over_image_{p}"] = round(out[f"{who}_rewrite_{p}_ms"] / out[f"{who}_image_{p}_ms"], 4)
    # accounting changed nothing the handles compute, and the map is that of one pass
    for p in () if off_only else PATTERNS:
        m = "rewrite_" + p
        t0 = time.perf_counter()
        view = bdi[m].rewrite_stats()
        out[f"bdi_{m}_get_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
        assert view["lines"] == n and view["distinct_lines"] == (n if p == "seq" else 1 if p == "one" else view["distinct_lines"])
        assert view["distinct_lines"] <= capacity[p] and view["bits"] == int(bdi[m].stats_vector()[2])
        assert view["rewrites"] == n - view["distinct_lines"] and view["distinct_lines"] == bdi["image_" + p].image_stats()["distinct_lines"]
        out[f"bdi_{m}_distinct"] = view["distinct_lines"]
        out[f"bdi_{m}_overflow_rate"] = round(view["overflow_rate"], 4)
        out[f"bdi_{m}_peak_granule_ratio"] = round(view["peak_granule_ratio"], 4)
        for i in range(len(BASELINES)):
            assert int(groups[m][0].rewrite_table(i)[0]) == n
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
