#!/usr/bin/env python3
"""What pack accounting costs on the MI355X (tests/test_pack_gpu.py checks the numbers; this measures the time).

A device-resident trace of --gib GiB (mpc_synth_fill "mixed") at 32-, 64- and 128-byte lines, evaluated through
mpc_compress_batch_device without a sizes array of the caller's:

  BDI      one handle with accounting off; one with its class table on (un-classed calls: class 0); one each with pack
           accounting on for blocks of 4, 64 and 1000 lines
  group    BDI+FPC+BPC (one shared kernel) the same way (no best-of, so that the numbers are the passes alone)

Class accounting is the comparison because both passes read the same 2-byte sizes over the same pieces: with either on
a batch is evaluated in pieces of 4 Mi lines, each followed by the accounting pass.  Blocks of 4 lines take the kernel's
lane form, of 64 the wave form, of 1000 the workgroup form.  Sectors of 32 bytes, or the smallest power of two above
that keeps a block within 1024 sectors.  Same process, the variants alternating, --rounds rounds after a warm-up pass of
each; HIP events on the launching stream around each call.  Per line size: the median of each, its round-to-round
spread (max - min), and on / off for each.  --off-only skips everything that needs the accounting entry points, so that
this file, copied into the tools/ of a checkout of an earlier commit, takes the same measurement there: the "off"
numbers of two builds are compared with their spreads.
    python tools/time_pack.py [--gib G] [--rounds N] [--off-only] [--out FILE]"""
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
CLASS_SECTOR = {32: 16, 64: 32, 128: 32}
BLOCKS = (4, 64, 1000)


def pack_sector(N, L):
    sb = 32
    while N * L > 1024 * sb:
        sb *= 2
    return sb


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
        if mode == "classes":
            group.enable_class_stats(CLASS_SECTOR[L])
        elif mode != "off":
            group.enable_pack_stats(mode, pack_sector(mode, L))
        return group, members

    def make_bdi(mode):
        ev = mpc.BDI(L, device=0)
        if mode == "classes":
            ev.enable_class_stats(CLASS_SECTOR[L])
        elif mode != "off":
            ev.enable_pack_stats(mode, pack_sector(mode, L))
        return ev

    modes = ["off"] if off_only else ["off", "classes", *BLOCKS]
    bdi = {m: make_bdi(m) for m in modes}
    groups = {m: make_group(m) for m in modes}

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        fn()
        b.record(st)
        return a, b

    def name(m):
        return m if isinstance(m, str) else f"pack{m}"

    def one_pass():
        rec = {}
        for m in modes:
            rec["bdi_" + name(m)] = timed(lambda ev=bdi[m]: ev.compress_device(buf.data_ptr(), n, stream=st.cuda_stream))
            rec["group_" + name(m)] = timed(lambda g=groups[m][0]: g.compress_device(buf.data_ptr(), n, stream=st.cuda_stream))
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
            out[f"{who}_{name(m)}_over_off"] = round(out[f"{who}_{name(m)}_ms"] / out[f"{who}_off_ms"], 4)
    # accounting changed nothing the handles compute, and it counted every line of every pass
    for N in modes[2:]:
        assert (bdi[N].stats_vector() == bdi["off"].stats_vector()).all()
        view = bdi[N].pack_stats()
        total = (rounds + 1) * n
        assert view["blocks"] == total // N and view["open_lines"] == total % N
        assert view["payload_bits"] + view["open_bits"] == int(bdi[N].stats_vector()[2])
        out[f"bdi_pack{N}_sector_ratio"] = round(view["sector_ratio"], 4)
        for i, (a, b) in enumerate(zip(groups[N][1], groups["off"][1])):
            assert (a.stats_vector() == b.stats_vector()).all()
            assert int(groups[N][0].pack_table(i)[0]) == total // N
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
