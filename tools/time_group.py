#!/usr/bin/env python3
"""Group timings on the MI355X (tests/test_group_gpu.py checks the numbers a group computes; this measures what it costs).

  device   a device-resident trace of --gib GiB (mpc_synth_fill: random, sine, mixed at 64 B, pointers at 128 B):
           the ONE launch of a BDI+FPC+BPC group (baselines_kernel) against the three launches of solo BDI, FPC and BPC
           handles (mpc_compress_batch_device, the code path a handle always had), same process, alternating, --rounds
           rounds after a warm-up pass of each; HIP events on the launching stream around each launch.  Per trace: the
           mean of each, their round-to-round spread (max - min), the ratio, the stream alone (mpc_read_bandwidth_probe)
           and the group's share of 8 TB/s counted on the trace read once.
  files    a .npy of --file-gib GiB in the page cache and a .log of --log-gib GiB of the same lines: one group pass over
           VPC + BDI + FPC + BPC against the four solo passes one after the other; wall clock around calls that end
           synchronised; GB/s of line data.

Counters of the shared kernel come from a `rocprofv3 --pmc` run of `--only device --rounds 1` on its own.
    python tools/time_group.py [--only device|files] [--gib G] [--rounds N] [--file-gib G] [--log-gib G] [--out FILE]"""
import argparse
import importlib
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

mpc = importlib.import_module("cal_22-mpc_amd")
cfgs = importlib.import_module("cal_22-mpc_amd.configs")
traces = importlib.import_module("cal_22-mpc_amd.traces")
PEAK = 8.0e12
BASELINES = ("BDI", "FPC", "BPC")


def device(L, kind, gib, rounds):
    n = (gib << 30) // L
    buf = torch.empty(n * L, dtype=torch.uint8, device="cuda:0")
    mpc.synth_fill(buf.data_ptr(), n, L, kind)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    solo = [getattr(mpc, c)(L, device=0) for c in BASELINES]
    members = [getattr(mpc, c)(L, device=0) for c in BASELINES]
    group = mpc.EvaluatorSet(members)
    assert group.form == "BDI+FPC+BPC: one kernel", group.form

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        fn()
        b.record(st)
        return a, b

    def solo_pass():
        return [timed(lambda ev=ev: ev.compress_device(buf.data_ptr(), n, stream=st.cuda_stream)) for ev in solo]

    def group_pass():
        return timed(lambda: group.compress_device(buf.data_ptr(), n, stream=st.cuda_stream))

    solo_pass(), group_pass()                      # warm-up: code objects loaded, clocks up
    torch.cuda.synchronize()
    probe = timed(lambda: mpc.read_bandwidth_probe(buf.data_ptr(), n * L, stream=st.cuda_stream))
    probe = timed(lambda: mpc.read_bandwidth_probe(buf.data_ptr(), n * L, stream=st.cuda_stream))
    rec = [(solo_pass(), group_pass()) for _ in range(rounds)]
    torch.cuda.synchronize()
    solo_ms = [[a.elapsed_time(b) for a, b in s] for s, _ in rec]
    group_ms = [g[0].elapsed_time(g[1]) for _, g in rec]
    sums = [sum(r) for r in solo_ms]
    # the group computed what the solo handles computed (rounds + 1 passes each)
    for ev, m in zip(solo, members):
        assert (ev.stats_vector() == m.stats_vector()).all()
    mean = lambda v: sum(v) / len(v)
    out = {"what": "device", "L": L, "kind": kind, "bytes": n * L, "rounds": rounds,
           "solo_ms": {c: round(mean([r[i] for r in solo_ms]), 4) for i, c in enumerate(BASELINES)},
           "solo_sum_ms": round(mean(sums), 4), "solo_sum_spread_ms": round(max(sums) - min(sums), 4),
           "group_ms": round(mean(group_ms), 4), "group_spread_ms": round(max(group_ms) - min(group_ms), 4),
           "group_over_solo_sum": round(mean(group_ms) / mean(sums), 4),
           "stream_alone_ms": round(probe[0].elapsed_time(probe[1]), 4),
           "group_TB_s": round(n * L / mean(group_ms) / 1e9, 3), "group_frac_8TBs": round(n * L / mean(group_ms) / 1e9 / 8.0, 4),
           "group_rounds_ms": [round(x, 4) for x in group_ms], "solo_sum_rounds_ms": [round(x, 4) for x in sums]}
    group.close()
    for ev in solo + members:
        ev.close()
    del buf
    torch.cuda.empty_cache()
    return out


def files(file_gib, log_gib, rounds):
    L = 64
    n = int(file_gib * (1 << 30)) // L
    lines = np.random.default_rng(1).integers(0, 256, (n, L), dtype=np.uint8)
    d = tempfile.mkdtemp(dir="/tmp")
    npy = traces.save_npy(os.path.join(d, "t.npy"), lines)
    n_log = int(log_gib * (1 << 30)) // L
    log = traces.write_gpgpusim_log(os.path.join(d, "t.log"), lines[:n_log])
    del lines

    def make():
        return [mpc.VPC(cfgs.probe_config(L)), mpc.BDI(L), mpc.FPC(L), mpc.BPC(L)]

    solo, members = make(), make()
    group = mpc.EvaluatorSet(members)
    res = []
    for what, path, data_bytes in ((".npy", npy, (n - 1) * L), (".log", log, n_log * L)):
        feed_one = (lambda ev: ev.compress_npy(path)) if what == ".npy" else (lambda ev: ev.compress_gpgpusim_log(path))
        t_solo, t_group = [], []
        for r in range(rounds + 1):                # round 0: warm-up (pinned slots allocated, page cache filled)
            t0 = time.perf_counter()
            for ev in solo:
                feed_one(ev)
                ev.sync()
            t1 = time.perf_counter()
            feed_one(group)
            group.sync()
            t2 = time.perf_counter()
            if r:
                t_solo.append(t1 - t0)
                t_group.append(t2 - t1)
        for ev, m in zip(solo, members):
            assert (ev.stats_vector() == m.stats_vector()).all()
        ms, mg = sum(t_solo) / rounds, sum(t_group) / rounds
        res.append({"what": "file " + what, "form": group.form, "line_bytes": data_bytes, "rounds": rounds,
                    "four_solo_passes_s": round(ms, 4), "group_pass_s": round(mg, 4), "group_over_four_solo": round(mg / ms, 4),
                    "solo_GB_s_per_pass": round(4 * data_bytes / ms / 1e9, 2), "group_GB_s": round(data_bytes / mg / 1e9, 2),
                    "solo_rounds_s": [round(x, 4) for x in t_solo], "group_rounds_s": [round(x, 4) for x in t_group]})
    group.close()
    for ev in solo + members:
        ev.close()
    os.remove(npy)
    os.remove(log)
    os.rmdir(d)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=("device", "files"), default="")
    ap.add_argument("--gib", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--file-gib", type=float, default=4.0)
    ap.add_argument("--log-gib", type=float, default=4.0)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    res = []
    if a.only != "files":
        for L, kind in ((64, "random_u32"), (64, "sine_f32"), (64, "mixed"), (128, "pointers_u64")):
            res.append(device(L, kind, a.gib, a.rounds))
            print(json.dumps(res[-1]), flush=True)
    if a.only != "device":
        for r in files(a.file_gib, a.log_gib, min(a.rounds, 3)):
            res.append(r)
            print(json.dumps(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
