#!/usr/bin/env python3
"""What a snapshot costs on the MI355X (tests/test_snapshot_gpu.py checks the bytes; this measures the time).

Per unit size U = 32, 64 and 128, on device-resident units (mpc_synth_fill "mixed"):

  add       add_device of --units units for three address patterns -- "seq" every unit at its own address p U (all
            distinct: every unit claims a slot and is copied), "rand" uniform over 2^20 units (the table stays small),
            "one" one address for all (the lanes of a wave combine, one unit per launch is copied) -- in units/s, the
            snapshot reset before every pass outside the timed span.  The yardstick, in the same run on the same
            addresses: a BDI handle's compress_device with image accounting on minus the same call with it off, the
            update pass of image accounting, in lines/s.
  plan      wall time of plan() (gather, sort, mark, scan; the sorted keys dropped before every pass) and of write_lines
            of all emitted lines, for D = 2^20 and 2^24 sequential units (--plan-log2, at most what fits) at L = U and 4 U.
  evaluate  evaluate() into BDI at L = 4 U (2 U at U = 128) next to a plain compress_device over the same lines
            materialised once with write_lines: what materialising through the scratch buffer adds.

Same process, the variants alternating, --rounds rounds after a warm-up pass of each; HIP events on the launching stream
around the asynchronous calls, wall time around the synchronising ones.  Per figure: the median and the round-to-round
spread (max - min).  Repeat the command to see the spread between runs.
    python tools/time_snapshot.py [--units N] [--rounds N] [--plan-log2 20,24] [--out FILE]"""
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
PATTERNS = ("seq", "rand", "one")
RAND_UNITS = 1 << 20


def med(xs):
    return round(statistics.median(xs), 4), round(max(xs) - min(xs), 4)


def event_ms(st, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(st)
    fn()
    b.record(st)
    return a, b


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def measure_add(U, n, rounds):
    buf = torch.empty(n * U, dtype=torch.uint8, device="cuda:0")
    mpc.synth_fill(buf.data_ptr(), n, U, "mixed")
    addresses = {"seq": torch.arange(n, dtype=torch.int64, device="cuda:0") * U,
                 "rand": torch.randint(0, RAND_UNITS, (n,), dtype=torch.int64, device="cuda:0", generator=torch.Generator("cuda:0").manual_seed(1)) * U,
                 "one": torch.full((n,), 4096 * U, dtype=torch.int64, device="cuda:0")}
    capacity = {"seq": n, "rand": RAND_UNITS, "one": 1}
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    snaps = {m: mpc.Snapshot(U, capacity[m], device=0) for m in PATTERNS}
    image = {}
    for m in PATTERNS:
        image[m] = mpc.BDI(U, device=0)
        image[m].enable_image_stats(4, 32, 0, capacity[m])
    off = mpc.BDI(U, device=0)
    off.enable_class_stats(16 if U == 32 else 32)           # the same pieces of 4 Mi lines over a sizes scratch, no image

    def one_pass():
        rec = {}
        for m in PATTERNS:
            snaps[m].reset()
            image[m].reset()
            rec["add_" + m] = event_ms(st, lambda m=m: snaps[m].add_device(buf.data_ptr(), n, addresses[m].data_ptr(), st.cuda_stream))
            rec["image_" + m] = event_ms(st, lambda m=m: image[m].compress_device(buf.data_ptr(), n, stream=st.cuda_stream, addresses=addresses[m].data_ptr()))
        rec["image_off"] = event_ms(st, lambda: off.compress_device(buf.data_ptr(), n, stream=st.cuda_stream))
        return rec

    one_pass()
    torch.cuda.synchronize()
    recs = [one_pass() for _ in range(rounds)]
    torch.cuda.synchronize()
    out = {"U": U, "units": n, "rounds": rounds}
    ms = {key: [r[key][0].elapsed_time(r[key][1]) for r in recs] for key in recs[0]}
    for m in PATTERNS:
        out[f"add_{m}_ms"], out[f"add_{m}_spread_ms"] = med(ms["add_" + m])
        out[f"add_{m}_gunits_s"] = round(n / out[f"add_{m}_ms"] / 1e6, 3)
        upd = [a - b for a, b in zip(ms["image_" + m], ms["image_off"])]
        out[f"image_update_{m}_ms"], out[f"image_update_{m}_spread_ms"] = med(upd)
        out[f"image_update_{m}_glines_s"] = round(n / max(out[f"image_update_{m}_ms"], 1e-6) / 1e6, 3)
        st_ = snaps[m].stats()
        assert st_["units"] == n and st_["distinct_units"] == (n if m == "seq" else 1 if m == "one" else st_["distinct_units"])
    for s in snaps.values():
        s.close()
    for ev in list(image.values()) + [off]:
        ev.close()
    return out


def measure_plan(U, log2s, rounds):
    out = {"U": U}
    for lg in log2s:
        D = 1 << lg
        try:
            snap = mpc.Snapshot(U, D, device=0)
            buf = torch.empty(D * U, dtype=torch.uint8, device="cuda:0")
        except (mpc.MpcError, RuntimeError) as e:
            out[f"D2^{lg}"] = f"skipped: {e}"
            continue
        mpc.synth_fill(buf.data_ptr(), D, U, "mixed")
        addrs = torch.arange(D, dtype=torch.int64, device="cuda:0") * U
        torch.cuda.synchronize()
        snap.add_device(buf.data_ptr(), D, addrs.data_ptr())
        for L in (U, min(4 * U, 256)):
            n_out = D // (L // U)
            dst = torch.empty(n_out * L, dtype=torch.uint8, device="cuda:0")
            plans, writes = [], []
            for r in range(rounds + 1):
                snap.add_device(buf.data_ptr(), 1, addrs.data_ptr())       # drops the sorted keys: the next plan starts over
                plans.append(wall_ms(lambda: snap.plan(L)))
                writes.append(wall_ms(lambda: snap.write_lines(L, "skip", 0, n_out, dst.data_ptr())))
            assert snap.plan(L)["n_out"] == n_out
            out[f"plan_D2^{lg}_L{L}_ms"], out[f"plan_D2^{lg}_L{L}_spread_ms"] = med(plans[1:])
            out[f"write_D2^{lg}_L{L}_ms"], out[f"write_D2^{lg}_L{L}_spread_ms"] = med(writes[1:])
            del dst
        snap.close()
        del buf, addrs
        torch.cuda.empty_cache()
    return out


def measure_evaluate(U, n, rounds):
    L = min(4 * U, 256)
    k = L // U
    n -= n % k
    snap = mpc.Snapshot(U, n, device=0)
    buf = torch.empty(n * U, dtype=torch.uint8, device="cuda:0")
    mpc.synth_fill(buf.data_ptr(), n // k, L, "mixed")
    addrs = torch.arange(n, dtype=torch.int64, device="cuda:0") * U
    torch.cuda.synchronize()
    snap.add_device(buf.data_ptr(), n, addrs.data_ptr())
    n_out = snap.plan(L)["n_out"]
    assert n_out == n // k
    lines = torch.empty(n_out * L, dtype=torch.uint8, device="cuda:0")
    snap.write_lines(L, "skip", 0, n_out, lines.data_ptr())
    torch.cuda.synchronize()
    assert bool((lines == buf).all())
    a, b = mpc.BDI(L, device=0), mpc.BDI(L, device=0)

    def plain():
        b.compress_device(lines.data_ptr(), n_out)
        b.sync()

    ev, pl = [], []
    for r in range(rounds + 1):
        ev.append(wall_ms(lambda: snap.evaluate(a, L)))
        pl.append(wall_ms(plain))
    assert (a.stats_vector() == b.stats_vector()).all()
    out = {"U": U, "L": L, "lines": n_out}
    out["evaluate_ms"], out["evaluate_spread_ms"] = med(ev[1:])
    out["plain_ms"], out["plain_spread_ms"] = med(pl[1:])
    out["materialising_adds_ms"] = round(out["evaluate_ms"] - out["plain_ms"], 4)
    for x in (a, b, snap):
        x.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--units", type=int, default=1 << 24)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--plan-log2", default="20,24")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    res = []
    for U in (32, 64, 128):
        for part in (measure_add(U, a.units, a.rounds), measure_plan(U, [int(x) for x in a.plan_log2.split(",") if x], a.rounds),
                     measure_evaluate(U, a.units, a.rounds)):
            res.append(part)
            print(json.dumps(part), flush=True)
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
