#!/usr/bin/env python3
"""Where a launch of the VPC lane kernel ends: per-CU finish spread, idle share and the gap between a CU's workgroups.

    python tools/wg_spread.py [workload] [L]          # default: random_u32 64; one 16 GiB launch after two warm-up launches

Needs a library whose lane kernels stamp the wall clock (100 MHz) at the entry of every workgroup and after its
statistics flush, with the hardware ids of the CU (csrc/mpc_device.h: MPC_STAMPS).  To TIME a launch that is a build of
the product's kernels plus the stamps,

    tools/ab.py build stamp=-DMPC_STAMPS=1  &&  MPC_HIP_LIB=tools/ablate/libmpc_hip_stamp.so python tools/wg_spread.py

The test library (the default when MPC_HIP_LIB is not set) has the stamps too, but its route counters -- one same-address
atomic per 128-line block -- make a 16 GiB launch nine times longer: its stamps show where a launch ends when the
workgroups queue for one address, not where the product's does.  A -DMPC_STAMPS=1 build stamps in the built-in kernels
only (the probe configuration this tool runs): a module sequence compiled at creation stamps in the test library alone.
All times below are relative to the first entry of the launch.

  finish(CU)  = the last exit stamp of the workgroups that ran on the CU
  idle share  = 1 - mean(finish) / max(finish): the part of the launch's CU-time after a CU has run out of work
  gap         = on a CU that ran several workgroups one after the other, exit of one to entry of the next
"""
import ctypes
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault("MPC_HIP_LIB", os.path.join(ROOT, "cal_22-mpc_amd", "libmpc_hip_test.so"))
sys.path.insert(0, ROOT)
import numpy as np
import torch

mpc = importlib.import_module("cal_22-mpc_amd")
cfgs = importlib.import_module("cal_22-mpc_amd.configs")

STAMP_WGS = 1024          # MPC_STAMP_WGS
TICK_US = 0.01            # wall_clock64(): 100 MHz


def stamps(ev):
    f = mpc.lib().mpc_test_stamps
    f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    f.restype = ctypes.c_int
    out = (ctypes.c_uint64 * (3 * STAMP_WGS))()
    assert f(ev._h, out, 3 * STAMP_WGS) == 0
    a = np.frombuffer(out, dtype=np.uint64).reshape(STAMP_WGS, 3).copy()
    return a[a[:, 1] != 0]          # the workgroups of the launch


def main():
    wl = sys.argv[1] if len(sys.argv) > 1 else "random_u32"
    L = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    n = (16 << 30) // L
    buf = torch.empty(n * L, dtype=torch.uint8, device="cuda:0")
    mpc.synth_fill(buf.data_ptr(), n, L, wl)
    torch.cuda.synchronize()
    ev = mpc.VPC(cfgs.probe_config(L))
    st = torch.cuda.Stream()
    for _ in range(2):
        ev.compress_device(buf.data_ptr(), n, stream=st.cuda_stream)
    torch.cuda.synchronize()
    ev.reset()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(st)
    ev.compress_device(buf.data_ptr(), n, stream=st.cuda_stream)
    b.record(st)
    torch.cuda.synchronize()
    s = stamps(ev)
    t0 = int(s[:, 0].min())
    entry = (s[:, 0].astype(np.int64) - t0) * TICK_US
    exit_ = (s[:, 1].astype(np.int64) - t0) * TICK_US
    cu = ((s[:, 2] >> np.uint64(32)) & np.uint64(0xf)) << np.uint64(8) | ((s[:, 2] >> np.uint64(8)) & np.uint64(0xff))     # XCC, then SE / SH / CU of HW_ID
    finish, gaps, per_cu = [], [], {}
    for c in np.unique(cu):
        idx = np.nonzero(cu == c)[0]
        idx = idx[np.argsort(entry[idx])]
        per_cu[int(c)] = len(idx)
        finish.append(exit_[idx].max())
        for i, j in zip(idx[:-1], idx[1:]):
            gaps.append(entry[j] - exit_[i])
    finish, gaps = np.array(finish), np.array(gaps)
    end = exit_.max()
    counts = np.bincount(list(per_cu.values()))
    print(f"{os.path.basename(mpc.LIB_PATH)} VPC L={L} {wl}: {n} lines, event time {a.elapsed_time(b) * 1e3:.0f} us")
    print(f"workgroups {len(s)}, CUs {len(finish)}, workgroups per CU: " + ", ".join(f"{k}: {v} CUs" for k, v in enumerate(counts) if v))
    print(f"first entry 0 us, last entry of a CU's first workgroup {np.sort(entry)[len(finish) - 1]:.1f} us, launch end {end:.1f} us")
    q = np.percentile(finish, [0, 5, 25, 50, 75, 95, 100])
    print("per-CU finish (us): min %.1f  p5 %.1f  p25 %.1f  median %.1f  p75 %.1f  p95 %.1f  max %.1f" % tuple(q))
    print(f"finish spread (max - min) {q[6] - q[0]:.1f} us = {100 * (q[6] - q[0]) / end:.2f} % of the launch")
    print(f"idle share 1 - mean(finish) / max(finish) = {100 * (1 - finish.mean() / finish.max()):.2f} %")
    if len(gaps):
        print(f"gap between a CU's workgroups (us): n {len(gaps)}  mean {gaps.mean():.2f}  median {np.median(gaps):.2f}  max {gaps.max():.2f}"
              f"  = {100 * gaps.mean() / end:.2f} % of the launch (mean)")
    else:
        print("gap between a CU's workgroups: none (one workgroup per CU)")
    dur = exit_ - entry
    print(f"workgroup duration (us): min {dur.min():.1f}  mean {dur.mean():.1f}  max {dur.max():.1f}")
    ev.close()


if __name__ == "__main__":
    main()
