"""Fresh processes bound to libmpc_hip_test.so (cal_22-mpc_amd/build.py, -DMPC_TESTING=1), for the GPU tests that need what
only the test library has: the kernels' route counters, the cap on the launch grid (MPC_TEST_GRID), the lowered launch
cuts (MPC_TEST_LAUNCH_LINES) with their count of launches, and the lowered BDI deferral limit.  The library reads its environment variables once per
process, hence a process per test."""
import json
import os
import subprocess
import sys

ROUTE_NAMES = ["vpc_deferred", "vpc_drains", "vpc_paired_blocks", "vpc_plain_blocks", "vpc_to_paired", "vpc_to_plain",
               "vpc_tail_groups", "bdi_deferred", "bdi_drains"]        # MPC_RT_* of csrc/mpc_kernel_common.h

ROUTES_PRELUDE = r"""
import ctypes, importlib, json, sys
import numpy as np
sys.path.insert(0, %r)
mpc = importlib.import_module("cal_22-mpc_amd"); C = importlib.import_module("cal_22-mpc_amd.configs"); T = importlib.import_module("cal_22-mpc_amd.traces")
from oracle import oracle as O
assert mpc.LIB_PATH.endswith("libmpc_hip_test.so"), mpc.LIB_PATH
def routes(ev):
    # test library only: how often the kernels' alternative routes ran since the statistics were last reset
    f = mpc.lib().mpc_test_routes
    f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]; f.restype = ctypes.c_int
    out = (ctypes.c_uint64 * 16)()
    assert f(ev._h, out, 16) == 0
    return dict(zip(%r, [int(x) for x in out]))
def launches():
    # test library only: the launches that the launchers which cut a batch have made in this process, one per piece
    f = mpc.lib().mpc_test_launches
    f.argtypes = []; f.restype = ctypes.c_uint64
    return int(f())
"""


def _run_with_test_library(code: str, grid_cap: int, timeout: int = 900, env=None):
    """A fresh process bound to libmpc_hip_test.so (the product library has neither route counters nor the grid
    cap), MPC_TEST_GRID set (0: no cap) and whatever `env` adds; returns the JSON object the code printed behind
    'ROUTES '."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    test_lib = os.path.join(root, "cal_22-mpc_amd", "libmpc_hip_test.so")
    assert os.path.exists(test_lib), "libmpc_hip_test.so is missing: python cal_22-mpc_amd/build.py"
    env = dict(os.environ, MPC_TEST_GRID=str(grid_cap), MPC_HIP_LIB=test_lib, **(env or {}))
    r = subprocess.run([sys.executable, "-c", (ROUTES_PRELUDE % (root, ROUTE_NAMES)) + code], capture_output=True, text=True,
                       timeout=timeout, env=env, cwd=root)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    line = [l for l in r.stdout.split("\n") if l.startswith("ROUTES ")]
    assert line, r.stdout[-2000:]
    return json.loads(line[-1][7:])
