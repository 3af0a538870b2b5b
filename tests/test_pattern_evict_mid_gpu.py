"""The evicting Pattern set on the GPU between its two pinned extremes: capacities of 65537 and 262145 lines (257 and 1025
blocks per launch, so the scan's threads take 2 and 5 blocks each and the upper threads none, and a walk has hundreds of
batches) and the edge-driven trace (tests/pattern_evict_ref.py: edge_index), in the product library call by call, and in
the test library launch by launch, where the kind of every line and the set's cumulative counters are read out.

Every comparison is integer equality against the reference's own answers (tests/golden/ref_pattern_evict_mid_vectors.npz),
against the census derived from them (tests/golden/pattern_evict_coverage.json and pattern_evict_ref.census, which
tests/test_pattern_evict_mid_cpu.py ties to those answers) or against the line-analysis restatement (tests/pattern_ref.py),
never against the library itself."""
import functools
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from conftest import ROOT, pkg

import pattern_evict_ref as per
import pattern_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mpc():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("these tests need an MI355X")
    m = pkg()
    m.lib()
    return m


@pytest.fixture(scope="module")
def fixture(golden_dir):
    z = np.load(os.path.join(golden_dir, "ref_pattern_evict_mid_vectors.npz"))
    return z, json.loads(bytes(z["meta"]).decode())


@pytest.fixture(scope="module")
def coverage(golden_dir):
    with open(os.path.join(golden_dir, "pattern_evict_coverage.json")) as f:
        return json.load(f)


@functools.lru_cache(maxsize=2)
def _case(name):
    """(the case, its lines), built once for the tests that share it."""
    c = next(c for c in per.MID_CASES if c["name"] == name)
    lines = per.case_input(c)
    lines.setflags(write=False)
    return c, lines


def _flags(z, c):
    return np.unpackbits(z[c["name"] + "/existed"])[:c["n"]].astype(bool)


def _whole_vector(lines, flags):
    """The statistics vector of the whole trace: the line analysis from the restatement, T and [21] from the reference's flags."""
    v = pattern_ref.analyse(lines, with_set=False)[2]
    v[6], v[21] = lines.shape[1] * int(flags.sum()), int((~flags).sum())
    return v


def _feed_and_check(ev, lines, flags, cuts):
    """Feed lines[cuts[k]:cuts[k+1]] call by call; after every call (lines, T, insertions, Total) are the prefix sums of
    the reference's flags."""
    L = lines.shape[1]
    for a, b in zip(cuts[:-1], cuts[1:]):
        ev.compress_lines(lines[a:b], want_sizes=False, want_selected=False)
        v, hits = ev.stats_vector(), int(flags[:b].sum())
        got, want = (int(v[0]), int(v[6]), int(v[21]), int(v[8])), (b, L * hits, b - hits, L * b)
        print(f"after lines [{a}, {b}): (lines, T, insertions, Total) {got}, the reference's {want}")
        assert got == want, (f"after lines [{a}, {b})", got, want)
    assert ev.distinct_lines() == int((~flags[:cuts[-1]]).sum())


@pytest.mark.parametrize("name", [c["name"] for c in per.MID_CASES])
def test_mid_capacities_and_the_edge_trace(mpc, fixture, name):
    """Every case in one call and in calls that are no multiple of 256, a full launch, and a full launch plus one line,
    in the product library."""
    z, meta = fixture
    c, lines = _case(name)
    flags = _flags(z, c)
    assert per.digest(lines) == next(m for m in meta["cases"] if m["name"] == name)["sha256"]
    want = _whole_vector(lines, flags)
    for cuts in ([0, c["n"]], per.mid_cuts(c)):
        ev = mpc.Pattern(c["L"], on_full="evict", capacity=c["C"])
        assert ev.kernel_path == mpc.MPC_PATH_PATTERN_EVICTING
        _feed_and_check(ev, lines, flags, cuts)
        got = ev.stats_vector()
        assert (got == want).all(), [(int(i), int(got[i]), int(want[i])) for i in np.nonzero(got != want)[0][:8]]
        ev.close()


def test_device_path_on_alternating_streams(mpc, fixture):
    """A 64-byte case through compress_device, call after call on two streams in turn: the handle orders the set passes."""
    import torch
    z, meta = fixture
    c, lines = _case("C65537_L64_edge")
    flags, L = _flags(z, c), c["L"]
    ev = mpc.Pattern(L, on_full="evict", capacity=c["C"])
    d = torch.from_numpy(np.array(lines)).to("cuda:0")
    d_sizes = torch.zeros(len(lines), dtype=torch.int16, device="cuda:0")
    d_sel = torch.zeros(len(lines), dtype=torch.int8, device="cuda:0")
    side = torch.cuda.Stream()
    cuts = per.mid_cuts(c)
    for k, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
        stream = torch.cuda.current_stream().cuda_stream if k % 2 == 0 else side.cuda_stream
        ev.compress_device(d.data_ptr() + a * L, b - a, d_sizes.data_ptr() + 2 * a, d_sel.data_ptr() + a, stream=stream)
    ev.sync()
    torch.cuda.synchronize()
    got, want = ev.stats_vector(), _whole_vector(lines, flags)
    assert (got == want).all(), [(int(i), int(got[i]), int(want[i])) for i in np.nonzero(got != want)[0][:8]]
    want_sizes, want_sel, _ = pattern_ref.analyse(lines, with_set=False)
    assert (d_sizes.cpu().numpy().view(np.uint16) == want_sizes).all() and (d_sel.cpu().numpy() == want_sel).all()
    assert ev.distinct_lines() == int((~flags).sum())
    ev.close()


# The test library, one launch per call: usage  python -c CHILD <out.npz> <case> ...
CHILD = r"""
import ctypes, importlib, os, sys, time
sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, "tests"))
import numpy as np
mpc = importlib.import_module("cal_22-mpc_amd")
assert mpc.LIB_PATH.endswith("libmpc_hip_test.so"), mpc.LIB_PATH
import pattern_evict_ref as per
# test library only: the set's cumulative counters, and the MPC_ELINE_* kind of every line of the most recent launch
read_counters, read_kinds = mpc.lib().mpc_test_evict_counters, mpc.lib().mpc_test_evict_kinds
for f in (read_counters, read_kinds):
    f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]; f.restype = ctypes.c_int
out = {}
for name in sys.argv[2:]:
    c = next(c for c in per.MID_CASES if c["name"] == name)
    lines = per.case_input(c)
    ev = mpc.Pattern(c["L"], on_full="evict", capacity=c["C"])
    kinds, counters, t0 = [], [], time.time()
    for a, b in per.cut_launches(per.mid_cuts(c), min(c["C"], per.LAUNCH_LIMIT)):
        ev.compress_lines(lines[a:b], want_sizes=False, want_selected=False)
        k, w = np.zeros(b - a, dtype=np.uint8), (ctypes.c_uint64 * 8)()
        assert read_kinds(ev._h, k.ctypes.data, b - a) == 0 and read_counters(ev._h, w, 8) == 0
        kinds.append(k); counters.append([int(x) for x in w])
    out[name + "/seconds"] = np.array(time.time() - t0)
    out[name + "/kinds"], out[name + "/counters"], out[name + "/stats"] = np.concatenate(kinds), np.array(counters, dtype=np.uint64), ev.stats_vector()
    assert read_kinds(ev._h, k.ctypes.data, c["C"] + 1) != 0          # more lines than a launch has
    ev.close()
np.savez(sys.argv[1], **out)
"""


@pytest.mark.parametrize("bits", [None, 18])
def test_kinds_and_counters_launch_by_launch(mpc, fixture, coverage, tmp_path, bits):
    """The test library in a fresh process, fed one launch per call.  After every launch the kind of every line is the
    census's (existed or not per line, not only per call) and the cumulative counters are the coverage file's.  With the
    set's hash cut to 18 bits unequal lines share tags and start slots in tables of 2^19 slots, so the compare pass and
    the tail work through list B; nothing else may change."""
    z, meta = fixture
    names = per.TESTLIB_CASES if bits is None else ("C65537_L8_edge",)
    test_lib = os.path.join(ROOT, "cal_22-mpc_amd", "libmpc_hip_test.so")
    assert os.path.exists(test_lib), "libmpc_hip_test.so is missing: python cal_22-mpc_amd/build.py"
    env = dict(os.environ, MPC_HIP_LIB=test_lib)
    env.pop("MPC_TEST_PATTERN_TAG_BITS", None)
    if bits is not None:
        env["MPC_TEST_PATTERN_TAG_BITS"] = str(bits)
    out, t0 = str(tmp_path / "child.npz"), time.time()
    r = subprocess.run([sys.executable, "-c", CHILD % (ROOT, ROOT), out, *names], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    wall = time.time() - t0
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    got = np.load(out)
    print(f"tag bits {bits or 64}: the child took {wall:.2f} s; feeding alone " + ", ".join(f"{n} {float(got[n + '/seconds']):.2f} s" for n in names))
    for name in names:
        c, lines = _case(name)
        flags = _flags(z, c)
        entry = coverage["cases"][name]["cuts"]
        launches = per.cut_launches(entry["cuts"], min(c["C"], per.LAUNCH_LIMIT))
        assert entry["cuts"] == per.mid_cuts(c) and len(launches) == len(entry["after_launch"])
        want = per.census(per.case_index(c), c["C"], min(c["C"], per.LAUNCH_LIMIT), entry["cuts"])
        assert (want["flags"] == flags).all() and want["after_launch"] == entry["after_launch"]      # the census here is the committed one
        kinds, counters = got[name + "/kinds"], got[name + "/counters"]
        assert kinds.shape == (c["n"],) and counters.shape == (len(launches), 8)
        for k, (a, b) in enumerate(launches):
            wrong = np.nonzero(kinds[a:b] != want["kinds"][a:b])[0]
            assert len(wrong) == 0, (name, f"launch {k}, lines [{a}, {b})", [(int(i), int(kinds[a + i]), int(want["kinds"][a + i])) for i in wrong[:8]])
            assert [int(x) for x in counters[k, :5]] == entry["after_launch"][k], (name, f"after launch {k}", counters[k].tolist())
        assert not counters[:, 6:].any()
        if bits is None:
            assert not counters[:, 5].any()                      # whole 64-bit tags: no two unequal lines share one
        else:
            print(f"tag bits {bits}: {int(counters[-1, 5])} entries went through list B")
            assert counters[-1, 5] > 0 and (np.diff(counters[:, 5].astype(np.int64)) >= 0).all()
        v, want_v = got[name + "/stats"], _whole_vector(lines, flags)
        assert (v == want_v).all(), [(int(i), int(v[i]), int(want_v[i])) for i in np.nonzero(v != want_v)[0][:8]]
