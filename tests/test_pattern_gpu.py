"""The Pattern analyser on the GPU.  Every integer comparison is exact: against the reference's own numbers
(tests/golden/ref_pattern_vectors.npz) for the seeded cases, against the restatement (tests/pattern_ref.py) elsewhere.
Entropies: equal to the restatement's in this process (the same log2), and within 256 x 2^-52 of the doubles the reference
recorded (at most 256 terms, each below 0.54; another libm may differ in the last bit of a term)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, pkg

import pattern_ref

pytestmark = pytest.mark.gpu
ENTROPY_TOL = 256 * 2.0 ** -52


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
    z = np.load(os.path.join(golden_dir, "ref_pattern_vectors.npz"))
    return z, json.loads(bytes(z["meta"]).decode())["cases"]


def _mix(n, L, seed, period=None):
    """n lines of the kinds a trace has -- zero, word-same, small integers, pointers, floats, noise -- with repeats:
    line i is a function of i % period."""
    rng = np.random.default_rng(seed)
    period = period or n
    kind = rng.integers(0, 8, period)
    out = np.zeros((period, L), dtype=np.uint8)
    w = out.view("<u4")
    q = out.view("<u8")
    m = kind == 1
    w[m] = rng.integers(0, 1 << 32, (int(m.sum()), 1), dtype=np.uint64).astype("<u4")
    m = kind == 2
    w[m] = rng.integers(0, 300, (int(m.sum()), L // 4)).astype("<u4")
    m = kind == 3
    q[m] = (0x00007F0000000000 + rng.integers(0, 1 << 20, (int(m.sum()), 1), dtype=np.uint64) * 4096
            + rng.integers(0, 200, (int(m.sum()), L // 8), dtype=np.uint64)).astype("<u8")
    m = kind == 4
    w[m] = np.sin(rng.random((int(m.sum()), L // 4)) * 6.28).astype("<f4").view("<u4")
    m = kind == 5
    out[m] = rng.integers(0, 256, (int(m.sum()), L), dtype=np.uint8)
    m = kind == 6
    out.view("<u2")[m] = (0x4100 + rng.integers(0, 250, (int(m.sum()), L // 2))).astype("<u2")
    m = kind == 7
    w[m] = (0x80000000 + rng.integers(0, 60000, (int(m.sum()), L // 4), dtype=np.uint64)).astype("<u4")
    idx = np.arange(n) % period
    return np.ascontiguousarray(out[idx])


def _check(ev, lines, sizes=None, sel=None):
    """The handle's statistics (and a call's per-line outputs) against the restatement over all `lines` it has seen."""
    want_sizes, want_sel, want = pattern_ref.analyse(lines)
    got = ev.stats_vector()
    assert (got == want).all(), [(int(i), int(got[i]), int(want[i])) for i in np.nonzero(got != want)[0][:8]]
    if sizes is not None:
        assert (sizes == want_sizes[-len(sizes):]).all()
    if sel is not None:
        assert (sel == want_sel[-len(sel):]).all()
    return want


def test_fixture_cases(mpc, fixture):
    z, cases = fixture
    for c in cases:
        lines = pattern_ref.case_input(c)
        assert pattern_ref.digest(lines) == c["sha256"]
        ev = mpc.Pattern(c["L"])
        assert ev.kernel_path == mpc.MPC_PATH_PATTERN and ev.info.algorithm == 5 and ev.stats_len == 534
        sizes, sel = ev.compress_lines(lines)
        assert (sizes == z[c["name"] + "/sizes"]).all(), c["name"]
        assert (sel == z[c["name"] + "/sel"]).all(), c["name"]
        v = ev.stats_vector()
        want = z[c["name"] + "/stats"]
        assert (v == want).all(), (c["name"], [(int(i), int(v[i]), int(want[i])) for i in np.nonzero(v != want)[0][:8]])
        r = ev.result()
        assert r["entropy"] == pattern_ref.entropy(want[22:278]) and r["entropy_except"] == pattern_ref.entropy(want[278:534])
        ent = z[c["name"] + "/entropy"]
        assert abs(r["entropy"] - ent[0]) <= ENTROPY_TOL and abs(r["entropy_except"] - ent[1]) <= ENTROPY_TOL
        assert (r["Z"], r["R"], r["T"], r["U"], r["Total"]) == tuple(int(x) for x in want[4:9])
        assert r["original_bits"] == 0 and r["compressed_bits"] == 0 and r["comp_ratio"] == 0.0 and r["name"] == "Pattern Checker"
        assert ev.distinct_lines() == int(want[21])
        # line by line, as an unchanged reference driver calls it
        one = mpc.Pattern(c["L"])
        for i in range(len(lines)):
            s, k = one.compress_lines(lines[i:i + 1])
            assert s[0] == sizes[i] and k[0] == sel[i]
        assert (one.stats_vector() == want).all()
        ev.close()
        one.close()


@pytest.mark.parametrize("L", [8, 32, 64, 128, 256])
def test_duplicates_within_one_wave(mpc, L):
    base = _mix(7, L, seed=L)
    lines = base[np.random.default_rng(L).integers(0, 7, 64)]          # 64 lines, at most 7 different ones
    ev = mpc.Pattern(L)
    sizes, sel = ev.compress_lines(lines)
    want = _check(ev, lines, sizes, sel)
    assert int(want[21]) <= 7 and ev.distinct_lines() == int(want[21])
    ev.compress_lines(lines[::-1].copy())                              # all seen before
    assert int(ev.stats_vector()[6]) == int(want[6]) + 64 * L
    ev.close()


def test_duplicates_across_the_in_place_boundary(mpc):
    L = 64
    lines = _mix(512 + 513 + 100, L, seed=3, period=400)
    ev = mpc.Pattern(L)
    s1, k1 = ev.compress_lines(lines[:512])                             # in place
    _check(ev, lines[:512], s1, k1)
    s2, k2 = ev.compress_lines(lines[512:1025])                         # staged
    _check(ev, lines[:1025], s2, k2)
    s3, k3 = ev.compress_lines(lines[1025:])
    _check(ev, lines, s3, k3)
    ev.close()


def test_duplicates_across_staging_chunks(mpc):
    L = 64
    n = (1 << 20) + 70001                                               # a staging slot holds 2^20 lines of 64 bytes
    lines = _mix(n, L, seed=11, period=(1 << 20) - 12345)
    ev = mpc.Pattern(L)
    sizes, sel = ev.compress_lines(lines)
    want = _check(ev, lines, sizes, sel)
    assert int(want[6]) > 70000 * L
    ev.close()


def test_duplicates_across_calls_on_the_device_path(mpc):
    import torch
    L = 128
    lines = _mix(30000, L, seed=17, period=9000)
    ev = mpc.Pattern(L)
    d = torch.from_numpy(lines).to("cuda:0")
    d_sizes = torch.zeros(len(lines), dtype=torch.int16, device="cuda:0")
    d_sel = torch.zeros(len(lines), dtype=torch.int8, device="cuda:0")
    side = torch.cuda.Stream()
    cuts = [0, 1, 4097, 12000, 30000]
    for k in range(4):                                                  # alternating streams: the set passes are ordered by the handle
        a, b = cuts[k], cuts[k + 1]
        stream = torch.cuda.current_stream().cuda_stream if k % 2 == 0 else side.cuda_stream
        ev.compress_device(d.data_ptr() + a * L, b - a, d_sizes.data_ptr() + 2 * a, d_sel.data_ptr() + a, stream=stream)
    ev.sync()
    torch.cuda.synchronize()
    _check(ev, lines, d_sizes.cpu().numpy().view(np.uint16), d_sel.cpu().numpy())
    # the raw accumulators, device to device
    raw = torch.zeros(ev.stats_raw_len(), dtype=torch.int64, device="cuda:0")
    ev.stats_copy_raw_device(raw.data_ptr())
    torch.cuda.synchronize()
    assert (ev.stats_from_raw(raw.cpu().numpy().view(np.uint64)) == ev.stats_vector()).all()
    ev.close()


def test_reset_keeps_the_set(mpc):
    L = 32
    lines = _mix(3000, L, seed=5, period=1000)
    ev = mpc.Pattern(L)
    ev.compress_lines(lines)
    first = ev.stats_vector()
    ev.reset()
    assert not ev.stats_vector().any()
    ev.compress_lines(lines)
    v = ev.stats_vector()
    assert int(v[6]) == L * len(lines) and int(v[21]) == 0 and ev.distinct_lines() == int(first[21])
    keep = np.ones(534, bool)
    keep[[6, 21]] = False
    assert (v[keep] == first[keep]).all()
    ev.close()


def test_npy_and_log_ingestion(mpc, traces, tmp_path):
    L = 64
    lines = _mix(5000, L, seed=23, period=1700)
    npy = traces.save_npy(str(tmp_path / "t.npy"), lines)
    ev = mpc.Pattern(L)
    assert ev.compress_npy(npy) == len(lines) - 1                       # the driver never compresses the final row
    _check(ev, lines[:-1])
    ev.close()
    types = np.random.default_rng(3).integers(0, 9, len(lines))
    log = traces.write_gpgpusim_log(str(tmp_path / "t.log"), lines, types)
    kept = lines[(types == 0) | (types == 4)]
    ev = mpc.Pattern(L)
    assert ev.compress_gpgpusim_log(log) == (len(lines), len(kept))
    _check(ev, kept)
    ev.close()


@pytest.mark.parametrize("L", [64, 40])
def test_group_equals_solo(mpc, tmp_path, traces, L):
    lines = _mix(20000, L, seed=29, period=6000)
    solo = mpc.Pattern(L)
    s0, k0 = solo.compress_lines(lines)
    members = [mpc.BDI(L), mpc.FPC(L)] + ([mpc.BPC(L)] if L == 64 else []) + [mpc.Pattern(L)]
    alone = [type(m)(L) for m in members[:-1]]
    g = mpc.EvaluatorSet(members)
    assert g.form.endswith("PATTERN: own kernels"), g.form
    if L == 64:
        assert g.form == "BDI+FPC+BPC: one kernel; PATTERN: own kernels"
    out = g.compress_lines(lines[:300]) + []                            # in place, then staged
    out2 = g.compress_lines(lines[300:])
    assert (np.concatenate([out[-1][0], out2[-1][0]]) == s0).all() and (np.concatenate([out[-1][1], out2[-1][1]]) == k0).all()
    assert (members[-1].stats_vector() == solo.stats_vector()).all()
    for m, a in zip(members[:-1], alone):
        a.compress_lines(lines)
        assert (m.stats_vector() == a.stats_vector()).all()
    # a file through the group: the set has seen every line already
    npy = traces.save_npy(str(tmp_path / "t.npy"), lines)
    before = members[-1].stats_vector()
    assert g.compress_npy(npy) == len(lines) - 1
    after = members[-1].stats_vector()
    assert int(after[6]) - int(before[6]) == L * (len(lines) - 1) and after[21] == before[21]
    g.close()
    for m in members + alone + [solo]:
        m.close()


CHILD = r"""
import json, os, sys
sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, "tests"))
import importlib
import numpy as np
mpc = importlib.import_module("cal_22-mpc_amd")
assert mpc.LIB_PATH.endswith("libmpc_hip_test.so"), mpc.LIB_PATH
import pattern_ref
from test_pattern_gpu import _mix
out = {}
for c in pattern_ref.CASES:
    ev = mpc.Pattern(c["L"])
    ev.compress_lines(pattern_ref.case_input(c))
    out[c["name"]] = [int(x) for x in ev.stats_vector()]
    ev.close()
lines = _mix(6000, 64, seed=31, period=2500)
ev = mpc.Pattern(64)
ev.compress_lines(lines[:200]); ev.compress_lines(lines[200:4000]); ev.compress_lines(lines[4000:])
out["mix"] = [int(x) for x in ev.stats_vector()]
out["mix_distinct"] = ev.distinct_lines()
print("RESULT " + json.dumps(out))
"""


@pytest.mark.parametrize("bits", [1, 5])
def test_unequal_lines_that_collide_on_the_tag(mpc, fixture, bits):
    """The test library with the set's hash cut to a few bits: unequal lines share tags and chains, the compare pass and
    the tail have to walk them.  Nothing may change."""
    z, cases = fixture
    test_lib = os.path.join(ROOT, "cal_22-mpc_amd", "libmpc_hip_test.so")
    assert os.path.exists(test_lib), "libmpc_hip_test.so is missing: python cal_22-mpc_amd/build.py"
    env = dict(os.environ, MPC_HIP_LIB=test_lib, MPC_TEST_PATTERN_TAG_BITS=str(bits))
    r = subprocess.run([sys.executable, "-c", CHILD % (ROOT, ROOT)], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = json.loads(next(ln for ln in r.stdout.split("\n") if ln.startswith("RESULT "))[7:])
    for c in cases:
        assert out[c["name"]] == [int(x) for x in z[c["name"] + "/stats"]], c["name"]
    lines = _mix(6000, 64, seed=31, period=2500)
    want = pattern_ref.analyse(lines)[2]
    assert out["mix"] == [int(x) for x in want] and out["mix_distinct"] == int(want[21])


def test_the_limit(mpc):
    """2^24 - 1 distinct lines plus repeats are taken, with the exact T; one more distinct line is refused, and so is
    everything after it."""
    L, cap = 8, pattern_ref.CAPACITY
    vals = np.arange(cap, dtype="<u8") * np.uint64(0x9E3779B97F4A7C15 | 1)      # distinct: an odd multiplier is a bijection
    rep = vals[np.random.default_rng(7).integers(0, cap, 5000)]
    lines = np.concatenate([vals[:5000000], rep[:2000], vals[5000000:], rep[2000:]]).view(np.uint8).reshape(-1, L)
    ev = mpc.Pattern(L)
    ev.compress_lines(lines, want_sizes=False, want_selected=False)
    v = ev.stats_vector()
    assert int(v[0]) == cap + 5000 and int(v[6]) == L * 5000 and int(v[21]) == cap and int(v[8]) == L * (cap + 5000)
    assert ev.distinct_lines() == cap
    ev.compress_lines(lines[:1000])                                     # seen before: still fine at the capacity
    assert int(ev.stats_vector()[6]) == L * 6000
    one_more = np.array([cap], dtype="<u8") * np.uint64(0x9E3779B97F4A7C15 | 1)
    with pytest.raises(mpc.MpcError) as e:
        ev.compress_lines(one_more.view(np.uint8).reshape(1, L))
    assert e.value.code == -22 and "16777215" in str(e.value) and "distinct lines" in str(e.value)
    with pytest.raises(mpc.MpcError) as e:
        ev.compress_lines(lines[:10])
    assert e.value.code == -22
    with pytest.raises(mpc.MpcError) as e:
        ev.stats_vector()
    assert e.value.code == -22 and "distinct lines" in str(e.value)
    ev.close()
