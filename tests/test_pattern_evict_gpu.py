"""The evicting mode of the Pattern analyser on the GPU (mpc_create_pattern_evicting, Pattern(L, on_full="evict")).  Every
comparison is integer equality against the reference's own answers (tests/golden/ref_pattern_evict_vectors.npz and
ref_pattern_vectors.npz) or against the restatements (tests/pattern_evict_ref.py, tests/pattern_ref.py), never against the
library itself."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, pkg

import footprint as F
import pattern_evict_ref as per
import pattern_ref

pytestmark = pytest.mark.gpu
RAGGED = (1, 63, 64, 65, 511, 512, 513)          # then the rest: calls begin and end inside a launch and the at-risk window


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
    z = np.load(os.path.join(golden_dir, "ref_pattern_evict_vectors.npz"))
    return z, json.loads(bytes(z["meta"]).decode())


def _flags(z, c):
    return np.unpackbits(z[c["name"] + "/existed"])[:c["n"]].astype(bool)


def _cuts(n):
    cuts = [0]
    for k in RAGGED:
        cuts.append(min(n, cuts[-1] + k))
    return cuts + ([n] if cuts[-1] < n else [])


def _set_counts(v):
    """(lines, T, insertions, Total) of a statistics vector."""
    return int(v[0]), int(v[6]), int(v[21]), int(v[8])


def _want_counts(flags, upto, L):
    hits = int(flags[:upto].sum())
    return upto, L * hits, upto - hits, L * upto


def _feed_and_check(ev, lines, flags, cuts):
    """Feed lines[cuts[k]:cuts[k+1]] call by call; after every call the cumulative T and insertions are the prefix sums of
    the reference's flags."""
    L = lines.shape[1]
    for a, b in zip(cuts[:-1], cuts[1:]):
        ev.compress_lines(lines[a:b], want_sizes=False, want_selected=False)
        got, want = _set_counts(ev.stats_vector()), _want_counts(flags, b, L)
        assert got == want, (f"after lines [{a}, {b})", got, want)
    assert ev.distinct_lines() == int((~flags[:cuts[-1]]).sum())


def _whole_vector(lines, flags):
    """The statistics vector of the whole trace: the line analysis from the restatement, T and [21] from the reference's flags."""
    v = pattern_ref.analyse(lines, with_set=False)[2]
    v[6], v[21] = lines.shape[1] * int(flags.sum()), int((~flags).sum())
    return v


@pytest.mark.parametrize("name", [c["name"] for c in per.CASES])
def test_small_capacities(mpc, fixture, name):
    """Every small-capacity case in one call and in ragged calls, in the product library."""
    z, meta = fixture
    c = next(c for c in meta["cases"] if c["name"] == name)
    lines, flags = per.case_input(c), _flags(z, c)
    assert per.digest(lines) == c["sha256"]
    one = mpc.Pattern(c["L"], on_full="evict", capacity=c["C"])
    assert one.kernel_path == mpc.MPC_PATH_PATTERN_EVICTING and one.info.algorithm == 5 and one.stats_len == 534
    assert "evicting set passes" in (mpc.lib().mpc_kernel_form(one._h) or b"").decode()
    _feed_and_check(one, lines, flags, [0, len(lines)])
    assert (one.stats_vector() == _whole_vector(lines, flags)).all()
    one.close()
    ragged = mpc.Pattern(c["L"], on_full="evict", capacity=c["C"])
    _feed_and_check(ragged, lines, flags, _cuts(len(lines)))
    assert (ragged.stats_vector() == _whole_vector(lines, flags)).all()
    ragged.close()


TAG_CASES = ("C64_L64_mix", "C1000_L72_rand_2c")
CHILD = r"""
import json, os, sys
sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, "tests"))
import importlib
import numpy as np
mpc = importlib.import_module("cal_22-mpc_amd")
assert mpc.LIB_PATH.endswith("libmpc_hip_test.so"), mpc.LIB_PATH
import pattern_evict_ref as per
from test_pattern_evict_gpu import TAG_CASES, _cuts
out = {}
for c in per.CASES:
    if c["name"] not in TAG_CASES:
        continue
    lines = per.case_input(c)
    for how, cuts in (("one", [0, len(lines)]), ("ragged", _cuts(len(lines)))):
        ev = mpc.Pattern(c["L"], on_full="evict", capacity=c["C"])
        rows = []
        for a, b in zip(cuts[:-1], cuts[1:]):
            ev.compress_lines(lines[a:b], want_sizes=False, want_selected=False)
            v = ev.stats_vector()
            rows.append([int(v[0]), int(v[6]), int(v[21]), int(v[8])])
        out[c["name"] + "/" + how] = rows
        ev.close()
print("RESULT " + json.dumps(out))
"""


@pytest.mark.parametrize("bits", [1, 5])
def test_unequal_lines_that_collide_on_the_tag(mpc, fixture, bits):
    """Two cases again in the test library with the set's hash cut to a few bits, in a fresh process: unequal lines share
    tags and chains in both tables.  Nothing may change."""
    z, meta = fixture
    test_lib = os.path.join(ROOT, "cal_22-mpc_amd", "libmpc_hip_test.so")
    assert os.path.exists(test_lib), "libmpc_hip_test.so is missing: python cal_22-mpc_amd/build.py"
    env = dict(os.environ, MPC_HIP_LIB=test_lib, MPC_TEST_PATTERN_TAG_BITS=str(bits))
    r = subprocess.run([sys.executable, "-c", CHILD % (ROOT, ROOT)], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = json.loads(next(ln for ln in r.stdout.split("\n") if ln.startswith("RESULT "))[7:])
    for name in TAG_CASES:
        c = next(c for c in meta["cases"] if c["name"] == name)
        flags = _flags(z, c)
        for how, cuts in (("one", [0, c["n"]]), ("ragged", _cuts(c["n"]))):
            want = [list(_want_counts(flags, b, c["L"])) for b in cuts[1:]]
            assert out[name + "/" + how] == want, (name, how)


def test_below_the_capacity_both_modes_give_the_reference_numbers(mpc, golden_dir):
    """Every case of ref_pattern_vectors.npz: an evicting handle with the reference's capacity and the default handle."""
    z = np.load(os.path.join(golden_dir, "ref_pattern_vectors.npz"))
    for c in json.loads(bytes(z["meta"]).decode())["cases"]:
        lines = pattern_ref.case_input(c)
        want = z[c["name"] + "/stats"]
        for ev in (mpc.Pattern(c["L"], on_full="evict", capacity=None), mpc.Pattern(c["L"])):
            sizes, sel = ev.compress_lines(lines)
            v = ev.stats_vector()
            assert (v == want).all(), (c["name"], ev.on_full, [(int(i), int(v[i]), int(want[i])) for i in np.nonzero(v != want)[0][:8]])
            assert (sizes == z[c["name"] + "/sizes"]).all() and (sel == z[c["name"] + "/sel"]).all()
            assert ev.distinct_lines() == int(want[21])
            ev.close()


def test_the_real_capacity(mpc, fixture):
    """The five parts of the real-capacity case as five calls: the reference's own totals after each.  128 MiB of lines."""
    z, meta = fixture
    totals, insertions = z["real/totals"], z["real/insertions"]
    ev = mpc.Pattern(8, on_full="evict")
    for k, (a, b) in enumerate(per.REAL_PARTS):
        ev.compress_lines(per.real_lines(a, b), want_sizes=False, want_selected=False)
        v = ev.stats_vector()
        got = [int(v[0])] + [int(x) for x in v[4:9]] + [int(x) for x in v[9:21]]
        assert got == [int(x) for x in totals[k]], (k, got, totals[k].tolist())
        assert int(v[21]) == int(insertions[k]) and ev.distinct_lines() == int(insertions[k])
    ev.close()


@pytest.fixture(scope="module")
def paths_case(fixture):
    z, meta = fixture
    c = next(c for c in meta["cases"] if c["name"] == "C1000_L64_mix")
    return c, per.case_input(c), _flags(z, c)


def test_device_path(mpc, paths_case):
    import torch
    c, lines, flags = paths_case
    L = c["L"]
    ev = mpc.Pattern(L, on_full="evict", capacity=c["C"])
    d = torch.from_numpy(lines).to("cuda:0")
    d_sizes = torch.zeros(len(lines), dtype=torch.int16, device="cuda:0")
    d_sel = torch.zeros(len(lines), dtype=torch.int8, device="cuda:0")
    side = torch.cuda.Stream()
    cuts = _cuts(len(lines))
    for k, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):               # alternating streams: the set passes are ordered by the handle
        stream = torch.cuda.current_stream().cuda_stream if k % 2 == 0 else side.cuda_stream
        ev.compress_device(d.data_ptr() + a * L, b - a, d_sizes.data_ptr() + 2 * a, d_sel.data_ptr() + a, stream=stream)
    ev.sync()
    torch.cuda.synchronize()
    assert (ev.stats_vector() == _whole_vector(lines, flags)).all()
    want_sizes, want_sel, _ = pattern_ref.analyse(lines, with_set=False)
    assert (d_sizes.cpu().numpy().view(np.uint16) == want_sizes).all() and (d_sel.cpu().numpy() == want_sel).all()
    raw = torch.zeros(ev.stats_raw_len(), dtype=torch.int64, device="cuda:0")
    ev.stats_copy_raw_device(raw.data_ptr())
    torch.cuda.synchronize()
    assert (ev.stats_from_raw(raw.cpu().numpy().view(np.uint64)) == ev.stats_vector()).all()
    ev.close()


def test_npy_and_log_ingestion(mpc, traces, tmp_path, paths_case):
    c, lines, flags = paths_case
    L = c["L"]
    npy = traces.save_npy(str(tmp_path / "t.npy"), lines)
    ev = mpc.Pattern(L, on_full="evict", capacity=c["C"])
    assert ev.compress_npy(npy) == len(lines) - 1                       # the driver never compresses the final row
    assert (ev.stats_vector() == _whole_vector(lines[:-1], flags[:-1])).all()
    ev.close()
    types = np.random.default_rng(3).integers(0, 9, len(lines))
    log = traces.write_gpgpusim_log(str(tmp_path / "t.log"), lines, types)
    kept = lines[(types == 0) | (types == 4)]
    kept_flags, _ = per.fifo_flags(per.keys_of(kept), c["C"])           # another trace: the restatement decides
    assert kept_flags.any() and not kept_flags.all()
    ev = mpc.Pattern(L, on_full="evict", capacity=c["C"])
    assert ev.compress_gpgpusim_log(log) == (len(lines), len(kept))
    assert (ev.stats_vector() == _whole_vector(kept, kept_flags)).all()
    ev.close()


def test_group_equals_solo_with_a_size_histogram(mpc, paths_case):
    c, lines, flags = paths_case
    L = c["L"]
    members = [mpc.BDI(L), mpc.Pattern(L, on_full="evict", capacity=c["C"])]
    members[1].enable_size_histogram()
    alone = mpc.BDI(L)
    alone.compress_lines(lines)
    g = mpc.EvaluatorSet(members)
    assert g.form.endswith("PATTERN: own kernels"), g.form
    cut = 300                                                           # in place, then staged
    out = g.compress_lines(lines[:cut]) + []
    out2 = g.compress_lines(lines[cut:])
    want_sizes, want_sel, _ = pattern_ref.analyse(lines, with_set=False)
    assert (np.concatenate([out[1][0], out2[1][0]]) == want_sizes).all() and (np.concatenate([out[1][1], out2[1][1]]) == want_sel).all()
    assert (members[1].stats_vector() == _whole_vector(lines, flags)).all()
    assert (members[0].stats_vector() == alone.stats_vector()).all()
    hist = members[1].size_histogram()
    assert (hist == np.bincount(want_sizes, minlength=len(hist)).astype(np.uint64)).all()
    g.close()
    for m in members + [alone]:
        m.close()


def test_reset_keeps_the_set_and_its_stamps(mpc, paths_case):
    c, lines, flags = paths_case
    L, half = c["L"], len(lines) // 2 + 77
    ev = mpc.Pattern(L, on_full="evict", capacity=c["C"])
    ev.compress_lines(lines[:half])
    ev.reset()
    assert not ev.stats_vector().any() and ev.distinct_lines() == int((~flags[:half]).sum())
    ev.compress_lines(lines[half:])
    v = ev.stats_vector()
    want = pattern_ref.analyse(lines[half:], with_set=False)[2]
    want[6], want[21] = L * int(flags[half:].sum()), int((~flags[half:]).sum())      # the answers of the whole trace's second half
    assert (v == want).all()
    assert ev.distinct_lines() == int((~flags).sum())
    ev.close()


class EvictRef(F.PatternRef):
    """footprint.PatternRef with the reference's cache carried across the calls instead of a plain set."""

    def __init__(self, L, capacity):
        super().__init__(L)
        self.fifo, self.hits = per.Fifo(capacity), 0

    def feed(self, lines):
        out = super().feed(lines)
        self.hits += int(self.fifo.feed(per.keys_of(lines)).sum())
        return out

    def stats_vector(self):
        v = self.v.copy()
        v[21] = self.fifo.insertions
        v[6] = self.L * self.hits
        return v


@pytest.mark.parametrize("L", [64, 72])
def test_footprint(mpc, traces, L):
    """The device-path footprint sweep of tests/footprint.py with an evicting handle of capacity 1000: nothing outside the
    range a call was given is read or written, and the statistics follow the cache across the calls."""
    ev, ref = mpc.Pattern(L, on_full="evict", capacity=1000), EvictRef(L, 1000)
    pool = F.pattern_pool(traces, L, n=2520)                            # more distinct lines than the capacity
    # (offsets: multiples of 16 as the C ABI asks; footprint.offsets_for's third one is not a multiple of 16 at L = 72)
    calls = F.sweep(ev, [ref], pool, counts=F.LINE_COUNTS + (2500,), offsets=(0, 16, 48), tag="Pattern evict")
    distinct = len({bytes(r) for r in pool})
    assert calls > 100 and distinct > 1000 and ref.fifo.insertions > distinct      # lines were evicted and came back
    ev.close()


def test_host_class_and_compressor_set(paths_case, tmp_path):
    """comp::Pattern(L, comp::PatternOnFull::Evict, C) per line, in batches and as a member of a comp::CompressorSet
    (tests/native/pattern_evict_probe.cpp): the fixture's totals whichever way the lines came in."""
    c, lines, flags = paths_case
    host = os.path.join(ROOT, "cal_22-mpc_amd", "host")
    exe = str(tmp_path / "pattern_evict_probe")
    srcs = [os.path.join(host, f) for f in sorted(os.listdir(host)) if f.endswith(".cpp") and f != "main.cpp"]
    b = subprocess.run(["hipcc", "-O2", "-std=c++17", "-Wall", "-I", host, "-I", os.path.join(ROOT, "include"), "-o", exe,
                        os.path.join(ROOT, "tests", "native", "pattern_evict_probe.cpp"), *srcs,
                        "-L", os.path.join(ROOT, "cal_22-mpc_amd"), "-lmpc_hip",
                        "-Wl,-rpath," + os.path.join(ROOT, "cal_22-mpc_amd")], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe, "refuse", "64", str(1 << 24)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "16777216" in r.stdout + r.stderr and "not refused" not in r.stdout
    path = tmp_path / "lines.bin"
    lines.tofile(str(path))
    r = subprocess.run([exe, "run", str(path), str(c["L"]), str(c["C"])], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    n, hits = len(lines), int(flags.sum())
    row = f"{n} {c['L'] * hits} {c['L'] * n} {n - hits}"
    assert r.stdout.strip().split("\n") == [f"a {row}", f"c {row}", f"f {row}", "form BDI: own kernel; PATTERN: own kernels"]
