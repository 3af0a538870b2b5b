"""C-Pack with a per-line dictionary on the GPU.  Every comparison is exact integer equality: against the reference's own
numbers (tests/golden/ref_cpack_vectors.npz: a fresh reference comp::CPACK per line) for the seeded cases, against the
restatement (tests/cpack_ref.py, pinned to that fixture by tests/test_cpack_cpu.py) and the CPU oracles elsewhere --
never against per-line output of the library under test."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, pkg

import cpack_ref
import footprint as F

pytestmark = pytest.mark.gpu

BINS = 4096
NAMES = [c["name"] for c in cpack_ref.CASES]


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
    return cpack_ref.load_fixture(os.path.join(golden_dir, "ref_cpack_vectors.npz"))


def _case(fixture, name):
    """-> (case, lines, the reference's sizes, its per-line counts, the statistics vector of all the lines)"""
    meta, z = fixture
    c = next(c for c in meta["cases"] if c["name"] == name)
    lines = cpack_ref.case_input(c)
    st = z[name + ".stats"]
    v = np.array([c["n"], int(st[0]), int(st[1]), int(st[2])] + [int(x) for x in st[3:]], dtype=np.uint64)
    return c, lines, z[name + ".sizes"], z[name + ".counts"], v


def _same(tag, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{tag}: {bad.size} differ, first at {bad[:6].tolist()}: {got[bad[:6]].tolist()} vs {want[bad[:6]].tolist()}"


def _bincount(sizes):
    return np.bincount(np.asarray(sizes).astype(np.int64), minlength=BINS).astype(np.uint64)


class CpackRef:
    """The restatement over the calls of one handle (tests/footprint.py: feed / stats_vector).  Lines are independent and
    the statistics plain sums, so the restatement runs once per distinct batch."""

    def __init__(self, L):
        self.L, self.seen, self.total = L, {}, None

    def feed(self, lines):
        key = (lines.shape, lines.tobytes())
        if key not in self.seen:
            sizes, counts = cpack_ref.compress(lines, "line")
            self.seen[key] = (sizes, np.zeros(len(lines), np.int8), cpack_ref.stats_vector(self.L, sizes, counts))
        sizes, sel, v = self.seen[key]
        self.total = v.copy() if self.total is None else self.total + v
        return sizes, sel

    def stats_vector(self):
        return self.total


# ---- 1. the fixture, through the host batch path ------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_fixture_case(mpc, fixture, name):
    c, lines, want_sizes, want_counts, want = _case(fixture, name)
    L = c["L"]
    ev = mpc.CPACK(L)
    assert ev.kernel_path == mpc.MPC_PATH_CPACK == 8 and ev.info.algorithm == 6 and ev.info.num_clusters == 6
    assert ev.stats_len == 10 and ev.stats_raw_len() == 7 and ev.line_size == L
    form = (mpc.lib().mpc_kernel_form(ev._h) or b"").decode()
    assert form == ("unrolled" if L in (32, 64, 128) else "run-time loop")
    sizes, sel = ev.compress_lines(lines)                       # staged (more than 512 lines)
    _same(name + " sizes", sizes, want_sizes)
    assert not sel.any()
    _same(name + " statistics", ev.stats_vector(), want)
    r = ev.result()
    assert r["comp_ratio"] == float(fixture[1][name + ".ratio"][0])                       # the same double
    assert r["total_words"] == int(want[3]) and r["counts"] == [int(x) for x in want[4:]] and r["name"] == "C-Pack"
    assert (r["lines"], r["original_bits"], r["compressed_bits"]) == tuple(int(x) for x in want[:3])
    # ragged calls, most of them evaluated in place (up to 512 lines): tails of a wave, a group and the in-place limit
    one = mpc.CPACK(L, dictionary="line")
    at, got = 0, []
    for n in (1, 63, 64, 65, 511, 512, 513):
        got.append(one.compress_lines(lines[at:at + n])[0])
        at += n
    got.append(one.compress_lines(lines[at:])[0])
    _same(name + " sizes, ragged calls", np.concatenate(got), want_sizes)
    _same(name + " statistics, ragged calls", one.stats_vector(), want)
    one.reset()
    assert not one.stats_vector().any()
    ev.close()
    one.close()


# ---- 2. the other ingestion paths ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [32, 64, 128])
def test_device_npy_and_log_paths(mpc, fixture, traces, tmp_path, L):
    import torch
    c, lines, want_sizes, want_counts, want = _case(fixture, f"cpack_L{L}")
    n = len(lines)
    ev = mpc.CPACK(L)
    d = torch.from_numpy(lines).to("cuda:0")
    d_sizes = torch.zeros(n, dtype=torch.int16, device="cuda:0")
    d_sel = torch.full((n,), 7, dtype=torch.int8, device="cuda:0")
    cut = 777
    ev.compress_device(d.data_ptr(), cut, d_sizes.data_ptr(), d_sel.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    ev.compress_device(d.data_ptr() + cut * L, n - cut, d_sizes.data_ptr() + 2 * cut, d_sel.data_ptr() + cut)
    ev.sync()
    torch.cuda.synchronize()
    _same("device sizes", d_sizes.cpu().numpy().view(np.uint16), want_sizes)
    assert not d_sel.cpu().numpy().any()
    _same("device statistics", ev.stats_vector(), want)
    ev.close()
    # .npy: the driver never compresses the final row
    npy = traces.save_npy(str(tmp_path / "t.npy"), lines)
    ev = mpc.CPACK(L)
    assert ev.compress_npy(npy) == n - 1
    _same(".npy statistics", ev.stats_vector(), cpack_ref.stats_vector(L, want_sizes[:-1], want_counts[:-1]))
    ev.close()
    # .log: the GLOBAL_ACC_R (0) and GLOBAL_ACC_W (4) requests, in order
    types = np.random.default_rng(3).integers(0, 9, n)
    log = traces.write_gpgpusim_log(str(tmp_path / "t.log"), lines, types)
    keep = (types == 0) | (types == 4)
    ev = mpc.CPACK(L)
    assert ev.compress_gpgpusim_log(log) == (n, int(keep.sum()))
    _same(".log statistics", ev.stats_vector(), cpack_ref.stats_vector(L, want_sizes[keep], want_counts[keep]))
    ev.close()


# ---- 3. footprint -----------------------------------------------------------------------------------------------------------
def _footprint_pool(fixture, L, n=1260):
    """The first lines of the case (its hand-built lines, key-set lines and trace families, shuffled)."""
    return np.ascontiguousarray(_case(fixture, f"cpack_L{L}")[1][:n])


@pytest.mark.parametrize("L", [32, 64, 128, 36, 252])
def test_footprint(mpc, fixture, L):
    """32 / 64 / 128 bytes: the unrolled kernels; 36 and 252 bytes: the any-line-size kernel (lines that do not start on a
    16-byte boundary).  Line counts around the wave, group, block and workgroup edges, the line buffer at base + 0 / + 16 /
    + L/2 + 16, sizes 2-byte and `selected` 1-byte aligned, every combination of the two optional outputs."""
    ev = mpc.CPACK(L)
    form = (mpc.lib().mpc_kernel_form(ev._h) or b"").decode()
    assert ev.kernel_path == mpc.MPC_PATH_CPACK and form == ("unrolled" if L in (32, 64, 128) else "run-time loop")
    offsets = tuple(off - off % 16 for off in F.offsets_for(L))              # (252 / 2 + 16 is no multiple of 16: 128)
    calls = F.sweep(ev, [CpackRef(L)], _footprint_pool(fixture, L), offsets=offsets, tag="CPACK")
    assert len(set(offsets)) == (3 if L >= 64 else 2) and calls == 2 * len(offsets) * (len(F.LINE_COUNTS) + 3 * len(F.MODE_COUNTS))
    ev.close()


# ---- 4. groups, histograms, best-of -----------------------------------------------------------------------------------------
def _group_case(mpc, configs, oracle, fixture, L):
    c, lines, want_cpack, _, _ = _case(fixture, f"cpack_L{L}")
    if L == 64:
        names = ["BDI", "FPC", "BPC", "CPACK"]
        want = [oracle.BdiOracle(L).compress(lines)[0], oracle.FpcOracle(L).compress(lines), oracle.BpcOracle(L).compress(lines), want_cpack]
        make = [lambda: mpc.BDI(L), lambda: mpc.FPC(L), lambda: mpc.BPC(L), lambda: mpc.CPACK(L)]
        form = "BDI+FPC+BPC: one kernel; CPACK: own kernel"
    else:
        cfg = configs.probe_config(L)
        names = ["VPC", "CPACK"]
        want = [oracle.VpcOracle(cfg).compress(lines)[0], want_cpack]
        make = [lambda: mpc.VPC(cfg), lambda: mpc.CPACK(L)]
        form = "VPC: unrolled; CPACK: own kernel"
    return lines, names, [np.asarray(w).astype(np.int64) for w in want], make, form


@pytest.mark.parametrize("L", [64, 32])
def test_group_members_histograms_and_best_of(mpc, configs, oracle, fixture, L):
    lines, names, want, make, form = _group_case(mpc, configs, oracle, fixture, L)
    n = len(lines)
    solo = []
    for mk in make:
        ev = mk()
        ev.compress_lines(lines, want_sizes=False, want_selected=False)
        solo.append(ev.stats_vector())
        ev.close()
    members = [mk() for mk in make]
    for ev in members:
        ev.enable_size_histogram()
    group = mpc.EvaluatorSet(members)
    assert group.form == form, group.form
    group.enable_best()
    cut = 300                                                    # an in-place call, then a staged one
    out = group.compress_lines(lines[:cut])
    out2 = group.compress_lines(lines[cut:])
    for i, (name, ev) in enumerate(zip(names, members)):
        _same(f"{name} in the group: sizes", np.concatenate([out[i][0], out2[i][0]]).astype(np.int64), want[i])
        _same(f"{name} in the group: statistics against its solo run", ev.stats_vector(), solo[i])
        _same(f"{name} in the group: histogram", ev.size_histogram(), _bincount(want[i]))
    M = np.stack(want)
    best, winner = M.min(axis=0), M.argmin(axis=0)              # argmin: the first minimal member
    k = names.index("CPACK")
    assert int((winner == k).sum()) > 0 and int(((M == best).sum(axis=0) > 1).sum()) > 0      # C-Pack wins lines; there are ties
    got = group.best()
    _same("best-of histogram", got["bins"], _bincount(best))
    assert got["wins"].tolist() == [int((winner == i).sum()) for i in range(len(names))]
    assert got["best_bits"] == int(best.sum()) and got["lines"] == n
    assert got["tag_bits"] == {4: 2, 2: 1}[len(names)]
    # the device path, sizes arrays for C-Pack only (the others: the group's scratch)
    import torch
    group.reset_best()
    for ev in members:
        ev.reset()
    d_lines = torch.from_numpy(lines).to("cuda:0")
    d_sizes = torch.zeros(n, dtype=torch.int16, device="cuda:0")
    group.compress_device(d_lines.data_ptr(), n, [d_sizes.data_ptr() if name == "CPACK" else 0 for name in names],
                          stream=torch.cuda.current_stream().cuda_stream)
    group.sync()
    torch.cuda.synchronize()
    _same("C-Pack in the group, device path: sizes", d_sizes.cpu().numpy().view(np.uint16).astype(np.int64), want[k])
    for i, (name, ev) in enumerate(zip(names, members)):
        _same(f"{name} in the group, device path: histogram", ev.size_histogram(), _bincount(want[i]))
        _same(f"{name} in the group, device path: statistics", ev.stats_vector(), solo[i])
    got = group.best()
    _same("best-of histogram, device path", got["bins"], _bincount(best))
    assert got["wins"].tolist() == [int((winner == i).sum()) for i in range(len(names))] and got["best_bits"] == int(best.sum())
    group.close()
    for ev in members:
        ev.close()


def test_solo_histogram(mpc, fixture):
    """A single handle's histogram, through the pass over its 2-byte sizes: 36-byte lines, sizes above 8 L among them."""
    c, lines, want_sizes, _, want = _case(fixture, "cpack_L36")
    assert want_sizes.max() > 8 * 36
    ev = mpc.CPACK(36)
    ev.enable_size_histogram()
    ev.compress_lines(lines[:100], want_sizes=False, want_selected=False)
    ev.compress_lines(lines[100:], want_sizes=False, want_selected=False)
    _same("histogram", ev.size_histogram(), _bincount(want_sizes))
    _same("statistics", ev.stats_vector(), want)
    ev.close()


# ---- 5. merging -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [64, 132])
def test_two_halves_merge_into_the_whole(mpc, fixture, L):
    import torch
    c, lines, want_sizes, _, want = _case(fixture, f"cpack_L{L}")
    half = len(lines) // 2 + 3
    a, b = mpc.CPACK(L), mpc.CPACK(L)
    a.compress_lines(lines[:half], want_sizes=False, want_selected=False)
    b.compress_lines(lines[half:], want_sizes=False, want_selected=False)
    va, vb = a.stats_vector(), b.stats_vector()
    assert int(va[0]) == half and int(vb[0]) == len(lines) - half
    # the raw accumulators, device to device, summed as an all-reduce would
    raws = []
    for ev in (a, b):
        raw = torch.zeros(ev.stats_raw_len(), dtype=torch.int64, device="cuda:0")
        ev.stats_copy_raw_device(raw.data_ptr())
        torch.cuda.synchronize()
        raws.append(raw.cpu().numpy().view(np.uint64))
    _same("from_raw of one half", a.stats_from_raw(raws[0]), va)
    _same("from_raw of the sum", a.stats_from_raw(raws[0] + raws[1]), want)
    a.stats_merge(vb)
    _same("merged", a.stats_vector(), want)
    b.stats_set(want)
    _same("set", b.stats_vector(), want)
    b.compress_lines(lines[:10], want_sizes=False, want_selected=False)
    assert int(b.stats_vector()[0]) == len(lines) + 10
    a.close()
    b.close()


# ---- 6. the host classes ------------------------------------------------------------------------------------------------------
def test_host_class_and_compressor_set(fixture, traces, tmp_path):
    """comp::CPACK per line, in batches, from a .npy file and as a member of a comp::CompressorSet (tests/native/
    cpack_probe.cpp): the reference's sizes and, whichever way the lines came in, the reference's Print text."""
    meta, z = fixture
    rec = next(p for p in meta["print"] if p["case"] == "cpack_L64")
    c, lines, want_sizes, _, _ = _case(fixture, "cpack_L64")
    host = os.path.join(ROOT, "cal_22-mpc_amd", "host")
    exe = str(tmp_path / "cpack_probe")
    srcs = [os.path.join(host, f) for f in sorted(os.listdir(host)) if f.endswith(".cpp") and f != "main.cpp"]
    b = subprocess.run(["hipcc", "-O2", "-std=c++17", "-Wall", "-I", host, "-I", os.path.join(ROOT, "include"), "-o", exe,
                        os.path.join(ROOT, "tests", "native", "cpack_probe.cpp"), *srcs,
                        "-L", os.path.join(ROOT, "cal_22-mpc_amd"), "-lmpc_hip",
                        "-Wl,-rpath," + os.path.join(ROOT, "cal_22-mpc_amd")], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    npy = traces.save_npy(str(tmp_path / "trace.npy"), lines)
    out = tmp_path / "out"
    out.mkdir()
    r = subprocess.run([exe, "run", npy, str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    n = len(lines) - 1                                           # the loader drops the last row
    assert r.stdout.strip().split("\n") == [f"a {n}", f"c {n}", f"d {n}", f"f {n}", "form BDI+FPC+BPC: one kernel; CPACK: own kernel"]
    _same("CompressLine's sizes", np.fromfile(out / "a.sizes", dtype=np.uint16), want_sizes[:-1])
    want_text = rec["text"].replace(rec["npy"][:-4].replace("/", "_") + ",", "probe_trace,")
    assert want_text != rec["text"] and want_text.startswith(cpack_ref.HEADER)
    for route in "acdf":
        assert (out / f"{route}.csv").read_text() == want_text, route
