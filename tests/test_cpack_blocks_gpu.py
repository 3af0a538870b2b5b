"""C-Pack with a dictionary shared by blocks of N lines on the GPU.  Every comparison is exact integer equality against the
reference's own numbers -- tests/golden/ref_cpack_block_vectors.npz (a fresh reference comp::CPACK every N lines) and, at
the two ends, tests/golden/ref_cpack_vectors.npz (N = 1: a fresh object per line; N beyond the trace: one object) -- or
against the block restatement (tests/cpack_blocks_ref.py, pinned to both by tests/test_cpack_blocks_cpu.py) where the lines
are not a fixture case's; never against per-line output of the library under test."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, pkg

import cpack_blocks_ref as B
import cpack_ref
import footprint as F

pytestmark = pytest.mark.gpu

BINS = 4096
RAGGED = (1, 63, 64, 65, 511, 512, 513)
NAMES = [c["name"] for c in B.CASES]
ORDERED = [c["name"] for c in B.ORDERED]
SHUFFLED = [c["name"] for c in B.SHUFFLED]


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
    return B.load_fixture(os.path.join(golden_dir, "ref_cpack_block_vectors.npz"))


@pytest.fixture(scope="module")
def ends(golden_dir):
    return cpack_ref.load_fixture(os.path.join(golden_dir, "ref_cpack_vectors.npz"))


@pytest.fixture(scope="module")
def inputs(fixture):
    """{case: lines}, rebuilt once and checked against the recorded digests."""
    return {c["name"]: B.case_input(c) for c in fixture[0]["cases"]}


_restated = {}


def restated(name, lines, N):
    """The restatement of a case's lines (or of `lines` under a name of the test's), computed once per (name, N)."""
    if (name, N) not in _restated:
        _restated[(name, N)] = B.compress_blocks(lines, N)
    return _restated[(name, N)]


def _vec(n, st):
    """OriginalSize, CompressedSize, TotalWords, Counts[6] of the reference -> the library's statistics vector"""
    return np.array([n] + [int(x) for x in st], dtype=np.uint64)


def _same(tag, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{tag}: {bad.size} differ, first at {bad[:6].tolist()}: {got[bad[:6]].tolist()} vs {want[bad[:6]].tolist()}"


def _bincount(sizes):
    return np.bincount(np.asarray(sizes).astype(np.int64), minlength=BINS).astype(np.uint64)


def _ragged(ev, lines, cuts=RAGGED):
    at, got = 0, []
    for n in cuts:
        got.append(ev.compress_lines(lines[at:at + n])[0])
        at += n
    got.append(ev.compress_lines(lines[at:])[0])
    return np.concatenate(got)


def _form(N):
    return f"one lane per block of {N} line" + ("" if N == 1 else "s")


# ---- 1. every fixture (case, N), one host-batch call ------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_fixture_case(mpc, fixture, inputs, name):
    meta, z = fixture
    lines = inputs[name]
    n, L = lines.shape
    for N in B.BLOCKS:
        ev = mpc.CPACK(L, dictionary="block", block_lines=N)
        assert ev.kernel_path == mpc.MPC_PATH_CPACK_BLOCKS == 10 and ev.info.algorithm == 6 and ev.info.num_clusters == 6
        assert ev.stats_len == 10 and ev.stats_raw_len() == 7 and ev.line_size == L and ev.block_lines == N and ev.dictionary == "block"
        assert ev.kernel_form == (mpc.lib().mpc_kernel_form(ev._h) or b"").decode() == _form(N)
        sizes, sel = ev.compress_lines(lines)                       # staged (more than 512 lines)
        _same(f"{name} N={N} sizes", sizes, z[f"{name}.N{N}.sizes"])
        assert not sel.any()
        want = _vec(n, z[f"{name}.N{N}.stats"])
        _same(f"{name} N={N} statistics", ev.stats_vector(), want)
        r = ev.result()
        assert r["comp_ratio"] == float(z[f"{name}.N{N}.ratio"][0])                           # the same double
        assert r["total_words"] == int(want[3]) and r["counts"] == [int(x) for x in want[4:]] and r["name"] == "C-Pack"
        assert (r["lines"], r["original_bits"], r["compressed_bits"]) == tuple(int(x) for x in want[:3])
        ev.close()


# ---- 2. the same lines in ragged calls: every cut falls inside a block ------------------------------------------------------
@pytest.mark.parametrize("name", ORDERED)
def test_ragged_calls_reset_and_restart(mpc, fixture, inputs, name):
    meta, z = fixture
    lines = inputs[name]
    n, L = lines.shape
    for N in (3, 64, 1000):
        inside = [int(a) % N != 0 for a in np.cumsum(RAGGED)]         # cuts at 1, 64, 128, 193, 704, 1216, 1729
        assert all(inside) if N != 64 else inside == [True, False, False, True, False, False, True]
        ev = mpc.CPACK(L, dictionary="block", block_lines=N)
        # calls of up to 512 lines are evaluated in place, the others staged
        _same(f"{name} N={N} sizes, ragged calls", _ragged(ev, lines), z[f"{name}.N{N}.sizes"])
        _same(f"{name} N={N} statistics, ragged calls", ev.stats_vector(), _vec(n, z[f"{name}.N{N}.stats"]))
        ev.close()
        # reset() clears the statistics and leaves the open block; restart() begins a new one
        sizes, counts = restated(name, lines, N)
        _same("the restatement is the reference", sizes, z[f"{name}.N{N}.sizes"])
        ev = mpc.CPACK(L, dictionary="block", block_lines=N)
        a, b = 700, 1501
        assert a % N and b % N
        _same("before reset", ev.compress_lines(lines[:a])[0], sizes[:a])
        ev.reset()
        assert not ev.stats_vector().any()
        _same("after reset: the open block continues", ev.compress_lines(lines[a:b])[0], sizes[a:b])
        _same("after reset: statistics of the later lines", ev.stats_vector(), cpack_ref.stats_vector(L, sizes[a:b], counts[a:b]))
        ev.restart()
        _same("after restart: a new block", ev.compress_lines(lines[:200])[0], sizes[:200])
        _same("after restart: the statistics stay", ev.stats_vector(),
              cpack_ref.stats_vector(L, sizes[a:b], counts[a:b]) + cpack_ref.stats_vector(L, sizes[:200], counts[:200]))
        ev.close()


# ---- 3. the ends ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SHUFFLED)
def test_the_ends_are_the_per_line_and_the_carried_dictionary(mpc, ends, inputs, name):
    meta, z = ends
    lines = inputs[name]
    n, L = lines.shape
    ev = mpc.CPACK(L, dictionary="block", block_lines=1)
    _same("N = 1: sizes", ev.compress_lines(lines)[0], z[name + ".sizes"])
    _same("N = 1: statistics", ev.stats_vector(), _vec(n, z[name + ".stats"]))
    ev.close()
    big = 2 ** 32 - 1
    want = _vec(n, z[name + ".carried_stats"])
    ev = mpc.CPACK(L, dictionary="block", block_lines=big)
    assert ev.block_lines == big and ev.kernel_form == _form(big)
    _same("N = 2^32 - 1: sizes", ev.compress_lines(lines)[0], z[name + ".carried"])
    _same("N = 2^32 - 1: statistics", ev.stats_vector(), want)
    ev.close()
    ev = mpc.CPACK(L, dictionary="block", block_lines=big)
    _same("N = 2^32 - 1: sizes, ragged calls", _ragged(ev, lines), z[name + ".carried"])
    _same("N = 2^32 - 1: statistics, ragged calls", ev.stats_vector(), want)
    ev.close()


# ---- 4. the other ingestion paths -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [32, 64, 128])
def test_device_npy_and_log_paths(mpc, fixture, inputs, traces, tmp_path, L):
    import torch
    meta, z = fixture
    name, N = f"cpack_order_L{L}", 16
    lines = inputs[name]
    n = len(lines)
    want_sizes, want = z[f"{name}.N{N}.sizes"], _vec(n, z[f"{name}.N{N}.stats"])
    d = torch.from_numpy(lines).to("cuda:0")
    # the device path with the caller's arrays: two calls, the cut inside a block, the second on another stream
    ev = mpc.CPACK(L, dictionary="block", block_lines=N)
    d_sizes = torch.zeros(n, dtype=torch.int16, device="cuda:0")
    d_sel = torch.full((n,), 7, dtype=torch.int8, device="cuda:0")
    cut = 777
    assert cut % N
    ev.compress_device(d.data_ptr(), cut, d_sizes.data_ptr(), d_sel.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    ev.compress_device(d.data_ptr() + cut * L, n - cut, d_sizes.data_ptr() + 2 * cut, d_sel.data_ptr() + cut)
    ev.sync()
    torch.cuda.synchronize()
    _same("device sizes", d_sizes.cpu().numpy().view(np.uint16), want_sizes)
    assert not d_sel.cpu().numpy().any()
    _same("device statistics", ev.stats_vector(), want)
    ev.close()
    # ... and without them: the histogram comes from the handle's own scratch sizes
    ev = mpc.CPACK(L, dictionary="block", block_lines=N)
    ev.enable_size_histogram()
    ev.compress_device(d.data_ptr(), cut)
    ev.compress_device(d.data_ptr() + cut * L, n - cut)
    ev.sync()
    _same("device statistics, no arrays", ev.stats_vector(), want)
    _same("device histogram, no arrays", ev.size_histogram(), _bincount(want_sizes))
    ev.close()
    # .npy: the driver never compresses the final row; a second and third call continue the numbering (cuts inside a block)
    sizes, counts = restated(name, lines, N)
    _same("the restatement is the reference", sizes, want_sizes)
    npy = traces.save_npy(str(tmp_path / "t.npy"), lines)
    ev = mpc.CPACK(L, dictionary="block", block_lines=N)
    assert ev.compress_npy(npy) == n - 1
    _same(".npy statistics", ev.stats_vector(), cpack_ref.stats_vector(L, sizes[:-1], counts[:-1]))
    ev.close()
    ev = mpc.CPACK(L, dictionary="block", block_lines=N)
    assert ev.compress_npy(npy, first_row=0, n_rows=5) == 5 and ev.compress_npy(npy, first_row=5, n_rows=600) == 600
    assert ev.compress_npy(npy, first_row=605) == n - 1 - 605
    _same(".npy statistics, three calls", ev.stats_vector(), cpack_ref.stats_vector(L, sizes[:-1], counts[:-1]))
    ev.close()
    # .log: the GLOBAL_ACC_R (0) and GLOBAL_ACC_W (4) requests, in order -- another trace, with its own blocks
    types = np.random.default_rng(3).integers(0, 9, n)
    log = traces.write_gpgpusim_log(str(tmp_path / "t.log"), lines, types)
    keep = (types == 0) | (types == 4)
    ksizes, kcounts = B.compress_blocks(np.ascontiguousarray(lines[keep]), N)
    ev = mpc.CPACK(L, dictionary="block", block_lines=N)
    assert ev.compress_gpgpusim_log(log) == (n, int(keep.sum()))
    _same(".log statistics", ev.stats_vector(), cpack_ref.stats_vector(L, ksizes, kcounts))
    ev.close()


# ---- 5. a staged chunk that ends inside a block -----------------------------------------------------------------------------
def test_chunk_cut_inside_a_block(mpc, inputs):
    """N = 96 at 64 bytes: the stager's chunks of 2^20 lines end 64 lines into a block.  One seeded 96-line block tiled to
    a little over two chunks, and a 37-line tail."""
    L, N = 64, 96
    block = np.ascontiguousarray(inputs["cpack_order_L64"][256:256 + N])          # begins with a key-0 run
    sizes, counts = B.compress_blocks(block, N)
    assert (sizes != cpack_ref.compress(block, "line")[0]).any() and (1 << 20) % N == 64
    k = (2 << 20) // N + 1
    lines = np.concatenate([np.tile(block, (k, 1)), block[:37]])
    assert 2 << 20 < len(lines) < (2 << 20) + 2 * N
    ev = mpc.CPACK(L, dictionary="block", block_lines=N)
    got = ev.compress_lines(lines, want_selected=False)[0]
    want = np.concatenate([np.tile(sizes, k), sizes[:37]])
    _same("sizes", got, want)
    v = cpack_ref.stats_vector(L, sizes, counts) * np.uint64(k) + cpack_ref.stats_vector(L, sizes[:37], counts[:37])
    _same("statistics", ev.stats_vector(), v)
    ev.close()


# ---- 6. groups and accounting -----------------------------------------------------------------------------------------------
def test_group_members_histograms_and_best_of(mpc, oracle, fixture, ends, inputs):
    L, name = 64, "cpack_L64"
    lines = inputs[name]
    n = len(lines)
    z = fixture[1]
    names = ["BDI", "FPC", "BPC", "CPACK line", "CPACK 4", "CPACK 64"]
    want = [oracle.BdiOracle(L).compress(lines)[0], oracle.FpcOracle(L).compress(lines), oracle.BpcOracle(L).compress(lines),
            ends[1][name + ".sizes"], z[name + ".N4.sizes"], z[name + ".N64.sizes"]]
    want = [np.asarray(w).astype(np.int64) for w in want]
    make = [lambda: mpc.BDI(L), lambda: mpc.FPC(L), lambda: mpc.BPC(L), lambda: mpc.CPACK(L),
            lambda: mpc.CPACK(L, dictionary="block", block_lines=4), lambda: mpc.CPACK(L, dictionary="block", block_lines=64)]
    solo = []
    for mk in make:
        ev = mk()
        ev.compress_lines(lines, want_sizes=False, want_selected=False)
        solo.append(ev.stats_vector())
        ev.close()
    _same("solo block 4 against the reference", solo[4], _vec(n, z[name + ".N4.stats"]))
    _same("solo block 64 against the reference", solo[5], _vec(n, z[name + ".N64.stats"]))
    M = np.stack(want)
    best, winner = M.min(axis=0), M.argmin(axis=0)              # argmin: the first minimal member
    assert int((winner == 5).sum()) > 0 and int((winner == 4).sum()) > 0 and int((M[5] < M[3]).sum()) > 0
    for ragged in (False, True):
        members = [mk() for mk in make]
        for ev in members:
            ev.enable_size_histogram()
        group = mpc.EvaluatorSet(members)
        assert group.form == ("BDI+FPC+BPC: one kernel; CPACK: own kernel; CPACK: own kernel, dictionary per block of 4 lines; "
                              "CPACK: own kernel, dictionary per block of 64 lines"), group.form
        group.enable_best()
        outs, at = [], 0
        for k in (RAGGED if ragged else (301,)):                 # in-place calls and staged ones; cuts inside blocks of 4 and of 64
            outs.append(group.compress_lines(lines[at:at + k]))
            at += k
        assert at % 4 and at % 64
        outs.append(group.compress_lines(lines[at:]))
        for i, (nm, ev) in enumerate(zip(names, members)):
            _same(f"{nm} in the group: sizes", np.concatenate([o[i][0] for o in outs]).astype(np.int64), want[i])
            _same(f"{nm} in the group: statistics against its solo run", ev.stats_vector(), solo[i])
            _same(f"{nm} in the group: histogram", ev.size_histogram(), _bincount(want[i]))
        got = group.best()
        _same("best-of histogram", got["bins"], _bincount(best))
        assert got["wins"].tolist() == [int((winner == i).sum()) for i in range(len(names))]
        assert got["best_bits"] == int(best.sum()) and got["lines"] == n
        if not ragged:
            # the device path, two calls with the cut inside both blocks; sizes arrays for the block members only
            import torch
            group.reset_best()
            for ev in members:
                ev.reset()
                if isinstance(ev, mpc.CPACK) and ev.block_lines:
                    ev.restart()
            d_lines = torch.from_numpy(lines).to("cuda:0")
            d_sizes = [torch.zeros(n, dtype=torch.int16, device="cuda:0") for _ in names]
            cut = 777
            group.compress_device(d_lines.data_ptr(), cut, [t.data_ptr() if i >= 4 else 0 for i, t in enumerate(d_sizes)],
                                  stream=torch.cuda.current_stream().cuda_stream)
            group.compress_device(d_lines.data_ptr() + cut * L, n - cut, [t.data_ptr() + 2 * cut if i >= 4 else 0 for i, t in enumerate(d_sizes)])
            group.sync()
            torch.cuda.synchronize()
            for i in (4, 5):
                _same(f"{names[i]} in the group, device path: sizes", d_sizes[i].cpu().numpy().view(np.uint16).astype(np.int64), want[i])
            for i, (nm, ev) in enumerate(zip(names, members)):
                _same(f"{nm} in the group, device path: histogram", ev.size_histogram(), _bincount(want[i]))
                _same(f"{nm} in the group, device path: statistics", ev.stats_vector(), solo[i])
            got = group.best()
            _same("best-of histogram, device path", got["bins"], _bincount(best))
            assert got["wins"].tolist() == [int((winner == i).sum()) for i in range(len(names))] and got["best_bits"] == int(best.sum())
        group.close()
        for ev in members:
            ev.close()


def test_merge_and_set(mpc, fixture, inputs):
    """Two aligned halves on two handles merge into the whole; stats_set installs a vector."""
    name, L, N = "cpack_order_L36", 36, 4
    lines = inputs[name]
    n = len(lines)
    want = _vec(n, fixture[1][f"{name}.N{N}.stats"])
    b0, e0 = pkg("sharded").shard_range(n, 0, 2, align=N)
    b1, e1 = pkg("sharded").shard_range(n, 1, 2, align=N)
    assert (b0, e1) == (0, n) and e0 == b1 and b1 % N == 0 and (n // 2) % N
    a, b = mpc.CPACK(L, dictionary="block", block_lines=N), mpc.CPACK(L, dictionary="block", block_lines=N)
    sa = a.compress_lines(lines[b0:e0])[0]
    sb = b.compress_lines(lines[b1:e1])[0]
    _same("the shards' sizes", np.concatenate([sa, sb]), fixture[1][f"{name}.N{N}.sizes"])
    a.stats_merge(b.stats_vector())
    _same("merged", a.stats_vector(), want)
    b.stats_set(want)
    _same("set", b.stats_vector(), want)
    a.close()
    b.close()


# ---- 7. footprint -----------------------------------------------------------------------------------------------------------
class BlockRef:
    """The block restatement over the calls of one handle (tests/footprint.py: feed / stats_vector): it keeps the line
    number and the open block's dictionary, as the handle does."""

    def __init__(self, L, N):
        self.L, self.N, self.n, self.fifo, self.total = L, N, 0, [0] * 16, np.zeros(10, np.uint64)

    def feed(self, lines):
        sizes, counts = B.compress_blocks(lines, self.N, first_line=self.n, fifo=self.fifo)
        self.n += len(lines)
        self.total = self.total + cpack_ref.stats_vector(self.L, sizes, counts)
        return sizes, np.zeros(len(lines), np.int8)

    def stats_vector(self):
        return self.total


@pytest.mark.parametrize("L,N", [(32, 3), (64, 5), (36, 1000)])
def test_footprint(mpc, inputs, L, N):
    """No byte is read outside the batch and none written outside the outputs: line counts around the wave and workgroup
    edges, the line buffer at base + 0 / + 16 / + L/2 + 16, sizes 2-byte and `selected` 1-byte aligned, every combination
    of the two optional outputs, zero and random bytes around the lines.  The handle takes every call of the sweep, so
    nearly every call begins and ends inside a block (36-byte lines: a block starts on a 4-byte boundary only)."""
    ev = mpc.CPACK(L, dictionary="block", block_lines=N)
    assert ev.kernel_path == mpc.MPC_PATH_CPACK_BLOCKS
    pool = np.ascontiguousarray(inputs[f"cpack_order_L{L}"][200:200 + 1260])
    offsets = tuple(off - off % 16 for off in F.offsets_for(L))
    calls = F.sweep(ev, [BlockRef(L, N)], pool, offsets=offsets, tag=f"CPACK blocks of {N}")
    assert calls == 2 * len(offsets) * (len(F.LINE_COUNTS) + 3 * len(F.MODE_COUNTS))
    ev.close()


# ---- 8. the host classes ------------------------------------------------------------------------------------------------------
def test_host_class_and_compressor_set(fixture, inputs, traces, tmp_path):
    """comp::CPACK(L, PerBlock, N) alone and as a member of a comp::CompressorSet, through CompressFile
    (tests/native/cpack_blocks_probe.cpp): the totals of all rows but the last, and Restart() before a second pass."""
    name, L, N = "cpack_order_L64", 64, 64
    lines = inputs[name]
    sizes, counts = restated(name, lines, N)
    _same("the restatement is the reference", sizes, fixture[1][f"{name}.N{N}.sizes"])
    host = os.path.join(ROOT, "cal_22-mpc_amd", "host")
    exe = str(tmp_path / "cpack_blocks_probe")
    srcs = [os.path.join(host, f) for f in sorted(os.listdir(host)) if f.endswith(".cpp") and f != "main.cpp"]
    b = subprocess.run(["hipcc", "-O2", "-std=c++17", "-Wall", "-I", host, "-I", os.path.join(ROOT, "include"), "-o", exe,
                        os.path.join(ROOT, "tests", "native", "cpack_blocks_probe.cpp"), *srcs,
                        "-L", os.path.join(ROOT, "cal_22-mpc_amd"), "-lmpc_hip",
                        "-Wl,-rpath," + os.path.join(ROOT, "cal_22-mpc_amd")], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    npy = traces.save_npy(str(tmp_path / "trace.npy"), lines)
    r = subprocess.run([exe, "run", npy, str(N)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    n = len(lines) - 1                                           # the loader drops the last row
    assert (n % N) != 0                                          # the second pass would continue a block without Restart()
    v = cpack_ref.stats_vector(L, sizes[:-1], counts[:-1])
    ratio = cpack_ref.comp_ratio(L, sizes[:-1])
    row = lambda route, k: f"{route} {n} " + " ".join([str(k * int(v[1])), str(k * int(v[2])), float(ratio).hex(), str(k * int(v[3]))] + [str(k * int(x)) for x in v[4:]])      # noqa: E731
    out = r.stdout.strip().split("\n")
    got = [ln.split() for ln in out]
    want = [row("d", 1).split(), row("e", 2).split(), ["blocks", str(N)], row("f", 1).split(),
            ["form", "BDI+FPC+BPC:", "one", "kernel;", "CPACK:", "own", "kernel;", "CPACK:", "own", "kernel,", "dictionary", "per", "block", "of", "64", "lines"]]
    for g, w in zip(got, want):
        if g[0] in "def":
            assert float.fromhex(g[4]) == float.fromhex(w[4]) and g[:4] + g[5:] == w[:4] + w[5:], (g, w)
        else:
            assert g == w, (g, w)
    assert len(got) == len(want)
