"""Rewrite accounting without a device: the two restatements of the table against each other and a table worked out by
hand, the identities between its entries, the C ABI's declarations, exports and bindings, the refusals that need no
handle, the command line's refusals and the report's text."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, pkg

import rewrite_ref as R

BIN = os.path.join(ROOT, "bin")
MPC_E_INVAL = -22

# L = 32, g = 8: G = 4, classes end at 64, 128 and 192 bits; (address, size) in trace order
HAND = [(0, 100),       # key 0, first touch in class 2
        (32, 300),      # key 1, first touch; above 8 L: class 4
        (0, 40),        # key 0: 2 > 1
        (4096, 64),     # key 128, first touch, on the edge of class 1
        (33, 65),       # key 1 (misaligned): 4 > 2
        (0, 40),        # key 0: 1 > 1, the same bits
        (4096, 65),     # key 128: 1 > 2, one bit over the edge
        (64, 0),        # key 2, first touch with 0 bits: class 1
        (0, 129),       # key 0: 1 > 3
        (32, 65),       # key 1: 2 > 2, the same bits
        (4127, 64),     # key 128 (misaligned): 2 > 1
        (0, 128)]       # key 0: 3 > 2


def hand_table(capacity=0):
    t = np.zeros(R.TABLE_LEN, np.uint64)
    t[:16] = [12, 1060, 4, 2, 8, 2, 4, 2, 6, 10, 257, 494, 8, capacity, 4, 0]
    t[R.FIRST:R.FIRST + 4] = [2, 1, 0, 1]
    t[R.LATEST:R.LATEST + 4] = [2, 2, 0, 0]          # latest: key 0 128, key 1 65, key 128 64, key 2 0
    t[R.PEAK:R.PEAK + 4] = [1, 1, 1, 1]              # peak: 129, 300, 65, 0
    t[R.COUNT:R.COUNT + 3] = [1, 2, 1]               # counts 5, 3, 3, 1
    for (o, c), v in {(2, 1): 2, (4, 2): 1, (1, 1): 1, (1, 2): 1, (1, 3): 1, (2, 2): 1, (3, 2): 1}.items():
        t[R.TRANS + (o - 1) * 32 + (c - 1)] = v
    return t


@pytest.fixture(scope="module")
def mpc():
    pkg("build").build_lib()
    return pkg()


# ---- the reference ---------------------------------------------------------------------------------------------------
def test_reference_by_hand():
    addrs, sizes = [a for a, _ in HAND], [s for _, s in HAND]
    R.same_table("vectorised", R.rewrite_table(addrs, sizes, 32, 8, 99), hand_table(99))
    R.same_table("loop", R.rewrite_table_loop(addrs, sizes, 32, 8, 99), hand_table(99))
    assert R.ratios(hand_table(), 32) == (2 / 8, 16 / 6, 16 / 10, 12 * 256 / 1060)
    assert [R.class_of(s, 32, 8) for s in (0, 1, 64, 65, 128, 129, 192, 193, 256, 257, 65535)] == [1, 1, 1, 2, 2, 3, 3, 4, 4, 4, 4]
    assert [R.class_of(s, 32, 32) for s in (0, 256, 257, 9999)] == [1, 1, 1, 1]                 # the native lines at 32-byte granules: one class
    assert R.class_of(97, 64, 12) == 2 and R.classes_of(64, 12) == 6 and R.class_of(600, 64, 12) == 6
    assert int(R.rewrite_table([], [], 32, 8)[:12].sum()) == 0
    assert [R.slots_of(c) for c in (1, 2, 3, 4, 5, 1000, 1 << 24)] == [2, 4, 8, 8, 16, 2048, 1 << 25]


def draws(rng, n, L, keys):
    """Repeated addresses, misaligned addresses, addresses above 2^32 and at the top; sizes on class edges and above 8 L."""
    a = rng.integers(0, keys, n).astype(np.uint64) * np.uint64(L) + np.uint64(rng.integers(0, 2)) * np.uint64(1 << 40)
    if n:
        a[::5] += rng.integers(1, L, a[::5].size).astype(np.uint64)
        a[-1] = np.uint64((1 << 64) - 1)
    return a, rng.choice([0, 3, 64, 65, 127, 128, 129, 255, 256, 257, 512, 513, 600, 1024, 1025, 1089, 2240], n)


def test_the_two_restatements_agree_and_the_identities_hold():
    rng = np.random.default_rng(3)
    for L, g in ((32, 1), (32, 8), (32, 32), (64, 8), (64, 16), (64, 24), (128, 4), (128, 32), (128, 128), (40, 7)):
        for n, keys in ((0, 1), (1, 1), (2, 1), (500, 1), (500, 40), (3000, 700), (3000, 100000)):
            a, s = draws(rng, n, L, keys)
            t = R.rewrite_table(a, s, L, g, 77)
            R.same_table(f"L={L} g={g} n={n} keys={keys}", t, R.rewrite_table_loop(a, s, L, g, 77))
            D = int(t[2])
            trans = t[R.TRANS:].reshape(32, 32).astype(np.int64)
            assert int(t[0]) == n and int(t[R.FIRST:R.FIRST + 32].sum()) == D
            assert int(trans.sum()) == n - D == int(t[4]) == int(t[5]) + int(t[6]) + int(np.trace(trans))
            assert int(np.triu(trans, 1).sum()) == int(t[5]) and int(np.tril(trans, -1).sum()) == int(t[6])
            for at in (R.LATEST, R.PEAK, R.COUNT):
                assert int(t[at:at + 32].sum()) == D
            assert int(t[9]) >= int(t[8]) and int(t[11]) >= int(t[10]) and int(t[7]) <= int(np.trace(trans))
            G = R.classes_of(L, g)
            assert int(t[14]) == G and int(trans[G:].sum()) == 0 and int(trans[:, G:].sum()) == 0 and D <= int(t[8]) <= G * D
            if n >= 500:
                assert int(t[3]) > 0 and D < n


# ---- the C ABI -------------------------------------------------------------------------------------------------------
def test_symbols_declared_exported_and_bound(mpc):
    with open(os.path.join(ROOT, "include", "mpc_hip_rewrite.h")) as f:
        hdr = f.read()
    with open(os.path.join(ROOT, "include", "mpc_hip.h")) as f:
        assert '#include "mpc_hip_rewrite.h"' in f.read()
    declared = set(re.findall(r"^(?:int|uint64_t)\s+(mpc_[a-z_]+)\s*\(", hdr, flags=re.M))
    assert declared == set(mpc.EXPORTED_REWRITE_SYMBOLS) and len(declared) == 5
    pkg("build").build_lib(test=True)
    bound = mpc.lib()
    for path in (mpc.LIB_PATH, os.path.join(ROOT, "cal_22-mpc_amd", "libmpc_hip_test.so")):
        raw = C.CDLL(path)
        for name in sorted(declared):
            assert hasattr(raw, name), f"{name} is declared in mpc_hip_rewrite.h but not exported by {path}"
    for name in sorted(declared):
        assert getattr(bound, name).argtypes is not None and getattr(bound, name).restype is C.c_int, name
    assert (mpc.MPC_REWRITE_MAX_CLASSES, mpc.MPC_REWRITE_TABLE_LEN, mpc.MPC_REWRITE_MAX_CAPACITY) == (32, 1168, 1 << 28)
    assert (R.MAX_CLASSES, R.TABLE_LEN) == (32, 1168)
    assert re.search(r"#define MPC_REWRITE_MAX_CLASSES\s+32\b", hdr)
    assert re.search(r"#define MPC_REWRITE_TABLE_LEN\s+\(144 \+ MPC_REWRITE_MAX_CLASSES \* MPC_REWRITE_MAX_CLASSES\)", hdr)
    assert re.search(r"#define MPC_REWRITE_MAX_CAPACITY\s+\(1ull << 28\)", hdr)
    for word in ("restricted to writes", "best-of member", "shards", "viction", ".npy and .txt", "-a SC2", "saturates"):       # out of scope, said in the header
        assert word in hdr, word


def test_refusals_without_a_handle(mpc):
    L = mpc.lib()
    table = np.zeros(R.TABLE_LEN, np.uint64)
    assert L.mpc_rewrite_stats_enable(None, 16, 8) == MPC_E_INVAL
    assert L.mpc_rewrite_stats_get(None, table.ctypes.data, R.TABLE_LEN) == MPC_E_INVAL
    assert L.mpc_group_rewrite_stats_enable(None, 16, 8) == MPC_E_INVAL
    assert L.mpc_group_rewrite_stats_get(None, 0, table.ctypes.data, R.TABLE_LEN) == MPC_E_INVAL


def test_enable_refusals_that_need_no_device(mpc):
    def refused(line_size, granule, capacity=16):
        with pytest.raises(mpc.MpcError) as e:
            mpc.rewrite_check_values(line_size, granule, capacity)
        assert e.value.code == MPC_E_INVAL and "rewrite accounting" in str(e.value)
        return str(e.value)

    assert "granule_bytes" in refused(32, 0)                                       # g == 0
    assert "granule_bytes" in refused(32, 33) and "32" in refused(32, 33)          # g > L
    assert "granule_bytes" in refused(128, 129)
    assert "size classes" in refused(64, 1) and "more than 32" in refused(128, 3)  # G > 32
    assert "line_size" in refused(0, 8)
    assert "capacity_lines" in refused(32, 8, 0) and "capacity_lines" in refused(32, 8, (1 << 28) + 1)
    # the accepted edges: g == L (one class), G == 32, g below a sector, a g that does not divide L, both ends of the capacity
    for args in ((32, 32, 1), (32, 1, 1 << 28), (128, 4, 3), (128, 128, 1000), (64, 2, 1 << 24), (64, 24, 2), (40, 7, 16), (8, 8, 1)):
        mpc.rewrite_check_values(*args)
    for bad in ((32, -1, 16), (32, 8, -1), (32, 8, 1 << 64), (32, 1 << 32, 16)):
        with pytest.raises(mpc.MpcError, match="unsigned"):
            mpc.rewrite_check_values(*bad)


def test_python_interface(mpc):
    import inspect
    for cls in (mpc._Evaluator, mpc.EvaluatorSet):
        p = inspect.signature(cls.enable_rewrite_stats).parameters
        assert list(p) == ["self", "granule_bytes", "capacity"]
        assert (p["granule_bytes"].default, p["capacity"].default) == (32, 1 << 24)
        assert hasattr(cls, "rewrite_stats") and hasattr(cls, "rewrite_table")
    view = mpc.rewrite_table_view(hand_table(99), 32)
    assert (view["lines"], view["bits"], view["distinct_lines"], view["misaligned"], view["rewrites"], view["grows"], view["shrinks"], view["equal_bits"]) == \
        (12, 1060, 4, 2, 8, 2, 4, 2)
    assert (view["latest_granules"], view["peak_granules"], view["latest_bits"], view["peak_bits"], view["granule_bytes"], view["capacity"], view["classes"]) == \
        (6, 10, 257, 494, 8, 99, 4)
    assert view["first"].tolist() == [2, 1, 0, 1] and view["latest_classes"].tolist() == [2, 2, 0, 0] and view["peak_classes"].tolist() == [1, 1, 1, 1]
    assert view["count_log2"].tolist() == [1, 2, 1] + [0] * 29
    assert view["trans"].tolist() == [[2, 1, 0, 1], [1, 1, 1, 0], [2, 1, 0, 0], [0, 1, 0, 0], [0, 1, 0, 0]]       # row 0: the first touches
    assert (view["overflow_rate"], view["image_granule_ratio"], view["peak_granule_ratio"], view["traffic_ratio"]) == R.ratios(hand_table(), 32)
    empty = mpc.rewrite_table_view(R.rewrite_table([], [], 32, 8), 32)
    assert (empty["overflow_rate"], empty["image_granule_ratio"], empty["peak_granule_ratio"], empty["traffic_ratio"]) == (0.0, 0.0, 0.0, 0.0)
    assert empty["trans"].shape == (5, 4)


# ---- the command line ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cli():
    pkg("build").build_all()
    return os.path.join(BIN, "compressor")


def run(cmd):
    return subprocess.run(cmd, cwd=BIN, capture_output=True, text=True, timeout=600)


def test_cli_refusals(cli, traces, tmp_path):
    d = tmp_path / "ds"
    d.mkdir()
    out = tmp_path / "out"
    out.mkdir()
    npy = traces.save_npy(str(d / "t.npy"), traces.zeros(8, 32))
    log = traces.write_gpgpusim_log(str(d / "t.log"), traces.zeros(8, 32))
    for trace, args, words in ((npy, ["--rewrites", "8"], ("--rewrites", ".log", "t.npy")),
                               (log, ["--rewrites", "0"], ("--rewrites", '"0"')),
                               (log, ["--rewrites", "eight"], ("--rewrites", '"eight"')),
                               (log, ["--rewrites=-8"], ("--rewrites", '"-8"')),
                               (log, ["--rewrites", "8", "--rewrite-capacity", "0"], ("--rewrite-capacity", "1 to 268435456", '"0"')),
                               (log, ["--rewrites", "8", "--rewrite-capacity", "268435457"], ("--rewrite-capacity", '"268435457"')),
                               (log, ["--rewrite-capacity", "8"], ("--rewrite-capacity", "--rewrites GRANULE")),
                               (log, ["--rewrites", "8", "--per-line"], ("--rewrites", "--per-line")),
                               (log, ["--rewrites", "8", "--snapshot", "64"], ("--rewrites", "--snapshot", "once")),
                               (log, ["--rewrites", "33"], ("--rewrites 33", "32-byte lines", "granule_bytes"))):      # needs the trace's line size
        for algorithm in ("BDI", "BDI,FPC"):
            if "--per-line" in args and "," in algorithm:
                continue
            r = run([cli, "-a", algorithm, "-i", trace, *args, "-o", str(out)])
            assert r.returncode == 1, (args, r.stdout, r.stderr)
            assert len(r.stdout.strip().splitlines()) == 1 and all(w in r.stdout for w in words), (args, r.stdout)
    assert os.listdir(out) == []
    for args in (["--rewrites"], ["--rewrites", "8", "--rewrite-capacity"]):
        r = run([cli, "-a", "BDI", "-i", log, *args])
        assert r.returncode == 1 and "missing an argument" in r.stdout
    text = run([cli, "-h"]).stdout
    assert "--rewrites arg" in text and "--rewrite-capacity arg" in text
    with open(os.path.join(BIN, "run")) as f:
        assert "--rewrites GRANULE" in f.read()


# ---- comp::RewriteReport ---------------------------------------------------------------------------------------------
HOST = os.path.join(ROOT, "cal_22-mpc_amd", "host")
@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("rewrite_report_probe") / "rewrite_report_probe")
    srcs = [os.path.join(ROOT, "tests", "native", "rewrite_report_probe.cpp")] + [os.path.join(HOST, f) for f in ("RewriteReport.cpp", "CompResult.cpp", "utils.cpp")]
    # host code only: the host compiler, as the other native probes of the suite are built
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "include"), "-I", HOST, *srcs, "-o", out], check=True, capture_output=True, text=True)
    return out


def test_rewrite_report_text(probe, tmp_path):
    def report(csv, workload, t, L):
        G = int(t[14])
        args = [str(int(x)) for x in t[:15]] + [f"0>{c}:{int(t[R.FIRST + c - 1])}" for c in range(1, G + 1) if int(t[R.FIRST + c - 1])]
        args += [f"{o}>{c}:{int(t[R.TRANS + (o - 1) * 32 + c - 1])}" for o in range(1, G + 1) for c in range(1, G + 1) if int(t[R.TRANS + (o - 1) * 32 + c - 1])]
        r = subprocess.run([probe, csv, str(L), workload, *args], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)

    rng = np.random.default_rng(8)
    csv = str(tmp_path / "BDI_results_rewrites.csv")
    a1, s1 = draws(rng, 3000, 32, 700)
    a2, s2 = draws(rng, 5000, 128, 900)
    t1 = R.rewrite_table(a1, s1, 32, 8, 1024)
    t2 = R.rewrite_table(a2, s2, 128, 4, 1 << 24)                     # 32 classes
    t3 = hand_table()
    assert len(np.nonzero(t1[R.TRANS:])[0]) >= 10 and len(np.nonzero(t2[R.TRANS:])[0]) >= 40
    report(csv, "ds_t", t1, 32)
    with open(csv) as f:
        assert f.read() == R.CSV_HEADER + R.csv_row("ds_t", t1, 32)
    report(csv, "ds_u", t2, 128)                   # a second report appends its row without a second header
    report(csv, "ds_v", t3, 32)
    with open(csv) as f:
        assert f.read() == R.CSV_HEADER + R.csv_row("ds_t", t1, 32) + R.csv_row("ds_u", t2, 128) + R.csv_row("ds_v", t3, 32)
    assert R.csv_row("ds_v", t3, 32) == (f"ds_v,32,8,12,4,8,2,4,2,6,10,{R.fmt_double(16 / 6)},1.6,"
                                         "0>1:2;0>2:1;0>4:1;1>1:1;1>2:1;1>3:1;2>1:2;2>2:1;3>2:1;4>2:1,\n")
    empty = str(tmp_path / "empty.csv")
    report(empty, "ds_t", R.rewrite_table([], [], 32, 8), 32)
    with open(empty) as f:
        assert f.read() == R.CSV_HEADER + "ds_t,32,8,0,0,0,0,0,0,0,0,0,0,,\n"
