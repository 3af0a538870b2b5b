"""Pack accounting without a device: the numpy reference against a per-block loop and hand-made cases, the C ABI's
declarations, exports and bindings, the refusals and helpers that need no handle, and the command line's refusals."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, pkg

import pack_ref as R

BIN = os.path.join(ROOT, "bin")
MPC_E_INVAL = -22


@pytest.fixture(scope="module")
def mpc():
    pkg("build").build_lib()
    return pkg()


# ---- the reference ---------------------------------------------------------------------------------------------------
def test_reference_by_hand():
    # 4 lines of 32 bytes a block, 32-byte sectors: 256 bits a sector, S_B = 4
    sizes = [0, 0, 0, 0, 64, 64, 64, 64, 64, 64, 64, 65, 260, 260, 260, 260, 100, 7]
    t = R.pack_table(sizes, 4, 32, 32)
    assert t[:8].tolist() == [4, 256 + 257 + 1040, 1 + 1 + 2 + 4, 2, 107, 4, 32, 0]
    assert t[8:12].tolist() == [2, 1, 0, 1] and int(t[12:].sum()) == 0
    # 3 header bits: the block of exactly 256 bits takes a second sector, the all-zero block stays at the floor of 1
    t = R.pack_table(sizes, 4, 32, 32, 3)
    assert t[:3].tolist() == [4, 1553, 1 + 2 + 2 + 4] and t[8:12].tolist() == [1, 2, 0, 1] and int(t[7]) == 3
    assert R.tail(t, 32) == (1, 2) and R.sector_ratio(t, 32) == (4 * 4 + 2) / (9 + 1) and R.sector_ratio(t, 32, close_tail=False) == 16 / 9
    # a sector that does not divide the block: S_B = ceil(96 / 40) = 3
    assert R.pack_table([300, 300, 41, 0, 0, 0], 3, 32, 40)[8:11].tolist() == [1, 0, 1]
    assert (R.pack_table([], 4, 32, 32)[[0, 1, 2, 3, 4]] == 0).all()


def test_reference_against_a_loop():
    rng = np.random.default_rng(3)
    for N, L, sb, hb in ((1, 32, 32, 0), (1, 64, 16, 5), (2, 32, 8, 0), (3, 32, 24, 17), (5, 64, 100, 1), (33, 32, 64, 255), (64, 128, 8, 0),
                         (1000, 32, 32, 65535), (1000, 128, 128, 9), (4097, 64, 4096, 0)):
        for n in (0, 1, N - 1, N, N + 1, 3 * N + N // 2, 10007):
            sizes = rng.choice([0, 3, 17, 255, 256, 257, 600, 1089, 2240], n)
            got, want = R.pack_table(sizes, N, L, sb, hb), R.pack_table_loop(sizes, N, L, sb, hb)
            assert (got == want).all(), (N, L, sb, hb, n)
            assert int(got[8:].sum()) == int(got[0]) == n // N and int(got[3]) == n % N


def test_one_line_blocks_are_the_size_sectors(mpc):
    rng = np.random.default_rng(4)
    for L, sb in ((32, 32), (64, 32), (128, 32), (64, 24), (256, 32)):
        sizes = rng.integers(0, 2300, 5000)
        t = R.pack_table(sizes, 1, L, sb, 0)
        sectors = mpc.size_sectors(np.bincount(sizes, minlength=4096).astype(np.uint64), L, sb)
        S = R.block_sectors(1, L, sb)
        assert (t[8:8 + S] == sectors["classes"]).all() and int(t[2]) == sectors["total_sectors"]
        assert mpc.pack_table_view(t, L)["sector_ratio"] == sectors["ratio"] == R.sector_ratio(t, L)


def test_sectors_of_tail(mpc):
    rng = np.random.default_rng(5)
    for N, L, sb, hb in ((4, 32, 32, 0), (1000, 32, 32, 77), (64, 128, 100, 3), (7, 64, 448, 0)):
        sizes = rng.integers(0, 600, 5 * N)
        for k in (0, 1, N - 1):
            t = R.pack_table(sizes[:2 * N + k], N, L, sb, hb)
            assert int(t[3]) == k
            assert mpc.pack_sectors_of_tail(t, L) == R.tail(t, L)
            view = mpc.pack_table_view(t, L)
            assert (view["tail_sectors"], view["tail_cap"]) == R.tail(t, L) and view["sector_ratio"] == R.sector_ratio(t, L)
            assert mpc.pack_table_view(t, L, close_tail=False)["sector_ratio"] == view["sector_ratio_closed"] == R.sector_ratio(t, L, False)
            if k == 0:
                assert R.tail(t, L) == (0, 0)
            else:
                assert R.tail(t, L)[1] == -(-k * L // sb) and 1 <= R.tail(t, L)[0] <= R.tail(t, L)[1]
    # a heavy tail is capped at its own uncompressed sectors, a light one is one sector; header bits count
    t = R.pack_table([2240] * 3, 4, 32, 32, 0)
    assert mpc.pack_sectors_of_tail(t, 32) == (3, 3)
    t = R.pack_table([100, 100, 56], 4, 32, 32, 1)
    assert mpc.pack_sectors_of_tail(t, 32) == (2, 3)
    lib = mpc.lib()
    s, c = C.c_uint64(), C.c_uint64()
    assert lib.mpc_pack_sectors_of_tail(None, R.TABLE_LEN, 32, C.byref(s), C.byref(c)) == MPC_E_INVAL
    assert lib.mpc_pack_sectors_of_tail(t.ctypes.data, R.TABLE_LEN - 1, 32, C.byref(s), C.byref(c)) == MPC_E_INVAL
    t[3] = 4                                       # open lines are below block_lines
    assert lib.mpc_pack_sectors_of_tail(t.ctypes.data, R.TABLE_LEN, 32, C.byref(s), C.byref(c)) == MPC_E_INVAL


def test_reference_merge_rules():
    rng = np.random.default_rng(6)
    N, L, sb, hb = 10, 64, 32, 4
    sizes = rng.integers(0, 600, 137)
    whole = R.pack_table(sizes, N, L, sb, hb)
    a, b, c = R.pack_table(sizes[:50], N, L, sb, hb), R.pack_table(sizes[50:100], N, L, sb, hb), R.pack_table(sizes[100:], N, L, sb, hb)
    assert (R.merge(R.merge(a, b), c) == whole).all() and int(whole[3]) == 7
    assert (R.merge(c, R.merge(a, b)) == whole).all()         # the open block is taken over from either side
    with pytest.raises(ValueError, match="open"):
        R.merge(c, c)
    for field in (5, 6, 7):
        other = b.copy()
        other[field] += 1
        with pytest.raises(ValueError, match="values"):
            R.merge(a, other)


# ---- the C ABI -------------------------------------------------------------------------------------------------------
def test_symbols_declared_exported_and_bound(mpc):
    with open(os.path.join(ROOT, "include", "mpc_hip_pack.h")) as f:
        hdr = f.read()
    with open(os.path.join(ROOT, "include", "mpc_hip.h")) as f:
        assert '#include "mpc_hip_pack.h"' in f.read()
    declared = set(re.findall(r"^int\s+(mpc_[a-z_]+)\s*\(", hdr, flags=re.M))
    assert declared == set(mpc.EXPORTED_PACK_SYMBOLS) and len(declared) == 7
    raw = C.CDLL(mpc.LIB_PATH)
    bound = mpc.lib()
    for name in sorted(declared):
        assert hasattr(raw, name), f"{name} is declared in mpc_hip_pack.h but not exported"
        assert getattr(bound, name).argtypes is not None and getattr(bound, name).restype is C.c_int, name
    assert (mpc.MPC_PACK_MAX_SECTORS, mpc.MPC_PACK_TABLE_LEN, mpc.MPC_PACK_BEST) == (1024, 1032, -1) == (R.MAX_SECTORS, R.TABLE_LEN, -1)
    assert re.search(r"#define MPC_PACK_MAX_SECTORS\s+1024\b", hdr) and re.search(r"#define MPC_PACK_BEST\s+\(-1\)", hdr)
    assert re.search(r"#define MPC_PACK_TABLE_LEN\s+\(8 \+ MPC_PACK_MAX_SECTORS\)", hdr)


def test_refusals_without_a_handle(mpc):
    L = mpc.lib()
    table = np.zeros(R.TABLE_LEN, np.uint64)
    assert L.mpc_pack_stats_enable(None, 4, 32, 0) == MPC_E_INVAL
    assert L.mpc_pack_stats_get(None, table.ctypes.data, R.TABLE_LEN) == MPC_E_INVAL
    assert L.mpc_pack_stats_merge(None, table.ctypes.data, R.TABLE_LEN) == MPC_E_INVAL
    assert L.mpc_group_pack_stats_enable(None, 4, 32, 0) == MPC_E_INVAL
    assert L.mpc_group_pack_stats_get(None, 0, table.ctypes.data, R.TABLE_LEN) == MPC_E_INVAL


def test_enable_refusals_that_need_no_device(mpc):
    """mpc_pack_check_values gives the refusals of mpc_pack_stats_enable that depend on the values alone."""
    def refused(*args):
        with pytest.raises(mpc.MpcError) as e:
            mpc.pack_check_values(*args)
        assert e.value.code == MPC_E_INVAL and "pack accounting" in str(e.value)
        return str(e.value)

    assert "block_lines" in refused(32, 0, 32, 0)
    assert "block_lines" in refused(32, (1 << 19) + 1, 1 << 20, 0) and "32 bits" in refused(32, 1 << 20, 1 << 20, 0)
    assert "sector_bytes" in refused(32, 4, 0, 0)
    assert "sector_bytes" in refused(32, 4, 129, 0) and "128" in refused(32, 4, 129, 0)      # above block_lines x line_size
    assert "1024 sectors" in refused(32, 1000, 31, 0)          # ceil(32000 / 31) = 1033
    assert "1024 sectors" in refused(128, 1000, 64, 0)
    assert "header_bits" in refused(32, 4, 32, 65536)
    assert "line_size" in refused(0, 4, 32, 0)
    # and what it accepts: one line a block, the whole block one sector, exactly 1024 sectors, the largest values
    for args in ((32, 1, 32, 0), (32, 1, 1, 0), (32, 4, 128, 0), (32, 1000, 32, 0), (32, 1024, 32, 65535), (128, 1000, 125, 0),
                 (64, 1 << 19, 1 << 15, 0)):
        mpc.pack_check_values(*args)
    for bad in ((32, -1, 32, 0), (32, 4, -1, 0), (32, 4, 32, -1), (32, 1 << 64, 32, 0), (32, 4, 1 << 32, 0)):
        with pytest.raises(mpc.MpcError, match="unsigned"):
            mpc.pack_check_values(*bad)


def test_python_interface(mpc):
    import inspect
    for cls in (mpc._Evaluator, mpc.EvaluatorSet):
        p = inspect.signature(cls.enable_pack_stats).parameters
        assert list(p) == ["self", "block_lines", "sector_bytes", "header_bits"] and p["sector_bytes"].default == 32 and p["header_bits"].default == 0
        assert inspect.signature(cls.pack_stats).parameters["close_tail"].default is True
    assert hasattr(mpc._Evaluator, "pack_table") and hasattr(mpc._Evaluator, "pack_stats_merge") and hasattr(mpc.EvaluatorSet, "pack_table")
    t = R.pack_table([10, 20, 300, 40, 50, 60, 7], 3, 32, 16, 2)
    view = mpc.pack_table_view(t, 32)
    assert view["block_sectors"] == 6 and view["blocks"] == 2 and view["payload_bits"] == 480 and view["sectors"] == 3 + 2
    assert view["histogram"].tolist() == [0, 1, 1, 0, 0, 0] and (view["open_lines"], view["open_bits"]) == (1, 7)
    assert (view["block_lines"], view["sector_bytes"], view["header_bits"]) == (3, 16, 2)
    assert (view["tail_sectors"], view["tail_cap"]) == (1, 2) and view["sector_ratio"] == 14 / 6 and view["sector_ratio_closed"] == 12 / 5


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
    for args, words in ((["--pack", "0"], ("--pack", "1 to 524288", '"0"')),
                        (["--pack", "four"], ("--pack", '"four"')),
                        (["--pack=-4"], ("--pack", '"-4"')),
                        (["--pack", "524289"], ("--pack", '"524289"')),
                        (["--pack", "4x"], ("--pack", '"4x"')),
                        (["--pack", "4", "--pack-header", "65536"], ("--pack-header", "0 to 65535", '"65536"')),
                        (["--pack", "4", "--pack-header=-1"], ("--pack-header", '"-1"')),
                        (["--pack", "4", "--pack-header", "bits"], ("--pack-header", '"bits"')),
                        (["--pack-header", "8"], ("--pack-header", "--pack N")),
                        (["--pack", "4", "--per-line"], ("--pack", "--per-line")),
                        (["--pack", "4", "--sector", "129"], ("--pack 4", "--sector 129", "128 bytes")),      # needs the trace's line size
                        (["--pack", "1000", "--sector", "31"], ("--pack 1000", "--sector 31", "1024 sectors"))):
        for algorithm in ("BDI", "BDI,FPC"):
            if "--per-line" in args and "," in algorithm:
                continue
            r = run([cli, "-a", algorithm, "-i", npy, *args, "-o", str(out)])
            assert r.returncode == 1, (args, r.stdout, r.stderr)
            assert len(r.stdout.strip().splitlines()) == 1 and all(w in r.stdout for w in words), (args, r.stdout)
    assert os.listdir(out) == []
    r = run([cli, "-a", "BDI", "-i", npy, "--pack"])
    assert r.returncode == 1 and "missing an argument" in r.stdout
    r = run([cli, "-a", "BDI", "-i", npy, "--pack", "4", "--pack-header"])
    assert r.returncode == 1 and "missing an argument" in r.stdout
    text = run([cli, "-h"]).stdout
    assert "--pack arg" in text and "--pack-header arg" in text
    with open(os.path.join(BIN, "run")) as f:
        assert "--pack N" in f.read()


# ---- comp::PackReport -------------------------------------------------------------------------------------------------
HOST = os.path.join(ROOT, "cal_22-mpc_amd", "host")
CSV_HEADER = "Workload,Line Size,Block Lines,Sector Bytes,Header Bits,Blocks,Tail Lines,Sector Ratio,Histogram,\n"


def fmt_double(x: float) -> str:
    """The host code's text of a double (mpctext::num): shortest round-trip, no trailing ".0"."""
    r = repr(float(x))
    return r[:-2] if r.endswith(".0") else r


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("pack_report_probe") / "pack_report_probe")
    srcs = [os.path.join(ROOT, "tests", "native", "pack_report_probe.cpp")] + [os.path.join(HOST, f) for f in ("PackReport.cpp", "CompResult.cpp", "utils.cpp")]
    # host code only: the host compiler, as the other native probes of the suite are built
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "include"), "-I", HOST, *srcs, "-o", out], check=True, capture_output=True, text=True)
    return out


def test_pack_report_text(probe, tmp_path):
    def row(workload, t, L):
        S = R.block_sectors(t[5], L, t[6])
        hist = ";".join(f"{k}:{int(t[8 + k - 1])}" for k in range(1, S + 1) if int(t[8 + k - 1]))
        return f"{workload},{L},{int(t[5])},{int(t[6])},{int(t[7])},{int(t[0])},{int(t[3])},{fmt_double(R.sector_ratio(t, L))},{hist},\n"

    def report(csv, workload, t, L):
        S = R.block_sectors(t[5], L, t[6])
        args = [str(int(x)) for x in t[:8]] + [f"{k}:{int(t[8 + k - 1])}" for k in range(1, S + 1) if int(t[8 + k - 1])]
        r = subprocess.run([probe, csv, str(L), workload, *args], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)

    rng = np.random.default_rng(8)
    csv = str(tmp_path / "BDI_results_pack.csv")
    t1 = R.pack_table(rng.integers(0, 600, 1003), 4, 32, 32, 0)            # a tail of three lines
    t2 = R.pack_table(rng.integers(0, 2300, 5000), 1000, 128, 125, 65535)   # 1024 sectors a block, no tail
    t3 = R.pack_table([5, 6], 4, 32, 32, 9)                                 # nothing closed: the ratio is the tail's
    assert int(t1[3]) == 3 and int(t2[3]) == 0 and len(np.nonzero(t1[8:])[0]) >= 3 and int(t3[0]) == 0
    report(csv, "ds_t", t1, 32)
    with open(csv) as f:
        assert f.read() == CSV_HEADER + row("ds_t", t1, 32)
    report(csv, "ds_u", t2, 128)                   # a second report appends its row without a second header
    report(csv, "ds_v", t3, 32)
    with open(csv) as f:
        assert f.read() == CSV_HEADER + row("ds_t", t1, 32) + row("ds_u", t2, 128) + row("ds_v", t3, 32)
    assert row("ds_v", t3, 32) == "ds_v,32,4,32,9,0,2,2,,\n"
    empty = str(tmp_path / "empty.csv")
    report(empty, "ds_t", R.pack_table([], 4, 32, 32, 0), 32)
    with open(empty) as f:
        assert f.read() == CSV_HEADER + "ds_t,32,4,32,0,0,0,0,,\n"
