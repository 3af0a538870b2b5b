"""Image accounting without a device: the numpy reference against a per-line loop, the issue's worked example and the
pack reference, the C ABI's declarations, exports and bindings, the refusals and the hash that need no handle, the
command line's refusals and the report's text."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, pkg

import image_ref as R
import pack_ref

BIN = os.path.join(ROOT, "bin")
MPC_E_INVAL = -22


@pytest.fixture(scope="module")
def mpc():
    pkg("build").build_lib()
    return pkg()


# ---- the reference ---------------------------------------------------------------------------------------------------
def test_reference_by_hand():
    # L = 32, N = 4, 32-byte sectors, no header: key 0 -> 40, key 1 -> 300, key 128 -> 256
    addrs, sizes = [0, 32, 0, 4096], [100, 300, 40, 256]
    t = R.image_table(addrs, sizes, 4, 32, 32)
    assert t[:8].tolist() == [4, 696, 3, 596, 2, 3, 3, 0]
    assert t[8:16].tolist() == [4, 32, 0, 0, 0, 0, 0, 0]
    assert t[16:20].tolist() == [1, 1, 0, 0] and int(t[20:].sum()) == 0
    assert (t == R.image_table_loop(addrs, sizes, 4, 32, 32)).all()
    assert R.ratios(t, 32) == (4 * 256 / 696, 3 * 256 / 596, 1.0)
    # 173 header bits put block 0 on 513 bits: it stays at its cap of two sectors; block 32 takes no second one
    assert R.image_table(addrs, sizes, 4, 32, 32, 173)[16:20].tolist() == [1, 1, 0, 0]
    # a misaligned address counts under its key: 33 is key 1 and overwrites it
    t = R.image_table(addrs + [33], sizes + [7], 4, 32, 32)
    assert t[:8].tolist() == [5, 703, 3, 303, 2, 2, 3, 1]
    assert int(R.image_table([], [], 4, 32, 32)[:8].sum()) == 0


def draws(rng, n, L, keys):
    """Repeated addresses, partially touched blocks, misaligned addresses, addresses above 2^32 and at the top."""
    a = rng.integers(0, keys, n).astype(np.uint64) * np.uint64(L) + np.uint64(rng.integers(0, 2)) * np.uint64(1 << 40)
    if n:
        a[::5] += rng.integers(1, L, a[::5].size).astype(np.uint64)
        a[-1] = np.uint64((1 << 64) - 1)
    return a, rng.choice([0, 3, 17, 255, 256, 257, 600, 1089, 2240], n)


def test_reference_against_a_loop():
    rng = np.random.default_rng(3)
    for N, L, sb, hb in ((1, 32, 32, 0), (1, 64, 16, 5), (2, 32, 8, 0), (3, 32, 24, 17), (5, 64, 100, 1), (33, 32, 64, 255), (64, 128, 8, 0),
                         (1000, 32, 32, 65535), (1000, 128, 128, 9), (4097, 64, 4096, 0)):
        for n, keys in ((0, 1), (1, 1), (N + 1, 2 * N), (500, 40), (3000, 700), (3000, 100000)):
            a, s = draws(rng, n, L, keys)
            got, want = R.image_table(a, s, N, L, sb, hb, 77), R.image_table_loop(a, s, N, L, sb, hb, 77)
            assert (got == want).all(), (N, L, sb, hb, n, keys)
            assert int(got[16:].sum()) == int(got[4]) and int(got[0]) == n and int(got[2]) <= n and int(got[5]) <= int(got[6])
            if n >= 500:
                assert int(got[7]) > 0 and int(got[2]) < n


def test_sequential_addresses_are_the_pack_table():
    """With addresses p L the image's blocks are pack accounting's, its tail closed as a short block."""
    rng = np.random.default_rng(4)
    for N, L, sb, hb in ((1, 32, 32, 0), (4, 32, 32, 3), (5, 64, 100, 1), (1000, 128, 128, 9)):
        for n in (N, 3 * N + N // 2 + 1, 10007):
            sizes = rng.choice([0, 3, 17, 255, 256, 257, 600, 1089, 2240], n)
            img = R.image_table(np.arange(n, dtype=np.uint64) * np.uint64(L), sizes, N, L, sb, hb)
            pk = pack_ref.pack_table(sizes, N, L, sb, hb)
            tail_sectors, tail_cap = pack_ref.tail(pk, L)
            S = pack_ref.block_sectors(N, L, sb)
            hist = pk[8:8 + S].copy()
            if tail_sectors:
                hist[tail_sectors - 1] += np.uint64(1)
            assert int(img[4]) == int(pk[0]) + (1 if int(pk[3]) else 0)                # blocks
            assert int(img[3]) == int(pk[1]) + int(pk[4]) == int(img[1])              # payload: every line is its key's latest
            assert int(img[5]) == int(pk[2]) + tail_sectors and int(img[6]) == int(pk[0]) * S + tail_cap
            assert (img[16:16 + S] == hist).all() and int(img[2]) == n


# ---- the C ABI -------------------------------------------------------------------------------------------------------
def test_symbols_declared_exported_and_bound(mpc):
    with open(os.path.join(ROOT, "include", "mpc_hip_image.h")) as f:
        hdr = f.read()
    with open(os.path.join(ROOT, "include", "mpc_hip.h")) as f:
        assert '#include "mpc_hip_image.h"' in f.read()
    declared = set(re.findall(r"^(?:int|uint64_t)\s+(mpc_[a-z_]+)\s*\(", hdr, flags=re.M))
    assert declared == set(mpc.EXPORTED_IMAGE_SYMBOLS) and len(declared) == 10
    pkg("build").build_lib(test=True)
    bound = mpc.lib()
    for path in (mpc.LIB_PATH, os.path.join(ROOT, "cal_22-mpc_amd", "libmpc_hip_test.so")):
        raw = C.CDLL(path)
        for name in sorted(declared):
            assert hasattr(raw, name), f"{name} is declared in mpc_hip_image.h but not exported by {path}"
    for name in sorted(declared):
        assert getattr(bound, name).argtypes is not None and getattr(bound, name).restype is (C.c_uint64 if name == "mpc_image_hash" else C.c_int), name
    assert (mpc.MPC_IMAGE_MAX_SECTORS, mpc.MPC_IMAGE_TABLE_LEN, mpc.MPC_IMAGE_MAX_CAPACITY) == (1024, 1040, 1 << 28)
    assert (R.MAX_SECTORS, R.TABLE_LEN) == (1024, 1040)
    assert re.search(r"#define MPC_IMAGE_MAX_SECTORS\s+1024\b", hdr) and re.search(r"#define MPC_IMAGE_TABLE_LEN\s+\(16 \+ MPC_IMAGE_MAX_SECTORS\)", hdr)
    assert re.search(r"#define MPC_IMAGE_MAX_CAPACITY\s+\(1ull << 28\)", hdr)
    for word in ("best-of image", "shards", "viction", ".npy and .txt"):       # out of scope, said in the header
        assert word in hdr, word


def test_refusals_without_a_handle(mpc):
    L = mpc.lib()
    table = np.zeros(R.TABLE_LEN, np.uint64)
    assert L.mpc_image_stats_enable(None, 16, 4, 32, 0) == MPC_E_INVAL
    assert L.mpc_image_stats_get(None, table.ctypes.data, R.TABLE_LEN) == MPC_E_INVAL
    assert L.mpc_compress_batch_addressed(None, None, 0, None, None, None) == MPC_E_INVAL
    assert L.mpc_compress_batch_device_addressed(None, None, 0, None, None, None, None) == MPC_E_INVAL
    assert L.mpc_group_image_stats_enable(None, 16, 4, 32, 0) == MPC_E_INVAL
    assert L.mpc_group_image_stats_get(None, 0, table.ctypes.data, R.TABLE_LEN) == MPC_E_INVAL
    assert L.mpc_group_compress_batch_addressed(None, None, 0, None, None, None) == MPC_E_INVAL
    assert L.mpc_group_compress_batch_device_addressed(None, None, 0, None, None, None, None) == MPC_E_INVAL


def test_enable_refusals_that_need_no_device(mpc):
    """mpc_image_check_values gives the refusals of mpc_image_stats_enable that depend on the values alone: those of
    mpc_pack_check_values, and the capacity's."""
    def refused(line_size, block_lines, sector_bytes, header_bits, capacity=16):
        with pytest.raises(mpc.MpcError) as e:
            mpc.image_check_values(line_size, block_lines, sector_bytes, header_bits, capacity)
        assert e.value.code == MPC_E_INVAL and "image accounting" in str(e.value)
        return str(e.value)

    assert "block_lines" in refused(32, 0, 32, 0)
    assert "block_lines" in refused(32, (1 << 19) + 1, 1 << 20, 0)
    assert "sector_bytes" in refused(32, 4, 0, 0)
    assert "sector_bytes" in refused(32, 4, 129, 0) and "128" in refused(32, 4, 129, 0)
    assert "1024 sectors" in refused(32, 1000, 31, 0) and "1024 sectors" in refused(128, 1000, 64, 0)
    assert "header_bits" in refused(32, 4, 32, 65536)
    assert "line_size" in refused(0, 4, 32, 0)
    assert "capacity_lines" in refused(32, 4, 32, 0, 0) and "capacity_lines" in refused(32, 4, 32, 0, (1 << 28) + 1)
    for args in ((32, 1, 32, 0, 1), (32, 1, 1, 0, 1 << 28), (32, 4, 128, 0, 3), (32, 1000, 32, 0, 1000), (128, 1000, 125, 65535, 1 << 24),
                 (64, 1 << 19, 1 << 15, 0, 2)):
        mpc.image_check_values(*args)
    for bad in ((32, -1, 32, 0, 16), (32, 4, -1, 0, 16), (32, 4, 32, -1, 16), (32, 4, 32, 0, -1), (32, 4, 32, 0, 1 << 64)):
        with pytest.raises(mpc.MpcError, match="unsigned"):
            mpc.image_check_values(*bad)


def test_hash_is_a_function_of_the_key_and_finds_slots(mpc):
    keys = [0, 1, 2, 1 << 32, (1 << 62) - 1, 12345678901234567]
    first = [mpc.image_hash(k) for k in keys]
    assert first == [mpc.image_hash(k) for k in keys] and len(set(first)) == len(keys)      # the key alone; a bijection's values differ
    assert all(0 <= h < 1 << 64 for h in first) and mpc.image_hash(0) == 0 and mpc.image_hash(1) == 0xb456bcfc34c2cb2c
    lib = mpc.lib()
    assert [int(lib.mpc_image_hash(k)) for k in keys] == first
    # keys found through it land on the intended first slot, for every capacity's table
    for capacity, slots in ((1, 2), (2, 4), (3, 8), (4, 8), (5, 16), (1000, 2048), (1 << 24, 1 << 25)):
        assert R.slots_of(capacity) == slots
        if slots > 2048:
            continue
        for slot0 in (0, slots - 1):
            found = [k for k in range(1, 40000) if mpc.image_hash(k) & (slots - 1) == slot0][:4]
            assert len(found) == 4 and all(mpc.image_hash(k) % slots == slot0 for k in found), (capacity, slot0)
    # the low bits spread: 4096 consecutive keys over 2048 slots leave no slot with more than a handful
    load = np.bincount([mpc.image_hash(k) & 2047 for k in range(4096)], minlength=2048)
    assert int(load.max()) <= 12 and int((load == 0).sum()) < 2048 // 4


def test_python_interface(mpc):
    import inspect
    for cls in (mpc._Evaluator, mpc.EvaluatorSet):
        p = inspect.signature(cls.enable_image_stats).parameters
        assert list(p) == ["self", "block_lines", "sector_bytes", "header_bits", "capacity"]
        assert (p["sector_bytes"].default, p["header_bits"].default, p["capacity"].default) == (32, 0, 1 << 24)
        for fn in (cls.compress_lines, cls.compress_device):
            assert inspect.signature(fn).parameters["addresses"].kind is inspect.Parameter.KEYWORD_ONLY
        assert hasattr(cls, "image_stats") and hasattr(cls, "image_table")
    t = R.image_table([0, 32, 0, 4096], [100, 300, 40, 256], 4, 32, 32, 0, 99)
    view = mpc.image_table_view(t, 32)
    assert (view["lines"], view["bits"], view["distinct_lines"], view["image_bits"], view["blocks"], view["sectors"], view["caps"], view["misaligned"]) == \
        (4, 696, 3, 596, 2, 3, 3, 0)
    assert (view["block_lines"], view["sector_bytes"], view["header_bits"], view["capacity"], view["block_sectors"]) == (4, 32, 0, 99, 4)
    assert view["histogram"].tolist() == [1, 1, 0, 0]
    assert (view["traffic_ratio"], view["image_ratio"], view["image_sector_ratio"]) == R.ratios(t, 32)
    empty = mpc.image_table_view(R.image_table([], [], 4, 32, 32), 32)
    assert (empty["traffic_ratio"], empty["image_ratio"], empty["image_sector_ratio"]) == (0.0, 0.0, 0.0)


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
    for trace, args, words in ((npy, ["--image", "4"], ("--image", ".log", "t.npy")),
                               (log, ["--image", "0"], ("--image", "1 to 524288", '"0"')),
                               (log, ["--image", "four"], ("--image", '"four"')),
                               (log, ["--image=-4"], ("--image", '"-4"')),
                               (log, ["--image", "524289"], ("--image", '"524289"')),
                               (log, ["--image", "4", "--image-capacity", "0"], ("--image-capacity", "1 to 268435456", '"0"')),
                               (log, ["--image", "4", "--image-capacity", "268435457"], ("--image-capacity", '"268435457"')),
                               (log, ["--image", "4", "--image-header", "65536"], ("--image-header", "0 to 65535", '"65536"')),
                               (log, ["--image-header", "8"], ("--image-header", "--image N")),
                               (log, ["--image-capacity", "8"], ("--image-capacity", "--image N")),
                               (log, ["--image", "4", "--per-line"], ("--image", "--per-line")),
                               (log, ["--image", "4", "--sector", "129"], ("--image 4", "--sector 129", "128 bytes")),      # needs the trace's line size
                               (log, ["--image", "1000", "--sector", "31"], ("--image 1000", "--sector 31", "1024 sectors"))):
        for algorithm in ("BDI", "BDI,FPC"):
            if "--per-line" in args and "," in algorithm:
                continue
            r = run([cli, "-a", algorithm, "-i", trace, *args, "-o", str(out)])
            assert r.returncode == 1, (args, r.stdout, r.stderr)
            assert len(r.stdout.strip().splitlines()) == 1 and all(w in r.stdout for w in words), (args, r.stdout)
    assert os.listdir(out) == []
    for args in (["--image"], ["--image", "4", "--image-header"], ["--image", "4", "--image-capacity"]):
        r = run([cli, "-a", "BDI", "-i", log, *args])
        assert r.returncode == 1 and "missing an argument" in r.stdout
    text = run([cli, "-h"]).stdout
    assert "--image arg" in text and "--image-header arg" in text and "--image-capacity arg" in text
    with open(os.path.join(BIN, "run")) as f:
        assert "--image N" in f.read()


# ---- comp::ImageReport ------------------------------------------------------------------------------------------------
HOST = os.path.join(ROOT, "cal_22-mpc_amd", "host")
@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("image_report_probe") / "image_report_probe")
    srcs = [os.path.join(ROOT, "tests", "native", "image_report_probe.cpp")] + [os.path.join(HOST, f) for f in ("ImageReport.cpp", "CompResult.cpp", "utils.cpp")]
    # host code only: the host compiler, as the other native probes of the suite are built
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "include"), "-I", HOST, *srcs, "-o", out], check=True, capture_output=True, text=True)
    return out


def test_image_report_text(probe, tmp_path):
    def report(csv, workload, t, L):
        S = R.ceil_div(int(t[8]) * L, int(t[9]))
        args = [str(int(x)) for x in t[:12]] + [f"{k}:{int(t[16 + k - 1])}" for k in range(1, S + 1) if int(t[16 + k - 1])]
        r = subprocess.run([probe, csv, str(L), workload, *args], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)

    rng = np.random.default_rng(8)
    csv = str(tmp_path / "BDI_results_image.csv")
    a1, s1 = draws(rng, 3000, 32, 700)
    a2, s2 = draws(rng, 5000, 128, 100000)
    t1 = R.image_table(a1, s1, 4, 32, 32, 0, 1024)
    t2 = R.image_table(a2, s2, 1000, 128, 125, 65535, 1 << 24)              # 1024 sectors a block
    t3 = R.image_table([0, 32, 0, 4096], [100, 300, 40, 256], 4, 32, 32)
    assert len(np.nonzero(t1[16:])[0]) >= 3
    report(csv, "ds_t", t1, 32)
    with open(csv) as f:
        assert f.read() == R.CSV_HEADER + R.csv_row("ds_t", t1, 32)
    report(csv, "ds_u", t2, 128)                   # a second report appends its row without a second header
    report(csv, "ds_v", t3, 32)
    with open(csv) as f:
        assert f.read() == R.CSV_HEADER + R.csv_row("ds_t", t1, 32) + R.csv_row("ds_u", t2, 128) + R.csv_row("ds_v", t3, 32)
    assert R.csv_row("ds_v", t3, 32) == f"ds_v,32,4,32,0,4,3,2,{R.fmt_double(1024 / 696)},{R.fmt_double(768 / 596)},1,1:1;2:1,\n"
    empty = str(tmp_path / "empty.csv")
    report(empty, "ds_t", R.image_table([], [], 4, 32, 32), 32)
    with open(empty) as f:
        assert f.read() == R.CSV_HEADER + "ds_t,32,4,32,0,0,0,0,0,0,0,,\n"
