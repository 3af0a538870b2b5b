"""Snapshots without a device: the dict-loop reference against the numpy one, the plan identities, the C ABI's
declarations, exports and bindings, the refusals that need no device, the command line's refusals and the report's
text."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, pkg

import snapshot_ref as R

BIN = os.path.join(ROOT, "bin")
HOST = os.path.join(ROOT, "cal_22-mpc_amd", "host")
MPC_E_INVAL = -22


@pytest.fixture(scope="module")
def mpc():
    pkg("build").build_lib()
    return pkg()


# ---- the reference ---------------------------------------------------------------------------------------------------
def test_reference_by_hand():
    U = 32
    unit = lambda v: np.full(U, v, dtype=np.uint8)
    # keys 0, 1 (line 0 of 64 bytes, complete), key 5 (line 2, unit 1 alone), key 0 rewritten, and a misaligned address of key 1
    units = np.stack([unit(1), unit(2), unit(3), unit(4), unit(5)])
    addrs = np.array([0, 32, 5 * 32, 0, 32 + 7], dtype=np.uint64)
    for snap in (R.LoopSnapshot(U, 8),):
        snap.add(units, addrs)
        assert snap.stats() == {"units": 5, "distinct_units": 3, "misaligned": 1, "capacity": 8, "unit_bytes": 32}
        assert snap.plan(64, "skip") == dict(zip(R.PLAN_KEYS, (2, 1, 1, 1, 1, 1)))
        assert snap.plan(64, "zero") == dict(zip(R.PLAN_KEYS, (2, 1, 1, 1, 1, 2)))
        lines, la, pres = snap.read(64, "zero")
        assert la.tolist() == [0, 128] and pres.tolist() == [3, 2]
        assert lines[0].tolist() == [4] * 32 + [5] * 32 and lines[1].tolist() == [0] * 32 + [3] * 32
        lines, la, pres = snap.read(64, "skip")
        assert la.tolist() == [0] and pres.tolist() == [3] and lines[0].tolist() == [4] * 32 + [5] * 32
        lines, la, pres = snap.read(32, "skip")
        assert la.tolist() == [0, 32, 160] and pres.tolist() == [1, 1, 1] and lines[:, 0].tolist() == [4, 5, 3]
    assert R.stats(units, addrs, U, 8) == snap.stats()


def drawn(rng, U, n, keys, hi=False):
    units = rng.integers(0, 256, (n, U), dtype=np.uint8)
    base = np.uint64(0x7fff00000000 if hi else 0)
    addrs = base + rng.integers(0, keys, n).astype(np.uint64) * np.uint64(U)
    addrs[::5] += rng.integers(1, U, addrs[::5].size).astype(np.uint64)
    return units, addrs


def test_reference_against_a_loop():
    rng = np.random.default_rng(5)
    for U in R.UNITS:
        for n, keys in ((0, 1), (1, 1), (40, 7), (500, 300), (900, 64)):
            units, addrs = drawn(rng, U, n, keys, hi=n == 500)
            loop = R.LoopSnapshot(U, 1024)
            cut = n // 3
            loop.add(units[:cut], addrs[:cut])          # calls do not matter: positions run across them
            loop.add(units[cut:], addrs[cut:])
            assert loop.stats() == R.stats(units, addrs, U, 1024)
            for k in R.KS:
                L = k * U
                if L > R.MAX_LINE:
                    continue
                for partial in ("skip", "zero"):
                    p = R.plan(units, addrs, U, L, partial, 1024)
                    assert p == loop.plan(L, partial), (U, n, L, partial)
                    R.plan_identities(p, k, loop.stats()["distinct_units"], partial)
                    a, b = R.read(units, addrs, U, L, partial, 1024), loop.read(L, partial)
                    for x, y in zip(a, b):
                        assert x.dtype == y.dtype and x.shape == y.shape and (x == y).all(), (U, n, L, partial)
                    assert len(a[0]) == p["n_out"] and (np.diff(a[1].astype(object)) > 0).all()
                    if partial == "skip":
                        assert (a[2] == (1 << k) - 1).all()


def test_reference_capacity():
    rng = np.random.default_rng(6)
    units = rng.integers(0, 256, (9, 32), dtype=np.uint8)
    addrs = np.arange(9, dtype=np.uint64) * np.uint64(32)
    loop = R.LoopSnapshot(32, 8)
    loop.add(units[:8], addrs[:8])
    loop.add(units[:8], addrs[:8])                      # known keys are no new ones
    assert R.stats(np.concatenate([units[:8]] * 2), np.concatenate([addrs[:8]] * 2), 32, 8)["distinct_units"] == 8
    with pytest.raises(R.Overflow):
        loop.add(units[8:], addrs[8:])
    with pytest.raises(R.Overflow):
        R.latest(units, addrs, 32, 8)


# ---- the C ABI -------------------------------------------------------------------------------------------------------
def test_symbols_declared_exported_and_bound(mpc):
    with open(os.path.join(ROOT, "include", "mpc_hip_snapshot.h")) as f:
        hdr = f.read()
    with open(os.path.join(ROOT, "include", "mpc_hip.h")) as f:
        assert '#include "mpc_hip_snapshot.h"' in f.read()
    declared = set(re.findall(r"^(?:int|void|const char \*)\s*(mpc_[a-z_]+)\s*\(", hdr, flags=re.M))
    assert declared == set(mpc.EXPORTED_SNAPSHOT_SYMBOLS) and len(declared) == 14
    pkg("build").build_lib(test=True)
    bound = mpc.lib()
    for path in (mpc.LIB_PATH, os.path.join(ROOT, "cal_22-mpc_amd", "libmpc_hip_test.so")):
        raw = C.CDLL(path)
        for name in sorted(declared):
            assert hasattr(raw, name), f"{name} is declared in mpc_hip_snapshot.h but not exported by {path}"
    for name in sorted(declared):
        want = {"mpc_snapshot_destroy": None, "mpc_snapshot_last_error": C.c_char_p}.get(name, C.c_int)
        assert getattr(bound, name).argtypes is not None and getattr(bound, name).restype is want, name
    assert (mpc.MPC_SNAPSHOT_MAX_CAPACITY, mpc.MPC_SNAPSHOT_TABLE_LEN, mpc.SNAPSHOT_PARTIAL) == (1 << 28, 8, {"skip": 0, "zero": 1})
    assert re.search(r"#define MPC_SNAPSHOT_MAX_CAPACITY\s+\(1ull << 28\)", hdr) and re.search(r"#define MPC_SNAPSHOT_MAX_LINE\s+256\b", hdr)
    assert re.search(r"#define MPC_SNAPSHOT_PARTIAL_SKIP\s+0\b", hdr) and re.search(r"#define MPC_SNAPSHOT_PARTIAL_ZERO\s+1\b", hdr)
    for word in ("16 + U bytes per slot", "1.5 GiB", "as of", "viction", ".npy and", "shards"):       # the memory and what is out of scope, said in the header
        assert word in hdr, word


def test_refusals_without_a_snapshot(mpc):
    L = mpc.lib()
    t = np.zeros(8, np.uint64)
    assert L.mpc_snapshot_create(32, 16, -1, None) == MPC_E_INVAL
    assert L.mpc_snapshot_reset(None) == MPC_E_INVAL
    assert L.mpc_snapshot_add(None, None, 0, None) == MPC_E_INVAL
    assert L.mpc_snapshot_add_device(None, None, 0, None, None) == MPC_E_INVAL
    assert L.mpc_snapshot_add_gpgpusim_log(None, b"x.log", None) == MPC_E_INVAL
    assert L.mpc_snapshot_stats(None, t.ctypes.data) == MPC_E_INVAL
    assert L.mpc_snapshot_plan(None, 32, 0, t.ctypes.data) == MPC_E_INVAL
    assert L.mpc_snapshot_write_lines(None, 32, 0, 0, 0, None, None, None, None) == MPC_E_INVAL
    assert L.mpc_snapshot_read_lines(None, 32, 0, 0, 0, None, None, None) == MPC_E_INVAL
    assert L.mpc_snapshot_evaluate(None, None, 32, 0, 0) == MPC_E_INVAL
    assert L.mpc_snapshot_evaluate_group(None, None, 32, 0, 0) == MPC_E_INVAL
    L.mpc_snapshot_destroy(None)


def test_check_values(mpc):
    """mpc_snapshot_check_values gives the refusals of a create and of a plan that depend on the values alone, and the
    reference knows the same ones."""
    def refused(U, capacity, L=0):
        with pytest.raises(mpc.MpcError) as e:
            mpc.snapshot_check_values(U, capacity, L)
        assert e.value.code == MPC_E_INVAL and "snapshot" in str(e.value)
        assert R.check_values(U, capacity, L) in str(e.value), (U, capacity, L, str(e.value))
        return str(e.value)

    for U in (0, 16, 48, 96, 256):
        assert "unit_bytes" in refused(U, 16) and str(U) in refused(U, 16)
    assert "capacity_units" in refused(32, 0) and "capacity_units" in refused(128, (1 << 28) + 1)
    for U, L in ((32, 16), (32, 48), (32, 96), (32, 160), (64, 32), (64, 192), (128, 64), (128, 384)):
        assert "is not 1, 2, 4 or 8 units" in refused(U, 16, L) or L > 256
    for U, L in ((32, 512), (64, 512), (128, 512), (128, 1024), (32, 288)):
        assert "above 256" in refused(U, 16, L)
    for U in R.UNITS:
        for capacity in (1, 8, 1 << 24, 1 << 28):
            mpc.snapshot_check_values(U, capacity)
            for k in R.KS:
                if k * U <= 256:
                    mpc.snapshot_check_values(U, capacity, k * U)
                    assert R.check_values(U, capacity, k * U) is None
    for bad in ((-1, 16, 0), (32, -1, 0), (32, 16, -1), (32, 1 << 64, 0)):
        with pytest.raises(mpc.MpcError, match="unsigned"):
            mpc.snapshot_check_values(*bad)
    with pytest.raises(mpc.MpcError, match="unit_bytes"):        # the constructor refuses before it looks for a device
        mpc.Snapshot(48, 16)
    with pytest.raises(mpc.MpcError, match="capacity_units"):
        mpc.Snapshot(32, 0)


def test_python_interface(mpc):
    import inspect
    S = mpc.Snapshot
    p = inspect.signature(S.__init__).parameters
    assert list(p) == ["self", "unit_bytes", "capacity", "device"] and (p["unit_bytes"].default, p["capacity"].default, p["device"].default) == (32, 1 << 24, -1)
    assert list(inspect.signature(S.add).parameters) == ["self", "units", "addresses"]
    assert list(inspect.signature(S.add_device).parameters) == ["self", "d_units", "n", "d_addresses", "stream"]
    assert list(inspect.signature(S.plan).parameters) == ["self", "line_size", "partial"] and inspect.signature(S.plan).parameters["partial"].default == "skip"
    p = inspect.signature(S.evaluate).parameters
    assert list(p) == ["self", "evaluator_or_set", "line_size", "partial", "by_presence"] and (p["partial"].default, p["by_presence"].default) == ("skip", False)
    assert inspect.signature(S.read_lines).parameters["partial"].default == "skip"
    for name in ("add_gpgpusim_log", "stats", "write_lines", "reset", "close"):
        assert callable(getattr(S, name))
    with pytest.raises(ValueError, match="partial"):
        mpc._snapshot_partial("drop")


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
    log64 = traces.write_gpgpusim_log(str(d / "u.log"), traces.zeros(8, 64))
    for trace, args, words in ((npy, ["--snapshot", "128"], ("--snapshot", ".log", "t.npy")),
                               (log, ["--snapshot", "0"], ("--snapshot", "at most 256", '"0"')),
                               (log, ["--snapshot", "wide"], ("--snapshot", '"wide"')),
                               (log, ["--snapshot=-128"], ("--snapshot", '"-128"')),
                               (log, ["--snapshot", "512"], ("--snapshot", '"512"')),
                               (log, ["--snapshot", "96"], ("--snapshot 96", "32-byte requests", "is not 1, 2, 4 or 8 units")),      # needs the trace's line size
                               (log64, ["--snapshot", "32"], ("--snapshot 32", "64-byte requests", "is not 1, 2, 4 or 8 units")),
                               (log, ["--snapshot", "128", "--snapshot-partial", "drop"], ("--snapshot-partial", "skip or zero", '"drop"')),
                               (log, ["--snapshot", "128", "--snapshot-capacity", "0"], ("--snapshot-capacity", "1 to 268435456", '"0"')),
                               (log, ["--snapshot", "128", "--snapshot-capacity", "268435457"], ("--snapshot-capacity", '"268435457"')),
                               (log, ["--snapshot-partial", "zero"], ("--snapshot-partial", "--snapshot L")),
                               (log, ["--snapshot-capacity", "8"], ("--snapshot-capacity", "--snapshot L")),
                               (log, ["--snapshot", "128", "--per-line"], ("--snapshot", "--per-line")),
                               (log, ["--snapshot", "128", "--by", "kernel"], ("--by kernel", "--snapshot", "no single record")),
                               (log, ["--snapshot", "128", "--by", "rw"], ("--by rw", "--snapshot", "no single record")),
                               (log, ["--snapshot", "128", "--by", "mftype"], ("--by mftype", "--snapshot", "no single record")),
                               (log, ["--snapshot", "128", "--sector", "129"], ("--sector 129", "128-byte lines"))):      # sectors are checked against the snapshot's lines
        for algorithm in ("BDI", "BDI,FPC"):
            if "--per-line" in args and "," in algorithm:
                continue
            r = run([cli, "-a", algorithm, "-i", trace, *args, "-o", str(out)])
            assert r.returncode == 1, (args, r.stdout, r.stderr)
            assert len(r.stdout.strip().splitlines()) == 1 and all(w in r.stdout for w in words), (args, r.stdout)
    assert os.listdir(out) == []
    for args in (["--snapshot"], ["--snapshot", "128", "--snapshot-partial"], ["--snapshot", "128", "--snapshot-capacity"]):
        r = run([cli, "-a", "BDI", "-i", log, *args])
        assert r.returncode == 1 and "missing an argument" in r.stdout
    text = run([cli, "-h"]).stdout
    assert "--snapshot arg" in text and "--snapshot-partial arg" in text and "--snapshot-capacity arg" in text


# ---- the report's text -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("snapshot_report_probe") / "snapshot_report_probe")
    srcs = [os.path.join(ROOT, "tests", "native", "snapshot_report_probe.cpp")] + [os.path.join(HOST, f) for f in ("SnapshotReport.cpp", "CompResult.cpp", "utils.cpp")]
    # host code only: the host compiler, as the other native probes of the suite are built
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "include"), "-I", HOST, *srcs, "-o", out], check=True, capture_output=True, text=True)
    return out


def test_snapshot_report_text(probe, tmp_path):
    rng = np.random.default_rng(9)
    csv = str(tmp_path / "BDI_results_snapshot.csv")
    want = R.CSV_HEADER
    for U, L, partial, n, keys in ((32, 128, "skip", 700, 400), (32, 128, "zero", 700, 400), (64, 128, "zero", 90, 300), (128, 256, "skip", 0, 1),
                                   (32, 32, "skip", 50, 20)):
        units, addrs = drawn(rng, U, n, keys)
        st, p = R.stats(units, addrs, U, 1 << 24), R.plan(units, addrs, U, L, partial)
        args = [str(st[k]) for k in ("units", "distinct_units", "misaligned", "capacity", "unit_bytes")] + [str(p[k]) for k in R.PLAN_KEYS]
        r = subprocess.run([probe, csv, str(L), partial, f"ds_t@snapshot{L}", *args], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
        want += R.csv_row(f"ds_t@snapshot{L}", U, L, partial, st, p)
    with open(csv) as f:
        assert f.read() == want
    assert want.splitlines()[1] != want.splitlines()[2] and want.count("\n") == 6
    # the largest counts a table can hold print as integers
    big = str(tmp_path / "big.csv")
    top = (1 << 64) - 1
    r = subprocess.run([probe, big, "256", "zero", "w", *([str(top)] * 4), "128", *([str(top)] * 6)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    with open(big) as f:
        assert f.read() == R.CSV_HEADER + f"w,128,256,zero,{top},{top},{top},{top},{top},{top},{top},{top},\n"
