"""Per-class accounting without a device: the numpy reference against hand-made cases, the C ABI's declarations,
exports and bindings, the refusals that need no handle, the command line's refusals and comp::ClassReport's text."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, pkg

import classes_ref as R


def fmt_double(x: float) -> str:
    """The host code's text of a double (mpctext::num): shortest round-trip, no trailing ".0"."""
    r = repr(float(x))
    return r[:-2] if r.endswith(".0") else r


HOST = os.path.join(ROOT, "cal_22-mpc_amd", "host")
BIN = os.path.join(ROOT, "bin")
MPC_E_INVAL = -22
HEADER = "Workload,Class,Lines,Original Bits,Compressed Bits,Ratio,Sector Ratio,\n"


@pytest.fixture(scope="module")
def mpc():
    pkg("build").build_lib()
    return pkg()


# ---- the reference table ---------------------------------------------------------------------------------------------
def test_reference_sectors_by_hand():
    # 64-byte lines, 32-byte sectors: 256 bits a sector, S = 2
    sizes = [0, 1, 256, 257, 512, 513, 4095]
    assert R.sectors_of(sizes, 64, 32).tolist() == [1, 1, 1, 2, 2, 2, 2]
    # 128-byte lines: S = 4; exactly 8 x sector_bytes, one more, above S sectors, 4095
    assert R.sectors_of([0, 256, 257, 768, 769, 1024, 1025, 4095], 128, 32).tolist() == [1, 1, 2, 3, 4, 4, 4, 4]
    # a sector size that does not divide the line: S = ceil(64 / 24) = 3
    assert R.sectors_of([192, 193, 384, 385, 600], 64, 24).tolist() == [1, 2, 2, 3, 3]
    # one sector a line
    assert R.sectors_of([0, 300, 4095], 32, 32).tolist() == [1, 1, 1]


def test_reference_table_by_hand():
    classes = [0, 0, 7, 7, 7, 255, 0]
    sizes = [0, 256, 257, 4095, 12, 513, 300]
    t = R.class_table(classes, sizes, 64, 32)
    assert t.dtype == np.uint64 and t.shape == (256, 10)
    assert t[0].tolist() == [3, 556, 2, 1, 0, 0, 0, 0, 0, 0]
    assert t[7].tolist() == [3, 4364, 1, 2, 0, 0, 0, 0, 0, 0]
    assert t[255].tolist() == [1, 513, 0, 1, 0, 0, 0, 0, 0, 0]
    assert int(t.sum()) == int(t[[0, 7, 255]].sum())
    # column 0 is the sum of the sector columns, whatever the sizes
    rng = np.random.default_rng(2)
    t = R.class_table(rng.integers(0, 256, 5000), rng.integers(0, 4096, 5000), 128, 16)
    assert (t[:, 2:].sum(axis=1) == t[:, 0]).all() and int(t[:, 0].sum()) == 5000
    assert (R.class_table([], [], 64, 32) == 0).all()
    assert R.classes_of_selected(np.array([-1, 0, 5], np.int8)).tolist() == [0, 1, 6]


# ---- the C ABI -------------------------------------------------------------------------------------------------------
def test_symbols_declared_exported_and_bound(mpc):
    with open(os.path.join(ROOT, "include", "mpc_hip_classes.h")) as f:
        hdr = f.read()
    with open(os.path.join(ROOT, "include", "mpc_hip.h")) as f:
        assert '#include "mpc_hip_classes.h"' in f.read()
    declared = set(re.findall(r"^int\s+(mpc_[a-z_]+)\s*\(", hdr, flags=re.M))
    assert declared == set(mpc.EXPORTED_CLASS_SYMBOLS) and len(declared) == 13
    raw = C.CDLL(mpc.LIB_PATH)
    bound = mpc.lib()
    for name in sorted(declared):
        assert hasattr(raw, name), f"{name} is declared in mpc_hip_classes.h but not exported"
        assert getattr(bound, name).argtypes is not None and getattr(bound, name).restype is C.c_int, name
    assert (mpc.MPC_CLASS_COUNT, mpc.MPC_CLASS_ROW, mpc.MPC_CLASS_TABLE_LEN, mpc.MPC_CLASS_BEST) == (256, 10, 2560, -1)
    for macro, value in (("MPC_CLASS_COUNT", 256), ("MPC_CLASS_ROW", 10), ("MPC_CLASS_LOG_NONE", 0), ("MPC_CLASS_LOG_KERNEL", 1),
                         ("MPC_CLASS_LOG_RW", 2), ("MPC_CLASS_LOG_MFTYPE", 3)):
        assert re.search(rf"#define {macro}\s+{value}\b", hdr), macro
    assert mpc.CLASS_LOG_FIELDS == {None: 0, "kernel": 1, "rw": 2, "mftype": 3}


def test_refusals_without_a_handle(mpc):
    L = mpc.lib()
    table = np.zeros(2560, np.uint64)
    b = C.c_uint()
    assert L.mpc_class_stats_enable(None, 32) == MPC_E_INVAL
    assert L.mpc_class_stats_get(None, table.ctypes.data, 2560) == MPC_E_INVAL
    assert L.mpc_class_stats_merge(None, table.ctypes.data, 2560) == MPC_E_INVAL
    assert L.mpc_class_sector_bytes(None, C.byref(b)) == MPC_E_INVAL
    assert L.mpc_class_log_field(None, 1) == MPC_E_INVAL
    assert L.mpc_compress_batch_classed(None, None, 0, None, None, None) == MPC_E_INVAL
    assert L.mpc_compress_batch_device_classed(None, None, 0, None, None, None, None) == MPC_E_INVAL
    assert L.mpc_group_class_stats_enable(None, 32) == MPC_E_INVAL
    assert L.mpc_group_class_stats_get(None, 0, table.ctypes.data, 2560) == MPC_E_INVAL
    assert L.mpc_group_compress_batch_classed(None, None, 0, None, None, None) == MPC_E_INVAL
    assert L.mpc_group_compress_batch_device_classed(None, None, 0, None, None, None, None) == MPC_E_INVAL
    assert L.mpc_group_class_log_field(None, 1) == MPC_E_INVAL
    assert L.mpc_group_class_from_member(None, 0) == MPC_E_INVAL


def test_python_argument_checks(mpc):
    assert mpc._as_classes([0, 255, 3], 3).dtype == np.uint8
    assert mpc._as_classes(np.array([True, False]), 2).tolist() == [1, 0]
    for bad, n in (([0, 256], 2), ([-1, 0], 2), ([0.5, 1.0], 2), ([1, 2, 3], 2), ([[1, 2]], 2)):
        with pytest.raises(ValueError):
            mpc._as_classes(bad, n)
    with pytest.raises(ValueError):
        mpc._class_log_field("address")
    t = np.arange(2560, dtype=np.uint64)
    view = mpc.class_table_view(t, 128, 32)
    assert view["lines"].shape == (256,) and view["bits"][1] == 11 and view["sectors"].shape == (256, 4)
    assert view["sectors"][2].tolist() == [22, 23, 24, 25]
    # keyword-only, defaults and positional order unchanged
    import inspect
    for cls in (mpc._Evaluator, mpc.EvaluatorSet):
        p = inspect.signature(cls.compress_lines).parameters
        assert list(p)[:4] == ["self", "lines", "want_sizes", "want_selected"] and p["classes"].kind is inspect.Parameter.KEYWORD_ONLY
        assert p["classes"].default is None and p["want_sizes"].default is True
        p = inspect.signature(cls.compress_device).parameters
        assert list(p)[:5] == ["self", "d_lines", "n_lines", "d_sizes", "d_selected"] and p["classes"].kind is inspect.Parameter.KEYWORD_ONLY


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
    npy = traces.save_npy(str(d / "t.npy"), traces.zeros(8, 64))
    cfg = str(d / "none.json")
    for args, words in ((["-a", "BDI", "-i", npy, "--by", "kernel"], ("--by kernel", ".log")),
                        (["-a", "BDI", "-i", npy, "--by=rw"], ("--by rw", ".log")),
                        (["-a", "BDI,FPC", "-i", npy, "--by", "mftype"], ("--by mftype", ".log")),
                        (["-a", "BDI,FPC", "-i", npy, "--by", "cluster"], ("--by cluster", "VPC")),
                        (["-a", "BDI", "-i", npy, "--by", "cluster"], ("--by cluster", "VPC")),
                        (["-a", "VPC", "-c", cfg, "-i", npy, "--by", "cluster"], ("--by cluster", "list")),
                        (["-a", "BDI", "-i", npy, "--by", "address"], ("kernel, rw, mftype and cluster", "address")),
                        (["-a", "BDI", "-i", str(d / "t.log"), "--by", "rw", "--per-line"], ("--per-line",))):
        r = run([cli, *args, "-o", str(out)])
        assert r.returncode == 1, (args, r.stdout, r.stderr)
        assert len(r.stdout.strip().splitlines()) == 1 and all(w in r.stdout for w in words), (args, r.stdout)
    assert os.listdir(out) == []
    r = run([cli, "-a", "BDI", "-i", npy, "--by"])
    assert r.returncode == 1 and "missing an argument" in r.stdout
    assert "--by arg" in run([cli, "-h"]).stdout


# ---- comp::ClassReport ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("class_report_probe") / "class_report_probe")
    srcs = [os.path.join(ROOT, "tests", "native", "class_report_probe.cpp")] + [os.path.join(HOST, f) for f in ("ClassReport.cpp", "CompResult.cpp", "utils.cpp")]
    # host code only: the host compiler, as the other native probes of the suite are built
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "include"), "-I", HOST, *srcs, "-o", out], check=True, capture_output=True, text=True)
    return out


def run_probe(probe, *args):
    r = subprocess.run([probe, *[str(a) for a in args]], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    return r


def test_class_report_text(probe, tmp_path):
    csv = str(tmp_path / "BDI_results_classes.csv")
    # 64-byte lines, 32-byte sectors.  class 0: 3 lines in one sector, 1 in two, 600 bits; class 4: 2 lines, both two
    # sectors, 1024 bits; class 255: one line of 0 bits
    run_probe(probe, csv, 64, 32, "ds_t", "0:600:3;1", "4:1024:0;2", "255:0:1;0")
    rows = ["ds_t,0,4,2048,600," + fmt_double(2048 / 600) + "," + fmt_double(8 / 5) + ",",
            "ds_t,4,2,1024,1024,1,1,",
            "ds_t,255,1,512,0,0,2,"]
    with open(csv) as f:
        assert f.read() == HEADER + "\n".join(rows) + "\n"
    # a second report appends its rows without a second header
    run_probe(probe, csv, 64, 32, "ds_u", "9:100:1")
    with open(csv) as f:
        assert f.read() == HEADER + "\n".join(rows + ["ds_u,9,1,512,100,5.12,2,"]) + "\n"
    # no lines: the header alone; 128-byte lines with 16-byte sectors: 8 sector columns
    empty = str(tmp_path / "empty.csv")
    run_probe(probe, empty, 64, 32, "ds_t")
    with open(empty) as f:
        assert f.read() == HEADER
    wide = str(tmp_path / "wide.csv")
    run_probe(probe, wide, 128, 16, "w", "1:2048:1;1;1;1;1;1;1;1")
    with open(wide) as f:
        assert f.read() == HEADER + "w,1,8,8192,2048,4," + fmt_double(64 / 36) + ",\n"
    # more than 8 sectors a line, or a sector above the line: one message, exit 1
    for L, sb in ((128, 8), (32, 64), (64, 0)):
        r = subprocess.run([probe, str(tmp_path / "no.csv"), str(L), str(sb), "w", "1:1:1"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and "ClassReport" in r.stdout and not os.path.exists(tmp_path / "no.csv")
