"""Size accounting, what can be checked without a device: the sector arithmetic of mpc_size_sectors against a hand
computation, the text comp::SizeReport prints (a native probe with its own main, built with the address and
undefined-behaviour sanitizers), the command line's handling of --size-histogram / --sector, and the exported symbols."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT, pkg

BIN = os.path.join(ROOT, "bin")
HOST = os.path.join(ROOT, "cal_22-mpc_amd", "host")
BINS = 4096
MPC_E_INVAL = -22
HEADER = "Workload,Line Size,Lines,Sector Bytes,Sector Ratio,Sector Classes,Histogram,"


@pytest.fixture(scope="module")
def mpc():
    pkg("build").build_lib()
    return pkg()


def hist(pairs):
    bins = np.zeros(BINS, np.uint64)
    for size, count in pairs:
        bins[size] += count
    return bins


# ---- sectors -----------------------------------------------------------------------------------------------------------
def test_sectors_of_ten_lines_by_hand(mpc):
    """64-byte lines in 32-byte sectors (256 bits each), at most 2 sectors a line:
         size      0  1  256  257  511  512  513  4095
         sectors   1  1   1    2    2    2    2    2      (0 bits still occupies a sector; 513 and 4095 are capped at the line)
    with sizes 0 and 257 twice: ten lines, 4 in one sector and 6 in two: 16 sectors against 20 uncompressed."""
    bins = hist([(0, 2), (1, 1), (256, 1), (257, 2), (511, 1), (512, 1), (513, 1), (4095, 1)])
    got = mpc.size_sectors(bins, 64, 32)
    assert got["classes"].tolist() == [4, 6] and got["classes"].dtype == np.uint64
    assert got["total_sectors"] == 16 and got["ratio"] == 20 / 16
    assert mpc.size_sectors(bins, 64)["classes"].tolist() == [4, 6]                     # 32 bytes is the default


def test_sectors_when_the_line_is_no_multiple_of_the_sector(mpc):
    """40-byte lines in 32-byte sectors: ceil(40 / 32) = 2 classes; 256 bits fit one sector, 257 .. 324 need both."""
    bins = hist([(0, 1), (256, 3), (257, 2), (324, 1)])
    got = mpc.size_sectors(bins, 40, 32)
    assert got["classes"].tolist() == [4, 3] and got["total_sectors"] == 10 and got["ratio"] == 14 / 10


def test_sectors_as_large_as_the_line_and_small_ones(mpc):
    bins = hist([(0, 1), (100, 2), (516, 3), (4095, 1)])
    got = mpc.size_sectors(bins, 64, 64)                                                 # one class: nothing to gain
    assert got["classes"].tolist() == [7] and got["total_sectors"] == 7 and got["ratio"] == 1.0
    got = mpc.size_sectors(bins, 64, 8)                                                  # 8 classes of 64 bits
    assert got["classes"].tolist() == [1, 2, 0, 0, 0, 0, 0, 4] and got["total_sectors"] == 1 + 4 + 32
    assert got["ratio"] == 56 / 37
    none = mpc.size_sectors(np.zeros(BINS, np.uint64), 64, 32)
    assert none["classes"].tolist() == [0, 0] and none["total_sectors"] == 0 and none["ratio"] == 0.0


def test_sectors_rejections(mpc):
    bins = hist([(5, 1)])
    for line_size, sector in ((64, 0), (64, 65), (32, 64), (0, 32)):
        with pytest.raises(mpc.MpcError) as e:
            mpc.size_sectors(bins, line_size, sector)
        assert e.value.code == MPC_E_INVAL
    with pytest.raises(ValueError):
        mpc.size_sectors(bins[:100], 64, 32)
    fn = mpc.lib().mpc_size_sectors
    classes = np.zeros(4, np.uint64)
    total, ratio = C.c_uint64(), C.c_double()
    args = (C.byref(total), C.byref(ratio))
    assert fn(bins.ctypes.data, BINS, 64, 32, classes.ctypes.data, 2, *args) == 0 and classes.tolist() == [1, 0, 0, 0]
    assert fn(bins.ctypes.data, BINS, 64, 32, classes.ctypes.data, 3, *args) == MPC_E_INVAL      # n_classes != ceil(64 / 32)
    assert fn(bins.ctypes.data, BINS - 1, 64, 32, classes.ctypes.data, 2, *args) == MPC_E_INVAL   # n != MPC_SIZE_BINS
    assert fn(None, BINS, 64, 32, classes.ctypes.data, 2, *args) == MPC_E_INVAL
    assert fn(bins.ctypes.data, BINS, 64, 32, None, 0, None, None) == 0                           # every output is optional


# ---- comp::SizeReport --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    build = pkg("build")
    build.build_lib()
    out = str(tmp_path_factory.mktemp("size_report_probe") / "size_report_probe")
    srcs = [os.path.join(ROOT, "tests", "native", "size_report_probe.cpp")] + [os.path.join(HOST, f) for f in ("SizeReport.cpp", "CompResult.cpp", "utils.cpp")]
    pkg_dir = os.path.dirname(build.LIB)
    # host code only: the host compiler, as the other native probes of the suite are built
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "include"), "-I", HOST, *srcs, "-L", pkg_dir, "-lmpc_hip",
                    f"-Wl,-rpath,{pkg_dir}", "-o", out], check=True, capture_output=True, text=True)
    return out


def run_probe(probe, *args):
    # (the library's HIP runtime is loaded, never initialised: what it allocates while loading is not this program's leak)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    r = subprocess.run([probe, *[str(a) for a in args]], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stdout + r.stderr
    return r.stdout


def test_size_report_prints_a_header_once_and_a_row_per_workload(mpc, probe, tmp_path):
    csv = tmp_path / "BDI_results_sizes.csv"
    pairs = [(0, 2), (1, 1), (256, 1), (257, 2), (511, 1), (512, 1), (513, 1), (4095, 1)]
    run_probe(probe, csv, 64, 32, "ds_first", *[f"{s}:{c}" for s, c in pairs])
    run_probe(probe, csv, 64, 32, "ds_second", "516:3", "4:1")
    run_probe(probe, csv, 64, 32, "ds_empty")
    assert csv.read_text().split("\n") == [
        HEADER,
        "ds_first,64,10,32,1.25,4;6,0:2;1:1;256:1;257:2;511:1;512:1;513:1;4095:1,",
        "ds_second,64,4,32,1.1428571428571428,1;3,4:1;516:3,",      # 8 / 7
        "ds_empty,64,0,32,0,0;0,,",
        ""]
    # the numbers are those of mpc_size_sectors, the ratio is formatted like CompRatio in the result classes
    assert mpc.size_sectors(hist(pairs), 64, 32)["ratio"] == 1.25 and mpc.size_sectors(hist([(516, 3), (4, 1)]), 64, 32)["ratio"] == 8 / 7
    # 40-byte lines, and to stdout without a file
    assert run_probe(probe, "", 40, 32, "w", "256:3", "257:2") == "w,40,5,32,1.4285714285714286,3;2,256:3;257:2,\n"


# ---- the command line --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cli():
    pkg("build").build_all()
    return os.path.join(BIN, "compressor")


@pytest.fixture()
def trace(traces, tmp_path):
    d = tmp_path / "ds"
    d.mkdir()
    return traces.save_npy(str(d / "t.npy"), traces.zeros(8, 64))


@pytest.mark.parametrize("args,text", [
    (["--sector", "0"], '--sector takes a number of bytes from 1 to the trace\'s line size, not "0".'),
    (["--sector", "x"], '--sector takes a number of bytes from 1 to the trace\'s line size, not "x".'),
    (["--sector", "-32"], 'not "-32".'),
    (["--sector", "32k"], 'not "32k".'),
    (["--sector=0"], 'not "0".'),
    (["--sector", "128"], "--sector 128: a sector cannot be larger than the trace's 64-byte lines."),
    (["--size-histogram", "--sector"], "Option 'sector' is missing an argument"),
])
def test_refused_sector_values_write_nothing(cli, trace, tmp_path, args, text):
    """Refused with a message and exit status 1 before any device is touched (--sector last: its value may be missing)."""
    out = tmp_path / "out"
    out.mkdir()
    r = subprocess.run([cli, "-a", "BDI", "-i", trace, "-o", str(out), *args], cwd=BIN, capture_output=True, text=True, timeout=600)
    assert r.returncode == 1 and text in r.stdout, r.stdout + r.stderr
    assert os.listdir(out) == []


def test_help_names_both_options(cli):
    text = subprocess.run([cli, "-h"], cwd=BIN, capture_output=True, text=True, timeout=600).stdout
    assert "--size-histogram" in text and "--sector arg" in text and "Default=32" in text


def test_run_script_hands_options_to_the_compressor(tmp_path):
    """bin/run: arguments from the first `--` option on go to every ./compressor run, with or without a configuration."""
    fake = tmp_path / "compressor"
    fake.write_text('#!/bin/bash\necho "ARGS $*"\n')
    fake.chmod(0o755)
    ds = tmp_path / "ds"
    ds.mkdir()
    (ds / "a.npy").write_bytes(b"")
    run = os.path.join(BIN, "run")
    r = subprocess.run([run, "BDI,FPC", str(ds), "out", "--sector", "16"], cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert f"ARGS -a BDI,FPC -i {ds}/a.npy -o out/ --sector 16" in r.stdout, r.stdout + r.stderr
    r = subprocess.run([run, "VPC", str(ds), "out", "cfg.json", "--size-histogram"], cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert f"ARGS -a VPC -i {ds}/a.npy -c cfg.json -o out/ --size-histogram" in r.stdout, r.stdout + r.stderr
    r = subprocess.run([run, "VPC", str(ds), "out", "cfg.json"], cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert f"ARGS -a VPC -i {ds}/a.npy -c cfg.json -o out/\n" in r.stdout, r.stdout + r.stderr
    assert subprocess.run([run, "VPC", str(ds), "--sector", "16"], cwd=tmp_path, capture_output=True, text=True, timeout=60).returncode == 1


# ---- the library -------------------------------------------------------------------------------------------------------
SIZE_SYMBOLS = ["mpc_size_hist_enable", "mpc_size_hist_get", "mpc_group_best_enable", "mpc_group_best_get", "mpc_group_best_reset",
                "mpc_size_sectors"]


def test_new_symbols_are_declared_exported_and_bound(mpc):
    with open(os.path.join(ROOT, "include", "mpc_hip_sizes.h")) as f:
        hdr = f.read()
    assert set(re.findall(r"\bint (mpc_\w+)\s*\(", hdr)) == set(SIZE_SYMBOLS) == set(mpc.EXPORTED_SIZE_SYMBOLS)
    assert re.search(r"#define MPC_SIZE_BINS\s+4096\b", hdr) and mpc.MPC_SIZE_BINS == 4096
    with open(os.path.join(ROOT, "include", "mpc_hip.h")) as f:
        main_hdr = f.read()
    assert '#include "mpc_hip_sizes.h"' in main_hdr and re.search(r"#define MPC_ABI_VERSION\s+1\b", main_hdr)
    raw = C.CDLL(mpc.LIB_PATH)
    for name in SIZE_SYMBOLS:
        assert hasattr(raw, name), name
        assert getattr(mpc.lib(), name).argtypes is not None, name
    for cls, names in ((mpc._Evaluator, ("enable_size_histogram", "size_histogram")), (mpc.EvaluatorSet, ("enable_best", "best"))):
        for name in names:
            assert callable(getattr(cls, name)), name
    assert callable(mpc.size_sectors)


def test_accounting_kernel_in_the_code_object(mpc, tmp_path):
    """mpc_sizes.hip is in the library's gfx950 code object: one instantiation per number of arrays (1 .. 8), each
    without scratch memory or spilled VGPRs, 256 lanes, and no static LDS beyond the few sums (the histograms are dynamic)."""
    from test_group_cpu import _gfx950_code_objects
    build = pkg("build")
    readelf = shutil.which("llvm-readelf") or "/opt/rocm/llvm/bin/llvm-readelf"
    assert os.path.exists(readelf), "llvm-readelf (ROCm's LLVM tools) not found"
    kernels = {}
    for i, obj in enumerate(_gfx950_code_objects(build.build_lib())):
        path = tmp_path / f"co{i}.elf"
        path.write_bytes(obj)
        notes = subprocess.run([readelf, "--notes", str(path)], capture_output=True, text=True, check=True).stdout
        for block in notes.split("- .agpr_count:")[1:]:
            m = re.match(r"_Z20sizes_account_kernelILi(\d+)E", re.search(r"\.name:\s+(\S+)", block).group(1))
            if m:
                kernels[int(m.group(1))] = {k: int(re.search(rf"\.{k}:\s+(\d+)", block).group(1))
                                            for k in ("private_segment_fixed_size", "vgpr_spill_count", "max_flat_workgroup_size", "group_segment_fixed_size")}
    assert sorted(kernels) == list(range(1, 9)), sorted(kernels)
    for key, k in kernels.items():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, (key, k)
        assert k["max_flat_workgroup_size"] == 256 and k["group_segment_fixed_size"] <= 128, (key, k)
