"""The Pattern analyser without a device: the restatement (tests/pattern_ref.py) against the reference's own numbers
(tests/golden/ref_pattern_vectors.npz), the new entry points, the argument checks of mpc_create_pattern, the analysis
kernels in the gfx950 code object of the built library, and comp::PatternResult's text."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT, pkg

import pattern_ref
from test_group_cpu import _gfx950_code_objects

HOST = os.path.join(ROOT, "cal_22-mpc_amd", "host")
ENTROPY_TOL = 256 * 2.0 ** -52      # at most 256 terms, each below 0.54; another libm may differ in a term's last bit


@pytest.fixture(scope="module")
def mpc():
    m = pkg()
    m.lib()
    return m


@pytest.fixture(scope="module")
def fixture(golden_dir):
    z = np.load(os.path.join(golden_dir, "ref_pattern_vectors.npz"))
    meta = json.loads(bytes(z["meta"]).decode())
    return z, meta["cases"]


def test_fixture_covers_the_issue_cases(fixture):
    z, cases = fixture
    assert {c["L"] for c in cases} == set(pattern_ref.LINE_SIZES)
    for c in cases:
        sel = z[c["name"] + "/sel"]
        patterns = [k for k in range(6) if 8 % pattern_ref.PATTERNS[k][0] == 0 and pattern_ref.PATTERNS[k][0] <= c["L"]]
        won = set(sel.tolist())
        if c["L"] >= 16:
            assert won >= set(patterns) | {9}, (c["name"], won)        # every pattern wins somewhere
        v = z[c["name"] + "/stats"]
        assert v[4] >= 4 * c["L"] and v[5] > v[4] and v[6] >= 5 * c["L"]   # zero lines, word-same lines, duplicates
        assert (z[c["name"] + "/sizes"] == 8 * c["L"] + 4).any()       # nothing beat 8 L
    # the two ties: the earlier pattern keeps the line
    lines = pattern_ref.case_input(next(c for c in cases if c["name"] == "menu_L64"))
    tie = [i for i in range(len(lines)) if pattern_ref.check_pattern(lines[i].tobytes(), 8, 1)[0] == 408
           and pattern_ref.check_pattern(lines[i].tobytes(), 4, 1)[0] == 408]
    assert tie and all(z["menu_L64/sel"][i] == 0 for i in tie)
    lines = pattern_ref.case_input(next(c for c in cases if c["name"] == "menu_L128"))
    tie = [i for i in range(len(lines)) if pattern_ref.check_pattern(lines[i].tobytes(), 8, 4)[0] == 560
           and pattern_ref.check_pattern(lines[i].tobytes(), 4, 2)[0] == 560 and z["menu_L128/sizes"][i] == 564]
    assert tie and all(z["menu_L128/sel"][i] == 2 for i in tie)


@pytest.mark.parametrize("which", ["scalar", "numpy"])
def test_restatement_equals_the_reference(fixture, which):
    z, cases = fixture
    for c in cases:
        lines = pattern_ref.case_input(c)
        assert pattern_ref.digest(lines) == c["sha256"], "the seeded input generator drifted"
        sizes, sel, v = (pattern_ref.analyse_scalar if which == "scalar" else pattern_ref.analyse)(lines)
        assert (sizes == z[c["name"] + "/sizes"]).all(), c["name"]
        assert (sel == z[c["name"] + "/sel"]).all(), c["name"]
        assert (v == z[c["name"] + "/stats"]).all(), (c["name"], np.nonzero(v != z[c["name"] + "/stats"])[0][:8])
        ent = z[c["name"] + "/entropy"]
        assert abs(pattern_ref.entropy(v[22:278]) - ent[0]) <= ENTROPY_TOL
        assert abs(pattern_ref.entropy(v[278:534]) - ent[1]) <= ENTROPY_TOL


def test_reduce_sign_is_the_range_test():
    rng = np.random.default_rng(5)
    xs = [0, 1, 2, 127, 128, 255, 256, 65535, 65536, (1 << 32) - 1, 1 << 32, (1 << 63) - 1, 1 << 63, (1 << 64) - 1, (1 << 64) - 2]
    for D in (1, 2, 4):
        h = 1 << (8 * D - 1)
        xs += [(1 << 64) - h, (1 << 64) - h - 1, (1 << 64) - h + 1, (1 << (8 * D)) - 1, 1 << (8 * D)]
    xs += [int(x) for x in rng.integers(0, 1 << 64, 2000, dtype=np.uint64)]
    xs += [((1 << 64) - int(x)) & pattern_ref.M64 for x in rng.integers(0, 1 << 34, 2000)]
    a = np.array(xs, dtype=np.uint64)
    for D in (1, 2, 4):
        want = np.array([pattern_ref.reduce_sign(x) <= (1 << (8 * D)) - 1 for x in xs])
        assert (pattern_ref._fits(a, D) == want).all()


def test_new_symbols_are_declared_exported_and_bound(mpc):
    with open(os.path.join(ROOT, "include", "mpc_hip.h")) as f:
        hdr = f.read()
    for name in ("mpc_create_pattern", "mpc_pattern_distinct_lines"):
        assert re.search(rf"\bint {name}\s*\(", hdr), name
        assert name in mpc.EXPORTED_SYMBOLS
        assert hasattr(C.CDLL(mpc.LIB_PATH), name)
        assert getattr(mpc.lib(), name).argtypes is not None
    assert re.search(r"#define MPC_PATH_PATTERN\s+7\b", hdr) and mpc.MPC_PATH_PATTERN == 7
    assert hasattr(mpc, "Pattern") and callable(mpc.Pattern.distinct_lines)


@pytest.mark.parametrize("L", [0, 4, 12, 264, 260, 1024])
def test_create_refuses_a_bad_line_size_before_touching_a_device(mpc, L):
    h = C.c_void_p()
    env_before = dict(os.environ)
    rc = mpc.lib().mpc_create_pattern(L, 10 ** 6, C.byref(h))       # (a device ordinal no machine has: it is never looked at)
    assert rc == -22 and not h
    assert b"multiple of 8" in mpc.lib().mpc_last_error(None)
    assert dict(os.environ) == env_before
    with pytest.raises(mpc.MpcError) as e:
        mpc.Pattern(L)
    assert e.value.code == -22


def test_analysis_kernels_in_the_code_object(tmp_path):
    """pattern_kernel<NW> for 32-, 64- and 128-byte lines (NW = 8, 16, 32) and the set passes are in the library's gfx950
    code object; the analysis kernels use 0 bytes of scratch and spill no VGPR."""
    build = pkg("build")
    lib_path = build.build_lib()
    readelf = shutil.which("llvm-readelf") or os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(build.HIPCC))), "llvm", "bin", "llvm-readelf")
    if not os.path.exists(readelf):
        readelf = "/opt/rocm/llvm/bin/llvm-readelf"
    assert os.path.exists(readelf), "llvm-readelf (ROCm's LLVM tools) not found"
    kernels, others = {}, set()
    for i, obj in enumerate(_gfx950_code_objects(lib_path)):
        path = tmp_path / f"co{i}.elf"
        path.write_bytes(obj)
        notes = subprocess.run([readelf, "--notes", str(path)], capture_output=True, text=True, check=True).stdout
        for block in notes.split("- .agpr_count:")[1:]:
            name = re.search(r"\.name:\s+(\S+)", block).group(1)
            m = re.match(r"_Z14pattern_kernelILi(\d+)E", name)
            if m or name.startswith("_Z18pattern_any_kernel"):
                kernels[int(m.group(1)) if m else 0] = {
                    k: int(re.search(rf"\.{k}:\s+(\d+)", block).group(1))
                    for k in ("private_segment_fixed_size", "vgpr_spill_count", "max_flat_workgroup_size", "group_segment_fixed_size")}
            elif "pattern_" in name:
                others.add(re.match(r"_Z\d+(pattern_[a-z]+_kernel)", name).group(1))
    assert sorted(kernels) == [0, 8, 16, 32], sorted(kernels)
    for key, k in kernels.items():
        assert k["private_segment_fixed_size"] == 0, (key, k)      # no scratch
        assert k["vgpr_spill_count"] == 0, (key, k)
        assert k["max_flat_workgroup_size"] == 256, (key, k)
        assert k["group_segment_fixed_size"] <= 64 * 1024, (key, k)
    assert others == {"pattern_claim_kernel", "pattern_compare_kernel", "pattern_tail_kernel"}


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    build = pkg("build")
    build.build_lib()
    out = str(tmp_path_factory.mktemp("pattern_probe") / "pattern_probe")
    srcs = [os.path.join(ROOT, "tests", "native", "pattern_probe.cpp")] + [os.path.join(HOST, f) for f in ("Pattern.cpp", "DeviceCompressor.cpp", "CompResult.cpp", "Compressor.cpp", "utils.cpp")]
    srcs += [os.path.join(HOST, f) for f in sorted(os.listdir(HOST)) if f.startswith("Loader") and f.endswith(".cpp")]
    pkg_dir = os.path.dirname(build.LIB)
    subprocess.run([build.HIPCC, "-O2", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", HOST, *srcs, "-L", pkg_dir,
                    "-lmpc_hip", f"-Wl,-rpath,{pkg_dir}", "-o", out], check=True, capture_output=True, text=True)
    return out


def test_pattern_result_prints_the_reference_text(probe, fixture, tmp_path):
    """comp::PatternResult filled by hand from the fixture's counters: the reference's header and row, its entropies, and
    the three CompResult numbers the reference's Pattern never updates."""
    z, cases = fixture
    for c in cases:
        v = z[c["name"] + "/stats"]
        stats = tmp_path / "stats.bin"
        v.astype("<u8").tofile(str(stats))
        csv = tmp_path / f"{c['name']}.csv"
        r = subprocess.run([probe, str(stats), c["name"], str(csv)], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        out = r.stdout.strip().split("\n")
        got = [float.fromhex(x) for x in out[0].split()[1:]]
        ent = z[c["name"] + "/entropy"]
        assert abs(got[0] - ent[0]) <= ENTROPY_TOL and abs(got[1] - ent[1]) <= ENTROPY_TOL
        assert out[1] == "counts " + " ".join(str(int(x)) for x in v[4:9])
        assert out[2] == f"maps {int((v[22:278] != 0).sum())} {int((v[278:534] != 0).sum())}"
        assert out[3] == "result 0 0 0x0p+0"
        text = csv.read_text().split("\n")
        assert text[0] == c["header"] and text[1] + "\n" == c["print"], (text[:2], c["print"])
        assert pattern_ref.print_text(c["name"], v) == c["print"]
