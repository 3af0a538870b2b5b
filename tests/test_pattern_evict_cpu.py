"""The evicting mode of the Pattern analyser without a device: the restatements of the reference's line cache
(tests/pattern_evict_ref.py) against the reference's own answers (tests/golden/ref_pattern_evict_vectors.npz), the new entry
point and its argument checks, and the new kernels in the gfx950 code object of the built library.

The real-capacity case of the fixture (16.8 million lines) is not replayed here in Python: its totals are what the FIFO
rule says in closed form (checked below), and the GPU test feeds it to the library."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT, pkg

import pattern_evict_ref as per
from test_group_cpu import _gfx950_code_objects


@pytest.fixture(scope="module")
def mpc():
    m = pkg()
    m.lib()
    return m


@pytest.fixture(scope="module")
def fixture(golden_dir):
    z = np.load(os.path.join(golden_dir, "ref_pattern_evict_vectors.npz"))
    return z, json.loads(bytes(z["meta"]).decode())


def _flags(z, c):
    return np.unpackbits(z[c["name"] + "/existed"])[:c["n"]].astype(bool)


def test_fixture_covers_the_issue_cases(fixture):
    z, meta = fixture
    cases = meta["cases"]
    assert [c["name"] for c in cases] == [c["name"] for c in per.CASES] and len(cases) == 5 * 3 * 8
    assert {c["C"] for c in cases} == {1, 2, 5, 64, 1000} and {c["L"] for c in cases} == {8, 64, 72}
    for c in cases:
        f = _flags(z, c)
        assert c["n"] >= 3000 and int(z[c["name"] + "/insertions"]) == int((~f).sum())
        if c["trace"] == "cyc_c":
            assert not f[:c["C"]].any() and f[c["C"]:].all()
        if c["trace"] == "cyc_c+1":
            assert not f.any()
        u = {"rand_c+1": c["C"] + 1, "rand_2c": 2 * c["C"], "rand_3c+1": 3 * c["C"] + 1, "mix": c["C"] + 1}.get(c["trace"])
        if u:
            # more insertions than distinct lines: lines come back after their eviction.  (Random draws from C + 1 lines miss
            # the one evicted line with probability C / (C + 1) per draw: there only the eviction itself is certain.)
            assert f.any() and int((~f).sum()) >= u + (0 if c["trace"] == "rand_c+1" else 1)
    t = z["real/totals"]
    assert meta["real_parts"] == [list(p) for p in per.REAL_PARTS] and t.shape == (5, len(per.REAL_FIELDS))
    # the FIFO rule in closed form: parts two and five miss throughout, parts three and four hit
    lines = np.cumsum([b - a for a, b in per.REAL_PARTS])
    assert t[:, 0].tolist() == lines.tolist()
    assert z["real/insertions"].tolist() == [lines[0], lines[1], lines[1], lines[1], lines[1] + 6000]
    assert (t[:, 3] == 8 * (t[:, 0] - z["real/insertions"])).all() and (t[:, 5] == 8 * t[:, 0]).all()


def test_restatement_reproduces_every_fixture_case(fixture):
    z, meta = fixture
    for c in meta["cases"]:
        lines = per.case_input(c)
        assert per.digest(lines) == c["sha256"], "the seeded input generator drifted"
        flags, ins = per.fifo_flags(per.keys_of(lines), c["C"])
        assert (flags == _flags(z, c)).all() and ins == int(z[c["name"] + "/insertions"]), c["name"]


@pytest.mark.parametrize("which", ["1", "C/2", "C"])
def test_launch_by_launch_decomposition_equals_the_cache(fixture, which):
    z, meta = fixture
    for c in meta["cases"]:
        C_ = c["C"]
        launch = {"1": 1, "C/2": max(1, C_ // 2), "C": C_}[which]
        if which == "1" and C_ == 1000 and c["L"] != 64:
            continue                                # (a launch per line in Python: one line size is enough at this capacity)
        keys = [int(k) for k in per.case_index(c)]
        flags, ins = per.launch_flags(keys, C_, launch)
        assert (flags == _flags(z, c)).all() and ins == int(z[c["name"] + "/insertions"]), (c["name"], launch)


def test_new_symbol_is_declared_exported_and_bound(mpc):
    with open(os.path.join(ROOT, "include", "mpc_hip.h")) as f:
        hdr = f.read()
    name = "mpc_create_pattern_evicting"
    assert re.search(rf"\bint {name}\s*\(unsigned line_size, uint64_t capacity, int device, mpc_handle \*\*out\)", hdr)
    assert name in mpc.EXPORTED_SYMBOLS
    assert hasattr(C.CDLL(mpc.LIB_PATH), name)
    assert getattr(mpc.lib(), name).argtypes is not None
    assert re.search(r"#define MPC_ABI_VERSION\s+1\b", hdr)
    assert re.search(r"#define MPC_PATH_PATTERN_EVICTING\s+9\b", hdr) and mpc.MPC_PATH_PATTERN_EVICTING == 9


@pytest.mark.parametrize("L,capacity,words", [(64, (1 << 24), ("16777216", "2^24 - 1")), (8, 1 << 40, ("capacity",)), (64, (1 << 64) - 1, ("capacity",)),
                                              (0, 0, ("multiple of 8",)), (12, 5, ("multiple of 8",)), (264, 1000, ("multiple of 8",)),
                                              (4, 1 << 30, ("multiple of 8",))])
def test_create_refuses_before_touching_a_device(mpc, L, capacity, words):
    h = C.c_void_p()
    env_before = dict(os.environ)
    rc = mpc.lib().mpc_create_pattern_evicting(L, capacity, 10 ** 6, C.byref(h))       # (a device ordinal no machine has: it is never looked at)
    assert rc == -22 and not h
    msg = mpc.lib().mpc_last_error(None).decode()
    assert msg.startswith("Pattern") and all(w in msg for w in words), msg
    assert dict(os.environ) == env_before
    if capacity < 1 << 63:
        with pytest.raises(mpc.MpcError) as e:
            mpc.Pattern(L, on_full="evict", capacity=capacity or None)
        assert e.value.code == -22


def test_python_binding_refuses_other_modes(mpc):
    for bad in ("lru", "", "Evict", None, 0, True):
        with pytest.raises(ValueError):
            mpc.Pattern(64, on_full=bad)
    with pytest.raises(ValueError):
        mpc.Pattern(64, capacity=100)               # a capacity belongs to the evicting set
    for bad in (0, -1, 2.5):
        with pytest.raises(ValueError):
            mpc.Pattern(64, on_full="evict", capacity=bad)


def test_evicting_kernels_in_the_code_object(tmp_path):
    """The ten passes of the evicting set are in the library's gfx950 code object, use 0 bytes of scratch and spill no
    VGPR; the walk's LDS is a few KiB."""
    build = pkg("build")
    lib_path = build.build_lib()
    readelf = shutil.which("llvm-readelf") or os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(build.HIPCC))), "llvm", "bin", "llvm-readelf")
    if not os.path.exists(readelf):
        readelf = "/opt/rocm/llvm/bin/llvm-readelf"
    assert os.path.exists(readelf), "llvm-readelf (ROCm's LLVM tools) not found"
    kernels = {}
    for i, obj in enumerate(_gfx950_code_objects(lib_path)):
        path = tmp_path / f"co{i}.elf"
        path.write_bytes(obj)
        notes = subprocess.run([readelf, "--notes", str(path)], capture_output=True, text=True, check=True).stdout
        for block in notes.split("- .agpr_count:")[1:]:
            m = re.match(r"_Z\d+(evict_[a-z]+_kernel)", re.search(r"\.name:\s+(\S+)", block).group(1))
            if m:
                kernels[m.group(1)] = {k: int(re.search(rf"\.{k}:\s+(\d+)", block).group(1))
                                       for k in ("private_segment_fixed_size", "vgpr_spill_count", "max_flat_workgroup_size", "group_segment_fixed_size")}
    assert sorted(kernels) == sorted(f"evict_{p}_kernel" for p in ("begin", "clear", "claim", "compare", "tail", "classify", "scan", "scatter",
                                                                     "walk", "finish")), sorted(kernels)
    for name, k in kernels.items():
        assert k["private_segment_fixed_size"] == 0, (name, k)      # no scratch
        assert k["vgpr_spill_count"] == 0, (name, k)
        assert k["group_segment_fixed_size"] <= 8 * 1024, (name, k)
