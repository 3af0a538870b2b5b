"""C-Pack with a per-line dictionary, without a device: the restatement (tests/cpack_ref.py) in both dictionary scopes
against the reference's own numbers (tests/golden/ref_cpack_vectors.npz), the closed forms the kernels use against the
restatement, the argument checks of mpc_create_cpack, the new symbol and constants, the kernels in the gfx950 code object
of the built library, and comp::CPACKResult's text (a native probe with its own main, built with the address and
undefined-behaviour sanitizers)."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, pkg

import cpack_ref
from test_group_cpu import _gfx950_code_objects

HOST = os.path.join(ROOT, "cal_22-mpc_amd", "host")
NAMES = [c["name"] for c in cpack_ref.CASES]


@pytest.fixture(scope="module")
def mpc():
    m = pkg()
    m.lib()
    return m


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return cpack_ref.load_fixture(os.path.join(golden_dir, "ref_cpack_vectors.npz"))


def _case(fixture, name):
    return next(c for c in fixture[0]["cases"] if c["name"] == name)


@pytest.fixture(scope="module")
def restated(fixture):
    """{case: (lines, sizes, counts)} of the restatement with a per-line dictionary, computed once."""
    out = {}
    for c in fixture[0]["cases"]:
        lines = cpack_ref.case_input(c)
        out[c["name"]] = (lines,) + cpack_ref.compress(lines, "line")
    return out


def test_fixture_covers_the_issue_cases(fixture):
    meta, z = fixture
    assert [{k: c[k] for k in ("name", "L", "seed")} for c in meta["cases"]] == cpack_ref.CASES
    assert [c["L"] for c in meta["cases"]] == [4, 8, 12, 32, 36, 64, 68, 96, 128, 132, 252, 256]
    assert [p["case"] for p in meta["print"]] == list(cpack_ref.PRINT_CASES)
    for c in meta["cases"]:
        L, name = c["L"], c["name"]
        sizes, counts = z[name + ".sizes"], z[name + ".counts"]
        assert c["n"] >= cpack_ref.MIN_LINES and sizes.shape == (c["n"],) and counts.shape == (c["n"], 6)
        assert sizes.dtype == np.uint16 and counts.dtype == np.uint8 and z[name + ".carried"].dtype == np.uint16
        assert (counts.sum(axis=1) == L // 4).all()
        assert (sizes == counts.astype(np.int64) @ np.array(cpack_ref.BITS)).all()       # lengths in enum order, not m_PatternLength's
        assert (sizes == 34 * (L // 4)).any() and sizes.max() > 8 * L                     # W distinct keys: not capped
        assert (sizes == 2 * (L // 4)).any()                                              # all-zero
        assert (z[name + ".carried"] != sizes).any()                                      # the carried dictionary gives other numbers
        seen = counts.astype(np.int64).sum(axis=0) > 0
        assert seen[[0, 1, 4, 5]].all() and (seen.all() or L == 4), (name, seen)          # (one word per line: no MMMM / MMMX)


@pytest.mark.parametrize("L", cpack_ref.LINE_SIZES)
def test_hand_built_lines_are_in_the_cases_with_the_outcomes_the_issue_names(fixture, L):
    """Each hand-built line sits in its case, and the reference gave it the pattern counts the issue says."""
    meta, z = fixture
    c = _case(fixture, f"cpack_L{L}")
    lines = cpack_ref.case_input(c)
    index = {bytes(row): i for i, row in enumerate(lines)}
    W = L // 4
    hand = cpack_ref.hand_lines(L)
    got = [z[c["name"] + ".counts"][index[bytes(row)]].tolist() for row in hand]
    assert got[0] == [W, 0, 0, 0, 0, 0] and got[1] == [0, W, 0, 0, 0, 0]
    assert got[7] == [0, 0, 0, 0, 0, W]
    if W >= 7:
        assert got[3] == [W - 7, 0, 0, 0, 5, 2]           # key 0, b2 != 0, before 16 misses: MMXX against a zero entry
    if W >= 3:
        assert got[4] == [W - 3, 0, 0, 2, 0, 1]           # MMMX twice: the stored word is not updated
        assert got[5] == [W - 3, 0, 0, 0, 2, 1]           # MMXX twice: MMXX does not push
    if W >= 17:
        assert got[8] == [W - 17, 0, 1, 0, 0, 16]         # A, 15 others, A: a hit
    if W >= 18:
        assert got[9] == [W - 18, 0, 0, 0, 0, 18]         # A, 16 others, A: evicted
    if W >= 19:
        assert got[11] == [W - 19, 0, 1, 0, 0, 18]        # a hit does not refresh
    if W >= 20:
        assert got[12] == [W - 20, 0, 1, 0, 1, 18]        # pushed again: the later entry decides
    if W >= 32:
        assert got[14] == [W - 22, 1, 2, 1, 1, 17]        # key 0 after 16 misses: a miss, then hits on its own entry
        assert got[15][4] == 1 and got[15][2] == 1 and got[15][5] == 30
        assert got[16][2] == 1 and got[16][5] == 31


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_the_reference_in_both_scopes(fixture, restated, name):
    meta, z = fixture
    c = _case(fixture, name)
    lines, sizes, counts = restated[name]
    assert (sizes == z[name + ".sizes"]).all() and (counts == z[name + ".counts"]).all()
    v, st = cpack_ref.stats_vector(c["L"], sizes, counts), z[name + ".stats"]
    assert int(v[0]) == c["n"] and (v[1:4] == st[:3]).all() and (v[4:] == st[3:]).all()
    assert cpack_ref.comp_ratio(c["L"], sizes) == float(z[name + ".ratio"][0])            # the same double
    csizes, ccounts = cpack_ref.compress(lines, "carried")
    assert (csizes == z[name + ".carried"]).all()
    cv, cst = cpack_ref.stats_vector(c["L"], csizes, ccounts), z[name + ".carried_stats"]
    assert (cv[1:4] == cst[:3]).all() and (cv[4:] == cst[3:]).all()


def test_the_generator_reproduces_the_fixture_where_the_reference_is():
    ref = os.environ.get("REF", "/root/reference")             # (as oracle/Makefile)
    if not os.path.isfile(os.path.join(ref, "src", "compressor", "CPACK.cpp")):
        pytest.skip("the reference sources are not here")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "make_ref_cpack_vectors.py"), "--check"],
                       capture_output=True, text=True, timeout=600, env=dict(os.environ, REF=ref))
    assert r.returncode == 0 and "no difference" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.parametrize("name", NAMES)
def test_closed_forms_equal_the_restatement(fixture, restated, name):
    """What cpack_line computes (csrc/mpc_baselines.h), restated on numpy arrays: the latest earlier miss with the word's
    key and the liveness test at every line size; the first earlier word with the key where nothing can be evicted."""
    lines, sizes, counts = restated[name]
    s, k = cpack_ref.closed_form(lines)
    assert (s == sizes).all() and (k == counts).all()
    if lines.shape[1] <= 64:
        s, k = cpack_ref.closed_form_no_eviction(lines)
        assert (s == sizes).all() and (k == counts).all()


def test_the_identities_of_the_closed_forms(restated):
    """No eviction and a zero entry always there up to 64 bytes; a key-0 word misses only after 16 misses."""
    for name, (lines, sizes, counts) in restated.items():
        L = lines.shape[1]
        if L <= 64:
            assert int(counts[:, 5].max()) <= 16
        words = lines.view("<u4")
        key0 = ((words & 0xFFFF) == 0) & ((words & 0xFFFFFF) != 0)
        few = counts[:, 5] < 16                               # fewer than 16 misses in the whole line
        rows = np.nonzero(few & key0.any(axis=1))[0]
        assert (counts[rows, 4] >= key0[rows].sum(axis=1)).all(), name          # each of them MMXX


def test_new_symbol_is_declared_exported_and_bound(mpc):
    with open(os.path.join(ROOT, "include", "mpc_hip.h")) as f:
        hdr = f.read()
    assert re.search(r"\bint mpc_create_cpack\s*\(unsigned line_size, int dictionary_scope, int device, mpc_handle \*\*out\)", hdr)
    assert "mpc_create_cpack" in mpc.EXPORTED_SYMBOLS and hasattr(C.CDLL(mpc.LIB_PATH), "mpc_create_cpack")
    assert mpc.lib().mpc_create_cpack.argtypes is not None
    assert re.search(r"#define MPC_PATH_CPACK\s+8\b", hdr) and mpc.MPC_PATH_CPACK == 8
    assert re.search(r"#define MPC_CPACK_DICT_CARRIED\s+0\b", hdr) and mpc.MPC_CPACK_DICT_CARRIED == 0
    assert re.search(r"#define MPC_CPACK_DICT_PER_LINE\s+1\b", hdr) and mpc.MPC_CPACK_DICT_PER_LINE == 1
    assert re.search(r"#define MPC_ABI_VERSION\s+1\b", hdr)
    with open(os.path.join(ROOT, "cal_22-mpc_amd", "csrc", "mpc_device.h")) as f:
        assert re.search(r"#define MPC_CPACK_RAW_LEN\s+7\b", f.read())
    assert hasattr(mpc, "CPACK") and mpc.CPACK.PATTERNS == cpack_ref.PATTERNS


@pytest.mark.parametrize("scope,L,words", [(0, 64, ("carried", "DESIGN.md", "8")), (2, 64, ("dictionary_scope 2",)), (-1, 64, ("dictionary_scope -1",)),
                                           (1, 0, ("multiple of 4",)), (1, 6, ("multiple of 4",)), (1, 260, ("multiple of 4", "256")),
                                           (0, 6, ("carried",))])
def test_create_refuses_before_touching_a_device(mpc, scope, L, words):
    h = C.c_void_p()
    env_before = dict(os.environ)
    rc = mpc.lib().mpc_create_cpack(L, scope, 10 ** 6, C.byref(h))       # (a device ordinal no machine has: it is never looked at)
    assert rc == -22 and not h
    msg = mpc.lib().mpc_last_error(None).decode()
    assert msg.startswith("C-Pack") and all(w in msg for w in words), msg
    assert dict(os.environ) == env_before


def test_python_binding_refuses_every_other_dictionary(mpc):
    for d in ("carried", "global", "", 0, 2):
        with pytest.raises(mpc.MpcError) as e:
            mpc.CPACK(64, dictionary=d)
        assert e.value.code == -22 and "C-Pack" in str(e.value)
    with pytest.raises(mpc.MpcError) as e:
        mpc.CPACK(64, "carried")
    assert "DESIGN.md" in str(e.value) and "not offered" in str(e.value)
    with pytest.raises(mpc.MpcError) as e:
        mpc.CPACK(6)
    assert e.value.code == -22 and "multiple of 4" in str(e.value)


def test_kernels_in_the_code_object(tmp_path):
    """cpack_kernel<NW> for 32-, 64- and 128-byte lines (NW = 8, 16, 32) and the any-line-size kernel are in the library's
    gfx950 code object; none uses scratch or spills a VGPR."""
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
            name = re.search(r"\.name:\s+(\S+)", block).group(1)
            m = re.match(r"_Z12cpack_kernelILi(\d+)E", name)
            if m or name.startswith("_Z16cpack_any_kernel"):
                kernels[int(m.group(1)) if m else 0] = {
                    k: int(re.search(rf"\.{k}:\s+(\d+)", block).group(1))
                    for k in ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count", "max_flat_workgroup_size", "group_segment_fixed_size")}
    assert sorted(kernels) == [0, 8, 16, 32], sorted(kernels)
    for key, k in kernels.items():
        assert k["private_segment_fixed_size"] == 0, (key, k)      # no scratch
        assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (key, k)
        assert k["max_flat_workgroup_size"] == (256 if key else 128), (key, k)
        assert k["group_segment_fixed_size"] <= 64 * 1024, (key, k)


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    build = pkg("build")
    build.build_lib()
    out = str(tmp_path_factory.mktemp("cpack_probe") / "cpack_probe")
    srcs = [os.path.join(ROOT, "tests", "native", "cpack_probe.cpp")] + [os.path.join(HOST, f) for f in sorted(os.listdir(HOST)) if f.endswith(".cpp") and f != "main.cpp"]
    pkg_dir = os.path.dirname(build.LIB)
    # host code only: the host compiler, as the other native probes of the suite are built
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "include"), "-I", HOST, *srcs, "-L", pkg_dir, "-lmpc_hip",
                    f"-Wl,-rpath,{pkg_dir}", "-o", out], check=True, capture_output=True, text=True)
    return out


def _run_probe(probe, *args, ok=0):
    # (the library's HIP runtime is loaded, never initialised: what it allocates while loading is not this program's leak)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    r = subprocess.run([probe, *[str(a) for a in args]], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == ok and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stdout + r.stderr
    return r.stdout


def test_cpack_result_prints_the_reference_text(probe, fixture, restated, tmp_path):
    """comp::CPACKResult filled from the totals of all lines but the last: the reference's header and row, byte for byte."""
    meta, z = fixture
    for rec in meta["print"]:
        c = _case(fixture, rec["case"])
        lines, sizes, counts = restated[rec["case"]]
        v = cpack_ref.stats_vector(c["L"], sizes[:-1], counts[:-1])
        workload = rec["npy"][:-4].replace("/", "_")
        csv = tmp_path / f"{rec['case']}.csv"
        out = _run_probe(probe, "print", c["L"], workload, csv, *[int(x) for x in v])
        assert csv.read_text() == rec["text"], rec["case"]
        assert rec["text"].split("\n")[0] + "\n" == cpack_ref.HEADER
        ratio = float.fromhex(out.split()[3])
        assert out.split()[:3] == ["result", str(int(v[1])), str(int(v[2]))] and ratio == cpack_ref.comp_ratio(c["L"], sizes[:-1])
        assert cpack_ref.print_text(workload, v, rec["text"].split("\n")[1].split(",")[3]) == rec["text"].split("\n")[1] + "\n"
        _run_probe(probe, "print", c["L"], workload, csv, *[int(x) for x in v])          # a second row, no second header
        assert csv.read_text() == rec["text"] + rec["text"].split("\n")[1] + "\n"


def test_host_class_refuses_the_carried_dictionary(probe):
    """comp::CPACK(lineSize, CPACKDictionary::Carried): the library's message and exit(1), without a device."""
    out = _run_probe(probe, "refuse", 0, 64, ok=1)
    assert out.startswith("CPACK: cannot create the evaluator (-22): C-Pack:") and "DESIGN.md" in out
    out = _run_probe(probe, "refuse", 1, 6, ok=1)
    assert "multiple of 4" in out
    with open(os.path.join(HOST, "CPACK.h")) as f:
        assert re.search(r"CPACK\(unsigned lineSize, CPACKDictionary scope\);", f.read())        # no default for the scope
