"""BDI, FPC and BPC without a device: the CPU oracle (oracle/mpc_oracle.c) and the host result classes against the
reference's own compressors, as recorded in tests/golden/ref_baseline_vectors.npz (tests/golden/
make_ref_baseline_vectors.py, reference BDI.cpp / FPC.cpp / BPC.cpp compiled unmodified).  The inputs are rebuilt from
their seeds (tests/baseline_ref.py) and checked against the recorded digests."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, pkg

import baseline_ref
import test_cli

ORACLES = {"BDI": "BdiOracle", "FPC": "FpcOracle", "BPC": "BpcOracle"}
NAMES = [c["name"] for c in baseline_ref.CASES]


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return baseline_ref.load_fixture(os.path.join(golden_dir, "ref_baseline_vectors.npz"))


def _case(fixture, name):
    return next(c for c in fixture[0]["cases"] if c["name"] == name)


def test_fixture_covers_the_issue_cases(fixture):
    meta, arrays = fixture
    assert [{k: c[k] for k in ("name", "comp", "L", "seed")} for c in meta["cases"]] == baseline_ref.CASES
    for comp, sizes in baseline_ref.SIZES.items():
        assert sorted(c["L"] for c in meta["cases"] if c["comp"] == comp) == sorted(sizes)
    for c in meta["cases"]:
        assert c["n"] >= baseline_ref.MIN_LINES and arrays[c["name"] + ".sizes"].shape == (c["n"],)
        counts = arrays[c["name"] + ".stats"][3:]
        if c["comp"] == "BDI" and c["L"] >= 16:
            assert (counts > 0).all(), c["name"]                     # every BDIState
        if c["comp"] == "FPC":
            assert (counts > 0).all(), c["name"]                     # every prefix
        if c["comp"] == "BPC":
            # the reference never counts ZeroDBP (5); AllOnes (6) needs DBX == 0x7fffffff, i.e. 31 deltas (L = 128),
            # although every case has all-ones planes of its own width; Uncomp needs three deltas
            assert counts[5] == 0 and (counts[6] > 0) == (c["L"] == 128) and (counts[[1, 2, 3]] > 0).all(), c["name"]
            assert (counts[4] > 0) == (c["L"] >= 12) and (counts[0] > 0) == (c["L"] >= 16), c["name"]


@pytest.mark.parametrize("name", NAMES)
def test_inputs_rebuild_from_their_seeds(fixture, name):
    baseline_ref.case_input(_case(fixture, name))


@pytest.mark.parametrize("name", NAMES)
def test_oracle_reproduces_the_reference(oracle, fixture, name):
    meta, arrays = fixture
    case = _case(fixture, name)
    comp, L = case["comp"], case["L"]
    lines = baseline_ref.case_input(case)
    o = getattr(oracle, ORACLES[comp])(L)
    out = o.compress(lines)
    sizes = out[0] if comp == "BDI" else out
    want = arrays[name + ".sizes"]
    bad = np.nonzero(sizes != want)[0]
    assert bad.size == 0, f"{bad.size} sizes differ, first lines {bad[:5]}: {sizes[bad[:5]]} vs {want[bad[:5]]}"
    if comp == "BDI":
        bad = np.nonzero(out[1] != arrays[name + ".states"])[0]
        assert bad.size == 0, f"{bad.size} BDI states differ, first lines {bad[:5]}"
    stats = arrays[name + ".stats"]
    assert (o.stats_vector() == baseline_ref.stats_vector(comp, len(lines), stats)).all()
    assert o.st.comp_ratio == float(arrays[name + ".ratio"][0])               # the same double
    if comp != "BDI":
        assert o.st.total_words == int(stats[2])


def test_bdi_stage_pins(oracle, fixture):
    meta, arrays = fixture
    lib = oracle.lib()
    got = np.array([lib.mpc_o_bdi_reduce_sign(int(x)) for x in arrays["reduce_sign_in"]], dtype=np.uint64)
    bad = np.nonzero(got != arrays["reduce_sign_out"])[0]
    assert bad.size == 0, [(hex(int(arrays["reduce_sign_in"][i])), int(got[i]), int(arrays["reduce_sign_out"][i])) for i in bad]
    assert len(arrays["reduce_sign_in"]) >= 60
    combos = [(8, 1), (8, 2), (8, 4), (4, 1), (4, 2), (2, 1)]
    for name in meta["check"]["cases"]:
        case = _case(fixture, name)
        lines = baseline_ref.case_input(case)[:meta["check"]["lines"]]
        want = arrays["check_" + name]
        assert want.shape == (len(lines), 6)
        for i, line in enumerate(lines):
            line = np.ascontiguousarray(line)
            got = [lib.mpc_o_bdi_check(line.ctypes.data, case["L"], B, D) for B, D in combos]
            assert got == want[i].tolist(), (name, i, got, want[i].tolist())


def test_cli_headers_are_the_reference_headers(fixture):
    headers = {"BDI": test_cli.BDI_HEADER, "FPC": test_cli.FPC_HEADER, "BPC": test_cli.BPC_HEADER}
    seen = set()
    for rec in fixture[0]["print"]:
        assert rec["text"].split("\n", 1)[0] + "\n" == headers[rec["comp"]], rec["case"]
        seen.add(rec["comp"])
    assert seen == set(headers)


def _row_vector(rec, n_lines):
    """The ABI statistics vector behind a recorded CSV row (original, compressed, [total words,] counts)."""
    f = rec["text"].split("\n")[1].split(",")
    assert f[-1] == "" and f[0] == rec["npy"][:-4].replace("/", "_")
    ints = [int(x) for x in f[1:3]] + [int(x) for x in f[4:-1]]
    if rec["comp"] == "FPC":
        assert ints[2] == sum(ints[3:])                  # TotalWords
        ints = ints[:2] + ints[3:]
    return np.array([n_lines] + ints, dtype=np.uint64)


def test_recorded_print_rows_are_the_oracle_totals(oracle, fixture):
    """The recorded CSV rows (all lines but the last, as the command line reads a .npy) hold the oracle's totals."""
    for rec in fixture[0]["print"]:
        case = _case(fixture, rec["case"])
        lines = baseline_ref.case_input(case)[:-1]
        o = getattr(oracle, ORACLES[case["comp"]])(case["L"])
        o.compress(lines)
        assert (_row_vector(rec, len(lines)) == o.stats_vector()).all(), rec["case"]
        assert rec["text"].split("\n")[1].split(",")[3] == test_cli.fmt_double(o.st.comp_ratio)


def test_host_result_print_is_the_reference_text(fixture, tmp_path):
    """BDIResult / FPCResult / BPCResult::Print of the host classes, filled from the recorded totals, write the
    reference's text byte for byte (header on a new file, then the row)."""
    pkg().lib()                                           # libmpc_hip.so is built
    host = os.path.join(ROOT, "cal_22-mpc_amd", "host")
    libdir = os.path.join(ROOT, "cal_22-mpc_amd")
    exe = str(tmp_path / "result_print_probe")
    srcs = [os.path.join(host, f) for f in ("BDI.cpp", "FPC.cpp", "BPC.cpp", "VPC.cpp", "DeviceCompressor.cpp", "Compressor.cpp", "CompResult.cpp",
                                            "LoaderNPY.cpp", "LoaderGPGPU.cpp", "LoaderAPSim.cpp", "utils.cpp")]
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", host, "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "native", "result_print_probe.cpp"), *srcs,
                        "-L", libdir, "-lmpc_hip", f"-Wl,-rpath,{libdir}", "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    for rec in fixture[0]["print"]:
        case = _case(fixture, rec["case"])
        csv = tmp_path / f"{rec['case']}.csv"
        v = _row_vector(rec, case["n"] - 1)
        r = subprocess.run([exe, rec["comp"], str(case["L"]), rec["npy"][:-4].replace("/", "_"), str(csv)]
                           + [str(int(x)) for x in v], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stdout + r.stderr
        assert csv.read_text() == rec["text"], rec["case"]
