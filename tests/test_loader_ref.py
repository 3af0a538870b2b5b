"""The trace readers against the reference's own loaders (CPU only).  tests/golden/ref_loader_vectors.json records what
trace::gpgpusim::LoaderGPGPU, trace::apsim::LoaderGPGPU and trace::LoaderNPY -- the reference's sources compiled
unmodified by tests/golden/make_ref_loader_vectors.py -- report and deliver for the seeded trace files of
tests/loader_ref.py.  Here the files are rebuilt from their recipes and the same numbers are asked of

- the Python restatements the other tests take their expected lines from (oracle/gpgpusim_log.py, oracle/apsim_txt.py,
  numpy slicing for .npy);
- the host mirrors (host/Loader{GPGPU,APSim,NPY}.cpp) through the stand-alone, sanitizer-built loader_probe, per request
  and in batches of 1, 7 and 100 lines;
- the C ABI's probes mpc_npy_shape and mpc_gpgpusim_log_line_size.

All comparisons are exact: integers and sha256 digests of the delivered bytes.  Where the library deliberately differs
from the reference the test states both: what the reference recorded and what the library does instead."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, pkg

import loader_ref
from oracle import apsim_txt as A
from oracle import gpgpusim_log as G
from test_native_cpu import loader_probe  # noqa: F401  (the probe, built as that module builds it)

with open(os.path.join(ROOT, "tests", "golden", "ref_loader_vectors.json")) as _f:
    FIXTURE = json.load(_f)
CASES = FIXTURE["cases"]
BY_NAME = {c["name"]: c for c in CASES}
OF = lambda fmt: [c for c in CASES if c["fmt"] == fmt]      # noqa: E731
IDS = lambda cases: [c["name"] for c in cases]              # noqa: E731
RW = {"R": "0", "W": "1"}                                  # trace::rw_t: READ, WRITE (NA = 2)


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """Every case's trace file, written once."""
    d = str(tmp_path_factory.mktemp("loader_ref"))
    return {c["name"]: loader_ref.build_input(c, d) for c in CASES}


def test_fixture_and_recipes_agree():
    """The fixture was generated from the cases of tests/loader_ref.py as they are now, and holds every kind the readers
    distinguish."""
    assert [{k: v for k, v in c.items() if k not in ("sha256", "ref")} for c in CASES] == json.loads(json.dumps(loader_ref.CASES))
    logs, npys = OF("log"), OF("npy")
    assert {c["ref"]["line_size"] for c in logs} == {32, 64, 128} == {c["ref"]["line_size"] for c in npys}
    assert {c["tail"] for c in logs} == {"none", "short1", "hdr17", "hdr62"}
    assert sorted(c["n"] for c in npys if c["L"] == 64) == [1, 2, 777, 12001]
    big = BY_NAME["log_big_64"]["ref"]
    assert big["num_lines"] == 12000 and big["delivered"] > 10000 and BY_NAME["npy_big_64"]["ref"]["delivered"] == 12000
    assert BY_NAME["log_none_evaluated"]["ref"]["delivered"] == 0 and BY_NAME["log_first_not_evaluated"]["parts"][0]["types"]["first"] == 2
    for c in OF("txt"):
        assert sorted(c["ref"]) == ["32", "64"] and all(sorted(v) == ["after", "fresh"] for v in c["ref"].values())


@pytest.mark.parametrize("case", CASES, ids=IDS(CASES))
def test_inputs_rebuild_to_the_recorded_digest(inputs, case):
    assert loader_ref.file_digest(inputs[case["name"]]) == case["sha256"]


# ---- the Python restatements ---------------------------------------------------------------------------------------
def restated(case, path, line_size=None):
    """(line size, GetNumLines, delivered lines as bytes, delivered count) by the Python restatement."""
    if case["fmt"] == "log":
        recs = G.read_records(path)
        kept = G.evaluated_lines(path)
        return G.line_size(path), len(recs), kept.tobytes(), len(kept)
    if case["fmt"] == "npy":
        a = np.load(path)
        return a.shape[1], a.shape[0], a[:-1].tobytes(), len(a) - 1      # LoaderNPY.cpp:28-32 + main.cpp:240: the last row is the end
    lines = A.lines(path, line_size)
    return line_size, len(lines), lines.tobytes(), len(lines)


def same_as_reference(got, ref, tag):
    L, num, data, n = got
    assert (L, num, n) == (ref["line_size"], ref["num_lines"], ref["delivered"]), tag
    assert loader_ref.bytes_digest(data) == ref["delivered_sha256"], tag
    assert ref["delivered_sizes"] == ({str(L): n} if n else {}), tag


PLAIN = [c for c in CASES if c["fmt"] != "txt" and "deviation" not in c]
TXT = OF("txt")
DEVIATIONS = [c for c in CASES if "deviation" in c]


@pytest.mark.parametrize("case", PLAIN, ids=IDS(PLAIN))
def test_restatement_delivers_what_the_reference_delivers(inputs, case):
    same_as_reference(restated(case, inputs[case["name"]]), case["ref"], case["name"])


@pytest.mark.parametrize("case", TXT, ids=IDS(TXT))
def test_txt_restatement_delivers_what_a_fresh_reference_loader_delivers(inputs, case):
    path = inputs[case["name"]]
    rw = RW[A.read_rows(path)[0]]
    for L in case["line_sizes"]:
        ref = case["ref"][str(L)]["fresh"]
        same_as_reference(restated(case, path, L), ref, (case["name"], L))
        # the single-beat form reports READ whatever the trace is, and a request size of 64 at both line sizes
        n = ref["delivered"]
        assert ref["req_sizes"] == ({"64": n} if n else {}) and ref["rw"] == ({("0" if L == 32 else rw): n} if n else {})


# ---- the host mirrors ----------------------------------------------------------------------------------------------
def probe(exe, path, mode, tmp_path, line_size=None, fresh=False):
    """-> (line size, GetNumLines, delivered bytes, delivered count, {reqSize: n}, {rw: n})"""
    dump = str(tmp_path / "dump.bin")
    args = [exe, path] + (["line", "0"] if mode == "line" else ["batch", str(mode)]) + [str(line_size or 32), dump] + (["fresh"] if fresh else [])
    r = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (args, r.stdout, r.stderr[-3000:])
    out = [ln.split() for ln in r.stdout.strip().split("\n")]
    assert out[0][0] == "lines" and out[0][2] == "line_size" and out[1][0] == "delivered"
    maps = [{kv.split(":")[0]: int(kv.split(":")[1]) for kv in ln[1:]} for ln in out[2:4]] if mode == "line" else [None, None]
    with open(dump, "rb") as f:
        data = f.read()
    return int(out[0][3]), int(out[0][1]), data, int(out[1][1]), maps[0], maps[1]


MODES = ("line", 1, 7, 100)


@pytest.mark.parametrize("case", PLAIN, ids=IDS(PLAIN))
def test_host_mirror_delivers_what_the_reference_delivers(loader_probe, inputs, tmp_path, case):   # noqa: F811
    for mode in MODES:
        got = probe(loader_probe, inputs[case["name"]], mode, tmp_path)
        same_as_reference(got[:4], case["ref"], (case["name"], mode))


@pytest.mark.parametrize("case", TXT, ids=IDS(TXT))
def test_txt_host_mirror_delivers_what_a_fresh_reference_loader_delivers(loader_probe, inputs, tmp_path, case):   # noqa: F811
    """In both orders of calls: as constructed, and after GetNumLines() (which ends in Reset()).  The mirror's Reset()
    empties the beat queues, so both orders give the fresh loader's lines."""
    for L in case["line_sizes"]:
        ref = case["ref"][str(L)]["fresh"]
        for mode in MODES:
            for fresh in (True, False):
                got = probe(loader_probe, inputs[case["name"]], mode, tmp_path, L, fresh)
                same_as_reference(got[:4], ref, (case["name"], L, mode, fresh))
                if mode == "line":
                    assert (got[4], got[5]) == (ref["req_sizes"], ref["rw"]), (case["name"], L, fresh)


def test_reference_reuses_a_stale_beat_after_reset():
    """The deviation the mirror does not copy: the reference's apsim Reset() leaves m_MemReqChQueue as it is.  A channel
    that held an unpaired beat when GetNumLines() reached the end of the file keeps it, and the next pass glues it to the
    channel's first new beat: one line more per such channel, and every later line of that channel shifted by a beat.
    The reference's driver asks for 32-byte lines and never gets there; at 32 bytes both orders agree."""
    for c in TXT:
        lo = c["ref"]["32"]
        assert lo["fresh"] == lo["after"], c["name"]
        fresh, after = c["ref"]["64"]["fresh"], c["ref"]["64"]["after"]
        assert fresh["num_lines"] == after["num_lines"] == fresh["delivered"], c["name"]
        extra = after["delivered"] - fresh["delivered"]
        assert 0 <= extra <= 4 and (extra > 0) == (fresh["delivered_sha256"] != after["delivered_sha256"]), c["name"]
        # a channel with an odd number of beats holds one at the end, and with it an even number in the second pass
        assert extra == lo["fresh"]["delivered"] - 2 * fresh["delivered"], c["name"]
    read = BY_NAME["txt_read"]["ref"]["64"]
    assert (read["fresh"]["delivered"], read["after"]["delivered"]) == (250, 251)
    assert BY_NAME["txt_odd_rows"]["ref"]["64"]["fresh"] == BY_NAME["txt_odd_rows"]["ref"]["64"]["after"]      # no beat left over: no difference


# ---- the C ABI's probes ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mpc():
    pkg("build").build_lib()
    return pkg()


def test_c_abi_probes_report_the_reference_shape(mpc, inputs):
    for c in OF("npy"):
        rows, cols = C.c_uint64(), C.c_uint64()
        assert mpc.lib().mpc_npy_shape(inputs[c["name"]].encode(), C.byref(rows), C.byref(cols)) == 0
        assert (rows.value, cols.value) == (c["ref"]["num_lines"], c["ref"]["line_size"]), c["name"]
    for c in OF("log"):
        assert mpc.gpgpusim_log_line_size(inputs[c["name"]]) == c["ref"]["line_size"], c["name"]


# ---- the two documented .log deviations -----------------------------------------------------------------------------
@pytest.mark.parametrize("case", DEVIATIONS, ids=IDS(DEVIATIONS))
def test_log_deviations(loader_probe, inputs, tmp_path, case):   # noqa: F811
    """Evaluated requests of two sizes, and an evaluated request without payload: the reference hands each request to
    CompressLine as it is (recorded: the sizes of what it delivers); the batch interface refuses the trace."""
    path, ref = inputs[case["name"]], case["ref"]
    recs = G.read_records(path)
    kept = [d for (t, sz, d) in recs if t in (0, 4)]
    assert (G.line_size(path), len(recs), len(kept)) == (ref["line_size"], ref["num_lines"], ref["delivered"])
    assert loader_ref.bytes_digest(b"".join(d.tobytes() for d in kept)) == ref["delivered_sha256"]
    other = {"zero_size": 0, "two_sizes": 32}[case["deviation"]]
    assert ref["delivered_sizes"] == {"64": 20 if other == 0 else 10, str(other): 1 if other == 0 else 4}
    with pytest.raises(ValueError, match="mixed request sizes"):
        G.evaluated_lines(path)
    for cap in ("1", "7", "100"):
        r = subprocess.run([loader_probe, path, "batch", cap], capture_output=True, text=True, timeout=300)
        assert r.returncode == 1 and f"The GPGPU-sim trace mixes request sizes ({other} after 64 bytes): not supported." in r.stdout, r.stdout
