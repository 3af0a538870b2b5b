"""The ingestion paths on the MI355X against the lines the reference's own loaders deliver.  For every trace file of
tests/golden/ref_loader_vectors.json (recorded from the reference's LoaderGPGPU.cpp / LoaderNPY.cpp, see
tests/test_loader_ref.py) the file is rebuilt, the Python restatement's lines are first checked against the recorded
digest, and only then fed to the CPU oracles (VpcOracle with the probe configuration, BdiOracle, FpcOracle, BpcOracle,
sc2_ref.SC2Ref with S from the reference's GetNumLines(), pattern_ref).  Against those:

- single handles: compress_gpgpusim_log / compress_npy (the C ABI's own file walkers) return the reference's counts and
  leave exactly the oracle's statistics (and SC2 table);
- an EvaluatorSet over the same file: the same, per member;
- `compressor -a VPC,BDI,FPC,BPC` on .log, .npy and .txt files: the CSV text filled from the oracles.  The CLI hands a
  .log or .npy file to the C ABI's walker as well; a .txt file goes through the host mirror's GetBatch, the only way it
  reaches the GPU.

All comparisons are exact."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, pkg

import loader_ref
import pattern_ref
import sc2_ref
import test_cli as cli_text
from test_loader_ref import CASES, DEVIATIONS, IDS, PLAIN, TXT, restated

pytestmark = pytest.mark.gpu

BIN = os.path.join(ROOT, "bin")
NAMES = ["VPC", "BDI", "FPC", "BPC"]


@pytest.fixture(scope="module")
def mpc():
    m = pkg()
    m.lib()
    return m


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("loader_ref_gpu") / "ds"
    d.mkdir()
    return {c["name"]: loader_ref.build_input(c, str(d)) for c in CASES}


@pytest.fixture(scope="module")
def expected(oracle, configs, inputs):
    """case name -> what the CPU oracles say about the lines the reference delivers (computed once per case)."""
    cache = {}

    def get(case):
        if case["name"] in cache:
            return cache[case["name"]]
        path = inputs[case["name"]]
        ref = case["ref"]["32"]["fresh"] if case["fmt"] == "txt" else case["ref"]
        L, num, data, n = restated(case, path, 32 if case["fmt"] == "txt" else None)
        # the expected input is the reference's, not merely the restatement's
        assert (L, num, n) == (ref["line_size"], ref["num_lines"], ref["delivered"])
        assert loader_ref.bytes_digest(data) == ref["delivered_sha256"]
        lines = np.frombuffer(data, dtype=np.uint8).reshape(n, L)
        e = {"L": L, "n": n, "num_lines": num, "S": sc2_ref.sampling_lines(num),
             "VPC": oracle.VpcOracle(configs.probe_config(L)), "BDI": oracle.BdiOracle(L), "FPC": oracle.FpcOracle(L), "BPC": oracle.BpcOracle(L)}
        e["SC2"] = sc2_ref.SC2Ref(L, e["S"])
        if n:
            for k in NAMES:
                e[k].compress(lines)
            e["SC2"].feed(lines)
        e["Pattern"] = pattern_ref.analyse(lines)[2] if n else np.zeros(pattern_ref.STATS_LEN, dtype=np.uint64)
        cache[case["name"]] = e
        return e
    return get


def make(mpc, configs, e, kind):
    L = e["L"]
    if kind == "VPC":
        return mpc.VPC(configs.probe_config(L))
    if kind == "SC2":
        return mpc.SC2(L, e["S"])
    return getattr(mpc, kind)(L)


def feed(target, case, path, e):
    """The file through the C ABI's walker; the counts are the reference's."""
    if case["fmt"] == "log":
        assert target.compress_gpgpusim_log(path) == (e["num_lines"], e["n"]), case["name"]      # (GetNumLines, delivered)
    else:
        assert target.compress_npy(path) == e["n"], case["name"]


def check_member(ev, kind, e, tag):
    want = e[kind] if kind == "Pattern" else e[kind].stats_vector()
    got = ev.stats_vector()
    assert got.shape == want.shape and (got == want).all(), f"{tag}: {kind} statistics differ at {np.nonzero(got != want)[0][:8]}"
    if kind == "SC2":
        sym, lens = ev.table()
        assert sym.tolist() == e["SC2"].table_syms.tolist() and lens.tolist() == e["SC2"].table_lens.tolist(), tag
        assert (len(sym) > 0) == (e["n"] > e["S"]), tag


@pytest.mark.parametrize("case", PLAIN, ids=IDS(PLAIN))
def test_single_handles(mpc, configs, inputs, expected, case):
    e, path = expected(case), inputs[case["name"]]
    if case["fmt"] == "npy":
        rows, cols = C.c_uint64(), C.c_uint64()
        assert mpc.lib().mpc_npy_shape(path.encode(), C.byref(rows), C.byref(cols)) == 0 and (rows.value, cols.value) == (e["num_lines"], e["L"])
    else:
        assert mpc.gpgpusim_log_line_size(path) == e["L"]
    for kind in NAMES + ["SC2", "Pattern"]:
        ev = make(mpc, configs, e, kind)
        feed(ev, case, path, e)
        check_member(ev, kind, e, case["name"])
        ev.close()


@pytest.mark.parametrize("case", PLAIN, ids=IDS(PLAIN))
def test_groups(mpc, configs, inputs, expected, case):
    e, path = expected(case), inputs[case["name"]]
    kinds = NAMES + (["SC2"] if e["n"] > e["S"] else []) + ["Pattern"]      # SC2 where the trace outlasts its warm-up
    members = [make(mpc, configs, e, k) for k in kinds]
    group = mpc.EvaluatorSet(members)
    feed(group, case, path, e)
    for kind, ev in zip(kinds, members):
        check_member(ev, kind, e, case["name"] + " (group)")
    group.close()
    for ev in members:
        ev.close()


def test_sc2_is_in_a_group_that_outlasts_its_warm_up(expected):
    for name in ("log_big_64", "npy_big_64"):
        e = expected(next(c for c in CASES if c["name"] == name))
        assert e["S"] == 10000 < e["n"] and len(e["SC2"].table_syms) > 0


@pytest.mark.parametrize("case", DEVIATIONS, ids=IDS(DEVIATIONS))
def test_log_deviations_are_refused(mpc, inputs, case):
    """What the reference hands on for these two traces is recorded (lines of 0 or 32 bytes among 64-byte ones,
    test_loader_ref.py); the walker of the C ABI refuses them, for a handle and for a group."""
    other = {"zero_size": 0, "two_sizes": 32}[case["deviation"]]
    assert case["ref"]["delivered_sizes"][str(other)] > 0
    a, b = mpc.BDI(64), mpc.FPC(64)
    group = mpc.EvaluatorSet([a, b])
    for target in (a, group):
        with pytest.raises(mpc.MpcError) as err:
            target.compress_gpgpusim_log(inputs[case["name"]])
        assert err.value.code == -22 and f"the GPGPU-sim trace mixes request sizes ({other} after 64 bytes)" in str(err.value)
    group.close()
    a.close()
    b.close()


# ---- the command line -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cli():
    pkg("build").build_all()
    return os.path.join(BIN, "compressor")


def expected_files(e, workload):
    """The CSV files `compressor -a VPC,BDI,FPC,BPC` writes (row formats: tests/test_cli.py)."""
    f = cli_text.fmt_double
    row, det = cli_text.vpc_expected_rows(e["VPC"], workload)
    h1, h2 = cli_text.vpc_headers(e["VPC"].M)
    L = e["L"]
    out = {f"probe{L}_results.csv": h1 + row + "\n", f"probe{L}_results_detail.csv": h2 + det + "\n"}
    for kind, header, counts, words in (("BDI", cli_text.BDI_HEADER, 9, False), ("FPC", cli_text.FPC_HEADER, 8, True), ("BPC", cli_text.BPC_HEADER, 7, True)):
        st = e[kind].st
        out[f"{kind}_results.csv"] = header + f"{workload},{st.original_bits},{st.compressed_bits},{f(st.comp_ratio)}," + \
            (f"{st.total_words}," if words else "") + "".join(f"{st.counts[i]}," for i in range(counts)) + "\n"
    return out


CLI_CASES = PLAIN + TXT


@pytest.mark.parametrize("case", CLI_CASES, ids=IDS(CLI_CASES))
def test_cli(cli, configs, inputs, expected, tmp_path, case):
    e, path = expected(case), inputs[case["name"]]
    cfg = configs.write_config(configs.probe_config(e["L"]), str(tmp_path / f"probe{e['L']}.json"))
    out = tmp_path / "out"
    out.mkdir()
    r = subprocess.run([cli, "-a", ",".join(NAMES), "-i", path, "-c", cfg, "-o", str(out)], cwd=BIN, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    got = r.stdout.strip().split("\n")[-len(NAMES):]
    workload = "ds_" + case["name"]
    if e["n"] == 0:
        # nothing delivered: CompRatio keeps its initial 0 (reference CompResult.h:24-27) and every sum is 0
        assert got == [f"{k} comp.ratio: 0" for k in NAMES]
        for name in (f"probe{e['L']}_results.csv", "BDI_results.csv", "FPC_results.csv", "BPC_results.csv"):
            assert (out / name).read_text().split("\n")[-2].startswith(f"{workload},0,0,0,"), name
        return
    assert got == [f"{k} comp.ratio: {cli_text.fmt_double(e[k].st.comp_ratio)}" for k in NAMES]
    want = expected_files(e, workload)
    assert sorted(os.listdir(out)) == sorted(want)
    for name, text in want.items():
        assert (out / name).read_text() == text, name


@pytest.mark.parametrize("case", DEVIATIONS, ids=IDS(DEVIATIONS))
def test_cli_refuses_the_log_deviations(cli, inputs, tmp_path, case):
    """The CLI hands a .log file to the group's walker in the C ABI (CompressorSet::CompressFile) and ends with its message."""
    other = {"zero_size": 0, "two_sizes": 32}[case["deviation"]]
    r = subprocess.run([cli, "-a", "BDI,FPC", "-i", inputs[case["name"]], "-o", str(tmp_path)], cwd=BIN, capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and f"CompressorSet::CompressFile (-22): the GPGPU-sim trace mixes request sizes ({other} after 64 bytes)" in r.stdout, \
        r.stdout + r.stderr
