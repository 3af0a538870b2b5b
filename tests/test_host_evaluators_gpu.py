"""The six GPU evaluators of cal_22-mpc_amd/host (comp::VPC, BDI, FPC, BPC, SC2, Pattern) share one
comp::DeviceCompressor: every route into it, for every class, through tests/native/evaluator_probe.cpp.  The sizes that
CompressLine returns are checked against the oracles and the numpy restatements (none of them the code under test), and
the text of Print / PrintDetail has to be the same whichever way the lines came in."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import pattern_ref
import sc2_ref

pytestmark = pytest.mark.gpu

TAGS = ("VPC", "BDI", "FPC", "BPC", "SC2", "Pattern")
L, WARMUP = 64, 100          # 100 = 14 * 7 + 2: SC2's table is built in the middle of a buffered flush of 7 lines


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    host = os.path.join(ROOT, "cal_22-mpc_amd", "host")
    exe = str(tmp_path_factory.mktemp("evaluator_probe") / "evaluator_probe")
    srcs = [os.path.join(host, f) for f in sorted(os.listdir(host)) if f.endswith(".cpp") and f != "main.cpp"]
    b = subprocess.run(["hipcc", "-O2", "-std=c++17", "-Wall", "-I", host, "-I", os.path.join(ROOT, "include"), "-o", exe,
                        os.path.join(ROOT, "tests", "native", "evaluator_probe.cpp"), *srcs,
                        "-L", os.path.join(ROOT, "cal_22-mpc_amd"), "-lmpc_hip",
                        "-Wl,-rpath," + os.path.join(ROOT, "cal_22-mpc_amd")], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    return exe


@pytest.fixture(scope="module")
def cfg(configs):
    return configs.probe_config(L)


@pytest.fixture(scope="module")
def cfg_path(cfg, configs, tmp_path_factory):
    return configs.write_config(cfg, str(tmp_path_factory.mktemp("cfg") / "probe64.json"))


@pytest.fixture(scope="module")
def trace(traces):
    """301 rows (the loader drops the last): the library's builders and 40 repeated lines, permuted; the request types
    of the .log and the lines it keeps (GLOBAL_ACC_R = 0, GLOBAL_ACC_W = 4)."""
    rows = np.concatenate([traces.structured(120, L, seed=31), traces.mixed(50, L), traces.random_u32(30, L),
                           traces.zeros(8, L), traces.word_same(8, L), traces.bdi_stress(45, L)])
    rows = np.concatenate([rows, rows[np.random.default_rng(5).integers(0, len(rows), 40)]])
    rows = rows[np.random.default_rng(12).permutation(len(rows))]
    assert rows.shape == (301, L)
    types = np.random.default_rng(3).integers(0, 9, 300)
    return rows, types, rows[:300][(types == 0) | (types == 4)]


@pytest.fixture(scope="module")
def routes(probe, cfg_path, trace, traces, tmp_path_factory):
    """One run of the probe: {(tag, route): lines evaluated} and the directory with its files."""
    rows, types, kept = trace
    d = tmp_path_factory.mktemp("routes")
    npy = traces.save_npy(str(d / "trace.npy"), rows)
    log = traces.write_gpgpusim_log(str(d / "trace.log"), rows[:300], types)
    kept_npy = traces.save_npy(str(d / "kept.npy"), np.concatenate([kept, rows[-1:]]))
    r = subprocess.run([probe, "run", cfg_path, npy, log, kept_npy, str(d)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    done = {}
    for row in r.stdout.strip().split("\n"):
        tag, route, n = row.split()
        done[(tag, route)] = int(n)
    return done, d


def _text(d, tag, route, detail=False):
    return (d / f"{tag}.{route}{'.detail' if detail else ''}.csv").read_text()


def test_every_route_saw_its_lines(routes, trace):
    done, _ = routes
    kept = len(trace[2])
    assert 0 < kept < 300
    assert done == {(t, r): (kept if r in "ek" else 300) for t in TAGS for r in "abcdefk"}


def test_per_line_sizes_are_the_references(routes, trace, oracle, cfg):
    """Route (a): one CompressLine per line returns the size of that line."""
    _, d = routes
    lines = trace[0][:300]
    want = {"VPC": oracle.VpcOracle(cfg).compress(lines)[0], "BDI": oracle.BdiOracle(L).compress(lines)[0],
            "FPC": oracle.FpcOracle(L).compress(lines), "BPC": oracle.BpcOracle(L).compress(lines),
            "SC2": sc2_ref.SC2Ref(L, WARMUP).feed(lines)[0], "Pattern": pattern_ref.analyse(lines)[0]}
    for tag in TAGS:
        got = np.fromfile(d / f"{tag}.a.sizes", dtype=np.uint16)
        assert len(got) == 300 and (got == np.asarray(want[tag]).astype(np.uint16)).all(), (tag, np.nonzero(got != want[tag])[0][:10])
    assert pattern_ref.analyse(lines)[2][6] > 0          # Pattern's T: lines seen before


@pytest.mark.parametrize("tag", TAGS)
def test_buffered_lines_return_zero(routes, tag):
    """Route (b): after SetLineBuffering(7) CompressLine returns 0; 300 = 42 * 7 + 6, GetResult() flushes the last six."""
    _, d = routes
    got = np.fromfile(d / f"{tag}.b.sizes", dtype=np.uint16)
    assert len(got) == 300 and not got.any()


@pytest.mark.parametrize("tag", TAGS)
def test_every_route_prints_the_same_text(routes, tag):
    """Per line, buffered, in two batches, as a .npy file and as a member of a set: one text."""
    _, d = routes
    want = _text(d, tag, "a")
    assert want.count("\n") >= 2 and "probe_trace," in want
    for route in "bcdf":
        assert _text(d, tag, route) == want, (tag, route)
    if tag == "VPC":                  # (the other results have no detail rows)
        detail = _text(d, tag, "a", detail=True)
        assert "probe_trace," in detail
        for route in "bcdf":
            assert _text(d, tag, route, detail=True) == detail, (tag, route)


@pytest.mark.parametrize("tag", TAGS)
def test_log_file_is_the_kept_lines(routes, tag):
    """Route (e): CompressFile of the .log evaluates its GLOBAL_ACC_R / GLOBAL_ACC_W requests, in order."""
    _, d = routes
    assert _text(d, tag, "e") == _text(d, tag, "k")
    assert _text(d, tag, "e") != _text(d, tag, "c")
    if tag == "VPC":
        assert _text(d, tag, "e", detail=True) == _text(d, tag, "k", detail=True)


REFUSALS = {
    "sc2-line": "SC2::SetSamplingCnt after the first line is not supported (the warm-up sample has begun).\n",
    "sc2-handle": "SC2::SetSamplingCnt after the first line is not supported (the warm-up sample has begun).\n",
    "bdi-short": "BDI: line of 32 bytes, expected 64.\n",
    "vpc-short": "VPC: line of 32 bytes, configuration lineSize is 64.\n",
}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_refusals(probe, cfg_path, case):
    """SetSamplingCnt once a line has arrived or the handle has been handed out; a 32-byte vector to a 64-byte evaluator."""
    message = REFUSALS[case]
    r = subprocess.run([probe, "refuse", case, cfg_path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and r.stdout == message, r.stdout + r.stderr
