"""SC2 without a device: the host table builder of the library (mpc_sc2_code_lengths, the code every SC2 handle uses)
and the numpy restatement (tests/sc2_ref.py) against the reference's own tables (tests/golden/ref_sc2_vectors.json),
the driver's warm-up formula, the exported names."""
import json
import os
import re

import numpy as np
import pytest

from conftest import ROOT, pkg

import sc2_ref


@pytest.fixture(scope="module")
def mpc():
    m = pkg()
    m.lib()
    return m


@pytest.fixture(scope="module")
def fixture(golden_dir):
    with open(os.path.join(golden_dir, "ref_sc2_vectors.json")) as f:
        return json.load(f)["cases"]


def _warmup_counts(case):
    lines = sc2_ref.case_input(case)
    assert sc2_ref.digest(lines) == case["sha256"], "the seeded input generator drifted"
    S = min(case["S"], len(lines))
    return np.unique(lines[:S].view("<u4").reshape(-1), return_counts=True)


def test_fixture_covers_the_issue_cases(fixture):
    names = {c["name"]: c for c in fixture}
    assert len(names["ties_at_cut_L64"]["table"]) == 1024
    assert max(t[1] for t in names["fibonacci_L256"]["table"]) > 32
    assert names["one_symbol_L64"]["table"] == [[0, 0]]
    assert names["fewer_than_S_L128"]["table"] == [] and names["fewer_than_S_L128"]["n"] < names["fewer_than_S_L128"]["S"]
    assert {c["L"] for c in fixture} >= {32, 64, 128, 256}


@pytest.mark.parametrize("builder", ["library", "python"])
def test_code_lengths_reproduce_every_reference_table(mpc, fixture, builder):
    for case in fixture:
        if not case["table"]:
            continue
        sym, cnt = _warmup_counts(case)
        perm = np.random.default_rng(1).permutation(len(sym))      # input order must not matter
        sym, cnt = sym[perm], cnt[perm]
        lens = (mpc.sc2_code_lengths(sym, cnt) if builder == "library"
                else np.array(sc2_ref.code_lengths(sym, cnt), dtype=np.int64))
        keep = lens != 0xFFFF
        got = sorted(zip(sym[keep].tolist(), lens[keep].tolist()))
        assert got == [tuple(t) for t in case["table"]], case["name"]


def test_library_and_restatement_agree_on_large_seeded_inputs(mpc):
    rng = np.random.default_rng(77)
    for n, hi in ((5000, 3), (1500, 40), (1024, 2), (1025, 2), (700, 1 << 40), (1, 9)):
        sym = rng.choice(1 << 32, size=n, replace=False).astype(np.uint32)
        cnt = rng.integers(1, hi + 1, size=n).astype(np.uint64)
        a = mpc.sc2_code_lengths(sym, cnt)
        b = np.array(sc2_ref.code_lengths(sym, cnt), dtype=np.uint16)
        assert (a == b).all(), n
        assert int((a != 0xFFFF).sum()) == min(n, 1024)


def test_code_lengths_reject_empty_and_repeated_symbols(mpc):
    with pytest.raises(mpc.MpcError):
        mpc.sc2_code_lengths(np.zeros(0, np.uint32), np.zeros(0, np.uint64))
    with pytest.raises(mpc.MpcError):
        mpc.sc2_code_lengths(np.array([5, 5], np.uint32), np.array([1, 2], np.uint64))


def test_one_symbol_has_length_zero(mpc):
    assert mpc.sc2_code_lengths(np.array([0xFFFFFFFF], np.uint32), np.array([7], np.uint64)).tolist() == [0]


@pytest.mark.parametrize("n", [0, 999_999, 1_000_000, 100_000_000, 200_000_000, 10**12])
def test_sampling_lines_is_the_driver_formula(mpc, n):
    want = max(10000, min(n // 100, 1000000))
    assert mpc.sc2_sampling_lines(n) == want == sc2_ref.sampling_lines(n)


def test_new_symbols_are_exported(mpc):
    for name in ("mpc_create_sc2", "mpc_sc2_sampling_lines", "mpc_sc2_code_lengths", "mpc_sc2_table"):
        assert name in mpc.EXPORTED_SC2_SYMBOLS
        assert hasattr(mpc.lib(), name)
    with open(os.path.join(ROOT, "include", "mpc_hip.h")) as f:
        hdr = f.read()
    declared = set(re.findall(r"\b(mpc_\w+)\s*\(", hdr)) - {"mpc_handle"}
    assert declared == set(mpc.EXPORTED_SYMBOLS) | set(mpc.EXPORTED_SC2_SYMBOLS)
    assert mpc.MPC_PATH_SC2 == 6
