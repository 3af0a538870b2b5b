"""The evicting Pattern set between its two pinned extremes, without a device: the mid-capacity cases and the edge-driven
trace (tests/pattern_evict_ref.py: MID_CASES, edge_index) against the reference's own answers
(tests/golden/ref_pattern_evict_mid_vectors.npz), the census of what a launch sequence makes the device do
(pattern_evict_ref.census) against the same answers and against the committed coverage file
(tests/golden/pattern_evict_coverage.json), and the floors that say which events those inputs must reach."""
import functools
import json
import os

import numpy as np
import pytest

from conftest import ROOT, pkg

import pattern_evict_ref as per

NAMES = [c["name"] for c in per.MID_CASES]


@pytest.fixture(scope="module")
def fixture(golden_dir):
    z = np.load(os.path.join(golden_dir, "ref_pattern_evict_mid_vectors.npz"))
    return z, json.loads(bytes(z["meta"]).decode())


@pytest.fixture(scope="module")
def old_fixture(golden_dir):
    return np.load(os.path.join(golden_dir, "ref_pattern_evict_vectors.npz"))


@pytest.fixture(scope="module")
def committed(golden_dir):
    with open(os.path.join(golden_dir, "pattern_evict_coverage.json")) as f:
        return json.load(f)


def _flags(z, c):
    return np.unpackbits(z[c["name"] + "/existed"])[:c["n"]].astype(bool)


def _case(name):
    return next(c for c in per.MID_CASES if c["name"] == name)


@functools.lru_cache(maxsize=None)
def _coverage(name):
    """(the coverage entry, the census results) of a case, computed once for all the tests here."""
    return per.coverage_of(_case(name))


def test_fixture_covers_the_issue_cases(fixture, golden_dir):
    z, meta = fixture
    assert os.path.getsize(os.path.join(golden_dir, "ref_pattern_evict_mid_vectors.npz")) < 1 << 20
    cases = meta["cases"]
    assert [{k: c[k] for k in ("name", "C", "L", "trace", "n", "seed")} for c in cases] == per.MID_CASES
    have = {}
    for c in cases:
        have.setdefault((c["C"], c["L"]), []).append(c["trace"])
    want = {(65537, 8): ["edge", "rand_2c", "mix", "cyc_c+1", "cyc_c"], (65537, 64): ["edge", "mix"], (262145, 8): ["edge", "rand_2c"]}
    want.update({(C_, 64): ["edge"] for C_ in (1, 2, 5, 64, 1000)})
    assert have == want and "edge" in per.TRACES
    assert meta["motifs"] == [list(m) for m in per.MOTIFS] and meta["edge_seed"] == per.EDGE_SEED
    assert dict(per.MOTIFS) == {"OFER": 6, "OR": 2, "FE": 2, "N": 1, "F": 3, "OFFEOR": 2, "D": 1, "EE": 1, "ONFE": 2}
    for c in cases:
        f = _flags(z, c)
        assert c["n"] == 3000 + 6 * c["C"] and int(z[c["name"] + "/insertions"]) == int((~f).sum()) and c["hits"] == int(f.sum())
        if c["trace"] == "cyc_c":
            assert not f[:c["C"]].any() and f[c["C"]:].all()
        if c["trace"] == "cyc_c+1":
            assert not f.any()
    # 65537 and 262145 lines: 257 and 1025 blocks, so the scan's threads take 2 and 5 blocks each and the upper ones none
    for C_, blocks, per_thread, busy in ((65537, 257, 2, 129), (262145, 1025, 5, 205)):
        assert -(-C_ // 256) == blocks and -(-blocks // 256) == per_thread and -(-blocks // per_thread) == busy < 256
    assert 257 % 2 == 1                             # ... and at 257 blocks the last busy thread takes fewer than the others


def test_the_calls_of_the_gpu_tests():
    """No multiple of 256, a full launch, and a full launch plus one line that the handle splits into C and 1."""
    c = _case("C65537_L8_edge")
    cuts = per.mid_cuts(c)
    assert [b - a for a, b in zip(cuts[:-1], cuts[1:])] == [1, 255, 256, 257, 30000, 65536, 65537, 65538, c["n"] - 227380]
    launches = per.cut_launches(cuts, c["C"])
    assert (161842, 227379) in launches and (227379, 227380) in launches and all(b - a <= c["C"] for a, b in launches)
    for s in per.MID_CASES:
        cuts = per.mid_cuts(s)
        assert cuts[0] == 0 and cuts[-1] == s["n"] and all(a < b for a, b in zip(cuts[:-1], cuts[1:]))


@pytest.mark.parametrize("name", NAMES)
def test_the_cache_reproduces_every_case(fixture, name):
    z, meta = fixture
    c = next(c for c in meta["cases"] if c["name"] == name)
    lines = per.case_input(c)
    assert lines.shape == (c["n"], c["L"]) and per.digest(lines) == c["sha256"], "the seeded input generator drifted"
    index = per.case_index(c)
    assert index.max() <= 3 * c["C"] and (np.ascontiguousarray(lines[:, :4]).view("<u4").ravel() == index).all()      # distinct numbers are distinct lines
    flags, ins = per.fifo_flags(per.keys_of(lines), c["C"])
    assert (flags == _flags(z, c)).all() and ins == int(z[name + "/insertions"])
    if c["trace"] == "edge":                                                        # what the generator intended, position for position
        assert (per.edge_index(c["C"], c["n"], c["seed"])[1] == _flags(z, c)).all()


@pytest.mark.parametrize("name", NAMES)
def test_the_census_reproduces_every_case_and_the_coverage_file(fixture, committed, name):
    """In one call and in the calls of the GPU tests, with launches of min(C, 2^22) lines; what it counts is what the
    committed coverage file says."""
    z, meta = fixture
    c = next(c for c in meta["cases"] if c["name"] == name)
    want = _flags(z, c)
    entry, runs = _coverage(name)
    for how, r in runs.items():
        assert (r["flags"] == want).all() and r["insertions"] == int(z[name + "/insertions"]), (name, how)
        k = r["kinds"]
        assert ((k == per.KIND_GONE_FIRST) | (k == per.KIND_RISK_MISS) == ~want).all()
        t = r["total"]
        assert t["gone_firsts"] + t["risk_misses"] == r["insertions"] and t["risk_hits"] + t["risk_misses"] == t["risk"]
        assert r["calls"][-1] == r["after_launch"][-1] == [t["launches"], t["rotations"], t["gone_firsts"], t["risk"], t["risk_misses"]]
        assert t["launches"] == len(per.cut_launches(entry[how]["cuts"], min(c["C"], per.LAUNCH_LIMIT)))
    assert json.loads(json.dumps(entry)) == committed["cases"][name]
    assert ("after_launch" in entry["cuts"]) == (name in per.TESTLIB_CASES)


def test_coverage_file_is_complete(committed):
    assert sorted(committed["cases"]) == sorted(NAMES) and committed["counters"] == list(per.COUNTERS)
    assert committed["cut_steps"] == list(per.CUT_STEPS) and committed["launch_limit"] == per.LAUNCH_LIMIT == 1 << 22
    assert set(per.TESTLIB_CASES) <= set(NAMES)


@pytest.mark.parametrize("which", ["1", "C/2", "C"])
def test_the_census_reproduces_every_small_capacity_case(old_fixture, which):
    """The cases of ref_pattern_evict_vectors.npz, as test_pattern_evict_cpu.py runs them through launch_flags."""
    z = old_fixture
    for c in per.CASES:
        C_ = c["C"]
        launch = {"1": 1, "C/2": max(1, C_ // 2), "C": C_}[which]
        r = per.census(per.case_index(c), C_, launch, [0, c["n"]])
        assert (r["flags"] == _flags(z, c)).all() and r["insertions"] == int(z[c["name"] + "/insertions"]), (c["name"], launch)
        assert r["total"]["launches"] == -(-c["n"] // launch)


@pytest.mark.parametrize("name,C_", [("C64_L64_edge", 64), ("C1000_L64_edge", 1000), ("C5_L64_edge", 5)])
def test_both_ways_of_counting_a_launch_agree(name, C_):
    """The census counts launches of a few lines in plain Python and longer ones with arrays: the same traces through
    either alone and through both in turn (calls of 1 to 40 lines) give equal results, field by field."""
    c = _case(name)
    index = per.case_index(c)
    cuts = [0]
    while cuts[-1] < c["n"]:
        cuts.append(min(c["n"], cuts[-1] + 1 + (7 * len(cuts)) % 40))
    for launch in (1, 3, min(16, C_), min(17, C_), C_):
        a, b, m = (per.census(index, C_, launch, cuts, few=few) for few in (0, 1 << 30, 16))
        for other in (b, m):
            assert sorted(other) == sorted(a)
            for k in a:
                assert (a[k] == other[k]).all() if isinstance(a[k], np.ndarray) else a[k] == other[k], (launch, k)
        assert a["total"]["rotations"] > 0 and a["total"]["found_older_live"] > 0
        assert a["total"]["risk_misses"] > 0 or launch == 1         # (the only at-risk stamp of a one-line launch is I_0 - C: a hit)


def test_coverage_floors_of_the_edge_trace(committed):
    """What `edge` at C = 65537 must reach in one call.  Conditions, not measurements: a faithful edge_index is far above
    each (the committed file says by how much)."""
    t = committed["cases"]["C65537_L8_edge"]["one"]["total"]
    assert t["same_hit_miss"] >= 5000 and t["same_miss_hit"] >= 5000
    assert t["later_hit_miss"] >= 50 and t["later_miss_hit"] >= 50
    assert t["rotations"] >= 2
    assert t["found_older_live"] >= 10000 and t["found_older_dead"] >= 1
    assert t["launches_risk_blocks_over_256"] >= 1 and t["launches_gone_first_blocks_over_256"] >= 1
    assert t["max_walk_batches"] >= 100


def test_coverage_floors_of_all_cases_together(committed):
    total = {}
    for entry in committed["cases"].values():
        for how in ("one", "cuts"):
            for k, v in entry[how]["total"].items():
                total[k] = total.get(k, 0) + v
    for where in ("same", "later"):
        assert total[where + "_miss_miss"] == 0
        for pair in ("hit_hit", "hit_miss", "miss_hit"):
            assert total[f"{where}_{pair}"] > 0, (where, pair)
    for k in ("found_newer", "found_older_live", "found_older_dead", "found_nowhere", "lines_gone", "lines_safe", "lines_risk",
              "gone_first_at_0", "gone_first_at_255", "risk_at_0", "risk_at_255", "walk_at_0", "walk_at_255"):
        assert total[k] > 0, k


def test_the_read_outs_are_in_the_test_library_only():
    build = pkg("build")
    with open(build.build_lib(), "rb") as f:
        product = f.read()
    with open(build.build_lib(test=True), "rb") as f:
        test = f.read()
    with open(os.path.join(ROOT, "include", "mpc_hip.h")) as f:
        hdr = f.read()
    for name in ("mpc_test_evict_counters", "mpc_test_evict_kinds"):
        assert name.encode() not in product and name.encode() in test and name not in hdr, name
