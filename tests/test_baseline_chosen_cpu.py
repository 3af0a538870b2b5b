"""The chosen BDI / FPC / BPC cases (tests/baseline_chosen.py) without a device: the builders build what they were asked
for, the CPU oracle and the plain restatements reproduce the reference's recorded numbers
(tests/golden/ref_baseline_chosen_vectors.npz) on the chosen cases and on the seeded ones of tests/baseline_ref.py, and
every named wrong variant of a restatement is rejected by chosen lines.

`python tests/test_baseline_chosen_cpu.py` rewrites tests/golden/baseline_chosen_coverage.json: built / requested per family
and line size, the reference's pattern, prefix and state counts, per wrong variant how many chosen lines reject it and, for
information only, whether any line of the seeded fixture does."""
import functools
import json
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
if os.path.dirname(HERE) not in sys.path:
    sys.path.insert(0, os.path.dirname(HERE))

import baseline_chosen as bc  # noqa: E402
import baseline_ref  # noqa: E402

GOLDEN = os.path.join(HERE, "golden")
COVERAGE = os.path.join(GOLDEN, "baseline_chosen_coverage.json")
ORACLES = {"BDI": "BdiOracle", "FPC": "FpcOracle", "BPC": "BpcOracle"}

# built / requested of the enumerated BPC cells at the three unrolled sizes, as counted when the inverse was prototyped:
# every (plane, row) single; every adjacent pair and every two ones apart but those of plane 31 (two deltas of 2^32 - 1
# exceed the span); every zero-DBX run
BPC_BUILT = {128: {"single": (1023, 1023), "pair": (960, 990), "apart": (13920, 14355), "runs": (561, 561)},
             64: {"single": (495, 495), "pair": (448, 462), "apart": (2912, 3003), "runs": (561, 561)},
             32: {"single": (231, 231), "pair": (192, 198), "apart": (480, 495), "runs": (561, 561)}}


@functools.lru_cache(maxsize=None)
def chosen_fixture():
    return bc.load_fixture(os.path.join(GOLDEN, "ref_baseline_chosen_vectors.npz"))


@functools.lru_cache(maxsize=None)
def old_fixture():
    return baseline_ref.load_fixture(os.path.join(GOLDEN, "ref_baseline_vectors.npz"))


def chosen_cases():
    """The recorded cases of baseline_chosen.CASES (the fixture also holds the group's lines and the random pools)."""
    return [c for c in chosen_fixture()[0]["cases"] if "lines" not in c]


def _case(name):
    return next(c for c in chosen_fixture()[0]["cases"] if c["name"] == name)


def chosen_input(name):
    lines, layout = bc.build(name)
    case = _case(name)
    assert len(lines) == case["n"] and bc.digest(lines) == case["sha256"], f"{name}: the builders drifted"
    return lines, layout


# ---- the builders ---------------------------------------------------------------------------------------------------
def test_fixture_holds_every_case():
    meta, arrays = chosen_fixture()
    assert [{k: c[k] for k in ("name", "comp", "L")} for c in chosen_cases()] == bc.CASES
    for c in meta["cases"]:
        assert arrays[c["name"] + ".sizes"].shape == (c["n"],) and arrays[c["name"] + ".sizes"].dtype == np.uint16
        assert (c["comp"] == "BDI") == (c["name"] + ".states" in arrays)
    for L in bc.GROUP_SIZES:
        n = sum(_case(f"{comp}_chosen_L{L}")["n"] for comp in ("bdi", "fpc", "bpc"))
        assert all(_case(f"group_L{L}.{comp}")["n"] == n for comp in ("BDI", "FPC", "BPC"))
    assert all(_case(f"pool_L{L}")["n"] == bc.POOL_LINES for L in bc.BDI_SIZES)
    assert (bc.FPC_SPECIAL == baseline_ref.FPC_SPECIAL).all()


@pytest.mark.parametrize("name", bc.NAMES)
def test_inputs_rebuild(name):
    lines, layout = chosen_input(name)
    ends = [layout[f]["rows"] for f in layout if f != "cells"]
    assert ends[0][0] == 0 and ends[-1][1] == len(lines) and all(a[1] == b[0] for a, b in zip(ends, ends[1:]))
    assert len(lines) <= 30000                          # a case stays a few milliseconds of kernel time


@pytest.mark.parametrize("L", bc.BPC_SIZES)
def test_bpc_lines_round_trip(L):
    lines, layout = chosen_input(f"bpc_chosen_L{L}")
    ND = L // 4 - 1
    planes = bc.dbx_of(lines)
    again, ok, why = bc.lines_for_dbx(L, planes)
    assert ok.all() and (why == "").all() and (again == lines).all()
    # the planes that were asked for are the planes of the built lines
    for fam, cands in (("single", bc._bpc_single(ND)), ("pair", bc._bpc_pair(ND)), ("top", bc._bpc_top(ND))):
        want = bc._planes(cands[0])
        _, ok, why = bc.lines_for_dbx(L, want)
        assert ok.sum() == layout[fam]["built"] and (planes[bc.family_rows(layout, fam)] == want[ok]).all(), fam
        if fam == "pair":                               # exactly the pairs of plane 31 are missing, and for the span
            c = np.repeat(np.arange(33), ND - 1)
            assert (c[~ok] == 31).all() and (~ok).sum() == ND - 1 and (why[~ok] == "the prefix sums span more than 2^32 - 1").all()


def test_unrealisable_planes_say_why():
    P = np.zeros((3, 33), np.uint64)
    P[0, 32] = P[0, 31] = 1                             # delta 0 = 1 0000...0 = -2^32
    P[1, 31] = 3                                        # two deltas of 2^32 - 1
    P[2, 5] = 0b101
    lines, ok, why = bc.lines_for_dbx(32, P)
    assert ok.tolist() == [False, False, True] and len(lines) == 1
    assert why.tolist() == ["a delta is -2^32", "the prefix sums span more than 2^32 - 1", ""]
    assert (bc.dbx_of(lines) == P[2:]).all()


@pytest.mark.parametrize("L", bc.BPC_SIZES)
def test_bpc_built_and_requested(L):
    _, layout = chosen_input(f"bpc_chosen_L{L}")
    ND = L // 4 - 1
    got = {f: (layout[f]["built"], layout[f]["requested"]) for f in bc.BPC_FAMILIES}
    apart = ND * (ND - 1) // 2 - (ND - 1)
    want = {"single": (33 * ND, 33 * ND), "pair": (32 * (ND - 1), 33 * (ND - 1)), "apart": (32 * apart, 33 * apart),
            # three placements of k = 3 .. ND ones per plane; plane 31 never builds (k deltas of 2^32 - 1, or one of -2^32)
            "count_k": (32 * 3 * (ND - 2), 33 * 3 * (ND - 2)),
            # x = one, two and three ones at every row, planes 0..30
            "zero_dbp": (31 * (3 * ND - 3),) * 2, "runs": (561, 561), "mixed": (bc.MIXED_LINES,) * 2,
            "two_runs": (got["two_runs"][1],) * 2, "top": (got["top"][1],) * 2}
    assert got == want
    if L in BPC_BUILT:
        assert {f: got[f] for f in BPC_BUILT[L]} == BPC_BUILT[L]


# ---- the reference's numbers ----------------------------------------------------------------------------------------
def _same(name, comp, got_sizes, got_states, got_stats, arrays, n):
    want = arrays[name + ".sizes"]
    bad = np.nonzero(got_sizes != want)[0]
    assert bad.size == 0, f"{name}: {bad.size} sizes differ, first lines {bad[:5]}: {got_sizes[bad[:5]]} vs {want[bad[:5]]}"
    if comp == "BDI":
        bad = np.nonzero(got_states != arrays[name + ".states"])[0]
        assert bad.size == 0, f"{name}: {bad.size} BDI states differ, first lines {bad[:5]}"
    assert (got_stats == arrays[name + ".stats"]).all(), name


@pytest.mark.parametrize("name", bc.NAMES)
def test_restatement_reproduces_the_reference_on_chosen_lines(name):
    arrays = chosen_fixture()[1]
    case = _case(name)
    lines, _ = chosen_input(name)
    s, k, st = bc.ref(case["comp"], lines)
    _same(name, case["comp"], s, k, st, arrays, len(lines))
    if case["comp"] == "BDI":
        assert (bc.bdi_ref(lines, costs=True)[3] == arrays[name + ".check"]).all()


@pytest.mark.parametrize("name", bc.NAMES)
def test_oracle_reproduces_the_reference_on_chosen_lines(oracle, name):
    arrays = chosen_fixture()[1]
    case = _case(name)
    comp, L = case["comp"], case["L"]
    lines, _ = chosen_input(name)
    o = getattr(oracle, ORACLES[comp])(L)
    out = o.compress(lines)
    stats = arrays[name + ".stats"]
    _same(name, comp, out[0] if comp == "BDI" else out, out[1] if comp == "BDI" else None, stats, arrays, len(lines))
    assert (o.stats_vector() == baseline_ref.stats_vector(comp, len(lines), stats)).all()
    assert o.st.comp_ratio == float(arrays[name + ".ratio"][0])
    if comp == "BDI":
        lib, check = oracle.lib(), arrays[name + ".check"]
        for i in range(0, len(lines), 7):               # mpc_o_bdi_check on every seventh line
            line = np.ascontiguousarray(lines[i])
            assert [lib.mpc_o_bdi_check(line.ctypes.data, L, B, D) for B, D in bc.COMBOS] == check[i].tolist(), (name, i)


@pytest.mark.parametrize("comp", ["BDI", "FPC", "BPC"])
def test_restatement_reproduces_the_reference_on_the_seeded_fixture(comp):
    meta, arrays = old_fixture()
    for case in meta["cases"]:
        if case["comp"] != comp:
            continue
        lines = baseline_ref.case_input(case)
        s, k, st = bc.ref(comp, lines)
        _same(case["name"], comp, s, k, st, arrays, len(lines))


# ---- BDI: the delta limits decide ------------------------------------------------------------------------------------
_CELL = re.compile(r"limits B(\d)D(\d) (\w+) q(\d+) p(\d+) d(.*)")


def limits_cells(L):
    """Per line of the `limits` family: (row, B, D, kind, q, p, index of the delta in LIMIT_DELTAS)."""
    _, layout = chosen_input(f"bdi_chosen_L{L}")
    a, b = layout["limits"]["rows"]
    out = []
    for i in range(a, b):
        m = _CELL.match(layout["cells"][i])
        out.append((i, int(m[1]), int(m[2]), m[3], int(m[4]), int(m[5]), bc.LIMIT_DELTAS.index(m[6])))
    return out


def limits_summary(L):
    """The condition of the `limits` family on the reference's own checkBDI sizes and states.  Deltas 2^(8D)-1, -2 and
    -2^(8D-1) fit: the scan of (B, D) succeeds and (B, D) is the line's state, in every cell.  Deltas 2^(8D), -1 and
    -2^(8D-1)-1 do not: the scan fails, and with the base at value 0 the line goes to another state.  Two kinds of cells
    cannot hold that, and are counted apart:
      immediate  8-byte values, `top` base, delta -2^(8D-1)-1: value p is base + 2^(8D-1) + 1 = 2^64 - 5, an immediate,
                 so that no delta is formed and the scan succeeds;
      cheapest   q >= 1: the scan fails, but q immediates before the base bring its failed size n + 8L - 8 imm (B - D) below
                 8L and below every other combination's, so that (B, D) remains the state."""
    arrays = chosen_fixture()[1]
    name = f"bdi_chosen_L{L}"
    states, check = arrays[name + ".states"], arrays[name + ".check"].astype(np.int64)
    res = {"fit": 0, "misfit": 0, "immediate": 0, "cheapest": 0}
    for i, B, D, kind, q, p, k in limits_cells(L):
        c = bc.COMBOS.index((B, D))
        n = L // B
        ok_cost = n + 8 * (B + (n - 1) * D)
        if k % 2 == 0:
            assert check[i, c] == ok_cost and states[i] == c + 2, (name, i)
            res["fit"] += 1
        elif B == 8 and kind == "top" and k == 5:
            assert check[i, c] == ok_cost, (name, i)
            res["immediate"] += 1
        else:
            assert check[i, c] != ok_cost and check[i, c] <= n + 8 * L - 8 * q * (B - D), (name, i)
            if states[i] == c + 2:
                assert q >= 1 and check[i, c] < 8 * L and check[i, c] == check[i].min(), (name, i)
                res["cheapest"] += 1
            else:
                res["misfit"] += 1
    return res


@pytest.mark.parametrize("L", bc.BDI_SIZES)
def test_bdi_limits_condition(L):
    res = limits_summary(L)
    cells = limits_cells(L)
    assert res["fit"] == len(cells) // 2 and res["misfit"] > 0
    # with the base at value 0 every misfitting line leaves the combination (but the immediates named above)
    assert res["misfit"] >= sum(1 for _, B, D, kind, q, p, k in cells if q == 0 and k % 2 and not (B == 8 and kind == "top" and k == 5))


def floor_summary(L):
    """`floor` family, on the reference's checkBDI sizes: per combination how many lines have its (failed) size below, at
    and above the best of 8L and the earlier combinations' sizes."""
    arrays = chosen_fixture()[1]
    name = f"bdi_chosen_L{L}"
    _, layout = chosen_input(name)
    check = arrays[name + ".check"].astype(np.int64)[bc.family_rows(layout, "floor")]
    out = {}
    best = np.full(len(check), 8 * L, np.int64)
    for c, (B, D) in enumerate(bc.COMBOS):
        out[f"B{B}D{D}"] = [int((check[:, c] < best).sum()), int((check[:, c] == best).sum()), int((check[:, c] > best).sum())]
        best = np.minimum(best, check[:, c])
    return out


@pytest.mark.parametrize("L", bc.BDI_SIZES)
def test_bdi_floor_family_sits_on_both_sides_of_the_best(L):
    res = floor_summary(L)
    for combo, (below, at, above) in res.items():
        assert below > 0 and above > 0, (L, combo)
    # equality needs n + 8 imm' (B' - D') = n' + 8 imm (B - D) in whole numbers: not every pair of combinations has one
    assert sum(at for _, at, _ in res.values()) > 0, L


# ---- wrong variants -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def coverage():
    meta, arrays = chosen_fixture()
    cov = {"built": {}, "reference_counts": {}, "faults": {}, "bdi_limits": {}, "bdi_floor": {}}
    for case in chosen_cases():
        name = case["name"]
        _, layout = chosen_input(name)
        cov["built"][name] = {f: [layout[f]["built"], layout[f]["requested"]] for f in layout if f != "cells"}
        cov["reference_counts"][name] = [int(x) for x in arrays[name + ".stats"][3:]]
    for L in bc.BDI_SIZES:
        cov["bdi_limits"][str(L)] = limits_summary(L)
        cov["bdi_floor"][str(L)] = floor_summary(L)
    old_meta = old_fixture()[0]
    for comp, faults in bc.FAULTS.items():
        chosen = [(c["name"], chosen_input(c["name"])[0]) for c in chosen_cases() if c["comp"] == comp]
        seeded = [baseline_ref.case_input(c) for c in old_meta["cases"] if c["comp"] == comp]
        good = {name: bc.ref_rows(comp, lines) for name, lines in chosen}
        good_seeded = [bc.ref_rows(comp, lines) for lines in seeded]
        for fault in faults:
            per_case = {name: int((bc.ref_rows(comp, lines, fault) != good[name]).any(axis=1).sum()) for name, lines in chosen}
            old = any((bc.ref_rows(comp, lines, fault) != g).any() for lines, g in zip(seeded, good_seeded))
            cov["faults"][f"{comp}.{fault}"] = {"chosen_lines_that_reject": per_case, "seeded_fixture_rejects": bool(old)}
    return cov


def coverage_text():
    return json.dumps(coverage(), indent=1, sort_keys=True) + "\n"


@pytest.mark.parametrize("fault", [f"{comp}.{f}" for comp, faults in bc.FAULTS.items() for f in faults])
def test_every_named_fault_is_rejected(fault):
    per_case = coverage()["faults"][fault]["chosen_lines_that_reject"]
    assert sum(per_case.values()) > 0, fault
    if fault != "BPC.all_ones_at_any_nd":                # (at 31 deltas, 128 bytes, that variant is the reference)
        unrolled = [n for n in per_case if n.rsplit("L", 1)[1] in ("32", "64", "128")]
        assert all(per_case[n] > 0 for n in unrolled), (fault, per_case)


def test_coverage_file_reproduces():
    with open(COVERAGE) as f:
        assert f.read() == coverage_text()


if __name__ == "__main__":
    with open(COVERAGE, "w") as f:
        f.write(coverage_text())
    print(COVERAGE, os.path.getsize(COVERAGE), "bytes")
