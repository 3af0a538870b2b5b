"""The synthesiser of tests/vpc_synth.py and its line families, on the CPU oracle alone.

The synthesiser is right: every line it calls built gives the requested scanned array back exactly through the oracle's
mpc_o_scanned (and through the reference's own stage classes where oracle/_ref is built), every refusal names a
constraint that residue_constraints reports, and a module without forced bytes and cycles builds every request.

The families do what they claim: per configuration and module what was built, how often the oracle's selector picks the
target module, what is kept and what ends uncompressed, which (module, row, column) places of the winners' scanned
arrays show a single one and an adjacent pair, and which encoder sizes the threshold ladder reaches around 8 L.  The
counts are the oracle's and are stored in tests/golden/vpc_synth_coverage.json; the test regenerates the file's text
byte for byte, so the generators cannot drift unnoticed.  (Rewrite it with `python tests/test_vpc_synth_cpu.py`.)"""
import functools
import json
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import ROOT, pkg  # noqa: E402

import vpc_ref  # noqa: E402
import vpc_synth as S  # noqa: E402
from vpc_synth_cases import ALL, COMPANIONS, built, config_of, filler, form_of, needs_companion  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "vpc_synth_coverage.json")


# ---- coverage -------------------------------------------------------------------------------------------------------
def _places(scanned: np.ndarray):
    """(row, column) places at which rows of [n, R] scanned arrays hold a single one / an adjacent pair (left column)."""
    one, pair = set(), set()
    for c in range(16):
        for r in np.unique(np.nonzero(scanned == np.uint16(1 << (15 - c)))[1]):
            one.add((int(r), c))
        if c < 15:
            for r in np.unique(np.nonzero(scanned == np.uint16(3 << (14 - c)))[1]):
                pair.add((int(r), c))
    return one, pair


def winner_places(cfg: dict, lines: np.ndarray):
    """Over the lines that reach the selector: {(module, row, column)} of single ones and of adjacent pairs in the winning
    module's scanned array."""
    O = S._oracle()
    pm = S.pred_modules(cfg)
    _, sel = O.VpcOracle(cfg).compress(lines)
    lines = lines[(sel < 0) | (sel >= pm[0])]
    sc = [S.oracle_scanned(cfg, k, lines) for k in pm]
    nz = [s != 0 for s in sc]
    z = np.stack([np.where(m.any(axis=1), np.argmax(m, axis=1), m.shape[1]) for m in nz], axis=1)
    win = vpc_ref.winner(z)
    one, pair = set(), set()
    for q, k in enumerate(pm):
        o, p = _places(sc[q][win == q])
        one |= {(k,) + x for x in o}
        pair |= {(k,) + x for x in p}
    return one, pair


@functools.lru_cache(maxsize=None)
def coverage(name: str) -> dict:
    cfg = config_of(name)
    O = S._oracle()
    L, pm = int(cfg["overview"]["lineSize"]), S.pred_modules(cfg)
    out = {"line_size": L, "form": form_of(name), "modules": {}, "families": []}
    for k in pm:
        cons = S.residue_constraints(cfg, k)
        out["modules"][str(k)] = {"kind": cons["kind"], "forced_bytes": sorted(cons["forced"]),
                                  "cycles": [len(c["bytes"]) for c in cons["cycles"]], "requested": 0, "built": 0}
    pool = []
    for b in built(name):
        k, lines = b["module"], b["lines"]
        rec = {"family": b["family"], "module": k, "requested": b["requested"], "built": len(lines),
               "refused": dict(sorted(b["refused"].items()))}
        out["modules"][str(k)]["requested"] += b["requested"]
        out["modules"][str(k)]["built"] += len(lines)
        if len(lines):
            z = S.leading_zero_rows(cfg, lines)
            _, sel = O.VpcOracle(cfg).compress(lines)
            rec["target_wins"] = int((np.array(pm)[vpc_ref.winner(z)] == k).sum())
            rec["kept_by_target"] = int((sel == k).sum())
            rec["kept_by_other"] = int(((sel >= 0) & (sel != k)).sum())
            rec["uncompressed"] = int((sel == -1).sum())
            if b["family"] == "ladder":
                enc = S.fpc_sizes(b["rows"]) - 8 * L
                rec["sizes_minus_8L"] = sorted({int(e) for e in enc if abs(e) <= 20})
                rec["below_8L"], rec["below_8L_kept_by_target"] = int((enc < 0).sum()), int(((enc < 0) & (sel == k)).sum())
                rec["from_8L"], rec["from_8L_uncompressed"] = int((enc >= 0).sum()), int(((enc >= 0) & (sel == -1)).sum())
            pool.append(lines)
        out["families"].append(rec)
    one, pair = winner_places(cfg, np.concatenate(pool)) if pool else (set(), set())
    out["winner_places"] = {"single_one": len(one), "single_one_of": 16 * 8 * L // 16 * len(pm),
                            "adjacent_pair": len(pair), "adjacent_pair_of": 15 * 8 * L // 16 * len(pm)}
    return out


def natural_mix(L: int) -> np.ndarray:
    """The largest natural mix a parity test uses (test_vpc_general_layout_twins)."""
    T = pkg("traces")
    return np.concatenate([T.structured(5000, L, seed=23), T.mixed(2500, L), T.random_u32(800, L), T.sine_f32(1024, L),
                           T.counters_u32(500, L), T.zeros(70, L), T.word_same(70, L)])


@functools.lru_cache(maxsize=None)
def before_after() -> dict:
    """Winner coverage of the probe configuration at 64 bytes: the natural mix alone, and with the synthesised families."""
    cfg = config_of("probe_L64")
    o0, p0 = winner_places(cfg, natural_mix(64))
    o1, p1 = winner_places(cfg, np.concatenate([b["lines"] for b in built("probe_L64")]))
    return {"configuration": "probe_L64", "natural_mix": {"single_one": len(o0), "adjacent_pair": len(p0)},
            "natural_mix_and_families": {"single_one": len(o0 | o1), "adjacent_pair": len(p0 | p1)},
            "single_one_of": 2048, "adjacent_pair_of": 1920}


def golden_text() -> str:
    doc = {"about": "counts of the CPU oracle for the line families of tests/vpc_synth.py (tests/test_vpc_synth_cpu.py)",
           "before_after": before_after(), "configurations": {name: coverage(name) for name in ALL}}
    text = json.dumps(doc, indent=1, sort_keys=True)
    return re.sub(r"\n {3,}", " ", text) + "\n"          # (one line per family record)


# ---- the synthesiser is right ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_built_lines_give_the_requested_array_and_refusals_name_a_constraint(name):
    cfg = config_of(name)
    for b in built(name):
        k = b["module"]
        cons, m = S.residue_constraints(cfg, k), S.Module(cfg, k)
        assert "NOT VERIFIED" not in b["refused"], (name, b["family"], k, b["refused"])
        # (build verified every line it kept; once more here, on its own, through the oracle and oracle/_ref)
        assert (S.oracle_scanned(cfg, k, b["lines"]) == b["rows"]).all(), (name, b["family"], k)
        if S._oracle().ref_lib() is not None:
            assert (S.oracle_scanned(cfg, k, b["lines"], ref=True) == b["rows"]).all(), (name, b["family"], k)
        named = {f"forced byte {p}" for p in cons["forced"]} | {f"cycle of {len(c['bytes'])} bytes through byte {min(c['bytes'])}" for c in cons["cycles"]}
        assert set(b["refused"]) <= named, (name, b["family"], k, set(b["refused"]) - named)
        if S.is_free(cons):
            assert not b["refused"] and len(b["lines"]) == b["requested"], (name, b["family"], k, b["refused"])
        assert (b["rows"] & ~m.table_mask() == 0).all()


def test_constraints_of_known_modules():
    """Byte 0 under _prev(L, 4) with a root other than 0 is its own base: DiffBase forces -Diff, WeightBase b - shift(b);
    ConsecutiveBase has cycles whose residues sum to 0; the probe's other modules are free."""
    cfg = config_of("root1_L64")
    d, w = S.residue_constraints(cfg, 4), S.residue_constraints(cfg, 5)
    assert d["forced"] == {0: [255]} and not d["cycles"] and 0 not in d["free"] and d["root"] == 1
    assert w["forced"] == {0: [0]} and w["residue_index"][0] == 1 and w["residue_index"][1] == 0
    c = S.residue_constraints(config_of("probe_L64"), 3)
    assert c["kind"] == "ConsecutiveBasePredictor" and c["cycles"] and all(x["sum"] == 0 for x in c["cycles"])
    for k in (2, 4, 5):
        assert S.is_free(S.residue_constraints(config_of("probe_L64"), k))
    # a refused request and a granted one, through the one-line entry point
    rows = np.zeros(32, np.uint16)
    assert S.line_for_scanned(cfg, 4, rows) is None                       # all-zero residues: byte 0 would need 0xFF
    rows[5] = 0x0180
    line = S.line_for_scanned(cfg, 2, rows)
    assert line is not None and line[1] == 0 and (S.oracle_scanned(cfg, 2, line[None, :])[0] == rows).all()
    rows[0] = 0x8000                                                      # the MSB of the raw root
    assert S.line_for_scanned(cfg, 2, rows)[1] == 0x80
    bad = np.zeros(32, np.uint16)
    bad[31] = 1
    assert S.line_for_scanned(config_of("trunc_L64"), 2, bad) is None     # a cell outside a truncated table


@pytest.mark.parametrize("name", ["probe_L64", "jit_bytemajor_L64", "perm_one_last_L64", "trunc_L64", "jit_root40_L64",
                                  "jit_weights_L64", "L48"])
def test_random_arrays_round_trip_on_free_modules(name):
    cfg = config_of(name)
    rng = np.random.default_rng(5)
    for k in S.pred_modules(cfg):
        m = S.Module(cfg, k)
        rows = rng.integers(0, 1 << 16, (200, m.R), dtype=np.uint32).astype(np.uint16) & m.table_mask()
        _, ok, reason = S.lines_for_scanned(cfg, k, rows)
        assert "NOT VERIFIED" not in set(reason[~ok]), (name, k)
        if S.is_free(S.residue_constraints(cfg, k)):
            assert ok.all(), (name, k, set(reason[~ok]))


# ---- the families do what they claim --------------------------------------------------------------------------------
def test_arrangements_hold_every_built_line_at_the_promised_places():
    b = built("probe_L32")
    n = sum(len(x["lines"]) for x in b)
    pool = np.concatenate([x["lines"] for x in b])
    for arrangement in ("dense", "planted", "cold"):
        calls = S.arrange(b, 32, arrangement, filler)
        assert [len(c[0]) % 128 for c in calls] == list(S.TAILS)
        org = np.concatenate([c[1] for c in calls])
        lines = np.concatenate([c[0] for c in calls])
        assert set(org[org >= 0]) == set(range(n)) and (lines[org >= 0] == pool[org[org >= 0]]).all()
        if arrangement == "planted":
            at = np.nonzero(org >= 0)[0]
            assert set(at % 64) == set(S.PLANT_LANES) and len(lines) >= 64 * n // 3
        if arrangement == "cold":          # built lines in the second group of a block only, per call
            for c in calls:
                assert ((np.nonzero(c[1] >= 0)[0] // 64) % 2 == 1).all()
    assert len(S.index(b)) == n
    # a sample per (family, module): every one of them stays in, in order
    calls = S.arrange(b, 32, "planted", filler, per_family=50)
    org = np.concatenate([c[1] for c in calls])
    idx = S.index(b)
    kept = org[org >= 0]
    assert {(idx[i][0], idx[i][1]) for i in kept} == {(x["family"], x["module"]) for x in b if len(x["lines"])}
    assert len(set(kept)) == sum(min(50, len(x["lines"])) for x in b)


@pytest.mark.parametrize("name", ALL)
def test_conditions(name):
    cfg, cov = config_of(name), coverage(name)
    pm = S.pred_modules(cfg)
    # a module that wins at least half of its own walking-one lines
    shares = [f["target_wins"] / f["built"] for f in cov["families"] if f["family"] == "walking_one" and f["built"]]
    assert shares and max(shares) >= 0.5, (name, shares)
    # what could not be built: more than a quarter only for ConsecutiveBase modules and modules with forced bytes
    for k, m in cov["modules"].items():
        if 4 * (m["requested"] - m["built"]) > m["requested"]:
            assert m["kind"] == "ConsecutiveBasePredictor" or m["forced_bytes"], (name, k, m)
    if needs_companion(cfg):
        assert name not in COMPANIONS and any(of == name for of, _, _ in COMPANIONS.values()), name
        return
    # the ladder of the last (free) module: kept below 8 L, uncompressed from 8 L on
    lad = next(f for f in cov["families"] if f["family"] == "ladder")
    assert lad["module"] == pm[-1] and lad["built"] == lad["requested"], (name, lad)
    assert 4 * lad["below_8L_kept_by_target"] >= 3 * lad["below_8L"], (name, lad)
    assert lad["from_8L_uncompressed"] == lad["from_8L"], (name, lad)
    # A truncated table leaves zero rows, so every size stays below 8 L there (trunc_L64, trunc16_L32, jit_planes_L32,
    # loop_trunc12_L32): those ladders cannot cross, test_every_form_has_a_ladder_across_8L asks it of the form instead.
    if S.Module(cfg, pm[-1]).ts == 8 * cov["line_size"]:
        assert lad["below_8L"] > 0 and lad["from_8L"] > 0, (name, lad)
        if cov["line_size"] >= 32:                            # (16 rows and more: the row costs reach within 3 bits of 8 L)
            near = set(lad["sizes_minus_8L"])
            assert near & {-3, -2, -1} and near & {0, 1, 2, 3}, (name, lad)


@pytest.mark.parametrize("form", vpc_ref.FORMS)
def test_every_form_has_a_ladder_across_8L(form):
    """Per kernel form at least two configurations whose ladder is built in full and puts sizes on both sides of 8 L, within 3 bits of it: only there does 'every line from 8 L on is
    uncompressed' say something, and only there can the incompressibility certificate close a line."""
    crossing = []
    for name in ALL:
        cov = coverage(name)
        lad = [f for f in cov["families"] if f["family"] == "ladder" and f["built"] == f["requested"] and f.get("from_8L", 0) > 0]
        if cov["form"] == form and lad and lad[0]["below_8L"] > 0:
            near = set(lad[0]["sizes_minus_8L"])
            if near & {-3, -2, -1} and near & {0, 1, 2, 3}:
                crossing.append(name)
    assert len(crossing) >= 2, (form, crossing)


@pytest.mark.parametrize("name", sorted(COMPANIONS))
def test_companions_keep_the_form_of_the_configuration_they_stand_in_for(name):
    of, form, make = COMPANIONS[name]
    assert form == vpc_ref._SPECS[of]["form"] and needs_companion(vpc_ref._CONFIGS[of]()) and not needs_companion(make())
    mpc = pkg()
    d = mpc.describe_config(make())
    assert d["rc"] == 0 and vpc_ref.described_form(d) == form, (name, d)


def test_coverage_file_is_reproduced_byte_for_byte():
    with open(GOLDEN) as f:
        want = f.read()
    got = golden_text()
    if got != want:
        a, b = json.loads(want), json.loads(got)
        diff = [n for n in ALL if a["configurations"].get(n) != b["configurations"].get(n)]
        raise AssertionError(f"tests/golden/vpc_synth_coverage.json differs: configurations {diff}, "
                             f"before_after {a.get('before_after')} vs {b['before_after']}")


if __name__ == "__main__":
    with open(GOLDEN, "w") as f:
        f.write(golden_text())
    print(GOLDEN, os.path.getsize(GOLDEN), "bytes")
