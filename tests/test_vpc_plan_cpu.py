"""The VPC planner's decision table, walked without a device (tests/vpc_plan_cases.py).

For every named and drawn configuration, with the run-time compiler predicted and with MPC_JIT=0:
 * mpc_config_describe (path, reason, scan order, needs, runtime_only, general layout, sequence, base form per module)
   equals expected_plan, the table restated from DESIGN.md 4.1c-e;
 * the plan read back from the kernel's own inputs (kernel_base / kernel_shift / kernel_diff: what the planned lane kernel
   reads and does per byte, mpc::read_back_vpc_module) agrees with the configuration's BaseIndexTable, WeightTable and
   DiffTable.  A WeightBase module with BaseIndexTable[i] = i - 8 and three or more shift distances used to be planned
   as "windowed" with the selectors of an i - 4 table; this test then failed with
     back8_3_shift_classes_root_0_L128 (compiler): module 2: kernel_base[8] = 4, BaseIndexTable[8] = 0
The cases reach every row of the table and every base form at least twice; the drawn cases' bytes are all free; the
walking-one family of every free module builds completely, and the oracle that the GPU test trusts agrees with the live
reference build, where there is one, on every built line."""
import pytest

from conftest import pkg

import vpc_plan_cases as P
import vpc_synth as S


@pytest.fixture(scope="module")
def mpc():
    m = pkg()
    m.lib()
    return m


def _describe(mpc, monkeypatch, cfg, compiler):
    monkeypatch.delenv("MPC_JIT_MAX_MODULES", raising=False)
    if compiler:
        monkeypatch.delenv("MPC_JIT", raising=False)
    else:
        monkeypatch.setenv("MPC_JIT", "0")
    d = mpc.describe_config(cfg)
    assert d["rc"] == 0, d
    return d


def check_read_back(name, cfg, d, want):
    """The read-back of every prediction module against the configuration's own tables."""
    L, pm = P._pred(cfg)
    for m in pm:
        got, tag = d["modules"][m["k"]], f"{name}: module {m['k']}"
        kb = got["kernel_base"]
        assert len(kb) == L, tag
        if m["kind"] in ("OneBase", "ConsecutiveBase"):
            assert kb == [-1] * L and "kernel_shift" not in got and "kernel_diff" not in got and "base_form" not in got, tag
            continue
        assert got["base_form"] == want["base_form"][m["k"]], f"{tag}: base_form {got['base_form']!r}, expected {want['base_form'][m['k']]!r}"
        weight = m["kind"] == "WeightBase"
        const = got["kernel_shift" if weight else "kernel_diff"]
        assert ("kernel_diff" if weight else "kernel_shift") not in got and len(const) == L, tag
        for i, x in enumerate(P.module_tables(m, L)):
            if x is None:
                assert kb[i] == -1 and const[i] == (99 if weight else 0), f"{tag}: root byte {i}: kernel_base {kb[i]}, constant {const[i]}"
                continue
            b, c = x
            assert const[i] == c, f"{tag}: kernel_{'shift' if weight else 'diff'}[{i}] = {const[i]}, the table's is {c}"
            if not (weight and c == 99):
                assert kb[i] == b, f"{tag}: kernel_base[{i}] = {kb[i]}, BaseIndexTable[{i}] = {b}"


@pytest.mark.parametrize("compiler", [True, False], ids=["compiler", "MPC_JIT=0"])
@pytest.mark.parametrize("name", list(P.ALL))
def test_plan_is_the_table_and_reads_the_configured_bytes(mpc, monkeypatch, name, compiler):
    cfg = P.ALL[name]()
    d = _describe(mpc, monkeypatch, cfg, compiler)
    want = P.expected_plan(cfg, compiler)
    got = {"path": d["path"], "reason": P.reason_category(d["why_generic"]), "scan_order": d["scan_order"], "needs": d["needs"],
           "runtime_only": d["runtime_only"], "general_layout": d["general_layout"], "sequence": d["sequence"]}
    assert got == {k: want[k] for k in got}, f"{name} ({'compiler' if compiler else 'MPC_JIT=0'}): {d['why_generic']!r}"
    L, pm = P._pred(cfg)
    planned = "kernel_base" in d["modules"][pm[0]["k"]]
    assert planned == (want["path"] == "fast" or want["reason"] == "no compiler"), name
    if planned:
        check_read_back(f"{name} ({'compiler' if compiler else 'MPC_JIT=0'})", cfg, d, want)


def test_cases_reach_every_row_and_base_form():
    rows, forms = dict.fromkeys(P.ROWS, 0), dict.fromkeys(P.BASE_FORMS, 0)
    for name, make in P.ALL.items():
        want = P.expected_plan(make(), True)
        rows[want["row"]] += 1
        for f in set(want["base_form"].values()):
            forms[f] += 1
    print("cases per row:", rows)
    print("cases per base form:", forms)
    assert set(rows) == set(P.ROWS) and min(rows.values()) >= 2, rows
    assert min(forms.values()) >= 2, forms
    # both columns of the table: every sequence with and without the compiler
    seqs = {(c, P.expected_plan(make(), c)["sequence"]) for make in P.ALL.values() for c in (True, False)}
    assert seqs == {(True, "unrolled"), (True, "run-time loop"), (True, ""), (False, "unrolled"), (False, "run-time loop"), (False, "")}


def test_drawn_and_listed_cases_have_free_bytes():
    for name, make in P.ALL.items():
        cfg = make()
        L, pm = P._pred(cfg)
        # (ConsecutiveBase has no table: its sources are the byte-plane-shuffled order, which the families account for)
        free = [S.is_free(S.residue_constraints(cfg, m["k"])) for m in pm if m["kind"] != "ConsecutiveBase"]
        if name in P.NOT_FREE:
            assert not all(free), f"{name} is listed as not free but is"
            continue
        assert all(free), (name, free)
        if name in P.DRAWN:
            for m in pm:
                if m["kind"] in ("DiffBase", "WeightBase"):
                    for i, x in enumerate(P.module_tables(m, L)):
                        assert x is None or x[0] < i or x[0] // 4 == i // 4, (name, m["k"], i, x)


@pytest.mark.parametrize("L", P.SIZES)
def test_walking_one_builds_and_oracle_matches_reference(oracle, L):
    """vpc_synth.build counts a line as built only when the oracle's scanned array of it (and the reference's own stages',
    where oracle/_ref is built) is the requested one: nothing may be refused for a free module, nothing NOT VERIFIED."""
    for name, make in P.ALL.items():
        cfg = make()
        if int(cfg["overview"]["lineSize"]) != L:
            continue
        for b in S.build(cfg, families=("walking_one",)):
            assert "NOT VERIFIED" not in b["refused"], (name, b["module"], b["refused"])
            if S.is_free(S.residue_constraints(cfg, b["module"])):
                assert not b["refused"] and len(b["lines"]) == b["requested"], (name, b["module"], b["refused"])
            if name in P.NAMED and oracle.ref_lib() is not None and len(b["lines"]):
                ours = S.oracle_scanned(cfg, b["module"], b["lines"])
                assert (ours == S.oracle_scanned(cfg, b["module"], b["lines"], ref=True)).all() and (ours == b["rows"]).all(), (name, b["module"])
