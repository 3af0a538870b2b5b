"""Configurations that walk the VPC planner's decision table (build_vpc_plan, csrc/mpc_config.h; route_vpc,
csrc/mpc_capi.hip), and the table written again (tests/test_vpc_plan_cpu.py, tests/test_vpc_plan_gpu.py).

NAMED: boundary cases, each with one threshold of the table on both of its sides -- TableSize, roots, the window of the
base bytes, the shift classes of a WeightTable, DiffTable entries outside a byte, the number of prediction modules, the
room the line rings have beside the histogram, and pairs of conditions the table sends to the generic kernel.  A case
runs at one line size (32 / 64 / 128 in turn over the list); those made with `all_l` run at all three.
DRAWN: 24 seeded configurations per line size that draw every axis independently from the same values.
Base tables of the drawn cases have base[i] < i or stay inside the own dword and lead to the root, so every byte but
the root is free (vpc_synth.is_free); the named cases in NOT_FREE have a byte that is its own source or a cycle.

expected_plan restates DESIGN.md 4.1c-e: which layouts the built-in kernels have, which a kernel compiled at creation
has, what the run-time module loop has, and what is left to the generic kernel.  numpy and configs.py only."""
import importlib
import itertools
import math
import os
import sys

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)
C = importlib.import_module("cal_22-mpc_amd.configs")

AZ, AWS = {"name": "AllZero"}, {"name": "AllWordSame"}
SIZES = (32, 64, 128)


# ---- building blocks ------------------------------------------------------------------------------------------------
def plane(L, ts):
    return {"TableSize": ts, "Rows": [i // L for i in range(ts)], "Cols": [i % L for i in range(ts)]}


def byte(L, ts):
    return {"TableSize": ts, "Rows": [i % 8 for i in range(ts)], "Cols": [i // 8 for i in range(ts)]}


def permuted(L, seed):
    p = np.random.default_rng(seed).permutation(8 * L)
    return {"TableSize": 8 * L, "Rows": [int(q) // L for q in p], "Cols": [int(q) % L for q in p]}


def prev(L, e, root=0):
    """base[i] = i - e (byte 0 where that is before the line); the bytes before a root inside word 0 take the root."""
    return [root if i < root else max(i - e, 0) for i in range(L)]


def cyc(L, values, shift=0):
    return [values[(i + shift) % len(values)] for i in range(L)]


def patched(table, **at):
    t = list(table)
    for i, v in at.items():
        t[int(i[1:])] = v
    return t


def seq(L, mods, bits=None, aws=True):
    mods = [AZ] + ([AWS] if aws else []) + list(mods)
    return C.make_config(L, mods, bits(len(mods)) if callable(bits) else bits)


def two(L, scan_a=None, scan_b=None, root_a=0, root_b=0):
    """OneBase and a periodic DiffBase (i - 4): a built-in sequence without the probe's four compilations."""
    return [C.one_base(L, root_a, True, scan_a), C.diff_base(L, prev(L, 4, root_b), cyc(L, [1, 0, 0, 0]), root_b, False, scan_b)]


NAMED, NOT_FREE = {}, set()
_turn = itertools.cycle(SIZES)


def case(name, make, all_l=False, free=True):
    for L in (SIZES if all_l else (next(_turn),)):
        full = f"{name}_L{L}"
        assert full not in NAMED, full
        NAMED[full] = (lambda L=L: make(L))
        if not free:
            NOT_FREE.add(full)


# ---- TableSize ------------------------------------------------------------------------------------------------------
for _ts in ("0", "1", "15", "16", "17", "L-1", "L", "L+1", "3*L", "8*L-1", "8*L"):
    case(f"plane_ts_{_ts}", lambda L, e=_ts: seq(L, two(L, plane(L, eval(e)), plane(L, eval(e)))))
for _ts in ("15", "16", "8*L-8", "8*L"):
    case(f"byte_ts_{_ts}", lambda L, e=_ts: seq(L, two(L, byte(L, eval(e)), byte(L, eval(e)))), all_l=True)
case("one_entry_both_orders", lambda L: seq(L, [C.consecutive_base(L, 0, True, byte(L, 1)), C.one_base(L, 0, False, plane(L, 1))]))
case("planes_4_and_6", lambda L: seq(L, two(L, plane(L, 4 * L), plane(L, 6 * L))))
case("planes_8_and_1", lambda L: seq(L, two(L, None, plane(L, L))))
case("cut_among_whole_planes", lambda L: seq(L, two(L, plane(L, 4 * L), plane(L, 5 * L + 7))))
case("byte_major_among_plane_major", lambda L: seq(L, two(L, None, byte(L, 8 * L))))
case("plane_major_among_byte_major", lambda L: seq(L, two(L, byte(L, 8 * L), None)))
case("one_module_permuted", lambda L: seq(L, two(L, None, permuted(L, 9))))
# ---- roots ----------------------------------------------------------------------------------------------------------
for _r in ("15", "16", "L-1"):
    case(f"onebase_root_{_r}", lambda L, e=_r: seq(L, two(L, root_a=eval(e))))
case("root_16_and_planes_differ", lambda L: seq(L, two(L, plane(L, 4 * L), plane(L, 6 * L), root_a=16)))
case("root_15_and_planes_differ", lambda L: seq(L, two(L, plane(L, 4 * L), plane(L, 6 * L), root_a=15)))
case("byte_major_root_0", lambda L: seq(L, two(L, byte(L, 8 * L), byte(L, 8 * L))))
case("byte_major_root_1", lambda L: seq(L, two(L, byte(L, 8 * L), byte(L, 8 * L), root_a=1)))
case("back8_root_7", lambda L: seq(L, [C.diff_base(L, prev(L, 8), cyc(L, [1, 0, 0, 0, 0, 0, 0, 0]), 7, True)]), free=False)
case("back8_root_8", lambda L: seq(L, [C.diff_base(L, prev(L, 8), cyc(L, [1, 0, 0, 0, 0, 0, 0, 0]), 8, True)]), free=False)
# ---- bases (byte 13: word 3, whose window is bytes 8..15) -----------------------------------------------------------
_d = [2, -1, 0, 1]
case("base_window_low_edge", lambda L: seq(L, [C.diff_base(L, patched(prev(L, 4), i13=8), cyc(L, _d), 0, True)]))
case("base_below_window", lambda L: seq(L, [C.diff_base(L, patched(prev(L, 4), i13=7), cyc(L, _d), 0, True)]))
case("base_window_high_edge", lambda L: seq(L, [C.diff_base(L, patched(prev(L, 4), i13=15), cyc(L, _d), 0, True)]))
case("base_above_window", lambda L: seq(L, [C.diff_base(L, patched(prev(L, 4), i13=16), cyc(L, _d), 0, True)]))
case("base_4_in_word_0", lambda L: seq(L, [C.weight_base(L, patched(prev(L, 4), i2=4), cyc(L, [1.0, 0.5]), 0, True)]))
case("base_is_own_byte", lambda L: seq(L, [C.diff_base(L, patched(prev(L, 4), i13=13), cyc(L, _d), 0, True)]), free=False)
case("forward_in_own_dword", lambda L: seq(L, [C.weight_base(L, patched(prev(L, 4), i12=14), cyc(L, [1.0, 0.5]), 0, False)]))
case("back4_periodic", lambda L: seq(L, [C.diff_base(L, prev(L, 4), cyc(L, _d), 0, True), C.one_base(L, 0, False)]))
case("back4_one_word_differs", lambda L: seq(L, [C.diff_base(L, prev(L, 4), patched(cyc(L, _d), i21=5), 0, True), C.one_base(L, 0, False)]))
case("back8_repeating", lambda L: seq(L, [C.weight_base(L, prev(L, 8), cyc(L, [1.0, 1.0, 0.5, 0.5, 1.0, 0.5, 0.5, 0.5]), 0, True)]))
case("back8_not_repeating", lambda L: seq(L, [C.diff_base(L, prev(L, 8), cyc(L, [-3, -2, -1, 0, 1, 2, 3]), 0, True)]))
for _n, _r in itertools.product((3, 4), (0, 5)):
    case(f"back8_{_n}_shift_classes_root_{_r}",
         lambda L, n=_n, r=_r: seq(L, [C.weight_base(L, prev(L, 8), cyc(L, [1.0, 0.5, 0.25, 2.0][:n]), r, True)]), free=_r == 0)
case("back8_two_classes_root_5", lambda L: seq(L, [C.weight_base(L, prev(L, 8), cyc(L, [1.0, 0.5]), 5, True)]), free=False)
case("back8_gathered_byte_in_word_1", lambda L: seq(L, [C.diff_base(L, patched(prev(L, 8), i5=9), cyc(L, [1, 0]), 0, False)]))
case("back8_gathered_byte_in_word_0", lambda L: seq(L, [C.weight_base(L, patched(prev(L, 8), i2=6), cyc(L, [1.0, 0.5]), 0, False)]))
# ---- weights --------------------------------------------------------------------------------------------------------
for _name, _w in (("one_class", [1.0]), ("one_shifted_class", [0.5]), ("classes_0_and_minus", [1.0, 0.25]), ("classes_plus_then_0", [1.0, 4.0]),
                  ("classes_0_and_plus", [4.0, 1.0]), ("classes_plus_and_minus", [0.5, 2.0]), ("classes_minus_and_minus", [0.25, 0.5]),
                  ("three_classes", [1.0, 0.5, 0.25]), ("two_classes_and_no_class_entries", [1.0, 256.0, 0.5, 1 / 256, 512.0, 1.0, 1 / 512]),
                  ("shifts_of_7", [128.0, 1 / 128]), ("shifts_of_8", [256.0, 1 / 256]), ("not_powers_of_two", [3.0, 0.3, 3.9, 0.49])):
    # (byte 0 is the root: byte 1, the first to get a class, takes the SECOND entry of the cycle)
    case(f"weights_{_name}", lambda L, w=_w: seq(L, [C.one_base(L, 0, True), C.weight_base(L, prev(L, 4), cyc(L, w), 0, False)]))
case("weights_three_classes_back1", lambda L: seq(L, [C.weight_base(L, prev(L, 1), cyc(L, [1.0, 2.0, 0.5]), 0, True)]))
case("diffs_outside_a_byte", lambda L: seq(L, [C.diff_base(L, prev(L, 1), cyc(L, [200, -200, 128, -129, 127, -128, 300]), 0, True)]))
# ---- sequence length, LDS -------------------------------------------------------------------------------------------
def _many(L, n):
    return [C.one_base(L, j % 4, bool(j & 1)) if j % 3 else C.diff_base(L, prev(L, 1 + j % 4), cyc(L, [j % 5 - 2, 0]), 0, bool(j & 2))
            for j in range(n)]


case("modules_12", lambda L: seq(L, _many(L, 12)))
case("modules_13", lambda L: seq(L, _many(L, 13)))
# 128-byte lines, four clusters: 8 waves' rings leave 32 KiB for sums and histogram, 7 / 6 / 5 / 4 waves 48 / 64 / 80 / 96 KiB
for _bits in (500, 900, 3700, 4000):
    NAMED[f"rings_id_bits_{_bits}_L128"] = lambda b=_bits: seq(128, [C.one_base(128, 0, True), C.one_base(128, 2, False)], bits=[3, 3, b, 3, 3])
    NAMED[f"rings_built_in_id_bits_{_bits}_L128"] = lambda b=_bits: seq(128, two(128), bits=[3, 3, b, 3, 3])
# ---- two conditions at once -----------------------------------------------------------------------------------------
case("gather_and_ts_15", lambda L: seq(L, [C.diff_base(L, prev(L, 12), cyc(L, _d), 0, True, plane(L, 15))]))
case("gather_and_ts_16", lambda L: seq(L, [C.diff_base(L, prev(L, 12), cyc(L, _d), 0, True, plane(L, 16))]))
case("many_shifts_and_root_16", lambda L: seq(L, [C.one_base(L, 16, True), C.weight_base(L, prev(L, 4), cyc(L, [1.0, 0.5, 0.25]), 0, False)]))
case("many_shifts_and_root_15", lambda L: seq(L, [C.one_base(L, 15, True), C.weight_base(L, prev(L, 4), cyc(L, [1.0, 0.5, 0.25]), 0, False)]))
case("gather_and_planes_differ", lambda L: seq(L, [C.one_base(L, 0, True, plane(L, 4 * L)), C.diff_base(L, prev(L, 12), cyc(L, _d), 0, True, plane(L, 6 * L))]))
case("gather_and_byte_major", lambda L: seq(L, [C.diff_base(L, prev(L, 16), cyc(L, _d), 0, True, byte(L, 8 * L))]))
case("back8_many_shifts_and_root_16", lambda L: seq(L, [C.one_base(L, 16, True), C.weight_base(L, prev(L, 8), cyc(L, [1.0, 0.5, 0.25]), 0, False)]))

BACK8_MANY_SHIFTS = sorted(n for n in NAMED if n.startswith("back8_3_shift") or n.startswith("back8_4_shift"))


# ---- seeded draws ---------------------------------------------------------------------------------------------------
WEIGHT_SETS = ([1.0], [1.0, 0.25], [4.0, 1.0], [0.5, 2.0], [0.25, 0.5], [1.0, 0.5, 0.25], [1.0, 0.5, 0.25, 2.0],
               [1.0, 256.0, 0.5, 1 / 512], [128.0, 1 / 128], [256.0, 1 / 256], [3.0, 0.3])


def _drawn_base(rng, L, root, how):
    """A base table whose every byte leads to the root (root 0..3): base[i] < i, or the root / a later byte of the own
    dword."""
    if how == "windowed":
        b = [int(rng.integers(max(4 * (i // 4) - 4, 0), i)) if i else 0 for i in range(L)]
    elif how == "below_window":
        b = prev(L, 4)
        b[13] = 7
    elif how == "anywhere":
        b = [int(rng.integers(0, i)) if i else 0 for i in range(L)]
    elif how == "forward_in_dword":
        b = prev(L, 4)
        b[12] = 14
    else:
        b = prev(L, int(how))
    return [root if i < root else b[i] for i in range(L)]


def draw(L, j):
    rng = np.random.default_rng(1000 * L + j)
    pick = lambda values: values[int(rng.integers(0, len(values)))]      # noqa: E731
    order = pick(("plane", "plane", "plane", "byte"))
    if order == "plane":
        ts = pick((0, 1, 15, 16, 17, L - 1, L, L + 1, 3 * L, 8 * L - 1, 8 * L, 8 * L, 8 * L, 8 * L))
    else:
        ts = pick((15, 16, 8 * L - 8, 8 * L, 8 * L))
    own_planes = order == "plane" and rng.random() < 0.15
    mods = []
    for _ in range(int(rng.integers(1, 7))):
        kind = pick(("one", "consec", "diff", "weight", "diff", "weight"))
        scan = (plane if order == "plane" else byte)(L, L * int(rng.integers(1, 9)) if own_planes else ts)
        cx = bool(rng.integers(0, 2))
        if kind == "one":
            mods.append(C.one_base(L, pick((0, 0, 0, 1, 5, 7, 8, 15, 16, L - 1)), cx, scan))
        elif kind == "consec":
            mods.append(C.consecutive_base(L, 0, cx, scan))
        else:
            root = pick((0, 0, 0, 1, 3))
            base = _drawn_base(rng, L, root, pick(("1", "4", "4", "8", "8", "windowed", "below_window", "anywhere", "forward_in_dword")))
            if kind == "diff":
                diff = cyc(L, pick(([0], [1, 0, 0, 0], [1, 0, 0, 0, 0, 0, 0, 0], [int(x) for x in rng.integers(-4, 5, 7)],
                                    [200, -200, 128, -129])))
                mods.append(C.diff_base(L, base, diff, root, cx, scan))
            else:
                w = pick(WEIGHT_SETS)
                mods.append(C.weight_base(L, base, cyc(L, w, int(rng.integers(0, len(w)))), root, cx, scan))
    aws = bool(rng.integers(0, 2))
    bits = None if rng.random() < 0.5 else [int(x) for x in rng.integers(0, 13, len(mods) + 2 + int(aws))]
    return seq(L, mods, bits, aws)


DRAWN = {f"draw_{j:02d}_L{L}": (lambda L=L, j=j: draw(L, j)) for L in SIZES for j in range(24)}
ALL = {**NAMED, **DRAWN}


# ---- the table, restated --------------------------------------------------------------------------------------------
def _pred(cfg):
    L = int(cfg["overview"]["lineSize"])
    out = []
    for k in range(int(cfg["overview"]["num_modules"])):
        spec = cfg["modules"][str(k)]
        if spec["name"] != "PredComp":
            continue
        sub = spec["submodules"]
        p, sc = sub["ResidueModule"]["PredictorModule"], sub["ScanModule"]
        ts = int(sc["TableSize"])
        cells = list(zip(sc["Rows"][:ts], sc["Cols"][:ts]))
        out.append({"k": k, "kind": p["name"][:-len("Predictor")], "root": int(p["RootIndex"]), "p": p, "ts": ts,
                    "plane": cells == [(i // L, i % L) for i in range(ts)], "byte": cells == [(i % 8, i // 8) for i in range(ts)]})
    return L, out


def shift_of(w):
    """(int)log2f(weight); 99 where base << s or base >> -s leaves nothing of a byte."""
    s = int(np.log2(np.float32(w)))
    return s if -8 < s < 8 else 99


def module_tables(m, L):
    """What the predictor of a DiffBase / WeightBase module does per byte: (base, constant); constant = the shift or
    99 (WeightBase), DiffTable & 255 (DiffBase).  None at the root."""
    p, out = m["p"], []
    for i in range(L):
        if i == m["root"]:
            out.append(None)
        elif m["kind"] == "WeightBase":
            out.append((int(p["BaseIndexTable"][i]), shift_of(p["WeightTable"][i])))
        else:
            out.append((int(p["BaseIndexTable"][i]), int(p["DiffTable"][i]) & 255))
    return out


def _base_form(m, L):
    """-> (base_form, more than two shift distances, lane-kernel kind).  4.1b / 4.1e: a word's base bytes come from the
    own and the previous dword (one v_perm_b32); not at all where every word reads the word before it, or the word two
    before it from word 2 on, with entries that repeat; from anywhere, with the table as constants, otherwise."""
    t = module_tables(m, L)
    live = [(i, b, c) for i, x in enumerate(t) if x is not None for b, c in (x,)]
    shifts = []
    for _, _, c in live:
        if m["kind"] == "WeightBase" and c != 99 and c not in shifts:
            shifts.append(c)
    many = len(shifts) > 2
    if m["kind"] == "DiffBase":
        kind = "DF"
    else:
        plain = not many and (shifts in ([], [0]) or (len(shifts) == 2 and 0 in shifts and min(shifts) < 0))
        kind = "WT" if plain else "WT2"
    words = [tuple(None if x is None else x[1] for x in t[4 * w: 4 * w + 4]) for w in range(L // 4)]
    in_window = lambda i, b: max(4 * (i // 4) - 4, 0) <= b <= 4 * (i // 4) + 3      # noqa: E731
    two_back = m["root"] < 8 and all(b == i - 8 for i, b, _ in live if i >= 8)
    if two_back:
        # (words 2.. lie two words back: outside the window as soon as the periodic form is not taken)
        if any(not in_window(i, b) for i, b, _ in live if i < 8) or many:
            return "gathered", many, kind
        return ("two words back" if all(words[w] == words[2 + (w & 1)] for w in range(4, L // 4)) else "gathered"), many, kind
    if any(not in_window(i, b) for i, b, _ in live):
        return "gathered", many, kind
    if many:
        return "windowed", many, kind
    periodic = m["root"] < 4 and all(b == i - 4 for i, b, _ in live if i >= 4) and all(words[w] == words[1] for w in range(1, L // 4))
    return ("previous word" if periodic else "windowed"), many, kind


# the module sequences the library carries unrolled kernels for (4.1b, 4.1e): P = previous word, Q = two words back
BUILT_IN = [("OB", "CS", "DFP", "WTP"), ("OB", "CS", "DFQ", "WTQ"), ("OB", "CS", "DF", "WT"), ("OB", "CS"), ("OB",), ("CS",), ("DF",),
            ("WT",), ("DFP",), ("WTP",), ("DF", "DF", "DFP", "CS", "WTQ"), ("DFQ",), ("WTQ",)]


def _built_in(seq_kinds):
    """seq_kinds: (kind, base_form) per module.  A periodic instantiation needs the periodic table; the plain one runs
    every table that gathers through v_perm_b32, i.e. all but the two-words-back ones."""
    def fits(inst, kind, form):
        if inst[:2] != kind[:2] or (inst[:2] == "WT" and kind != "WT"):
            return False
        if inst.endswith("P"):
            return form == "previous word"
        if inst.endswith("Q"):
            return form == "two words back"
        return form != "two words back"
    return any(len(s) == len(seq_kinds) and all(fits(i, k, f) for i, (k, f) in zip(s, seq_kinds)) for s in BUILT_IN)


def _rings(L, M, bins):
    """Waves per workgroup the line rings (two stages of 64 lines per wave) fit with beside sums, histogram and, up to
    64-byte lines, queues of 256 / 192 / 160 / 96 / 0 entries per wave in the 160 KiB of LDS: (fits with the built-in
    workgroup, fits with 7/8, 3/4, 5/8 or 1/2 of it)."""
    K = M + 1
    stats = 16 * ((2 * K * 8 + 15) // 16) + 16 * (((K * bins + 2) * 4 + 15) // 16)
    full = 8 if L == 128 else 16

    def fit(w):
        return any(((stats + 4 * w * cap + 1023) // 1024) * 1024 + w * 2 * 64 * L <= 160 * 1024
                   for cap in ((256, 192, 160, 96, 0) if L <= 64 else (0,)))
    return fit(full), any(fit(w) for w in (full, full * 7 // 8, full * 3 // 4, full * 5 // 8, full // 2))


def expected_plan(cfg, compiler=True):
    """-> dict(path, reason, scan_order, needs, runtime_only, general_layout, sequence, base_form {module: form}, row).
    reason: "" | "line size" | "scan" | "sizes" | "combination" | "planes and root" | "no compiler".
    row: the row of the table above `twin` in build_vpc_plan the configuration lies in (whatever the compiler)."""
    L, pm = _pred(cfg)
    M = int(cfg["overview"]["num_modules"])
    assert pm, "a case needs a prediction module"
    generic = lambda reason, row: {"path": "generic", "reason": reason, "scan_order": "", "needs": [], "runtime_only": 0,      # noqa: E731
                                   "general_layout": "no", "sequence": "", "base_form": {}, "row": row}
    if L not in SIZES:
        return generic("line size", "line size")
    # one scan order for all: plane-major where the first module's table is (a table of one entry is both), else byte-major
    bm = not pm[0]["plane"] and pm[0]["byte"]
    ts0 = pm[0]["ts"]
    whole = lambda ts: ts == 8 * L or (ts >= L and ts % L == 0)      # noqa: E731
    planes_differ = False
    for m in pm:
        if not (m["byte"] if bm else m["plane"]):
            return generic("scan", "other scan tables")
        if m["ts"] != ts0:
            if bm or not whole(m["ts"]) or not whole(ts0):
                return generic("sizes", "other scan tables")
            planes_differ = True
    forms, seq_kinds, gather, wshift = {}, [], False, False
    for m in pm:
        if m["kind"] in ("OneBase", "ConsecutiveBase"):
            seq_kinds.append(("OB" if m["kind"] == "OneBase" else "CS", ""))
            continue
        form, many, kind = _base_form(m, L)
        forms[m["k"]] = form
        seq_kinds.append((kind, form))
        gather, wshift = gather or form == "gathered", wshift or many
    max_root = max(m["root"] for m in pm)
    twin = not bm and max_root <= 15 and ts0 >= 16          # the layouts of the built-in kernels
    needs, gen = [], False
    if gather or wshift:
        if not twin or planes_differ:
            return generic("combination", "combination")
        needs, row = (["GATHER"] if gather else []) + (["WSHIFT"] if wshift else []), "not windowed / many shifts"
        gen = max_root > 0 or ts0 != 8 * L
    elif planes_differ:
        if max_root > 15:
            return generic("planes and root", "combination")
        needs, row, gen = ["PLANES"], "planes differ", True
    elif bm:
        if ts0 >= 16 and max_root == 0:
            needs, row, gen = ["BM"], "byte-major, roots 0", ts0 != 8 * L
        else:
            row = "byte-major, other"
    elif ts0 < 16:
        row = "plane-major, under 16 entries"
    elif max_root > 15:
        needs, row, gen = ["ANYROOT"], "plane-major, root above 15", True
    else:
        gen = max_root > 0 or ts0 != 8 * L
        row = "plane-major, general layout" if gen else "plane-major, roots 0, full"
    runtime_only = int(not twin or bool(needs))
    eb = cfg["overview"].get("encoding_bits")
    bins = max(8 * L + (max(eb) if eb else int(math.ceil(math.log2(M + 1)))) + 1, 288)
    fit_full, fit_some = _rings(L, M, bins)
    unrolled = (not runtime_only and fit_full and _built_in(seq_kinds)) or \
               (compiler and (not runtime_only or needs) and len(pm) <= 12 and fit_some)
    out = {"path": "fast", "reason": "", "scan_order": "byte-major" if bm else "plane-major", "needs": needs, "runtime_only": runtime_only,
           "general_layout": "yes" if unrolled and gen else "no", "sequence": "unrolled" if unrolled else "run-time loop",
           "base_form": forms, "row": row}
    if not unrolled and set(needs) & {"PLANES", "GATHER", "WSHIFT"}:      # the run-time loop has none of the three
        out.update(path="generic", reason="no compiler", scan_order="", sequence="", general_layout="no")
    return out


def reason_category(why: str) -> str:
    """The category of mpc_config_describe's why_generic."""
    for text, cat in (("", ""), ("lineSize not in", "line size"), ("together with another layout", "combination"),
                      ("together with a RootIndex above 15", "planes and root"), ("run-time compilation is not available", "no compiler"),
                      ("could not be compiled", "no compiler"), ("neither a (truncated) plane-major", "scan"),
                      ("scan tables of different sizes", "sizes")):
        if (why == "") if text == "" else (text in why):
            return cat
    return "? " + why


ROWS = ("plane-major, roots 0, full", "plane-major, general layout", "plane-major, under 16 entries", "plane-major, root above 15",
        "planes differ", "not windowed / many shifts", "byte-major, roots 0", "byte-major, other", "combination", "other scan tables")
BASE_FORMS = ("windowed", "previous word", "two words back", "gathered")
