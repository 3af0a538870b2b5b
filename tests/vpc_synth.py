"""Lines built from a chosen scanned array, for the VPC tests (tests/test_vpc_synth_cpu.py, tests/test_vpc_synth_gpu.py).

Every later stage of a VPC evaluation (selector, row-0 prefilters, incompressibility certificate, encoder) looks at
one prediction module's scanned array: 8 L / 16 rows of 16 bits.  The stages before it invert, so a test can choose
that array and ask for the line that gives it: line_for_scanned undoes, in order, the scan table (ScanModule.cpp:6-22;
cells outside the table stay 0), the XOR in either flavour (XORModule.cpp:5-23; row 0 and column 0 are copies), the bit
planes (BitplaneModule.cpp:7-51; row 0 is the most significant plane), the residue order (ResidueModule.cpp:12-41: the
raw root byte first) and the predictor (PredictorModule.cpp).  numpy only: nothing of the package under test is
imported here (the random lines that the arrangements put around the built ones are handed in by the caller).
The oracle's stage functions are called to VERIFY a built line (verified), never to build one.

What cannot be built is said by residue_constraints: every byte but the root has one prediction source -- its
BaseIndexTable entry (WeightBase, DiffBase), the root (OneBase) or the byte before it in the byte-plane-shuffled order
(ConsecutiveBase, PredictorModule.cpp:133-173).  A byte that every chain of sources leads from to the root is free: any
residue can be had.  A byte that is its own source has a forced residue (-Diff, or one of b - shift(b)), and around a
longer cycle of sources the residues are tied to each other (with shifts of 0: they sum to minus the Diff entries).

The families (walking one, walking pairs, leading zero rows, row classes x zero runs, threshold ladder) are requests
for scanned arrays of one module; `build` turns them into lines and keeps count of what could not be built."""
from __future__ import annotations

import ctypes as C
import os
import sys

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)

FAMILIES = ("walking_one", "walking_pairs", "leading_zero_rows", "row_classes", "ladder")
PLANT_LANES = (0, 31, 63)
TAILS = (0, 1, 63, 65)


# ---- a prediction module, from the configuration's JSON -------------------------------------------------------------
def pred_modules(cfg: dict) -> list:
    """The indices of the prediction modules, in module order."""
    return [i for i in range(int(cfg["overview"]["num_modules"])) if cfg["modules"][str(i)]["name"] == "PredComp"]


def _shift_table(w) -> np.ndarray:
    """WeightBase's prediction per base value: base << s or base >> -s, s = (int)log2f(weight)."""
    s = int(np.log2(np.float32(w)))
    v = np.arange(256, dtype=np.int64)
    return ((v << s) if s >= 0 else (v >> -s)).astype(np.uint8)


class Module:
    """One prediction module: root, per byte the prediction source and the 256-entry prediction table, XOR flavour, scan
    table."""

    def __init__(self, cfg: dict, k: int):
        spec = cfg["modules"][str(k)]
        assert spec["name"] == "PredComp", (k, spec["name"])
        sub = spec["submodules"]
        p = sub["ResidueModule"]["PredictorModule"]
        self.k, self.L = k, int(cfg["overview"]["lineSize"])
        L = self.L
        self.R = 8 * L // 16
        self.kind, self.root = p["name"], int(p["RootIndex"])
        ident = np.arange(256, dtype=np.uint8)
        self.src = np.full(L, -1, np.int64)
        self.fn = np.tile(ident, (L, 1))
        for i in range(L):
            if i == self.root:
                continue
            if self.kind == "WeightBasePredictor":
                self.src[i], self.fn[i] = int(p["BaseIndexTable"][i]), _shift_table(p["WeightTable"][i])
            elif self.kind == "DiffBasePredictor":
                self.src[i], self.fn[i] = int(p["BaseIndexTable"][i]), ident + np.uint8(int(p["DiffTable"][i]) & 0xFF)
            elif self.kind == "OneBasePredictor":
                self.src[i] = self.root
            else:
                assert self.kind == "ConsecutiveBasePredictor" and self.root == 0, (self.kind, self.root)
                order = [j for plane in (3, 2, 1, 0) for j in range(plane, L, 4)]
                self.src[i] = order[i - 1]
        self.cx = bool(sub["XORModule"]["consecutiveXOR"])
        sc = sub["ScanModule"]
        self.ts = int(sc["TableSize"])
        self.trow = np.array(sc["Rows"][:self.ts], np.int64)
        self.tcol = np.array(sc["Cols"][:self.ts], np.int64)
        self.pos = [self.root] + [i for i in range(L) if i != self.root]      # residue order -> byte position
        self._walk()

    def _walk(self):
        """Cycles of the source graph (a byte that is its own source is a cycle of one) and an order in which every other
        byte comes after its source."""
        L, state = self.L, np.zeros(self.L, np.int64)            # 0 new, 1 on the current walk, 2 done
        state[self.root] = 2
        self.cycles = []
        for i in range(L):
            path, j = [], i
            while state[j] == 0:
                state[j] = 1
                path.append(j)
                j = int(self.src[j])
            if state[j] == 1:                                     # closed on this walk: path[at:] is a cycle
                cyc = path[path.index(j):]
                self.cycles.append(cyc[::-1])                     # so that src[c[j]] == c[j - 1]
            for q in path:
                state[q] = 2
        on_cycle = {q for c in self.cycles for q in c}
        done, self.order = on_cycle | {self.root}, []
        for i in range(L):
            path, j = [], i
            while j not in done:
                done.add(j)
                path.append(j)
                j = int(self.src[j])
            self.order += path[::-1]

    def table_mask(self) -> np.ndarray:
        """uint16[R]: the scanned cells that the table fills."""
        m = np.zeros(self.R, np.uint16)
        for i in range(self.ts):
            m[i // 16] |= np.uint16(1 << (15 - i % 16))
        return m


def residue_constraints(cfg: dict, k: int) -> dict:
    """Which residues of module k can be chosen.  Byte positions of the line; `residue_index` gives a byte's place in the
    residue order (root first).
      free    bytes whose chain of sources ends at the root (or behind a cycle): any residue
      forced  {byte: allowed residues} for a byte that is its own source (-Diff, or the values b - shift(b))
      cycles  longer cycles of sources, each with the sum its residues must have mod 256 (None where a shift is not 0:
              then the residues are tied by the shifts, and the synthesiser tries every start value)"""
    m = Module(cfg, k)
    ident = np.arange(256, dtype=np.uint8)
    forced, cycles = {}, []
    for c in m.cycles:
        if len(c) == 1:
            forced[c[0]] = sorted({int(x) for x in (ident - m.fn[c[0]])})
        else:
            plain = all(((m.fn[q] - ident) == (m.fn[q] - ident)[0]).all() for q in c)
            cycles.append({"bytes": list(c), "sum": int(sum(int((m.fn[q] - ident)[0]) for q in c) * -1 % 256) if plain else None})
    tied = set(forced) | {q for c in cycles for q in c["bytes"]}
    return {"kind": m.kind, "root": m.root, "free": [i for i in range(m.L) if i != m.root and i not in tied],
            "forced": forced, "cycles": cycles, "residue_index": {p: j for j, p in enumerate(m.pos)}}


def is_free(cons: dict) -> bool:
    """No forced byte and no cycle: every scanned array inside the table can be built."""
    return not cons["forced"] and not cons["cycles"]


# ---- rows -> lines --------------------------------------------------------------------------------------------------
def residues_for_scanned(m: Module, rows: np.ndarray):
    """Undo scan table, XOR and bit planes: (residues [n, L] in residue order, reason per request or None)."""
    rows = np.ascontiguousarray(rows, np.uint16).reshape(-1, m.R)
    n, L = len(rows), m.L
    bits = ((rows[:, :, None] >> (15 - np.arange(16, dtype=np.uint16))) & 1).astype(np.uint8).reshape(n, 8 * L)
    reason = np.full(n, None, object)
    reason[bits[:, m.ts:].any(axis=1)] = "a cell outside the scan table"
    x = np.zeros((n, 8, L), np.uint8)
    x[:, m.trow, m.tcol] = bits[:, :m.ts]
    twice = (x[:, m.trow, m.tcol] != bits[:, :m.ts]).any(axis=1)          # a table that names a cell twice
    reason[twice & (reason == None)] = "a cell the scan table reads twice"      # noqa: E711
    plane = x.copy()
    for r in range(1, 8):
        plane[:, r, 1:] = x[:, r, 1:] ^ (plane[:, r - 1, 1:] if m.cx else plane[:, 0, 1:])
    res = np.zeros((n, L), np.uint8)
    for r in range(8):
        res |= plane[:, r, :] << np.uint8(7 - r)
    return res, reason


def lines_for_residues(m: Module, res: np.ndarray, reason: np.ndarray):
    """Undo the residue order and the predictor: lines [n, L]; `reason` gains the constraint that forbids a request."""
    n, L = res.shape
    rpos = np.zeros((n, L), np.uint8)
    rpos[:, m.pos] = res
    line = np.zeros((n, L), np.uint8)
    line[:, m.root] = rpos[:, m.root]
    rows_i = np.arange(n)
    for c in m.cycles:
        start = np.tile(np.arange(256, dtype=np.uint8), (n, 1))           # every value of the cycle's last byte
        val = start
        for q in c:
            val = m.fn[q][val] + rpos[:, q][:, None]
        good = val == start
        bad = ~good.any(axis=1)
        what = f"forced byte {c[0]}" if len(c) == 1 else f"cycle of {len(c)} bytes through byte {min(c)}"
        reason[bad & (reason == None)] = what                             # noqa: E711
        v = np.argmax(good, axis=1).astype(np.uint8)
        for q in c:
            v = m.fn[q][v] + rpos[:, q]
            line[rows_i, q] = v
    for i in m.order:
        line[:, i] = m.fn[i][line[:, m.src[i]]] + rpos[:, i]
    return line


def lines_for_scanned(cfg: dict, k: int, rows: np.ndarray):
    """Batch form: (lines [n, L], built [n] bool, reasons [n]).  A line counts as built only when the oracle's
    mpc_o_scanned of it (and the reference's own stages, where oracle/_ref is built) gives `rows` back exactly."""
    m = Module(cfg, k)
    rows = np.ascontiguousarray(rows, np.uint16).reshape(-1, m.R)
    res, reason = residues_for_scanned(m, rows)
    lines = lines_for_residues(m, res, reason)
    ok = reason == None                                                    # noqa: E711
    same = verified(cfg, k, lines, rows)
    wrong = ok & ~same
    reason[wrong] = "NOT VERIFIED"
    return lines, ok & same, reason


def line_for_scanned(cfg: dict, k: int, rows: np.ndarray):
    """The line whose scanned array under module k of cfg is `rows` (uint16[8 L / 16]), or None when
    residue_constraints forbids it.  The root byte is 0 unless the array puts bits on it."""
    lines, ok, _ = lines_for_scanned(cfg, k, np.asarray(rows, np.uint16)[None, :])
    return lines[0] if ok[0] else None


# ---- verification through the oracle (and the reference's stages where built) ---------------------------------------
def _oracle():
    from oracle import oracle as O
    O.lib()
    return O


def oracle_scanned(cfg: dict, k: int, lines: np.ndarray, ref: bool = False) -> np.ndarray:
    """mpc_o_scanned (or ref_scanned) of every line under module k: uint16 [n, R]."""
    O = _oracle()
    oc = O.config_from_json(cfg)
    mod = oc.modules[k]
    L, R = oc.line_size, 8 * oc.line_size // 16
    lines = np.ascontiguousarray(lines, np.uint8)
    out = np.zeros((len(lines), R), np.uint16)
    lib, rl = O.lib(), O.ref_lib() if ref else None
    a = C.addressof
    for n in range(len(lines)):
        if ref:
            rl.ref_scanned(mod.pred_kind, mod.root, L, a(mod.base), a(mod.weight), a(mod.diff), mod.consecutive_xor,
                           mod.table_size, a(mod.rows), a(mod.cols), lines[n].ctypes.data, out[n].ctypes.data)
        else:
            lib.mpc_o_scanned(C.byref(mod), L, lines[n].ctypes.data, out[n].ctypes.data)
    return out


def verified(cfg: dict, k: int, lines: np.ndarray, rows: np.ndarray) -> np.ndarray:
    same = (oracle_scanned(cfg, k, lines) == rows).all(axis=1)
    if _oracle().ref_lib() is not None:
        same &= (oracle_scanned(cfg, k, lines, ref=True) == rows).all(axis=1)
    return same


def leading_zero_rows(cfg: dict, lines: np.ndarray) -> np.ndarray:
    """int [n, P]: per line and prediction module the oracle's count of leading zero rows."""
    out = []
    for k in pred_modules(cfg):
        sc = oracle_scanned(cfg, k, lines)
        nz = sc != 0
        out.append(np.where(nz.any(axis=1), np.argmax(nz, axis=1), sc.shape[1]))
    return np.stack(out, axis=1) if out else np.zeros((len(lines), 0), np.int64)


def fpc_sizes(rows: np.ndarray) -> np.ndarray:
    lib = _oracle().lib()
    rows = np.ascontiguousarray(rows, np.uint16)
    return np.array([lib.mpc_o_fpc_size(rows[n].ctypes.data, rows.shape[1]) for n in range(len(rows))], np.int64)


# ---- row alphabet ---------------------------------------------------------------------------------------------------
# ("both halves with bits only on 7 and 8" is the one row 0x0180, the pair at columns 7/8: one class, pair78)
ROW_CLASSES = ("single", "pair", "pair78", "front", "back", "both_out")


def _bit(c):
    return np.uint16(1 << (15 - int(c)))


def row_17(rng, n=None):
    """Rows that cost 17 bits: both halves set, not one adjacent pair (a bit outside columns 7/8)."""
    v = rng.integers(0, 1 << 16, n or 1, dtype=np.uint32).astype(np.uint16)
    v |= np.uint16(0x8001)
    return v if n is not None else v[0]


def row_of(cls: str, rng) -> np.uint16:
    if cls == "zero":
        return np.uint16(0)
    if cls == "single":
        return _bit(rng.integers(0, 16))
    if cls == "pair":
        c = int(rng.integers(0, 15))
        return _bit(c) | _bit(c + 1)
    if cls == "pair78":
        return np.uint16(0x0180)
    if cls in ("front", "back"):                   # two or more bits, not an adjacent pair, in columns 0..7 / 8..15
        while True:
            v = int(rng.integers(1, 256))
            ones = bin(v).count("1")
            if ones >= 3 or (ones == 2 and v & (v >> 1) == 0):
                return np.uint16(v << 8 if cls == "front" else v)
    if cls == "both_out":                          # both halves with a bit outside columns 7/8: 17 bits
        return np.uint16([0x8001, 0x0101, 0x0181, 0x8180, 0x4002][int(rng.integers(0, 5))])
    raise ValueError(cls)


# ---- the families: requests for scanned arrays of one module --------------------------------------------------------
def family_rows(m: Module, family: str, seed: int):
    """(rows uint16 [n, R], labels [n]) of a family for module m.  Requests are cut to the scan table (cells outside it
    stay 0 whatever the line), so a truncated table gets the part of every request that it can show."""
    R, rng = m.R, np.random.default_rng(seed)
    req, lab = [], []

    def put(a, label):
        req.append(np.asarray(a, np.uint16).copy())
        lab.append(label)

    def cells(*idx):
        a = np.zeros(R, np.uint16)
        for i in idx:
            a[i // 16] |= _bit(i % 16)
        return a
    if family == "walking_one":
        for i in range(m.ts):
            put(cells(i), f"scan position {i}")
    elif family == "walking_pairs":
        for i in range(m.ts - 1):
            put(cells(i, i + 1), f"scan positions {i},{i + 1}")
        for d in (2, 8):
            for r in range(R):
                for c in range(16 - d):
                    if 16 * r + c + d < m.ts:
                        put(cells(16 * r + c, 16 * r + c + d), f"row {r} columns {c},{c + d}")
    elif family == "leading_zero_rows":
        for z in range(R):
            for shape in ("col0", "col15", "17bit"):
                for tail in ("zero", "random"):
                    a = np.zeros(R, np.uint16)
                    a[z] = {"col0": np.uint16(0x8000), "col15": np.uint16(0x0001)}.get(shape, row_17(rng))
                    if tail == "random":
                        a[z + 1:] = rng.integers(0, 1 << 16, R - z - 1, dtype=np.uint32).astype(np.uint16)
                    put(a, f"z={z} row {shape} then {tail}")
    elif family == "row_classes":
        for run in sorted({1, 2, 3, R - 1}):
            if run < 1 or run > R - 1:
                continue
            for place in ("start", "middle", "end"):
                at = {"start": 0, "middle": (R - run) // 2, "end": R - run}[place]
                for cls in ROW_CLASSES:
                    for fill in ("same", "mixed"):
                        a, mix = np.zeros(R, np.uint16), ("zero", "zero") + ROW_CLASSES
                        for r in range(R):
                            if not at <= r < at + run:
                                beside = fill == "same" or r in (at - 1, at + run)
                                a[r] = row_of(cls if beside else mix[int(rng.integers(0, len(mix)))], rng)
                        put(a, f"{cls} rows ({fill}), zero run of {run} at the {place} (row {at})")
    elif family == "ladder":
        kinds = ("single", "pair78", "front", "zero", "mixed")
        for n17 in range(R + 1):
            for kind in kinds:
                for copy in range(1 if kind != "mixed" else 6):
                    a = np.zeros(R, np.uint16)
                    if n17:
                        a[:n17] = row_17(rng, n17)
                    mix = ("single", "pair78", "front", "back", "zero", "pair")
                    for r in range(n17, R):
                        a[r] = row_of(kind if kind != "mixed" else mix[int(rng.integers(0, 6))], rng)
                    put(a, f"n17={n17} then {kind} rows")
        # the sizes 8 L - 3 .. 8 L + 3 exactly, where rows of 17 / 7 / 8 / 12 bits and one zero row at the end (4 bits) add
        # up to them: 17 n + 7 a + 8 b + 12 c + 4 z with n + a + b + c + z = R, the most 17-bit rows first
        for t in range(-3, 4):
            sol = next(((n, R - z - n - b - c, b, c, z) for n in range(R, -1, -1) for z in (0, 1) for c in range(R - z - n + 1)
                        for b in range(R - z - n - c + 1)
                        if 17 * n + 7 * (R - z - n - b - c) + 8 * b + 12 * c + 4 * z == 16 * R + t), None)
            if sol is not None:
                kinds_t = ["17"] * sol[0] + ["single"] * sol[1] + ["pair"] * sol[2] + ["back"] * sol[3] + ["zero"] * sol[4]
                put([row_17(rng) if q == "17" else row_of(q, rng) for q in kinds_t], f"exactly 8L{t:+d}: rows of 17/7/8/12/4 bits {sol}")
    else:
        raise ValueError(family)
    rows = np.array(req, np.uint16).reshape(-1, R) & m.table_mask()[None, :]
    return rows, lab


def build(cfg: dict, seed: int = 0, families=FAMILIES) -> list:
    """Every family for its target modules (walking one, walking pairs and leading zero rows: every prediction module;
    row classes and the ladder: the last one, which takes the ties).  -> a list of dicts per (family, module):
    family, module, requested, rows (of the built ones), lines, labels, refused {reason: count}."""
    out, pm = [], pred_modules(cfg)
    for f_i, family in enumerate(families):
        for k in (pm if family in FAMILIES[:3] else pm[-1:]):
            m = Module(cfg, k)
            rows, labels = family_rows(m, family, 1000 * seed + 10 * k + f_i)
            lines, ok, reason = lines_for_scanned(cfg, k, rows)
            refused = {}
            for r in reason[~ok]:
                refused[r] = refused.get(r, 0) + 1
            out.append({"family": family, "module": k, "requested": len(rows), "rows": rows[ok], "lines": lines[ok],
                        "labels": [lb for lb, good in zip(labels, ok) if good], "refused": refused})
    return out


# ---- arrangements ---------------------------------------------------------------------------------------------------
def arrange(built: list, L: int, arrangement: str, filler, per_family: int = None):
    """The built lines of a configuration in one arrangement, cut into four calls of 128 k + r lines, r = 0, 1, 63, 65.
    -> a list of (lines [n, L], origin [n]); origin indexes `index` (family, module, label) or is -1 for a filler.
    filler(n, L, seed) gives the random lines (uint8 [n, L], writable) that the planted and cold arrangements put around
    the built ones.
      dense    the built lines one after the other (the last call is filled up from the first lines)
      planted  the built lines at lanes 0, 31 and 63 of groups of 64 random lines, rotated per group
      cold     blocks of 128 lines whose first group is random and whose second group is built lines: a wave evaluates a
               block's groups in order, so every built line comes behind a group that kept nothing (the kernels skip
               the incompressibility certificate behind a group that kept a line: dense and planted lines rarely meet it)
    per_family: of every (family, module) with more built lines than that, a seeded sample of that many, in their order."""
    pool = np.concatenate([b["lines"] for b in built]) if built else np.zeros((0, L), np.uint8)
    origin = np.arange(len(pool))
    if per_family is not None:
        keep, at = [], 0
        for q, b in enumerate(built):
            n = len(b["lines"])
            keep.append(at + (np.arange(n) if n <= per_family else
                              np.sort(np.random.default_rng(1000 * q + n).choice(n, per_family, replace=False))))
            at += n
        origin = np.concatenate(keep) if keep else origin
        pool = pool[origin]
    if arrangement == "planted":
        groups = (len(pool) + 2) // 3
        lines = filler(64 * groups, L, 4000 + L)
        org = np.full(64 * groups, -1, np.int64)
        for i in range(len(pool)):
            g, j = divmod(i, 3)
            at = 64 * g + PLANT_LANES[(j + g) % 3]
            lines[at], org[at] = pool[i], origin[i]
        pool, origin = lines, org
    elif arrangement == "cold":
        calls = []
        for j, r in enumerate(TAILS):
            part = np.arange(len(pool) * j // 4, len(pool) * (j + 1) // 4)
            blocks = max((len(part) + 63) // 64, 1)
            lines = filler(128 * blocks + r, L, 5000 + L + j)
            org = np.full(len(lines), -1, np.int64)
            at = 128 * (np.arange(len(part)) // 64) + 64 + np.arange(len(part)) % 64
            lines[at], org[at] = pool[part], origin[part]
            calls.append((np.ascontiguousarray(lines), org))
        return calls
    else:
        assert arrangement == "dense", arrangement
    calls, at, n = [], 0, len(pool)
    for j, r in enumerate(TAILS):
        want = max(n * (j + 1) // 4 - at, 1)
        size = 128 * max((want - r + 127) // 128, 1) + r if j == 3 else 128 * max((want - r) // 128, 1) + r
        idx = np.arange(at, at + size) % max(n, 1)
        calls.append((np.ascontiguousarray(pool[idx]), origin[idx]))
        at += size
    return calls


def index(built: list) -> list:
    """(family, module, label) per line of the pool that `arrange` numbers."""
    return [(b["family"], b["module"], lb) for b in built for lb in b["labels"]]
