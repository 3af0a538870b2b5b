"""The reference's Pattern analyser (src/compressor/Pattern.{h,cpp}, LRU.h) restated, independent of the library:

    line_scalar / analyse_scalar   plain Python, the source read line by line (reduceSign's bit loop, checkPattern,
                                   countPattern, UpdateCountMap, the set as a Python set)
    analyse                        the same in numpy, vectorised over the lines, for the large GPU inputs

and the seeded inputs of the parity fixture (tests/golden/ref_pattern_vectors.npz), so that the tests can rebuild them.
The statistics vector is the library's (include/mpc_hip.h, "Pattern layout")."""
from __future__ import annotations

import hashlib
import math

import numpy as np

M64 = (1 << 64) - 1
CAPACITY = (1 << 24) - 1
PATTERNS = ((8, 1), (8, 2), (8, 4), (4, 1), (4, 2), (2, 1))      # PatternState 0..5
NOT_DEFINED = 9
STATS_LEN = 534
LINE_SIZES = (8, 16, 24, 32, 40, 64, 128, 256)


# ---------------------------------------------------------------------------------------------------------------------
# plain Python
# ---------------------------------------------------------------------------------------------------------------------
def reduce_sign(x: int) -> int:
    """Pattern.cpp:348-363."""
    if x >> 63:
        for i in range(62, -1, -1):
            if ((x >> i) & 1) == 0:
                return x & (M64 >> (63 - (i + 1)))
    return x


def check_pattern(line: bytes, B: int, D: int):
    """Pattern.cpp:118-211 -> (size in bits, immediates, values)."""
    limit = (1 << (8 * D)) - 1
    vals = [int.from_bytes(line[i:i + B], "little") for i in range(0, len(line), B)]
    n = len(vals)
    mask = [reduce_sign(v) <= limit for v in vals]
    imm = sum(mask)
    base, base_idx = 0, 0
    for i in range(n):
        if not mask[i]:
            base, base_idx = vals[i], i
            break
    not_all = False
    for i in range(base_idx + 1, n):
        if not mask[i] and reduce_sign((base - vals[i]) & M64) > limit:
            not_all = True
            break
    if not_all:
        size = n + 8 * (imm * D + (n - imm) * B)
    else:
        size = (n + 8 * (imm * D + (B + (n - imm - 1) * D))) & 0xFFFFFFFF
    return size, imm, n


def line_scalar(line: bytes):
    """CompressLine without the set -> (returned size, selected, implicit bytes, explicit bytes, zero, word-same)."""
    L = len(line)
    best, select, sel_imm, sel_n = 8 * L, NOT_DEFINED, 0, 0
    for k, (B, D) in enumerate(PATTERNS):
        size, imm, n = check_pattern(line, B, D)
        if best > size:
            best, select, sel_imm, sel_n = size, k, imm, n
    if best == 8 * L:
        select = NOT_DEFINED
    zero = not any(line)
    same = all(line[i] == line[i % 4] for i in range(4, L))
    B = PATTERNS[select][0] if select != NOT_DEFINED else 0
    return best + 4, select, B * sel_imm, B * (sel_n - sel_imm), zero, same


def analyse_scalar(lines: np.ndarray):
    """Every line in order -> (sizes uint16, selected int8, statistics vector)."""
    n, L = lines.shape
    v = np.zeros(STATS_LEN, dtype=np.uint64)
    sizes, sel = np.zeros(n, np.uint16), np.zeros(n, np.int8)
    seen = set()
    for i in range(n):
        line = lines[i].tobytes()
        size, select, imp, exp, zero, same = line_scalar(line)
        sizes[i], sel[i] = size, select
        v[0] += 1
        v[3] += size
        v[4] += L if zero else 0
        v[5] += L if same else 0
        if line in seen:
            v[6] += L
        else:
            seen.add(line)
            v[21] += 1
        if select == NOT_DEFINED:
            v[7] += L
        else:
            v[9 + select] += imp
            v[15 + select] += exp
        v[8] += L
        for b in line:
            v[22 + b] += 1
            if not (zero or same):
                v[278 + b] += 1
    return sizes, sel, v


def entropy(counts) -> float:
    """PatternResult::ComputeEntropy (Pattern.h:124-154) over the symbols that occurred, ascending."""
    counts = [int(c) for c in counts]
    total = sum(counts)
    e = 0.0
    for c in counts:
        if c:
            p = float(c) / float(total)
            e += -p * math.log2(p)
    return e


def _fmt_double(x: float) -> str:
    """{fmt}'s "{}" of a double: shortest round-trip digits, fixed notation for exponents -4 .. 15."""
    r = repr(float(x))
    if "e" in r:
        m, e = r.split("e")
        return (m[:-2] if m.endswith(".0") else m) + "e" + e[0] + e[1:].rjust(2, "0")
    return r[:-2] if r.endswith(".0") else r


def print_text(workload: str, v) -> str:
    """The row PatternResult::Print writes (Pattern.h:199-213)."""
    out = [workload, _fmt_double(entropy(v[22:278])), _fmt_double(entropy(v[278:534]))]
    out += [str(int(v[4])), str(int(v[5])), str(int(v[6]))]
    for k in range(6):
        out += [str(int(v[9 + k])), str(int(v[15 + k]))]
    out += [str(int(v[7])), str(int(v[8]))]
    return ",".join(out) + ",\n"


# ---------------------------------------------------------------------------------------------------------------------
# numpy, vectorised over the lines
# ---------------------------------------------------------------------------------------------------------------------
def _fits(x: np.ndarray, D: int) -> np.ndarray:
    """reduce_sign(x) <= 2^(8D) - 1 for uint64 x: 0 <= x <= limit, or -2^(8D-1) <= x <= -2 as a signed number (the
    bit loop keeps the bits below the highest zero bit plus one sign bit, and returns -1 unchanged)."""
    limit = np.uint64((1 << (8 * D)) - 1)
    low = np.uint64((1 << 64) - (1 << (8 * D - 1)))
    return (x <= limit) | ((x >= low) & (x != np.uint64(M64)))


def analyse(lines: np.ndarray, with_set: bool = True):
    """(sizes uint16, selected int8, statistics vector) of all lines, T and [21] from numpy.unique."""
    lines = np.ascontiguousarray(lines, dtype=np.uint8)
    n, L = lines.shape
    best = np.full(n, 8 * L, dtype=np.int64)
    select = np.full(n, NOT_DEFINED, dtype=np.int64)
    sel_imm = np.zeros(n, dtype=np.int64)
    for k, (B, D) in enumerate(PATTERNS):
        vals = lines.view(f"<u{B}").astype(np.uint64)
        m = vals.shape[1]
        is_imm = _fits(vals, D)
        imm = is_imm.sum(axis=1).astype(np.int64)
        have_base = np.zeros(n, dtype=bool)
        not_all = np.zeros(n, dtype=bool)
        base = np.zeros(n, dtype=np.uint64)
        for i in range(m):
            v, im = vals[:, i], is_imm[:, i]
            with np.errstate(over="ignore"):
                not_all |= ~im & have_base & ~_fits(base - v, D)
            first = ~im & ~have_base
            base = np.where(first, v, base)
            have_base |= ~im
        size = np.where(not_all, m + 8 * (imm * D + (m - imm) * B), (m + 8 * (imm * D + (B + (m - imm - 1) * D))) & 0xFFFFFFFF)
        better = best > size
        best = np.where(better, size, best)
        select = np.where(better, k, select)
        sel_imm = np.where(better, imm, sel_imm)
    words = lines.view("<u4")
    zero = ~lines.any(axis=1)
    same = (words == words[:, :1]).all(axis=1)
    v = np.zeros(STATS_LEN, dtype=np.uint64)
    v[0] = n
    v[3] = int((best + 4).sum())
    v[4] = L * int(zero.sum())
    v[5] = L * int(same.sum())
    v[7] = L * int((select == NOT_DEFINED).sum())
    v[8] = L * n
    for k, (B, _) in enumerate(PATTERNS):
        mine = select == k
        v[9 + k] = B * int(sel_imm[mine].sum())
        v[15 + k] = B * int((L // B - sel_imm[mine]).sum())
    v[22:278] = np.bincount(lines.reshape(-1), minlength=256)
    v[278:534] = np.bincount(lines[~same].reshape(-1), minlength=256)
    if with_set:
        d = distinct(lines)
        v[21] = d
        v[6] = L * (n - d)
    return (best + 4).astype(np.uint16), select.astype(np.int8), v


def distinct(lines: np.ndarray) -> int:
    """Number of different lines."""
    lines = np.ascontiguousarray(lines, dtype=np.uint8)
    if len(lines) == 0:
        return 0
    L = lines.shape[1]
    if L == 8:
        return len(np.unique(lines.view("<u8").reshape(-1)))
    return len(np.unique(lines.view(np.dtype((np.void, L))).reshape(-1)))


# ---------------------------------------------------------------------------------------------------------------------
# the seeded cases
# ---------------------------------------------------------------------------------------------------------------------
def _values_line(vals, B: int, L: int) -> np.ndarray:
    a = np.array([int(x) & ((1 << (8 * B)) - 1) for x in vals], dtype=np.uint64).astype(f"<u{B}")
    out = a.view(np.uint8)
    assert out.size == L
    return out.copy()


def _menu(L: int, rng) -> list:
    """The lines of one case, in order.  See the issue's list: every pattern winning, all-immediate lines, deltas of -1
    and of exactly the limit (both signs), bit 63 / bit 31 set, sizes equal to 8 L, ties, zero and word-same lines."""
    out = []
    zeros = np.zeros(L, np.uint8)
    out.append(zeros)
    for _ in range(2):
        out.append(np.tile(rng.integers(1, 256, 4, dtype=np.uint8), L // 4))
    out.append(np.tile(np.array([7, 0, 0, 0], np.uint8), L // 4))                 # word-same and all-immediate
    for B, D in PATTERNS:
        n = L // B
        lim, h, top = (1 << (8 * D)) - 1, 1 << (8 * D - 1), 1 << (8 * B)
        def base():
            return int(rng.integers(0x40, 0x80)) << (8 * (B - 1)) | int(rng.integers(0, 1 << 16))
        def down(b, k):      # base - v = d in [0, lim]
            return [b] + [b - int(d) for d in rng.integers(0, lim + 1, k)]
        def up(b, k):        # base - v = -d, d in [2, h]
            return [b] + [b + int(d) for d in rng.integers(2, h + 1, k)]
        b = base()
        out.append(_values_line(down(b, n - 1), B, L))
        out.append(_values_line(up(b, n - 1), B, L))
        if n >= 2:
            for last in (b - lim, b - lim - 1, b + 1, b + h, b + h + 1, b + 2):
                # the delta of exactly the limit, one beyond, -1, exactly -2^(8D-1), one beyond, -2
                vals = down(b, n - 1)
                vals[-1] = last
                out.append(_values_line(vals, B, L))
        out.append(_values_line(rng.integers(0, lim + 1, n), B, L))               # every value an immediate
        out.append(_values_line([lim] * n, B, L))
        if n >= 2:                                                                # immediates among base + deltas
            vals = down(b, n - 1)
            for i in rng.choice(np.arange(1, n), size=max(1, n // 3), replace=False):
                vals[int(i)] = int(rng.integers(0, lim + 1))
            out.append(_values_line(vals, B, L))
            vals = down(b, n - 1)
            vals[0] = int(rng.integers(0, lim + 1))                               # the base is not the first value
            out.append(_values_line(vals, B, L))
        if B == 8:
            # bit 63 set: negative immediates -2 .. -2^(8D-1), -1 (never an immediate), and a negative base
            out.append(_values_line([top - int(d) for d in rng.integers(2, h + 1, n)], B, L))
            out.append(_values_line([top - 1] + [top - int(d) for d in rng.integers(2, h + 1, n - 1)], B, L))
            out.append(_values_line([top - 1] * n, B, L))
            nb = (1 << 63) | int(rng.integers(1 << 40, 1 << 41))
            out.append(_values_line(down(nb, n - 1), B, L))
            out.append(_values_line([top - h - 1] + [top - h] * (n - 1), B, L))
        if B == 4:
            # bit 31 set: zero-extended, so a large positive value
            nb = (1 << 31) | int(rng.integers(1 << 20, 1 << 21))
            out.append(_values_line(down(nb, n - 1), B, L))
            out.append(_values_line([top - 2] * n, B, L))
    for _ in range(6):
        out.append(rng.integers(0, 256, L, dtype=np.uint8))
    if L % 16 == 0:
        # B2D1 fails with L/16 immediates: n + 8 (imm + 2 (n - imm)) = 8 L exactly, which does not beat 8 L
        vals = [int(x) for x in rng.integers(0x1000, 0x10000, L // 2)]
        for i in rng.choice(L // 2, size=L // 16, replace=False):
            vals[int(i)] = int(rng.integers(0, 256))
        out.append(_values_line(vals, 2, L))
    if L == 64:
        # a tie: B8D1 fails with 2 immediates (8 L + 8 - 112) and B4D1 with 5 (8 L + 16 - 120); the earlier one keeps it
        vals = [int(x) for x in rng.integers(1 << 28, 1 << 31, 16)]
        vals[2:4] = [5, 0]
        vals[8:10] = [200, 0]
        vals[13] = 9
        out.append(_values_line(vals, 4, L))
    if L == 128:
        # a tie of two successes: B8D4 (16 + 8 (8 + 60)) and B4D2 (32 + 8 (4 + 62)) both give 560
        # (first value pair (b, c); every later pair (b + e, c - 1): the 8-byte delta is 2^32 - e, the 4-byte deltas are small)
        b, c = 0x11002222, 0x11002222 - 300
        vals = [b, c]
        for _ in range(15):
            vals += [b + int(rng.integers(2, 1000)), c - 1]
        out.append(_values_line(vals, 4, L))
    # duplicates: adjacent, far apart, of zero lines
    out.insert(5, out[4].copy())
    out.insert(len(out) // 2, zeros.copy())
    out.append(out[6].copy())
    out.append(out[-3].copy())
    out.append(zeros.copy())
    out.append(zeros.copy())
    return out


CASES = [{"name": f"menu_L{L}", "L": L, "seed": 1000 + L} for L in LINE_SIZES]


def case_input(spec) -> np.ndarray:
    rng = np.random.default_rng(spec["seed"])
    return np.ascontiguousarray(np.stack(_menu(spec["L"], rng)), dtype=np.uint8)


def digest(lines: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(lines).tobytes()).hexdigest()
