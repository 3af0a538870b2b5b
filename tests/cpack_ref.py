"""C-Pack with a per-line dictionary: the seeded inputs of the parity fixture (tests/golden/ref_cpack_vectors.npz, written
by tests/golden/make_ref_cpack_vectors.py from the reference's own CPACK.cpp), a plain restatement of CPACK.cpp:7-101
with both dictionary scopes -- "line" (a fresh dictionary per line: what the library evaluates) and "carried" (one
dictionary over the whole case: what the reference's driver does; here only to pin the restatement's other mode and to
show that the two differ) -- and the closed forms the gfx950 kernels use, restated on numpy arrays."""
from __future__ import annotations

import hashlib
import importlib
import os
import sys

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)
traces = importlib.import_module("cal_22-mpc_amd.traces")

LINE_SIZES = [4, 8, 12, 32, 36, 64, 68, 96, 128, 132, 252, 256]
PATTERNS = ("ZZZZ", "ZZZX", "MMMM", "MMMX", "MMXX", "XXXX")      # CPACKPattern order (CPACK.h:18-26)
BITS = (2, 12, 6, 16, 24, 34)                                     # ... and their lengths (NOT the order of m_PatternLength)
ENTRIES = 16
STATS_LEN = 10
MIN_LINES = 1800      # per case: more than the ragged calls of the GPU tests (1 + 63 + 64 + 65 + 511 + 512 + 513)
KEY_SETS = (1, 2, 3, 5, 17, 18, 40, 300)
PRINT_CASES = ("cpack_L64", "cpack_L128")

CASES = [{"name": f"cpack_L{L}", "L": L, "seed": 6000 + L} for L in LINE_SIZES]


def digest(lines: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(lines).tobytes()).hexdigest()


# ---- the restatement ---------------------------------------------------------------------------------------------------
def compress(lines: np.ndarray, scope: str = "line"):
    """-> (sizes uint16[n], counts uint8[n, 6]) of the [n, L] uint8 lines; scope "line" or "carried"."""
    assert scope in ("line", "carried")
    words = np.ascontiguousarray(lines).view("<u4")
    n, W = words.shape
    sizes = np.zeros(n, np.uint16)
    counts = np.zeros((n, 6), np.uint8)
    fifo = [0] * ENTRIES
    for r, row in enumerate(words.tolist()):
        if scope == "line":
            fifo = [0] * ENTRIES
        size = 0
        for w in row:
            if w & 0xFFFFFF == 0:
                pat = 0 if w == 0 else 1
            else:
                pat = 5
                for e in fifo:                                  # from the front: the oldest entry first
                    x = e ^ w
                    if x & 0xFFFF == 0:                         # the first entry with the same b0, b1 decides alone
                        pat = 4 if x & 0xFF0000 else (3 if x else 2)
                        break
                if pat == 5:
                    fifo.append(w)
                    fifo.pop(0)
            size += BITS[pat]
            counts[r, pat] += 1
        sizes[r] = size
    return sizes, counts


def stats_vector(L: int, sizes: np.ndarray, counts: np.ndarray) -> np.ndarray:
    """The library's statistics vector (include/mpc_hip.h) of these lines."""
    n = len(sizes)
    c = counts.astype(np.uint64).sum(axis=0)
    return np.array([n, 8 * L * n, int(sizes.astype(np.uint64).sum()), int(c.sum())] + [int(x) for x in c], dtype=np.uint64)


def comp_ratio(L: int, sizes) -> float:
    """CompRatio as CompResult::Update leaves it after the last line (CompResult.h: running totals, one division)."""
    total = int(np.asarray(sizes, dtype=np.uint64).sum())
    return float(8 * L * len(sizes)) / float(total) if total else 0.0


def print_text(workload: str, v: np.ndarray, ratio_text: str) -> str:
    return f"{workload},{int(v[1])},{int(v[2])},{ratio_text},{int(v[3])}," + "".join(f"{int(x)}," for x in v[4:10]) + "\n"


HEADER = "Workload,Original Size,Compressed Size,Compression Ratio,Total Words," + "".join(f"Pattern{i}," for i in range(6)) + "\n"


# ---- the closed forms of the kernels (csrc/mpc_baselines.h: cpack_line) ------------------------------------------------
def _nested(words, zzz, hit, x):
    a = zzz.sum(axis=1)
    b = (words == 0).sum(axis=1)
    c = hit.sum(axis=1)
    d = (hit & (x & 0xFF == 0)).sum(axis=1)
    e = (hit & (x == 0)).sum(axis=1)
    W = words.shape[1]
    counts = np.stack([b, a - b, e, d - e, c - d, W - a - c], axis=1)
    sizes = 34 * W - 22 * a - 10 * b - 10 * c - 8 * d - 10 * e
    return sizes.astype(np.uint16), counts.astype(np.uint8)


def closed_form_no_eviction(lines: np.ndarray):
    """Up to 16 words: a word with a non-zero key is decided by the FIRST earlier word of the line with its key."""
    words = np.ascontiguousarray(lines).view("<u4").astype(np.uint32)
    n, W = words.shape
    assert W <= 16
    key = words & 0xFFFF
    zzz = (words & 0xFFFFFF) == 0
    hit = np.zeros((n, W), bool)
    x = np.zeros((n, W), np.uint32)
    for i in range(W):
        m = ~words[:, i]
        for j in range(i - 1, -1, -1):
            m = np.where(key[:, j] == key[:, i], words[:, j], m)
        y = m ^ words[:, i]
        zero_entry = (key[:, i] == 0) & ~zzz[:, i]
        hit[:, i] = ~zzz[:, i] & ((key[:, i] == 0) | ((y & 0xFFFF) == 0))
        x[:, i] = np.where(zero_entry, 1, y >> 16)
    return _nested(words, zzz, hit, x)


def closed_form(lines: np.ndarray):
    """Any number of words: the LATEST earlier miss with the word's key, if fewer than 17 misses ago; the zero entries while
    there have been fewer than 16 misses."""
    words = np.ascontiguousarray(lines).view("<u4").astype(np.uint32)
    n, W = words.shape
    zzz = (words & 0xFFFFFF) == 0
    hit = np.zeros((n, W), bool)
    x = np.zeros((n, W), np.uint32)
    dk = np.zeros((n, W), np.uint32)
    pay = np.zeros((n, W), np.uint32)
    C = np.zeros(n, np.uint32)
    for i in range(W):
        key, hi = words[:, i] & 0xFFFF, words[:, i] >> 16
        m = np.full(n, 0xFFFF0000, np.uint32)
        for j in range(i):
            m = np.where(dk[:, j] == key, pay[:, j], m)
        zero_entry = (key == 0) & ~zzz[:, i] & (C < 16)
        there = (C - (m >> 16)).astype(np.uint32) <= 16
        hit[:, i] = ~zzz[:, i] & (zero_entry | there)
        x[:, i] = np.where(zero_entry, 1, (m & 0xFFFF) ^ hi)
        miss = ~zzz[:, i] & ~hit[:, i]
        dk[:, i] = np.where(miss, key, 0xFFFFFFFF)
        pay[:, i] = hi | (C << 16)
        C = C + miss.astype(np.uint32)
    return _nested(words, zzz, hit, x)


# ---- inputs ------------------------------------------------------------------------------------------------------------
def _wd(b0, b1, b2, b3):
    return b0 | (b1 << 8) | (b2 << 16) | (b3 << 24)


def _other(k):
    """Word of the k-th "other" key: distinct, non-zero, never key A."""
    return _wd(k + 1, 0x80 | (k >> 7), 0x30 + k % 7, 0x40 + k % 5)


A = (0x11, 0x22)


def hand_lines(L: int) -> np.ndarray:
    """The hand-built lines of the issue, each cut or zero-padded to L / 4 words; those that need more words than the line
    has are left out."""
    W = L // 4
    a = lambda b2, b3: _wd(A[0], A[1], b2, b3)      # noqa: E731
    others = lambda k0, k: [_other(i) for i in range(k0, k0 + k)]      # noqa: E731
    k0w = _wd(0, 0, 5, 7)
    rows = [
        [0] * W,                                                        # all-zero
        [_wd(0, 0, 0, 1 + i % 255) for i in range(W)],                  # ZZZX
        [_wd(0, 0, 0, 9) if i % 3 else 0 for i in range(W)],            # ZZZX among ZZZZ
        [k0w, k0w, _other(0), k0w, _wd(0, 0, 6, 7), _other(1), _wd(0, 0, 5, 8)],     # key 0, b2 != 0, before 16 misses: MMXX each
        [a(1, 1), a(1, 2), a(1, 2)],                                    # MMMX twice: the stored word is not updated
        [a(1, 1), a(2, 2), a(2, 2)],                                    # MMXX twice: MMXX does not push
        [a(1, 1), a(1, 1), a(1, 1), 0, a(1, 1)],                        # MMMM
        others(0, W),                                                   # W distinct non-zero keys: 34 W > 8 L
    ]
    if W >= 17:
        rows.append([a(1, 1)] + others(0, 15) + [a(1, 1)])              # A, 15 other keys, A: a hit
    if W >= 18:
        rows.append([a(1, 1)] + others(0, 16) + [a(1, 1)])              # A, 16 other keys, A: evicted, a miss
        rows.append([a(1, 1)] + others(0, 16) + [a(1, 2)])
    if W >= 19:
        rows.append([a(1, 1)] + others(0, 15) + [a(1, 1), _other(20), a(1, 1)])      # a hit does not refresh
    if W >= 20:
        rows.append([a(1, 1)] + others(0, 16) + [a(2, 2), a(2, 2), a(1, 1)])         # pushed again: the later entry decides
        rows.append([a(1, 1)] + others(0, 16) + [a(1, 1), a(1, 1), a(1, 9)])
    if W >= 32:
        # 16 misses, then key 0: a miss now; repeated: it hits its own entry; then MMMX and MMXX against it
        rows.append(others(0, 16) + [k0w, k0w, _wd(0, 0, 5, 8), _wd(0, 0, 6, 8), 0, _wd(0, 0, 0, 3), k0w])
        rows.append(others(0, 15) + [k0w] + [_other(15)] + [k0w, k0w] + others(16, 13))       # the 16th miss between two key-0 words
        rows.append(others(0, 16) + [k0w] + others(16, 14) + [k0w])                           # pushed key-0 entry still there after 14 more
    if W >= 40:
        rows.append(others(0, 16) + [k0w] + others(16, 16) + [k0w, k0w])                      # ... and evicted after 16 more
        rows.append(others(0, 40)[:W])
    out = np.zeros((len(rows), W), np.uint32)
    for r, row in enumerate(rows):
        row = row[:W]
        out[r, :len(row)] = row
    return out.astype("<u4").view(np.uint8).reshape(len(rows), L)


def _key_set_lines(k: int, L: int, rng) -> np.ndarray:
    """Words whose (b0, b1) come from a small set (1 .. 300 keys; key 0 forced into half of the lines) and whose b2, b3
    from very few values, with some zero words: hits of every kind, evictions from 17 keys on."""
    W = L // 4
    out = np.zeros((k, W), np.uint32)
    for r in range(k):
        nk = KEY_SETS[r % len(KEY_SETS)]
        keys = rng.integers(1, 1 << 16, nk).astype(np.uint32)
        if (r // len(KEY_SETS)) % 2:
            keys[0] = 0
        nv = int(rng.integers(1, 4))
        w = keys[rng.integers(0, nk, W)] | (rng.integers(0, nv, W).astype(np.uint32) << 16) | (rng.integers(0, nv, W).astype(np.uint32) << 24)
        w[rng.random(W) < 0.1] = 0
        z = rng.random(W) < 0.05
        w[z] = rng.integers(1, 256, int(z.sum())).astype(np.uint32) << 24
        out[r] = w
    return out.astype("<u4").view(np.uint8).reshape(k, L)


def _traced(fn, k: int, L: int, **kw) -> np.ndarray:
    """A trace family at any line size: generated at 128 or 256 bytes and cut to L."""
    return np.ascontiguousarray(fn(k, 128 if L <= 128 else 256, **kw)[:, :L])


def case_lines(spec: dict) -> np.ndarray:
    """The [n, L] uint8 lines of one fixture case (every family, in a seeded order)."""
    L = spec["L"]
    rng = np.random.default_rng(spec["seed"])
    hand = hand_lines(L)
    parts = [hand, hand, _key_set_lines(800, L, rng), _traced(traces.structured, 300, L, seed=L), _traced(traces.mixed, 150, L),
             _traced(traces.random_u32, 150, L, seed=L), _traced(traces.counters_u32, 100, L), _traced(traces.pointers_u64, 150, L),
             _traced(traces.sine_f32, 100, L), _traced(traces.word_same, 40, L), np.zeros((20, L), np.uint8)]
    lines = np.concatenate(parts)
    assert len(lines) >= MIN_LINES and lines.shape[1] == L, (spec["name"], lines.shape)
    return np.ascontiguousarray(lines[rng.permutation(len(lines))])


# ---- the fixture -------------------------------------------------------------------------------------------------------
def load_fixture(path: str):
    """-> (meta dict, {array name: array}) of tests/golden/ref_cpack_vectors.npz."""
    import json
    with np.load(path) as z:
        arrays = {k: z[k] for k in z.files}
    return json.loads(str(arrays.pop("meta"))), arrays


def case_input(case: dict) -> np.ndarray:
    """The lines of a fixture case, rebuilt and checked against the recorded digest."""
    lines = case_lines(case)
    assert len(lines) == case["n"] and digest(lines) == case["sha256"], f"{case['name']}: the input generator drifted"
    return lines
