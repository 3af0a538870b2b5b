"""Seeded inputs of the BDI / FPC / BPC parity fixture (tests/golden/ref_baseline_vectors.npz, written by
tests/golden/make_ref_baseline_vectors.py from the reference's own compressors), so that the CPU and GPU tests can
rebuild them.  One case per (compressor, line size); every case mixes hand-built edge families with the trace
families of cal_22-mpc_amd/traces.py, in a seeded order.  Lines built for a chosen plane, run, delta or immediate at a
chosen place are in tests/baseline_chosen.py, with a fixture of their own."""
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

SIZES = {
    "BDI": [8, 16, 24, 32, 40, 64, 120, 128, 136, 192, 248, 256],
    "FPC": [4, 8, 12, 20, 32, 60, 64, 100, 128, 132, 252, 256],
    "BPC": [8, 12, 16, 20, 32, 36, 64, 124, 128],
}
MIN_LINES = 1800      # per case: more than the ragged calls of the GPU tests (1 + 63 + 64 + 65 + 511 + 512 + 513)
_SEED = {"BDI": 1000, "FPC": 2000, "BPC": 3000}

CASES = [{"name": f"{comp.lower()}_L{L}", "comp": comp, "L": L, "seed": _SEED[comp] + L}
         for comp in ("BDI", "FPC", "BPC") for L in SIZES[comp]]


def digest(lines: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(lines).tobytes()).hexdigest()


def _values_to_lines(vals: np.ndarray, B: int) -> np.ndarray:
    """[k, n] uint64 values of B bytes -> [k, n*B] little-endian bytes."""
    k, n = vals.shape
    b = (vals[:, :, None] >> (np.arange(B, dtype=np.uint64) * np.uint64(8))) & np.uint64(0xFF)
    return b.astype(np.uint8).reshape(k, n * B)


def _traced(fn, k: int, L: int, **kw) -> np.ndarray:
    """A trace family at any line size: generated at 128 or 256 bytes and cut to L."""
    return np.ascontiguousarray(fn(k, 128 if L <= 128 else 256, **kw)[:, :L])


# ---- BDI ------------------------------------------------------------------------------------------------------------
_COMBOS = [(8, 1), (8, 2), (8, 4), (4, 1), (4, 2), (2, 1)]


def _bdi_delta_limits(k: int, L: int, rng) -> np.ndarray:
    """Line i uses combination i % 6 (base B, delta D): a base, then values base + d for d at the delta limits
    (+-2^(8D-1), 2^(8D-1) - 1, one past them, the 128..255-style deltas with the top bit set, -1, -2), immediates
    at and just past the limit (0, 1, 2^(8D) - 1, 2^(8D), small negatives), and random values.  Some bases sit
    near 2^(8B) or 2^(8B-1), so that `base - v` wraps in uint64 (and, for B < 8, differs from the B-byte delta)."""
    out = np.zeros((k, L), np.uint8)
    for i in range(k):
        B, D = _COMBOS[i % 6]
        n, bits = L // B, 8 * B
        M = (1 << bits) - 1
        h = 1 << (8 * D - 1)
        deltas = [0, 1, -1, -2, h, -h, h - 1, -h - 1, h + 1, 2 * h - 1, 2 * h, -(2 * h) + 1]
        imms = [0, 1, 2 * h - 1, 2 * h, h, h - 1, (-1) & M, (-2) & M, (-h) & M, (-h - 1) & M]
        kind = int(rng.integers(0, 4))
        if kind == 0:
            base = M - int(rng.integers(0, 2 * h))                        # near the top: v = base + d wraps
        elif kind == 1:
            base = (1 << (bits - 1)) + int(rng.integers(-2 * h, 2 * h))   # around the sign bit
        elif kind == 2:
            base = min(M, 2 * h + int(rng.integers(0, 4)))               # just above the immediate limit
        else:
            base = int(rng.integers(0, M, dtype=np.uint64, endpoint=True)) if bits == 64 else int(rng.integers(0, M + 1))
        vals = [base]
        p_imm = float(rng.choice([0.0, 0.15, 0.4]))
        p_rand = float(rng.choice([0.0, 0.0, 0.1]))
        for _ in range(n - 1):
            r = rng.random()
            if r < p_imm:
                vals.append(int(imms[int(rng.integers(0, len(imms)))]))
            elif r < p_imm + p_rand:
                vals.append(int(rng.integers(0, 1 << 63)) & M)
            elif rng.random() < 0.2:
                vals.append((base + int(rng.integers(h, 2 * h))) & M)
            else:
                vals.append((base + deltas[int(rng.integers(0, len(deltas)))]) & M)
        out[i] = _values_to_lines(np.array([vals], dtype=np.uint64), B)[0]
    return out


def _bdi_all_immediate(k: int, L: int, rng) -> np.ndarray:
    """Every B-byte value an immediate for D (some negative for B = 8): no base, the 32-bit wrap of BDI.cpp:200."""
    out = np.zeros((k, L), np.uint8)
    for i in range(k):
        B, D = _COMBOS[i % 6]
        n, h = L // B, 1 << (8 * D - 1)
        v = rng.integers(0, 2 * h, n).astype(np.int64)
        if B == 8:
            neg = rng.random(n) < 0.3
            v = np.where(neg, -rng.integers(2, h + 1, n), v)
        v[int(rng.integers(0, n))] = int(rng.integers(1, 2 * h))         # not all zero
        out[i] = _values_to_lines((v.astype(np.int64).view(np.uint64) & np.uint64((1 << (8 * B)) - 1))[None, :], B)[0]
    return out


def _nonimm_bytes(rng, shape) -> np.ndarray:
    return rng.integers(0x10, 0xF0, shape).astype(np.uint8)


def _bdi_ties(k: int, L: int, rng) -> np.ndarray:
    """B4D1 and B2D1 with the same cost below 8L (the earlier, B4D1, must win): a words [x,0,0,0] and b more
    2-byte immediates in the upper halves, b = a + L/32; all other bytes random in 0x10..0xEF.  L % 32 == 0."""
    W = L // 4
    a = L // 96 + 1
    b = a + L // 32
    out = np.zeros((k, L), np.uint8)
    for i in range(k):
        w = _nonimm_bytes(rng, (W, 4))
        pos = rng.permutation(W)
        w[pos[:a], 1:] = 0
        w[pos[a:a + b], 3] = 0
        out[i] = w.reshape(L)
    return out


def _bdi_exactly_uncompressed(k: int, L: int, rng) -> np.ndarray:
    """B2D1 costing exactly 8L (L/16 two-byte immediates, everything else fails): Uncompressed.  L % 16 == 0."""
    H = L // 2
    out = np.zeros((k, L), np.uint8)
    for i in range(k):
        h = _nonimm_bytes(rng, (H, 2))
        h[rng.permutation(H)[:L // 16], 1] = 0
        out[i] = h.reshape(L)
    return out


def _bdi_repeats(k: int, L: int, rng) -> np.ndarray:
    q = rng.integers(1, 1 << 63, k, dtype=np.uint64)
    q[::3] = np.uint64(0xFFFFFFFFFFFFFFFF)
    out = np.repeat(q[:, None], L // 8, axis=1).astype("<u8").view(np.uint8).reshape(k, L).copy()
    out[1::5, 0] ^= 1                        # almost a repeat: the first 8 bytes differ
    return out


def _bdi_lines(L: int, rng) -> np.ndarray:
    parts = [_bdi_delta_limits(600, L, rng), _bdi_all_immediate(120, L, rng), _bdi_repeats(60, L, rng),
             np.zeros((20, L), np.uint8)]
    if L % 32 == 0:
        parts.append(_bdi_ties(60, L, rng))
    if L % 16 == 0:
        parts.append(_bdi_exactly_uncompressed(40, L, rng))
    parts += [_traced(traces.bdi_stress, 400, L), _traced(traces.bdi_screen_stress, 400, L, seed=L),
              _traced(traces.pointers_u64, 100, L), _traced(traces.random_u32, 100, L, seed=L),
              _traced(traces.structured, 300, L, seed=L)]
    return np.concatenate(parts)


# ---- FPC ------------------------------------------------------------------------------------------------------------
# every prefix boundary (the list of test_fpc) and words that match several prefixes (the first match counts)
FPC_SPECIAL = np.array([0, 1, 7, 8, 0xFFFFFFF8, 0xFFFFFFF7, 0x7F, 0x80, 0xFFFFFF80, 0xFFFFFF7F, 0x7FFF, 0x8000,
                        0xFFFF8000, 0xFFFF7FFF, 0x10000, 0x12340000, 0x007F007F, 0xFF80FF80, 0x0080007F, 0xFF7FFF80,
                        0x007FFF80, 0xFF80007F, 0xABABABAB, 0x00000100, 0x01010101, 0x12345678, 0xFFFFFFFF,
                        0x80000000, 0xFF800000, 0x00800000, 0x7F7F7F7F, 0x80808080, 0xFFFF0000, 0x00010000,
                        0x0000FF80, 0x007F0000, 0xFF80FFFF, 0xFFFFFF00, 0x00FF00FF, 0x7FFF0000], dtype=np.uint32)


def _fpc_lines(L: int, rng) -> np.ndarray:
    W = L // 4
    k = 1100
    words = FPC_SPECIAL[rng.integers(0, len(FPC_SPECIAL), (k, W))]
    words[rng.random((k, W)) < 0.35] = 0                           # zero runs
    words[::7, -min(3, W):] = 0                                    # runs that reach the end of the line
    words[3::7, -1] = 0
    words[1::11, :] = 0                                            # all-zero lines
    lines = words.astype("<u4").view(np.uint8).reshape(k, L)
    return np.concatenate([lines, _traced(traces.structured, 400, L, seed=L), _traced(traces.mixed, 200, L),
                           _traced(traces.random_u32, 150, L, seed=L), _traced(traces.counters_u32, 100, L),
                           np.zeros((50, L), np.uint8)])


# ---- BPC ------------------------------------------------------------------------------------------------------------
BPC_STEPS = np.array([0, 1, 255, 256, 1 << 16, 1 << 31, (1 << 32) - 1], dtype=np.uint64)


def _bpc_lines(L: int, rng) -> np.ndarray:
    W = L // 4
    k = 300
    idx = np.arange(W, dtype=np.uint64)[None, :]
    M32 = np.uint64(0xFFFFFFFF)
    # ramps: every step of BPC_STEPS (2^32 - 1 borrows into the 33rd plane; 1, 256, 2^16, 2^31 give all-ones planes)
    base = rng.integers(0, 1 << 32, (k, 1), dtype=np.uint64)
    base[::4] = np.uint64(0)
    base[1::4] = np.uint64(0xFFFFFFF0)
    step = BPC_STEPS[np.arange(k) % len(BPC_STEPS)][:, None]
    ramps = (base + step * idx) & M32
    # constant deltas with one bump of 2^c or two bumps at adjacent rows: single / adjacent ones in a DBX
    m = 400
    c = rng.integers(0, 32, m).astype(np.uint64)
    d = np.repeat(rng.choice(BPC_STEPS, m)[:, None], W, axis=1)
    r = rng.integers(1, max(W - 1, 2), m)
    rows = np.arange(m)
    d[rows, np.minimum(r, W - 1)] += np.uint64(1) << c
    two = (rows % 2 == 1) & (W > 2)
    d[rows[two], np.minimum(r[two] + 1, W - 1)] += np.uint64(1) << c[two]
    d[:, 0] = rng.integers(0, 1 << 32, m, dtype=np.uint64)
    bumps = np.cumsum(d, axis=1) & M32
    # deltas that are all 2^c or all -2^c: DBX planes of all ones (pattern 6 only with 31 deltas, L = 128)
    q = 160
    c2 = (np.arange(q) % 32).astype(np.uint64)
    sgn = np.where(np.arange(q) % 3 == 0, np.uint64((1 << 32) - 1), np.uint64(1))
    ones = ((rng.integers(0, 1 << 32, (q, 1), dtype=np.uint64) + ((np.uint64(1) << c2) * sgn)[:, None] * idx) & M32)
    const = np.repeat(rng.integers(0, 1 << 32, (80, 1), dtype=np.uint64), W, axis=1)
    words = np.concatenate([ramps, bumps, ones, const]).astype("<u4")
    lines = words.view(np.uint8).reshape(-1, L)
    return np.concatenate([lines, _traced(traces.structured, 400, L, seed=L), _traced(traces.mixed, 150, L),
                           _traced(traces.random_u32, 150, L, seed=L), _traced(traces.counters_u32, 150, L),
                           _traced(traces.pointers_u64, 150, L), np.zeros((40, L), np.uint8)])


_FAMILIES = {"BDI": _bdi_lines, "FPC": _fpc_lines, "BPC": _bpc_lines}


def case_lines(spec: dict) -> np.ndarray:
    """The [n, L] uint8 lines of one fixture case (every family, in a seeded order)."""
    rng = np.random.default_rng(spec["seed"])
    lines = _FAMILIES[spec["comp"]](spec["L"], rng)
    assert len(lines) >= MIN_LINES and lines.shape[1] == spec["L"], (spec["name"], lines.shape)
    return np.ascontiguousarray(lines[rng.permutation(len(lines))])


# ---- the fixture ----------------------------------------------------------------------------------------------------
def load_fixture(path: str):
    """-> (meta dict, {array name: array}) of tests/golden/ref_baseline_vectors.npz."""
    import json
    with np.load(path) as z:
        arrays = {k: z[k] for k in z.files}
    return json.loads(str(arrays.pop("meta"))), arrays


def case_input(case: dict) -> np.ndarray:
    """The lines of a fixture case, rebuilt and checked against the recorded digest."""
    lines = case_lines(case)
    assert len(lines) == case["n"] and digest(lines) == case["sha256"], f"{case['name']}: the input generator drifted"
    return lines


def stats_vector(comp: str, n_lines: int, stats: np.ndarray) -> np.ndarray:
    """The library's statistics vector (mpc_stats_get layout) of n_lines lines from the reference's totals
    [OriginalSize, CompressedSize, TotalWords, Counts...]: BDI and FPC [lines, original, compressed, counts...],
    BPC [lines, original, compressed, total words, counts...]."""
    head = [n_lines, int(stats[0]), int(stats[1])] + ([int(stats[2])] if comp == "BPC" else [])
    return np.array(head + [int(x) for x in stats[3:]], dtype=np.uint64)
