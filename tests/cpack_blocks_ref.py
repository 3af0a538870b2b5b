"""C-Pack with a dictionary shared by blocks of N lines: the restatement of CPACK.cpp:7-101 with a fresh dictionary every
N lines (block b = lines [b N, (b + 1) N) of the trace), and the inputs of the parity fixture
(tests/golden/ref_cpack_block_vectors.npz, written by tests/golden/make_ref_cpack_block_vectors.py from the reference's
own CPACK.cpp, a fresh comp::CPACK every N lines): the cases of cpack_ref at six line sizes, whose lines are in a seeded
random order, and per line size one case in NATURAL order -- trace families whose neighbouring lines share keys, and
hand-built runs of lines that carry a dictionary entry across a line boundary."""
from __future__ import annotations

import numpy as np

import cpack_ref
from cpack_ref import traces, _traced, _wd

LINE_SIZES = [4, 32, 36, 64, 128, 256]
BLOCKS = [2, 3, 4, 16, 64, 1000]
MIN_LINES = cpack_ref.MIN_LINES
ALIGN = 64            # the key-0 run of every repetition starts a block of 2, 4, 16 and 64 lines

SHUFFLED = [c for c in cpack_ref.CASES if c["L"] in LINE_SIZES]
ORDERED = [{"name": f"cpack_order_L{L}", "L": L, "seed": 7000 + L} for L in LINE_SIZES]
CASES = SHUFFLED + ORDERED


# ---- the restatement ---------------------------------------------------------------------------------------------------
def compress_blocks(lines: np.ndarray, block_lines: int, first_line: int = 0, fifo=None):
    """-> (sizes uint16[n], counts uint8[n, 6]) of the [n, L] uint8 lines, which are lines first_line .. of a trace: the
    dictionary is 16 zero words at the first word of every line whose number is a multiple of block_lines and is carried
    otherwise (`fifo`: the dictionary the lines before left, for first_line inside a block; it is updated in place)."""
    words = np.ascontiguousarray(lines).view("<u4")
    n, W = words.shape
    sizes = np.zeros(n, np.uint16)
    counts = np.zeros((n, 6), np.uint8)
    if fifo is None:
        fifo = [0] * cpack_ref.ENTRIES
    for r, row in enumerate(words.tolist()):
        if (first_line + r) % block_lines == 0:
            fifo[:] = [0] * cpack_ref.ENTRIES
        size = 0
        for w in row:
            if w & 0xFFFFFF == 0:
                pat = 0 if w == 0 else 1
            else:
                pat = 5
                for e in fifo:                                  # from the front: the oldest entry first
                    x = e ^ w
                    if x & 0xFFFF == 0:
                        pat = 4 if x & 0xFF0000 else (3 if x else 2)
                        break
                if pat == 5:
                    fifo.append(w)
                    fifo.pop(0)
            size += cpack_ref.BITS[pat]
            counts[r, pat] += 1
        sizes[r] = size
    return sizes, counts


# ---- inputs ------------------------------------------------------------------------------------------------------------
def _fresh(k: int) -> int:
    """Word of the k-th "other" key: distinct non-zero keys, never a key of _a()."""
    return _wd(k & 0xFF, 0x40 | (k >> 8), 0x30 + k % 7, 0x40 + k % 5)


def _a(rep: int, b2: int, b3: int) -> int:
    return _wd(0x11 + rep, 0x22, b2, b3)


def hand_runs(L: int, rep: int):
    """The runs of the issue as word sequences; run i of repetition `rep` draws its other keys from a range of its own.
    Laid out by _lay: the first word of a run is the LAST word of a line, so the second begins the next line and every
    run spans at least one line boundary (with 16 others between, several)."""
    a = lambda b2, b3: _a(rep, b2, b3)      # noqa: E731
    base = [1 + 64 * (8 * rep + i) for i in range(8)]
    others = lambda i, k0, k: [_fresh(base[i] + j) for j in range(k0, k0 + k)]      # noqa: E731
    return [
        [a(1, 1), a(1, 1), a(1, 2), a(2, 2)],                                  # pushed in one line; MMMM, MMMX, MMXX in the next
        [a(3, 1)] + others(1, 0, 15) + [a(3, 1)],                              # 15 other misses between: a hit
        [a(4, 1)] + others(2, 0, 16) + [a(4, 1)],                              # 16: evicted, a miss
        [a(5, 1)] + others(3, 0, 15) + [a(5, 1)] + others(3, 20, 1) + [a(5, 1)],          # a hit does not refresh
        [a(6, 1)] + others(4, 0, 16) + [a(6, 2), a(6, 2), a(6, 1)],   # pushed again: the later entry decides
    ]


def key0_run(rep: int):
    """Key 0 with b2 != 0 before and after the 16th miss of the block (the run starts a block: ALIGN): MMXX against a zero
    entry, 15 misses, MMXX against the last zero entry, the 16th miss, then a miss (pushed) and MMMM / MMMX on its own entry."""
    k0w = _wd(0, 0, 5, 7)
    others = [_fresh(1 + 64 * (8 * rep + 7) + j) for j in range(16)]
    return [k0w] + others[:15] + [k0w, others[15], k0w, k0w, _wd(0, 0, 5, 8)]


def _lay(run, W: int) -> np.ndarray:
    """A run into lines of W words: W - 1 zero words (ZZZZ leaves the dictionary alone), the run, zero words to the end."""
    seq = [0] * (W - 1) + list(run)
    seq += [0] * (-len(seq) % W)
    return np.array(seq, dtype=np.uint32).reshape(-1, W)


def ordered_lines(spec: dict) -> np.ndarray:
    """The [n, L] uint8 lines of a natural-order case."""
    L = spec["L"]
    W = L // 4
    rng = np.random.default_rng(spec["seed"])
    families = [_traced(traces.pointers_u64, 400, L, seed=spec["seed"]), _traced(traces.structured, 500, L, seed=L),
                _traced(traces.counters_u32, 350, L), _traced(traces.mixed, 400, L)]
    parts, n = [], 0

    def put(block):
        nonlocal n
        parts.append(np.ascontiguousarray(block).view(np.uint8).reshape(len(block), L))
        n += len(block)

    for rep, fam in enumerate(families):
        put(fam[:len(fam) // 2])
        for run in hand_runs(L, rep):
            put(_lay(run, W).astype("<u4"))
            put(fam[len(fam) // 2:][:int(rng.integers(1, 6))])            # a few family lines between the runs
        if n % ALIGN:
            put(fam[len(fam) // 2:][: ALIGN - n % ALIGN])
        # the key-0 run begins with the first word of a line here: its first word is the block's first non-zero key
        seq = key0_run(rep)
        seq += [0] * (-len(seq) % W)
        put(np.array(seq, dtype=np.uint32).reshape(-1, W).astype("<u4"))
        put(fam[len(fam) // 2:])
    lines = np.concatenate(parts)
    assert len(lines) >= MIN_LINES and lines.shape[1] == L, (spec["name"], lines.shape)
    return np.ascontiguousarray(lines)


def case_lines(spec: dict) -> np.ndarray:
    return ordered_lines(spec) if spec["name"].startswith("cpack_order_") else cpack_ref.case_lines(spec)


def key0_run_starts(spec: dict):
    """Line numbers at which the key-0 runs of an ordered case begin (multiples of ALIGN)."""
    lines = ordered_lines(spec)
    first = np.ascontiguousarray(lines).view("<u4")[:, 0]
    return [int(i) for i in np.nonzero(first == _wd(0, 0, 5, 7))[0] if i % ALIGN == 0]


# ---- the fixture -------------------------------------------------------------------------------------------------------
load_fixture = cpack_ref.load_fixture


def case_input(case: dict) -> np.ndarray:
    """The lines of a fixture case, rebuilt and checked against the recorded digest."""
    lines = case_lines(case)
    assert len(lines) == case["n"] and cpack_ref.digest(lines) == case["sha256"], f"{case['name']}: the input generator drifted"
    return lines
