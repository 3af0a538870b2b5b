"""SC2 (reference src/compressor/SC2.cpp) restated in numpy / Python, independent of the library: the warm-up
counts, the eviction to 1024 symbols, the reference's MinHeap replayed step by step, the per-word sizing.  Also the
seeded inputs of the parity fixture (tests/golden/ref_sc2_vectors.json), so that the GPU tests can rebuild them."""
from __future__ import annotations

import hashlib

import numpy as np

ENTRIES = 1024
MISS_BITS = 33
EVICTED = 0xFFFF


def sampling_lines(num_lines: int) -> int:
    """main.cpp:110-113."""
    return max(10000, min(num_lines // 100, 1000000))


def code_lengths(symbols, freqs):
    """Code length per input symbol (EVICTED when outside the 1024 largest (freq, symbol) pairs)."""
    symbols = [int(s) for s in symbols]
    freqs = [int(f) for f in freqs]
    n = len(symbols)
    if n == 0:
        raise ValueError("empty frequency map")
    idx = list(range(n))
    if n > ENTRIES:
        idx.sort(key=lambda i: (freqs[i], symbols[i]))
        idx = idx[n - ENTRIES:]
    idx.sort(key=lambda i: symbols[i])                 # std::map order
    fr = [freqs[i] for i in idx]                       # node id -> freq (leaves first)
    left, right = [-1] * len(idx), [-1] * len(idx)
    heap = list(range(len(idx)))
    size = len(heap)

    def heapify(i):
        while True:
            m, l, r = i, 2 * i + 1, 2 * i + 2
            if l <= size - 1 and fr[heap[l]] < fr[heap[m]]:
                m = l
            if r <= size - 1 and fr[heap[r]] < fr[heap[m]]:
                m = r
            if m == i:
                return
            heap[i], heap[m] = heap[m], heap[i]
            i = m

    for i in range(size // 2 - 1, -1, -1):
        heapify(i)

    def extract():
        nonlocal size
        top = heap[0]
        heap[0], heap[size - 1] = heap[size - 1], heap[0]
        size -= 1
        heapify(0)
        return top

    while size > 1:
        a = extract()
        b = extract()
        fr.append(fr[a] + fr[b])
        left.append(a)
        right.append(b)
        node = len(fr) - 1
        if size < len(heap):
            heap[size] = node
        else:
            heap.append(node)
        size += 1
        i = size - 1
        while i > 0 and fr[heap[(i - 1) // 2]] > fr[heap[i]]:   # GetParent(i) = ceil(i / 2) - 1
            p = (i - 1) // 2
            heap[i], heap[p] = heap[p], heap[i]
            i = p
    out = [EVICTED] * n
    stack = [(heap[0], 0)]
    while stack:
        node, d = stack.pop()
        if left[node] < 0:
            out[idx[node]] = d
        else:
            stack.append((left[node], d + 1))
            stack.append((right[node], d + 1))
    return out


class SC2Ref:
    """comp::SC2(lineSize, S) over whole arrays of lines; feed() may be called repeatedly (lines counted across calls)."""

    def __init__(self, line_size: int, sampling: int):
        assert line_size % 4 == 0 and sampling > 0
        self.L, self.S = line_size, sampling
        self.seen = 0
        self.counts = {}
        self.table_syms = np.zeros(0, dtype=np.uint32)
        self.table_lens = np.zeros(0, dtype=np.uint16)
        self.built = False
        self.lines = self.warm = self.comp = self.found = 0

    def _build(self):
        syms = np.array(sorted(self.counts), dtype=np.uint32)
        lens = np.array(code_lengths(syms, [self.counts[int(s)] for s in syms]), dtype=np.int64)
        keep = lens != EVICTED
        self.table_syms, self.table_lens = syms[keep], lens[keep].astype(np.uint16)
        self.built = True

    def feed(self, lines: np.ndarray):
        """-> (sizes uint16[n], selected int8[n])"""
        lines = np.ascontiguousarray(lines, dtype=np.uint8)
        n, W = lines.shape[0], self.L // 4
        words = lines.view("<u4").reshape(n, W)
        sizes = np.zeros(n, dtype=np.uint16)
        sel = np.zeros(n, dtype=np.int8)
        warm = min(n, max(0, self.S - self.seen))
        if warm:
            u, c = np.unique(words[:warm], return_counts=True)
            for s, k in zip(u.tolist(), c.tolist()):
                self.counts[s] = self.counts.get(s, 0) + k
            sizes[:warm] = W * MISS_BITS
            self.comp += warm * W * MISS_BITS
            self.warm += warm
        if warm < n:
            if not self.built:
                self._build()
            rest = words[warm:]
            pos = np.searchsorted(self.table_syms, rest)
            pos = np.minimum(pos, max(len(self.table_syms) - 1, 0))
            hit = self.table_syms[pos] == rest
            bits = np.where(hit, self.table_lens[pos].astype(np.int64), MISS_BITS)
            sizes[warm:] = bits.sum(axis=1)
            sel[warm:] = 1
            self.comp += int(bits.sum())
            self.found += int(hit.sum())
        self.seen += n
        self.lines += n
        return sizes, sel

    def stats_vector(self) -> np.ndarray:
        return np.array([self.lines, self.lines * 8 * self.L, self.comp, self.warm, len(self.table_syms), self.found],
                        dtype=np.uint64)


# ---- seeded inputs of the parity fixture ---------------------------------------------------------------------------
def _fib(k):
    f = [1, 1]
    while len(f) < k:
        f.append(f[-1] + f[-2])
    return f[:k]


def case_lines(spec: dict) -> np.ndarray:
    """The lines of one fixture case: a warm-up sample of S lines with the frequencies the case is about, then
    `post` lines drawn from the same symbols with some random words (misses) mixed in."""
    L, S, post, kind = spec["L"], spec["S"], spec["post"], spec["kind"]
    if kind == "keys":            # chosen words (tests/sc2_keys.py): the builder makes the whole case, tail included
        import sc2_keys
        lines, bl, bs, _ = sc2_keys.build(spec["builder"])
        assert (bl, bs, len(lines) - bs) == (L, S, post), spec["name"]
        return lines
    W = L // 4
    rng = np.random.default_rng(spec["seed"])
    nw = S * W
    if kind == "ties":            # > 1024 distinct, a run of equal frequencies across rank 1024
        syms = rng.choice(1 << 32, size=1800, replace=False).astype(np.uint32)
        freq = np.concatenate([np.full(300, 5), np.full(1000, 2), np.full(500, 1)])
    elif kind == "equal":         # every symbol equally frequent: the heap's tie-breaks decide every length
        syms = rng.choice(1 << 32, size=nw // 4, replace=False).astype(np.uint32)
        freq = np.full(len(syms), 4)
    elif kind == "fib":           # Fibonacci frequencies: code lengths above 32
        syms = np.arange(1, 35, dtype=np.uint32) * np.uint32(0x01010101)
        freq = np.array(_fib(34), dtype=np.int64)
        freq[-1] += nw - int(freq.sum())                     # (the largest leaf takes the remainder: the chain stays)
    elif kind == "one":           # all-zero sample: one symbol, code length 0
        syms = np.zeros(1, dtype=np.uint32)
        freq = np.array([nw])
    elif kind == "zipf":          # a skewed pool with a long tail, 0 and 0xFFFFFFFF among the symbols
        pool = np.concatenate([np.array([0, 0xFFFFFFFF], dtype=np.uint32),
                               rng.choice(1 << 32, size=3000, replace=False).astype(np.uint32)])
        p = 1.0 / np.arange(1, len(pool) + 1) ** 1.1
        p /= p.sum()
        draw = rng.choice(len(pool), size=nw, p=p)
        syms, freq = np.unique(pool[draw], return_counts=True)
    else:
        raise ValueError(kind)
    freq = np.asarray(freq, dtype=np.int64)
    total = int(freq.sum())
    assert total <= nw, (kind, total, nw)
    sample = np.repeat(syms, freq)
    if total < nw:                # the remainder: one more symbol (0x7E7E7E7E)
        sample = np.concatenate([sample, np.full(nw - total, 0x7E7E7E7E, dtype=np.uint32)])
    sample = sample[rng.permutation(nw)]
    p = freq / freq.sum()
    tail = syms[rng.choice(len(syms), size=post * W, p=p)]
    noise = rng.random(post * W) < 0.2
    tail = np.where(noise, rng.integers(0, 1 << 32, size=post * W, dtype=np.uint64).astype(np.uint32), tail)
    words = np.concatenate([sample, tail]).astype("<u4")
    return words.view(np.uint8).reshape(S + post, L)


def digest(lines: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(lines).tobytes()).hexdigest()


CASES = [
    {"name": "ties_at_cut_L64", "kind": "ties", "L": 64, "S": 250, "post": 400, "seed": 101},
    {"name": "equal_freqs_L32", "kind": "equal", "L": 32, "S": 256, "post": 400, "seed": 102},
    {"name": "fibonacci_L256", "kind": "fib", "L": 256, "S": 233290, "post": 300, "seed": 103},
    {"name": "one_symbol_L64", "kind": "one", "L": 64, "S": 100, "post": 200, "seed": 104},
    {"name": "fewer_than_S_L128", "kind": "zipf", "L": 128, "S": 500, "post": 0, "seed": 105, "n": 300},
    {"name": "zipf_L32", "kind": "zipf", "L": 32, "S": 600, "post": 500, "seed": 106},
    {"name": "zipf_L64", "kind": "zipf", "L": 64, "S": 400, "post": 500, "seed": 107},
    {"name": "zipf_L128", "kind": "zipf", "L": 128, "S": 300, "post": 400, "seed": 108},
    {"name": "zipf_L256", "kind": "zipf", "L": 256, "S": 200, "post": 300, "seed": 109},
    # chosen words: the selection's early exit and first eviction, a count digit that holds exactly what is needed, a tie
    # decided in the low symbol byte with 0 evicted and 0xFFFFFFFF kept, 0 evicted from a sample, a bucket layout that
    # needs its second seed pair
    {"name": "keys_distinct_1024", "kind": "keys", "builder": "distinct_1024", "L": 64, "S": 65, "post": 80},
    {"name": "keys_distinct_1025", "kind": "keys", "builder": "distinct_1025", "L": 64, "S": 65, "post": 80},
    {"name": "keys_top_group_1024", "kind": "keys", "builder": "top_group_1024", "L": 64, "S": 160, "post": 120},
    {"name": "keys_tie_byte0", "kind": "keys", "builder": "tie_byte0_with_zero_and_ones", "L": 64, "S": 116, "post": 120},
    {"name": "keys_evicted_zero", "kind": "keys", "builder": "evicted_zero", "L": 64, "S": 65, "post": 100},
    {"name": "keys_retry_once", "kind": "keys", "builder": "retry_once", "L": 64, "S": 128, "post": 120},
]


def case_input(spec: dict) -> np.ndarray:
    """The lines the compressor sees (a case with "n" stops early: fewer lines than S)."""
    lines = case_lines(spec)
    return lines[:spec["n"]] if "n" in spec else lines
