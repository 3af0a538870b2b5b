"""The line cache of the reference's Pattern analyser (LRU.h as Pattern.cpp:109-116 drives it: ``exist``, and on a miss
``put``; ``get`` is never called, so the "LRU" is a FIFO over insertions) restated, independent of the library:

    fifo_flags          the cache itself: a set and the order of insertion, the oldest entry dropped beyond the capacity
    launch_flags        the same answer launch by launch, from insertion stamps alone (gone / safe / at risk), which is
                        how the evicting set of the library works
    Fifo                fifo_flags carried across calls, for the tests that feed a trace in pieces

and the seeded inputs of the parity fixture (tests/golden/ref_pattern_evict_vectors.npz), so that the tests can rebuild
them."""
from __future__ import annotations

import hashlib
from collections import OrderedDict

import numpy as np

CAPACITY = (1 << 24) - 1
CAPACITIES = (1, 2, 5, 64, 1000)
LINE_SIZES = (8, 64, 72)
TRACES = ("rand_c-1", "rand_c", "rand_c+1", "rand_2c", "rand_3c+1", "cyc_c", "cyc_c+1", "mix")
GOLDEN = 0x9E3779B97F4A7C15
# the real-capacity case: half-open ranges of v[i] = i * GOLDEN (8-byte lines), one call each
REAL_PARTS = ((0, CAPACITY + 5000), (0, 10000), (CAPACITY, CAPACITY + 5000), (20000, 21000), (10000, 16000))
# what the fixture records after every part of it
REAL_FIELDS = ("lines", "Z", "R", "T", "U", "Total") + tuple(f"implicit{k}" for k in range(6)) + tuple(f"explicit{k}" for k in range(6))


# ---------------------------------------------------------------------------------------------------------------------
# the cache
# ---------------------------------------------------------------------------------------------------------------------
class Fifo:
    """LRUCache<KEY, int> under exist / put only."""

    def __init__(self, capacity: int):
        self.capacity = capacity
        self.items = OrderedDict()          # oldest first
        self.insertions = 0

    def existed(self, key) -> bool:
        if key in self.items:               # exist(): nothing moves
            return True
        self.items[key] = 0                 # put(): to the front, then clean()
        self.insertions += 1
        while len(self.items) > self.capacity:
            self.items.popitem(last=False)
        return False

    def feed(self, keys) -> np.ndarray:
        return np.array([self.existed(k) for k in keys], dtype=bool)


def fifo_flags(keys, capacity: int):
    """(existed flag per key, insertions)."""
    f = Fifo(capacity)
    flags = f.feed(keys)
    return flags, f.insertions


def launch_flags(keys, capacity: int, launch: int):
    """The same, in launches of `launch` <= capacity keys.  A stamp is the number of insertions before an insertion; an
    entry is live while stamp >= insertions - capacity.  Per launch of n keys that starts at I0 insertions, a distinct key
    with latest stamp s is gone (no entry or s < I0 - C: its first occurrence misses, every later one hits), safe
    (s >= I0 + n - C: all hit) or at risk (the occurrence at p hits while s >= I0 + m(p) - C, m(p) the misses of the launch
    before p; the first one that fails re-inserts the key).  Only the at-risk occurrences are walked in order."""
    assert 1 <= launch <= capacity
    C = capacity
    stamps, I = {}, 0
    out = np.zeros(len(keys), dtype=bool)
    for at in range(0, len(keys), launch):
        part = keys[at:at + launch]
        n, I0 = len(part), I
        first = {}
        for p, k in enumerate(part):
            first.setdefault(k, p)
        kind = {}
        for k in first:
            s = stamps.get(k)
            kind[k] = "gone" if s is None or s < I0 - C else "safe" if s >= I0 + n - C else "risk"
        gone_first = np.array([kind[k] == "gone" and first[k] == p for p, k in enumerate(part)], dtype=np.int64)
        A = np.concatenate([[0], np.cumsum(gone_first)])[:-1]                     # first prefix sum
        miss = gone_first.astype(bool)
        risk_missed = 0
        for p, k in enumerate(part):                                                # the walk: at-risk occurrences only
            if kind[k] != "risk":
                continue
            if stamps[k] < I0 + int(A[p]) + risk_missed - C:
                miss[p] = True
                stamps[k] = I0 + int(A[p]) + risk_missed
                risk_missed += 1
        m = np.concatenate([[0], np.cumsum(miss)])                                  # second prefix sum
        for p, k in enumerate(part):
            if gone_first[p]:
                stamps[k] = I0 + int(m[p])
        I = I0 + int(m[-1])
        out[at:at + n] = ~miss
    return out, I


# ---------------------------------------------------------------------------------------------------------------------
# the seeded cases
# ---------------------------------------------------------------------------------------------------------------------
def _cases():
    out = []
    for C in CAPACITIES:
        for L in LINE_SIZES:
            for t, trace in enumerate(TRACES):
                out.append({"name": f"C{C}_L{L}_{trace}", "C": C, "L": L, "trace": trace, "n": 3000 + 6 * C,
                            "seed": 7000 + 100 * CAPACITIES.index(C) + 10 * LINE_SIZES.index(L) + t})
    return out


CASES = _cases()


def case_index(spec) -> np.ndarray:
    """Which distinct line stands at every position of the trace."""
    C, n, trace = spec["C"], spec["n"], spec["trace"]
    rng = np.random.default_rng(spec["seed"])
    if trace.startswith("rand_"):
        u = {"c-1": max(1, C - 1), "c": C, "c+1": C + 1, "2c": 2 * C, "3c+1": 3 * C + 1}[trace[5:]]
        return rng.integers(0, u, n)
    if trace == "cyc_c":
        return np.arange(n) % C                 # everything hits after the first sweep
    if trace == "cyc_c+1":
        return np.arange(n) % (C + 1)           # everything misses
    pick = rng.random(n) < 0.8                  # 80 / 20 mix of the two sweeps, each going on where it was
    a, b = np.cumsum(pick) - 1, np.cumsum(~pick) - 1
    return np.where(pick, a % C, b % (C + 1))


def pool(spec) -> np.ndarray:
    """3 C + 1 distinct lines of L bytes: random bytes, the line's number in the first four."""
    rng = np.random.default_rng(spec["seed"] + 50000)
    u = 3 * spec["C"] + 1
    out = rng.integers(0, 256, (u, spec["L"]), dtype=np.uint8)
    out[:, :4] = np.arange(u, dtype="<u4").view(np.uint8).reshape(u, 4)
    return out


def case_input(spec) -> np.ndarray:
    return np.ascontiguousarray(pool(spec)[case_index(spec)])


def keys_of(lines: np.ndarray) -> list:
    return [r.tobytes() for r in np.ascontiguousarray(lines)]


def real_lines(a: int, b: int) -> np.ndarray:
    """v[a:b] of the real-capacity case as [b - a, 8] uint8."""
    with np.errstate(over="ignore"):
        v = np.arange(a, b, dtype=np.uint64) * np.uint64(GOLDEN)
    return v.astype("<u8").view(np.uint8).reshape(-1, 8)


def digest(lines: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(lines).tobytes()).hexdigest()
