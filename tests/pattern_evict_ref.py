"""The line cache of the reference's Pattern analyser (LRU.h as Pattern.cpp:109-116 drives it: ``exist``, and on a miss
``put``; ``get`` is never called, so the "LRU" is a FIFO over insertions) restated, independent of the library:

    fifo_flags          the cache itself: a set and the order of insertion, the oldest entry dropped beyond the capacity
    launch_flags        the same answer launch by launch, from insertion stamps alone (gone / safe / at risk), which is
                        how the evicting set of the library works
    Fifo                fifo_flags carried across calls, for the tests that feed a trace in pieces
    census              launch_flags with the two table generations of the evicting set and a count of everything a
                        sequence of launches makes the device do: which test inputs reach which events

and the seeded inputs of the parity fixtures (tests/golden/ref_pattern_evict_vectors.npz and
ref_pattern_evict_mid_vectors.npz), so that the tests can rebuild them; edge_index draws a trace that aims at the
events of the at-risk walk."""
from __future__ import annotations

import functools
import hashlib
from collections import OrderedDict

import numpy as np

CAPACITY = (1 << 24) - 1
CAPACITIES = (1, 2, 5, 64, 1000)
LINE_SIZES = (8, 64, 72)
TRACES = ("rand_c-1", "rand_c", "rand_c+1", "rand_2c", "rand_3c+1", "cyc_c", "cyc_c+1", "mix", "edge")
FIXTURE_TRACES = TRACES[:8]             # the traces of ref_pattern_evict_vectors.npz
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
            for t, trace in enumerate(FIXTURE_TRACES):
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
    if trace == "edge":
        return edge_index(C, n, spec["seed"])[0]
    pick = rng.random(n) < 0.8                  # 80 / 20 mix of the two sweeps, each going on where it was
    a, b = np.cumsum(pick) - 1, np.cumsum(~pick) - 1
    return np.where(pick, a % C, b % (C + 1))


# ---------------------------------------------------------------------------------------------------------------------
# the edge-driven trace
# ---------------------------------------------------------------------------------------------------------------------
# A motif is a string of actions, each one position of the trace:
#   O  the oldest live entry: hits; its stamp is exactly insertions - C, so it is at risk in any launch
#   F  a line never seen: misses.  (Once all 3 C + 1 lines of the pool have been seen: the line whose eviction lies
#      furthest back, which misses as well.)
#   E  the most recently evicted line: misses
#   N  the newest entry: hits
#   R  the line of the previous position again: hits
#   D  a line evicted 2 C to 3 C evictions ago: what the cache says (it may have come back since)
# OFER is the point: hit, miss, miss-and-reinsert and hit on one entry within four positions.
MOTIFS = (("OFER", 6), ("OR", 2), ("FE", 2), ("N", 1), ("F", 3), ("OFFEOR", 2), ("D", 1), ("EE", 1), ("ONFE", 2))
EDGE_SEED = 77


@functools.lru_cache(maxsize=4)
def edge_index(C: int, n: int, seed: int):
    """(which distinct line stands at every position, the outcome every position intends: True = existed).  Drives a
    Fifo online: C fresh lines, then weighted motifs until n positions exist.  Lines are numbered as they first appear."""
    rng = np.random.default_rng(seed)
    w = np.array([m[1] for m in MOTIFS], dtype=np.float64)
    draw = rng.choice(len(MOTIFS), size=n, p=w / w.sum()).tolist()        # (one per motif: more than are used)
    back = rng.integers(2 * C, 3 * C + 1, size=n).tolist()                  # (one per position, read by D)
    fifo, fresh, pool_size = Fifo(C), 0, 3 * C + 1
    evicted = OrderedDict()                 # the lines outside the cache that were in it, in the order they left it
    log = []                                # every eviction, in order
    idx, want = [], []

    def visit(key, hit):
        if key not in fifo.items:
            if len(fifo.items) == C:
                victim = next(iter(fifo.items))
                evicted[victim] = 0
                log.append(victim)
            evicted.pop(key, None)
        assert fifo.existed(key) == hit, (len(idx), key, hit)
        idx.append(key)
        want.append(hit)

    def unseen():
        nonlocal fresh
        if fresh < pool_size:
            fresh += 1
            return fresh - 1
        return next(iter(evicted))

    while len(idx) < min(n, C):             # fill
        visit(unseen(), False)
    motif = 0
    while len(idx) < n:
        for action in MOTIFS[draw[motif]][0]:
            if len(idx) == n:
                break
            if action == "O":
                visit(next(iter(fifo.items)), True)
            elif action == "N":
                visit(next(reversed(fifo.items)), True)
            elif action == "R":
                visit(idx[-1], True)
            elif action == "E" and log:
                visit(log[-1], False)
            elif action == "D" and len(log) >= back[len(idx)]:
                key = log[len(log) - back[len(idx)]]
                visit(key, key in fifo.items)
            else:                           # F; E and D before enough lines have been evicted
                visit(unseen(), False)
        motif += 1
    out = np.array(idx, dtype=np.int64), np.array(want, dtype=bool)
    for a in out:
        a.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the census
# ---------------------------------------------------------------------------------------------------------------------
KIND_HIT, KIND_GONE_FIRST, KIND_RISK, KIND_RISK_MISS = 0, 1, 2, 3       # MPC_ELINE_* of csrc/mpc_pattern.h
BLOCK = 256                                                            # lines per block of classify / scatter, per walk batch
PAIRS = ("hit_hit", "hit_miss", "miss_hit", "miss_miss")
SUMMED = ("rotations", "found_newer", "found_older_live", "found_older_dead", "found_nowhere", "lines_gone", "lines_safe",
          "lines_risk", "gone_firsts", "risk", "risk_hits", "risk_misses") + tuple(f"{w}_{p}" for w in ("same", "later") for p in PAIRS) + (
          "gone_first_at_0", "gone_first_at_255", "risk_at_0", "risk_at_255", "walk_at_0", "walk_at_255")
COUNTERS = ("launches", "rotations", "gone_firsts", "risk", "risk_misses")      # what mpc_test_evict_counters returns, list B aside


def _count(mask) -> int:
    return int(np.count_nonzero(mask))


def _blocks(pos) -> int:
    """In how many different blocks the ascending positions lie."""
    return 1 + _count(np.diff(pos // BLOCK)) if len(pos) else 0


def cut_launches(cuts, launch_max: int):
    """The launches [a, b) that calls [cuts[k], cuts[k + 1]) are split into."""
    out = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        out += [(at, min(b, at + launch_max)) for at in range(a, b, launch_max)]
    return out


def _few_lines(keys, I0, C, stamp, newer, older, c):
    """One launch of the census in plain Python, position by position: the same counts as the array code of census(), which
    pays dozens of array calls per launch and so is slow where a trace is thousands of launches of a few lines each.
    tests/test_pattern_evict_mid_cpu.py runs both over the same traces and requires every result to be equal.  Returns
    (missed or not, KIND_*) per position; updates stamp, newer and the counters c."""
    n, first, state = len(keys), {}, {}
    for p, key in enumerate(keys):
        first.setdefault(key, p)
    for key in first:
        s, in_new, in_old = int(stamp[key]), bool(newer[key]), bool(older[key])
        assert (in_new or in_old) == (s >= 0)
        gone = s < 0 or s < I0 - C
        safe = not gone and s >= I0 + n - C
        c["found_newer"] += in_new
        c["found_nowhere"] += not (in_new or in_old)
        c["found_older_live"] += in_old and not in_new and not gone
        c["found_older_dead"] += in_old and not in_new and gone
        c["lines_gone"] += gone
        c["lines_safe"] += safe
        c["lines_risk"] += not (gone or safe)
        state[key] = [KIND_GONE_FIRST if gone else KIND_HIT if safe else KIND_RISK, s]
    miss, kind, misses, walk, last = [False] * n, [KIND_HIT] * n, 0, 0, {}
    blocks = {"gone_first": set(), "risk": set()}
    for p, key in enumerate(keys):
        st = state[key]
        if st[0] == KIND_HIT or (st[0] == KIND_GONE_FIRST and first[key] != p):
            continue
        name = "gone_first" if st[0] == KIND_GONE_FIRST else "risk"
        c[name + "_at_0"] += p % BLOCK == 0
        c[name + "_at_255"] += p % BLOCK == BLOCK - 1
        blocks[name].add(p // BLOCK)
        now = I0 + misses                               # the insertions before p
        if st[0] == KIND_GONE_FIRST:
            miss[p], kind[p], st[1] = True, KIND_GONE_FIRST, now
            c["gone_firsts"] += 1
        else:
            miss[p] = st[1] < now - C
            kind[p] = KIND_RISK_MISS if miss[p] else KIND_RISK
            if miss[p]:
                st[1] = now
            was = last.get(key)
            if was is not None:
                c[("same_" if was[0] // BLOCK == walk // BLOCK else "later_") + PAIRS[2 * was[1] + miss[p]]] += 1
            last[key] = (walk, int(miss[p]))
            c["walk_at_0"] += walk % BLOCK == 0
            c["walk_at_255"] += walk % BLOCK == BLOCK - 1
            c["risk"] += 1
            c["risk_misses" if miss[p] else "risk_hits"] += 1
            walk += 1
        misses += miss[p]
    assert c["same_miss_miss"] == 0 and c["later_miss_miss"] == 0
    for key, st in state.items():
        stamp[key], newer[key] = st[1], True
    c.update(n=n, blocks=-(-n // BLOCK), walk_batches=-(-walk // BLOCK), gone_first_blocks=len(blocks["gone_first"]), risk_blocks=len(blocks["risk"]))
    return miss, kind


def census(keys, capacity: int, launch_max: int, cuts, few: int = 16):
    """launch_flags over the calls keys[cuts[k]:cuts[k + 1]], each split into launches of at most launch_max keys, with
    the two table generations of the evicting set: at a launch boundary where the insertions since the last rotation have
    reached C the older table is emptied and becomes the newer one, and the newer one the older.  `keys` are small
    non-negative integers.  Returns a dict:
        flags, insertions   as launch_flags
        kinds               the KIND_* of every position
        launches            per launch a dict of counters (SUMMED, and n, blocks, walk_batches, gone_first_blocks, risk_blocks)
        total               the sums of SUMMED over the launches; launches; max_blocks, max_walk_batches; the launches whose
                            gone firsts / at-risk occurrences lie in more than 256 different blocks
        calls, after_launch after every call, and after every launch, the cumulative COUNTERS
    Found where (per launch, distinct lines): in the newer table; only in the older one with a live / a dead stamp; in
    neither.  Transitions: of one entry between consecutive at-risk occurrences of a launch, by same or later walk batch
    and by outcome pair; miss -> miss cannot happen, as a re-stamped entry outlives the launch (n <= C).
    Launches of at most `few` lines are counted by _few_lines (0: none are)."""
    keys = np.asarray(keys, dtype=np.int64)
    C = capacity
    assert 1 <= launch_max <= C and cuts[0] == 0 and cuts[-1] == len(keys) and all(a <= b for a, b in zip(cuts[:-1], cuts[1:]))
    U = int(keys.max()) + 1 if len(keys) else 1
    stamp = np.full(U, -1, dtype=np.int64)              # the latest stamp a table holds for the line, -1: none
    newer, older = np.zeros(U, dtype=bool), np.zeros(U, dtype=bool)
    I = I_rot = 0
    flags, kinds = np.zeros(len(keys), dtype=bool), np.zeros(len(keys), dtype=np.uint8)
    launches, calls, after, run = [], [], [], dict.fromkeys(COUNTERS, 0)
    for a, b in zip(cuts[:-1], cuts[1:]):
        for at, end in cut_launches([a, b], launch_max):
            part = keys[at:end]
            n, I0 = len(part), I
            c = dict.fromkeys(SUMMED, 0)
            if I - I_rot >= C:                          # rotate: what only the older table knew is forgotten, and was dead
                lost = older & ~newer
                assert (stamp[lost] < I0 - C).all()
                stamp[lost] = -1
                older, newer = newer, np.zeros(U, dtype=bool)
                I_rot, c["rotations"] = I, 1
            if n <= few:
                miss, k = _few_lines(part.tolist(), I0, C, stamp, newer, older, c)
                I = I0 + sum(miss)
                flags[at:end], kinds[at:end] = ~np.array(miss, dtype=bool), k
                launches.append(c)
                run["launches"] += 1
                for name in COUNTERS[1:]:
                    run[name] += c[name]
                after.append([run[name] for name in COUNTERS])
                continue
            uniq, first, inv = np.unique(part, return_index=True, return_inverse=True)
            inv = inv.reshape(-1)
            s = stamp[uniq]
            gone = (s < 0) | (s < I0 - C)
            safe = ~gone & (s >= I0 + n - C)
            risk = ~gone & ~safe
            in_new, in_old = newer[uniq], older[uniq]
            assert ((in_new | in_old) == (s >= 0)).all()            # a table knows the line, or nothing does
            # one histogram for the counts per line: bit 0 in the newer table, 1 in the older, 2 gone, 3 safe
            h = np.bincount(in_new.view(np.uint8) | in_old.view(np.uint8) << 1 | gone.view(np.uint8) << 2 | safe.view(np.uint8) << 3, minlength=16).tolist()
            c["found_newer"], c["found_nowhere"] = sum(h[1::2]), sum(h[0::4])
            c["found_older_live"], c["found_older_dead"] = h[2] + h[10], h[6]
            c["lines_gone"], c["lines_safe"] = sum(h[4:8]), sum(h[8:12])
            c["lines_risk"] = len(uniq) - c["lines_gone"] - c["lines_safe"]
            assert not any(h[12:])
            gone_first = np.zeros(n, dtype=bool)
            gone_first[first[gone]] = True
            A = np.cumsum(gone_first) - gone_first      # gone firsts before p
            risk_pos = np.flatnonzero(risk[inv])
            # the walk: the at-risk occurrences in order
            cur, missed, last, missed_at = s.tolist(), 0, {}, []
            for j, (e, before) in enumerate(zip(inv[risk_pos].tolist(), A[risk_pos].tolist())):
                now = I0 + before + missed
                miss = cur[e] < now - C
                if miss:
                    cur[e] = now
                    missed += 1
                    missed_at.append(j)
                was = last.get(e)
                if was is not None:
                    c[("same_" if was[0] // BLOCK == j // BLOCK else "later_") + PAIRS[2 * was[1] + miss]] += 1
                last[e] = (j, int(miss))
            assert c["same_miss_miss"] == 0 and c["later_miss_miss"] == 0
            miss = gone_first.copy()
            miss[risk_pos[missed_at]] = True
            m = np.cumsum(miss) - miss                  # misses before p
            stamp[uniq[gone]] = I0 + m[first[gone]]
            stamp[uniq[risk]] = np.array(cur, dtype=np.int64)[risk]
            newer[uniq] = True
            I = I0 + _count(miss)
            flags[at:end] = ~miss
            k = kinds[at:end]
            k[gone_first], k[risk_pos] = KIND_GONE_FIRST, KIND_RISK
            k[risk_pos[missed_at]] = KIND_RISK_MISS
            gf_pos, n_risk = np.flatnonzero(gone_first), len(risk_pos)
            c["gone_firsts"], c["risk"], c["risk_misses"], c["risk_hits"] = len(gf_pos), n_risk, missed, n_risk - missed
            for name, where in (("gone_first", gf_pos), ("risk", risk_pos)):
                r = where % BLOCK
                c[name + "_at_0"], c[name + "_at_255"] = _count(r == 0), _count(r == BLOCK - 1)
            c["walk_at_0"], c["walk_at_255"] = -(-n_risk // BLOCK), n_risk // BLOCK      # walk indices 0 .. n_risk - 1
            c.update(n=n, blocks=-(-n // BLOCK), walk_batches=-(-n_risk // BLOCK), gone_first_blocks=_blocks(gf_pos), risk_blocks=_blocks(risk_pos))
            launches.append(c)
            run["launches"] += 1
            for name in COUNTERS[1:]:
                run[name] += c[name]
            after.append([run[name] for name in COUNTERS])
        calls.append([run[name] for name in COUNTERS])
    total = {name: sum(c[name] for c in launches) for name in SUMMED}
    total.update(launches=len(launches), max_blocks=max((c["blocks"] for c in launches), default=0),
                 max_walk_batches=max((c["walk_batches"] for c in launches), default=0),
                 launches_gone_first_blocks_over_256=sum(c["gone_first_blocks"] > 256 for c in launches),
                 launches_risk_blocks_over_256=sum(c["risk_blocks"] > 256 for c in launches))
    return {"flags": flags, "insertions": I, "kinds": kinds, "launches": launches, "total": total, "calls": calls, "after_launch": after}


# ---------------------------------------------------------------------------------------------------------------------
# the mid-capacity cases (tests/golden/ref_pattern_evict_mid_vectors.npz)
# ---------------------------------------------------------------------------------------------------------------------
# 65537 lines are 257 blocks: the scan runs with per = 2, thread 128 takes one block and the threads above it none.
# 262145 lines are 1025 blocks: per = 5, the threads from 205 up idle.
MID_PLAN = ((65537, 8, ("edge", "rand_2c", "mix", "cyc_c+1", "cyc_c")), (65537, 64, ("edge", "mix")), (262145, 8, ("edge", "rand_2c"))) + tuple(
    (C, 64, ("edge",)) for C in CAPACITIES)
CUT_STEPS = (1, 255, 256, 257, 30000, "C-1", "C", "C+1")       # then the rest


def _mid_cases():
    out = []
    for C, L, traces in MID_PLAN:
        for trace in traces:
            out.append({"name": f"C{C}_L{L}_{trace}", "C": C, "L": L, "trace": trace, "n": 3000 + 6 * C,
                        "seed": EDGE_SEED if trace == "edge" else 9000 + len(out)})
    return out


MID_CASES = _mid_cases()


def mid_cuts(spec):
    """The call boundaries of the mid-capacity tests: no multiple of 256, a full launch, and a full launch plus one line."""
    C, n, cuts = spec["C"], spec["n"], [0]
    for step in CUT_STEPS:
        step = {"C-1": C - 1, "C": C, "C+1": C + 1}.get(step, step)
        if step > 0 and cuts[-1] < n:
            cuts.append(min(n, cuts[-1] + step))
    return cuts + ([n] if cuts[-1] < n else [])


# the cases that the test library replays launch by launch (tests/test_pattern_evict_mid_gpu.py)
TESTLIB_CASES = ("C65537_L8_edge", "C65537_L8_cyc_c+1", "C1000_L64_edge")
LAUNCH_LIMIT = 1 << 22                      # MPC_PATTERN_CHUNK of csrc/mpc_pattern.h


def coverage_of(spec):
    """(what tests/golden/pattern_evict_coverage.json holds for the case, the two census results it comes from): the
    census in one call ("one") and in the calls of mid_cuts ("cuts"), with launches of min(C, LAUNCH_LIMIT) lines."""
    idx, out, runs = case_index(spec), {}, {}
    for how, cuts in (("one", [0, spec["n"]]), ("cuts", mid_cuts(spec))):
        z = census(idx, spec["C"], min(spec["C"], LAUNCH_LIMIT), cuts)
        out[how] = {"cuts": [int(x) for x in cuts], "insertions": z["insertions"], "total": z["total"], "calls": z["calls"]}
        if how == "cuts" and spec["name"] in TESTLIB_CASES:
            out[how]["after_launch"] = z["after_launch"]
        runs[how] = z
    return out, runs


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
