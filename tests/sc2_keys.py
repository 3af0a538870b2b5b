"""Chosen words for SC2's hash structures (numpy only, independent of the library).

`mpc_sc2_hash` (csrc/mpc_sc2.h) is a bijection on 32-bit words: xor, odd multiply, xorshift, odd multiply, xorshift.
`sc2_hash_inv` undoes it, so a builder can write down the words that land in a chosen slot of the LDS counting table
(seed 0, 8192 slots), of the global counting table (seed 0x5C2, the power of two >= 2 S W slots) or in a chosen bucket
of the sizing table under a chosen seed pair of `mpcsc2::layout` (`layout_seeds`, `layout_model`).

Every builder returns `(lines, L, S, note)`: `lines` is uint8 [n, L] (S warm-up lines, then the tail that is sized from
the table), `note` says which structure the case is aimed at and which path it reaches.  A builder asserts its own
premise.  Nothing here says what SC2 should answer: expected sizes and tables always come from sc2_ref.SC2Ref."""
from __future__ import annotations

import functools

import numpy as np

M32 = 0xFFFFFFFF
ENTRIES = 1024
MAX_BUCKETS = 2048
LDS_SLOTS = 8192          # kCountSlots
GROUP_WORDS = 4096        # kCountWords: words counted by one workgroup
GLOBAL_SEED = 0x5C2
MIN_LINE = 4              # the smallest line size check_line_size(Algo::SC2) accepts (kAlgo: min_line 4, multiple 4)
_MUL1, _MUL2 = 0x9E3779B1, 0x2C1B3C6D
_INV1, _INV2 = pow(_MUL1, -1, 1 << 32), pow(_MUL2, -1, 1 << 32)
_M = np.uint64(M32)


def sc2_hash(k, seed):
    """mpc_sc2_hash(k, seed), vectorised over uint32."""
    h = (np.asarray(k).astype(np.uint64) ^ np.uint64(seed & M32)) & _M
    h = (h * np.uint64(_MUL1)) & _M
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(_MUL2)) & _M
    h ^= h >> np.uint64(12)
    return h.astype(np.uint32)


def sc2_hash_inv(y, seed):
    """The word k with sc2_hash(k, seed) == y."""
    h = np.asarray(y).astype(np.uint64) & _M
    h ^= (h >> np.uint64(12)) ^ (h >> np.uint64(24))
    h = (h * np.uint64(_INV2)) & _M
    h ^= (h >> np.uint64(15)) ^ (h >> np.uint64(30))
    h = (h * np.uint64(_INV1)) & _M
    return (h ^ np.uint64(seed & M32)).astype(np.uint32)


def words_at(slot: int, bits: int, seed: int) -> np.ndarray:
    """All 2^(32 - bits) words whose hash under `seed` has `slot` in its low `bits` bits, in ascending hash order."""
    hi = np.arange(1 << (32 - bits), dtype=np.uint64) << np.uint64(bits)
    return sc2_hash_inv(hi | np.uint64(slot), seed)


def random_words_at(rng, slot: int, bits: int, seed: int, n: int) -> np.ndarray:
    """n distinct words of words_at(slot, bits, seed), drawn without writing all of them down."""
    hi = np.unique(rng.integers(0, 1 << (32 - bits), size=4 * n + 16, dtype=np.uint64))
    assert len(hi) >= n
    hi = hi[rng.permutation(len(hi))[:n]]
    return sc2_hash_inv((hi << np.uint64(bits)) | np.uint64(slot), seed)


def global_mask(L: int, S: int) -> int:
    """mpc_create_sc2: the counting table has the power of two >= 2 S W slots (at least 2)."""
    slots = 2
    while slots < 2 * S * (L // 4):
        slots <<= 1
    return slots - 1


def layout_seeds(n: int):
    """The first n (seed1, seed2) pairs of mpcsc2::layout: splitmix64 from state 0x5C2, low 32 bits."""
    m64 = (1 << 64) - 1
    state, out = 0x5C2, []

    def nxt():
        nonlocal state
        state = (state + 0x9E3779B97F4A7C15) & m64
        z = state
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m64
        return (z ^ (z >> 31)) & M32

    for _ in range(n):
        a = nxt()
        out.append((a, nxt()))
    return out


def layout_model(keys, lens=None, max_attempts: int = 16):
    """mpcsc2::layout restated: keys in ascending order, nb = the power of two >= 2 n (2 .. 2048), a key goes to
    bucket h(k, seed1) or, only when that one is full, to h(k, seed2); the first seed pair under which every key fits.
    -> dict(attempt, seed1, seed2, mask, fill [nb], second (the keys that sit in their second bucket),
            image [nb, 4] uint32 as the kernel reads it (lens default to 0))"""
    keys = np.asarray(keys, dtype=np.uint32)
    order = np.argsort(keys)
    keys = keys[order]
    assert len(keys) <= ENTRIES and len(np.unique(keys)) == len(keys)
    lens = np.zeros(len(keys), dtype=np.int64) if lens is None else np.asarray(lens, dtype=np.int64)[order]
    nb = 2
    while nb < 2 * len(keys) and nb < MAX_BUCKETS:
        nb <<= 1
    mask = nb - 1
    for attempt, (s1, s2) in enumerate(layout_seeds(max_attempts)):
        b1 = (sc2_hash(keys, s1) & np.uint32(mask)).tolist()
        b2 = (sc2_hash(keys, s2) & np.uint32(mask)).tolist()
        image = np.zeros((nb, 4), dtype=np.uint32)
        fill = [0] * nb
        second, ok = [], True
        for i, k in enumerate(keys.tolist()):
            b = b1[i]
            if fill[b] == 3:
                b = b2[i]
                if fill[b] == 3:
                    ok = False
                    break
                second.append(k)
            c = fill[b]
            image[b, c] = k
            image[b, 3] = (int(image[b, 3]) & 0x3FFFFFFF) | (int(lens[i]) << (10 * c)) | ((c + 1) << 30)
            fill[b] = c + 1
        if ok:
            return {"attempt": attempt, "seed1": s1, "seed2": s2, "mask": mask, "fill": np.array(fill),
                    "second": np.array(second, dtype=np.uint32), "image": image}
    raise AssertionError(f"no layout within {max_attempts} attempts")


# ---- pieces shared by the builders -----------------------------------------------------------------------------------
def _lines(words, L):
    words = np.ascontiguousarray(words, dtype="<u4")
    assert words.size % (L // 4) == 0
    out = words.view(np.uint8).reshape(-1, L)
    out.setflags(write=False)
    return out


def _random_words(rng, n, exclude=()):
    """n distinct words, none of them 0, 0xFFFFFFFF or in `exclude`."""
    got = np.unique(rng.integers(1, M32, size=n + n // 4 + 64, dtype=np.uint64).astype(np.uint32))
    got = got[~np.isin(got, np.asarray(exclude, dtype=np.uint32))]
    assert len(got) >= n
    return got[rng.permutation(len(got))[:n]]


def _uneven(rng, n, total):
    """n counts >= 1 with a skewed spread that sum to `total`."""
    assert total >= n
    p = 1.0 / np.arange(1, n + 1)
    return 1 + rng.multinomial(total - n, p / p.sum())


def _tail(rng, keys, W, n_lines, must=(), noise=0.2):
    """n_lines lines: every word of `must`, every key while there is room, then draws from the keys with random
    words mixed in, shuffled."""
    n = n_lines * W
    keys = np.asarray(keys, dtype=np.uint32)
    head = np.concatenate([np.asarray(must, dtype=np.uint32), keys])[:n]
    assert len(head) >= len(must)
    rest = keys[rng.integers(0, len(keys), size=n - len(head))]
    miss = rng.random(len(rest)) < noise
    rest = np.where(miss, rng.integers(0, 1 << 32, size=len(rest), dtype=np.uint64).astype(np.uint32), rest)
    out = np.concatenate([head, rest])
    return out[rng.permutation(n)]


def _sample(rng, syms, freq, S, W, order="shuffle"):
    freq = np.asarray(freq, dtype=np.int64)
    assert int(freq.sum()) == S * W and (freq > 0).all() and len(np.unique(syms)) == len(syms), (int(freq.sum()), S * W)
    s = np.repeat(np.asarray(syms, dtype=np.uint32), freq)
    return s[rng.permutation(len(s))] if order == "shuffle" else s


def warmup_counts(lines, S):
    return np.unique(np.asarray(lines)[:S].view("<u4"), return_counts=True)


# ---- a. the LDS counting table: a probe chain that wraps past slot 8191 -------------------------------------------------
def lds_chain_one_group():
    L, S, W = 64, 256, 16
    rng = np.random.default_rng(0xA1)
    cand = words_at(LDS_SLOTS - 1, 13, 0)
    assert len(cand) == 1 << 19
    keys = cand[rng.choice(len(cand), size=1000, replace=False)]
    assert (sc2_hash(keys, 0) & np.uint32(LDS_SLOTS - 1) == LDS_SLOTS - 1).all() and S * W == GROUP_WORDS
    sample = _sample(rng, keys, _uneven(rng, len(keys), S * W), S, W)
    tail = _tail(rng, keys, W, 96, must=[0, M32])
    note = ("LDS table: 1000 distinct words share home slot 8191 of the one workgroup's table, so the chain runs "
            "8191, 0, 1, ... 998 (sc2_lds_add wraps); <= 1024 distinct words, so each one and its count reach the table")
    return _lines(np.concatenate([sample, tail]), L), L, S, note


def lds_chain_four_groups():
    L, S, W = 64, 1024, 16
    rng = np.random.default_rng(0xA2)
    slots = [8191, 8190, 0, 4095]
    chains = []
    for s in slots:
        cand = words_at(s, 13, 0)
        chains.append(cand[rng.choice(len(cand), size=256, replace=False)])
        assert (sc2_hash(chains[-1], 0) & np.uint32(LDS_SLOTS - 1) == s).all()
    parts = []
    for g in range(4):       # workgroup g: all of chain g and half of the next one, which it shares with workgroup g + 1
        syms = np.concatenate([chains[g], chains[(g + 1) % 4][:128]])
        parts.append(_sample(rng, syms, _uneven(rng, len(syms), GROUP_WORDS), GROUP_WORDS // W, W))
    keys = np.concatenate(chains)
    assert len(np.unique(keys)) == 1024 and S * W == 4 * GROUP_WORDS
    tail = _tail(rng, keys, W, 96, must=[0, M32])
    note = ("LDS table: four workgroups, each with its own chain of 256 words at home slot 8191, 8190, 0 and 4095 plus "
            "128 words of the next workgroup's chain (the 8191 and 8190 chains merge and wrap); the shared words are "
            "summed across workgroups in the global table; 1024 distinct words, none evicted")
    return _lines(np.concatenate(parts + [tail]), L), L, S, note


# ---- b. the global counting table ---------------------------------------------------------------------------------------
def global_chain_sixteen_groups():
    L, S, W = 64, 4096, 16                       # 2^16 words: 16 workgroups
    rng = np.random.default_rng(0xB1)
    mask = global_mask(L, S)
    assert mask == (1 << 17) - 1 and S * W == 16 * GROUP_WORDS
    cand = words_at(mask, 17, GLOBAL_SEED)
    keys = cand[rng.choice(len(cand), size=1000, replace=False)]
    assert (sc2_hash(keys, GLOBAL_SEED) & np.uint32(mask) == mask).all()
    parts = []
    for _ in range(16):                          # every word in every workgroup
        parts.append(_sample(rng, keys, _uneven(rng, len(keys), GROUP_WORDS), GROUP_WORDS // W, W))
    tail = _tail(rng, keys, W, 96, must=[0, M32])
    note = (f"global table (mask {mask:#x}): 1000 distinct words share home slot {mask:#x}, so the chain runs mask, 0, 1, "
            "... 998 (sc2_global_add wraps); every word is in all 16 workgroups, so claims (CAS) and adds race on one chain")
    return _lines(np.concatenate(parts + [tail]), L), L, S, note


def global_chain_knife_edge():
    L, S, W, c = 64, 960, 16, 7
    rng = np.random.default_rng(0xB2)
    mask = global_mask(L, S)
    assert mask == (1 << 15) - 1
    cand = words_at(mask, 15, GLOBAL_SEED)
    keys = np.sort(cand[rng.choice(len(cand), size=2048, replace=False)])
    i = np.arange(2048)                          # c + 1, c, c + 1, ... and from the middle on c, c + 1, ...: both ends count c + 1
    freq = np.where((i % 2 == 0) == (i < 1024), c + 1, c)
    assert 2048 <= S * W and int(freq.sum()) == S * W
    sample = _sample(rng, keys, freq, S, W)
    tail = _tail(rng, keys, W, 160, must=[0, M32], noise=0.05)
    note = (f"global table (mask {mask:#x}): a chain of 2048 words from slot {mask:#x} across the wrap, counts alternating "
            f"{c + 1} and {c} by ascending symbol (swapped from the middle on) and spread over 4 workgroups: the table is exactly the 1024 words of "
            f"count {c + 1}, one lost or doubled increment moves a word across the cut (decided in the low count byte)")
    return _lines(np.concatenate([sample, tail]), L), L, S, note


def _smallest_table(S):
    L, W = MIN_LINE, 1
    rng = np.random.default_rng(0xB3 + S)
    mask = global_mask(L, S)
    assert mask == 2 * S - 1
    keys = random_words_at(rng, mask, mask.bit_length(), GLOBAL_SEED, S)
    assert (sc2_hash(keys, GLOBAL_SEED) & np.uint32(mask) == mask).all() and len(np.unique(keys)) == S
    tail = _tail(rng, keys, W, 40, must=[0, M32], noise=0.3)
    note = (f"global table of {mask + 1} slots (L = {L}, S = {S}): {S} distinct word(s) at home slot {mask}"
            + (", the second one wraps to slot 0" if S > 1 else "") + "; one-word lines take the any-size sizing kernel")
    return _lines(np.concatenate([keys, tail]), L), L, S, note


def smallest_table_s1():
    return _smallest_table(1)


def smallest_table_s2():
    return _smallest_table(2)


# ---- c. the radix select ------------------------------------------------------------------------------------------------
def _distinct(n):
    L, S, W = 64, 65, 16              # 1040 words just hold 1025 distinct ones
    rng = np.random.default_rng(0xC100 + n)
    keys = _random_words(rng, n)
    freq = np.ones(n, dtype=np.int64)
    freq[rng.choice(n, size=S * W - n, replace=False)] += 1
    sample = _sample(rng, keys, freq, S, W)
    tail = _tail(rng, keys, W, 80, must=[0, M32])
    note = (f"selection: exactly {n} distinct words, " +
            ("no eviction (the total <= 1024 early exit after the first histogram)" if n <= ENTRIES else
             "one eviction: all eight passes run and the smallest count-1 symbol leaves"))
    return _lines(np.concatenate([sample, tail]), L), L, S, note


def distinct_1023():
    return _distinct(1023)


def distinct_1024():
    return _distinct(1024)


def distinct_1025():
    return _distinct(1025)


def _top_group(g):
    L, S, W = 64, 160, 16
    rng = np.random.default_rng(0xC200 + g)
    n1 = S * W - 2 * g
    keys = _random_words(rng, g + n1)
    freq = np.concatenate([np.full(g, 2), np.full(n1, 1)])
    sample = _sample(rng, keys, freq, S, W)
    u, c = warmup_counts(_lines(sample, L), S)
    assert int((c == 2).sum()) == g and int((c == 1).sum()) == n1 > 400
    tail = _tail(rng, keys, W, 120, must=[0, M32])
    what = {1023: "digit 2 holds 1023 < 1024: need drops to 1, the largest count-1 symbol joins",
            1024: "digit 2 holds exactly the 1024 still needed (hist[d] < need is false at equality)",
            1025: "digit 2 holds 1025: the smallest count-2 symbol is evicted in the symbol passes"}[g]
    note = f"selection: {g} words of count 2 over {n1} of count 1; in the low count byte {what}"
    return _lines(np.concatenate([sample, tail]), L), L, S, note


def top_group_1023():
    return _top_group(1023)


def top_group_1024():
    return _top_group(1024)


def top_group_1025():
    return _top_group(1025)


def _byte_tie(p):
    """512 words of count 1 that differ only in symbol byte p (two groups of 256), below 667 fillers of count >= 2:
    357 of the 512 are kept, so the cut falls inside the lower group and is decided in the pass over byte p.  For the
    top byte both groups span all of its values, two words per digit: 668 fillers, so that the 356 kept words are
    whole digits and the first symbol pass ends on a digit that holds exactly what is still needed."""
    L, S, W = 64, 116, 16
    rng = np.random.default_rng(0xC300 + p)
    i = np.arange(256, dtype=np.uint64) << np.uint64(8 * p)
    if p == 0:
        base_a, base_b = 0x00000000, 0xFFFFFF00                    # the tie includes 0 and 0xFFFFFFFF
    elif p == 3:
        base_a, base_b = 0x00000000, 0x00FFFFFF                    # (both groups span every top byte; 0 and 0xFFFFFFFF again)
    else:
        base_a = 0xAABBCCDD & ~(0xFF << (8 * p)) & M32
        base_b = base_a + (1 << (8 * (p + 1)))
    tied = np.concatenate([(i | np.uint64(base_a)), (i | np.uint64(base_b))]).astype(np.uint32)
    assert len(np.unique(tied)) == 512
    n_fill = 668 if p == 3 else 667
    n_kept = ENTRIES - n_fill
    fill = _random_words(rng, n_fill, exclude=tied)
    freq = np.concatenate([np.ones(512, dtype=np.int64), 1 + _uneven(rng, n_fill, S * W - 512 - n_fill)])
    sample = _sample(rng, np.concatenate([tied, fill]), freq, S, W)
    kept = np.sort(tied)[512 - n_kept:]
    lost = np.sort(tied)[:512 - n_kept]
    if p < 3:      # the cut is inside the lower group: kept and lost words around it differ in byte p alone
        assert (kept[0] ^ lost[-1]) >> (8 * p) < 256 and (kept[0] ^ lost[-1]) & ((1 << (8 * p)) - 1) == 0
    else:          # digits 0x4E .. 0xFF of the top byte, two words each, are kept
        assert lost[-1] == 0x4DFFFFFF and kept[0] == 0x4E000000
    tail = _tail(rng, np.concatenate([tied, fill]), W, 120, must=[0, M32])
    note = (f"selection: a tie of 512 count-1 words across rank 1024 that differ only in symbol byte {p} "
            f"({int(tied[0]):#010x}.. and {int(tied[256]):#010x}..), {n_kept} of them kept below {n_fill} words of count >= 2: the pass "
            f"over symbol byte {p} decides" + ("; 0 is evicted, 0xFFFFFFFF kept" if p in (0, 3) else ""))
    return _lines(np.concatenate([sample, tail]), L), L, S, note


def tie_byte0_with_zero_and_ones():
    return _byte_tie(0)


def tie_byte1():
    return _byte_tie(1)


def tie_byte2():
    return _byte_tie(2)


def tie_byte3():
    return _byte_tie(3)


def cut_in_second_count_byte():
    L, W = 256, 64
    rng = np.random.default_rng(0xC4)
    keys = _random_words(rng, 1100)
    freq = np.concatenate([512 + rng.integers(0, 40, size=600), 256 + rng.integers(0, 7, size=500)])
    total = int(freq.sum())
    S = -(-total // W)
    freq[0] += S * W - total
    assert (freq >= 256).all() and int((freq >> 8 == 2).sum()) == 600 and int((freq >> 8 == 1).sum()) == 500
    sample = _sample(rng, keys, freq, S, W)
    tail = _tail(rng, keys, W, 40, must=[0, M32])
    note = (f"selection (L = 256, S = {S}): 1100 words of count >= 256; the second count byte is 2 for 600 of them and 1 for "
            "500, so that pass takes digit 2 whole (need 1024 -> 424) and cuts inside digit 1; ties of equal count go on "
            "into the symbol bytes")
    return _lines(np.concatenate([sample, tail]), L), L, S, note


def count_2_24(second_heavy: bool = True):
    """The one large case: about 128 MiB.  Contiguous runs, so a workgroup sends one atomic per distinct word."""
    L, W = 256, 64
    rng = np.random.default_rng(0xC5)
    small = np.sort(_random_words(rng, 1500))
    heavy = np.array([0x5EED0001, 0x5EED0002], dtype=np.uint32)
    hf = [1 << 24, (1 << 24) - 1] if second_heavy else [1 << 24]
    n_small = 3009 if second_heavy else 3008
    sf = np.full(1500, 2)
    sf[rng.choice(1500, size=n_small - 3000, replace=False)] += 1
    total = sum(hf) + n_small
    assert total % W == 0 and not np.isin(heavy, small).any()
    S = total // W
    sample = _sample(rng, np.concatenate([heavy[:len(hf)], small]), np.concatenate([hf, sf]), S, W, order="runs")
    tail = _tail(rng, np.concatenate([heavy[:len(hf)], small]), W, 32, must=[0, M32])
    note = (f"selection (L = 256, S = {S}): counts {' and '.join(str(h) for h in hf)} over 1500 words of count 2 or 3: the "
            f"top digit (count >> 24) is 1 for one word, so need drops to 1023 in the first pass; a count kept modulo 2^24 "
            "loses that word")
    return _lines(np.concatenate([sample, tail]), L), L, S, note


# ---- d. the bucket image of the sizing table ----------------------------------------------------------------------------
def _sharing_both_buckets(rng, s1, s2, mask, n, exclude):
    """n words with one first and one second bucket under (s1, s2)."""
    bits = mask.bit_length()
    b1 = int(rng.integers(0, mask + 1))
    cand = words_at(b1, bits, s1)
    b2s = sc2_hash(cand, s2) & np.uint32(mask)
    b2 = int(b2s[int(rng.integers(0, len(cand)))])
    cand = cand[(b2s == b2) & ~np.isin(cand, np.asarray(exclude, dtype=np.uint32)) & (cand != 0) & (cand != M32)]
    assert b1 != b2 and len(cand) >= n
    return cand[rng.choice(len(cand), size=n, replace=False)], len(cand)


@functools.lru_cache(maxsize=None)
def bucket_plan(name: str):
    """A family d case with what it steers: dict(keys, model, misses {kind: words}, lines, L, S, note)."""
    L, S, W = 64, 128, 16
    rng = np.random.default_rng({"full_bucket": 0xD1, "retry_once": 0xD2, "retry_twice": 0xD3}[name])
    want_attempt, zero_fill = {"full_bucket": (0, 1), "retry_once": (1, 2), "retry_twice": (2, 0)}[name]
    seeds = layout_seeds(3)
    mask = MAX_BUCKETS - 1
    m32 = np.uint32(mask)
    s1, s2 = seeds[want_attempt]
    fillers = _random_words(rng, 880)
    special, premise = [], ""
    if name == "full_bucket":
        # seven words name bucket B first; the three smallest fill it, the other four go to four different second buckets
        B = int(rng.integers(0, mask + 1))
        cand = words_at(B, 11, s1)
        while True:
            seven = np.sort(cand[rng.choice(len(cand), size=7, replace=False)])
            second = sc2_hash(seven[3:], s2) & m32
            if len(set(second.tolist()) | {B}) == 5 and 0 not in seven and M32 not in seven:
                break
        special = seven
        f1 = sc2_hash(fillers, s1) & m32
        fillers = fillers[~np.isin(f1, np.concatenate([[B], second]))]
        f1 = sc2_hash(fillers, s1) & m32                   # no filler overflows: at most three per first bucket
        keep = np.ones(len(fillers), dtype=bool)
        seen = {}
        for i, b in enumerate(f1.tolist()):
            seen[b] = seen.get(b, 0) + 1
            keep[i] = seen[b] <= 3
        fillers = fillers[keep]
        premise = f"bucket {B} is full and four more keys name it first; they sit alone in second buckets {sorted(second.tolist())}"
    else:
        groups = []
        for a in range(want_attempt):
            g, n_cand = _sharing_both_buckets(rng, seeds[a][0], seeds[a][1], mask, 7, exclude=fillers)
            assert 700 < n_cand < 1400               # about 1000 words share both buckets
            groups.append(g)
        special = np.concatenate(groups)
        premise = " and ".join(f"seven keys share first and second bucket under seed pair {a}" for a in range(want_attempt))
    # word 0 as a miss: its first bucket under the successful seeds holds zero_fill keys
    B0 = int(sc2_hash(np.uint32(0), s1) & m32)
    fillers = fillers[(sc2_hash(fillers, s1) & m32) != B0]
    cand0 = words_at(B0, 11, s1)
    cand0 = cand0[(cand0 != 0) & (cand0 != M32) & ~np.isin(cand0, special)]
    zero_keys = cand0[rng.choice(len(cand0), size=zero_fill, replace=False)]
    keys = np.sort(np.concatenate([np.asarray(special, dtype=np.uint32), fillers, zero_keys]))
    assert 512 < len(keys) <= ENTRIES and len(np.unique(keys)) == len(keys) and 0 not in keys and M32 not in keys
    model = layout_model(keys)
    assert model["attempt"] == want_attempt and model["mask"] == mask, (name, model["attempt"])
    fill = model["fill"]
    assert fill[B0] == zero_fill, (name, fill[B0])
    if name == "full_bucket":
        assert sorted(model["second"].tolist()) == sorted(seven[3:].tolist()) and fill[B] == 3
    else:
        for a in range(want_attempt):      # the group alone defeats its seed pair: seven keys, two buckets, six places
            assert len(set((sc2_hash(groups[a], seeds[a][0]) & m32).tolist())) == 1
            assert len(set((sc2_hash(groups[a], seeds[a][1]) & m32).tolist())) == 1
    # steered misses: first bucket full, second bucket empty / partly filled / full
    full = np.nonzero(fill == 3)[0]
    assert len(full) >= 3
    misses = {"second_empty": [], "second_partial": [], "second_full": []}
    for F in full[:6].tolist():
        cand = words_at(F, 11, s1)
        cand = cand[~np.isin(cand, keys) & (cand != 0) & (cand != M32)]
        f2 = fill[(sc2_hash(cand, s2) & m32).astype(np.int64)]
        misses["second_empty"] += cand[f2 == 0][:6].tolist()
        misses["second_partial"] += cand[(f2 == 1) | (f2 == 2)][:6].tolist()
        misses["second_full"] += cand[f2 == 3][:6].tolist()
    assert all(len(v) >= 6 for v in misses.values()), {k: len(v) for k, v in misses.items()}
    misses = {k: np.array(v, dtype=np.uint32) for k, v in misses.items()}
    misses["zero_and_ones"] = np.array([0, M32], dtype=np.uint32)
    sample = _sample(rng, keys, _uneven(rng, len(keys), S * W), S, W)
    tail = _tail(rng, keys, W, 120, must=np.concatenate(list(misses.values())), noise=0.1)
    note = (f"buckets: {len(keys)} keys in 2048 buckets; {premise or 'no steered overflow'}; layout succeeds at seed pair "
            f"{want_attempt} with {len(model['second'])} keys in a second bucket; the tail holds every key, misses whose first "
            f"bucket is full and whose second is empty, partly filled and full, and the misses 0 and 0xFFFFFFFF, word 0 "
            f"naming a bucket with {zero_fill} key(s)")
    return {"keys": keys, "model": model, "misses": misses, "lines": _lines(np.concatenate([sample, tail]), L), "L": L,
            "S": S, "note": note}


def _planned(name):
    p = bucket_plan(name)
    return p["lines"], p["L"], p["S"], p["note"]


def full_bucket():
    return _planned("full_bucket")


def retry_once():
    return _planned("retry_once")


def retry_twice():
    return _planned("retry_twice")


@functools.lru_cache(maxsize=None)
def tiny_plan(n: int):
    """A table of n = 1 .. 4 keys (2, 4, 8, 8 buckets) with every key and misses of each first bucket in the tail."""
    L, S, W = 16, 4, 4
    rng = np.random.default_rng(0xD400 + n)
    keys = np.sort(_random_words(rng, n))
    model = layout_model(keys)
    nb = model["mask"] + 1
    assert nb == {1: 2, 2: 4, 3: 8, 4: 8}[n]
    miss = [0, M32]
    for b in range(nb):          # three misses per first bucket, whatever it holds
        cand = random_words_at(rng, b, nb.bit_length() - 1, model["seed1"], 8)
        cand = cand[~np.isin(cand, keys) & (cand != 0) & (cand != M32)]
        miss += cand[:3].tolist()
    miss = np.array(miss, dtype=np.uint32)
    sample = _sample(rng, keys, _uneven(rng, n, S * W), S, W)
    tail = _tail(rng, keys, W, 24, must=miss)
    note = (f"buckets: a table of {n} key(s) in {nb} buckets (fill {model['fill'].tolist()}); the tail holds every key, "
            "three misses per first bucket and the misses 0 and 0xFFFFFFFF")
    return {"keys": keys, "model": model, "misses": {"per_bucket": miss}, "lines": _lines(np.concatenate([sample, tail]), L),
            "L": L, "S": S, "note": note}


def _tiny(n):
    p = tiny_plan(n)
    return p["lines"], p["L"], p["S"], p["note"]


def tiny_table_1():
    return _tiny(1)


def tiny_table_2():
    return _tiny(2)


def tiny_table_3():
    return _tiny(3)


def tiny_table_4():
    return _tiny(4)


def evicted_zero():
    L, S, W = 64, 65, 16
    rng = np.random.default_rng(0xD5)
    keys = np.concatenate([np.zeros(1, dtype=np.uint32), _random_words(rng, 1029)])
    freq = np.ones(1030, dtype=np.int64)
    freq[1 + rng.choice(1029, size=S * W - 1030, replace=False)] += 1
    sample = _sample(rng, keys, freq, S, W)
    tail = _tail(rng, keys, W, 100, must=[0, 0, 0, M32])
    note = ("buckets: word 0 is in the sample with count 1, the smallest (count, symbol) of 1030 distinct words, and is "
            "evicted with five more; the tail holds 0 as a miss next to every word of the sample")
    return _lines(np.concatenate([sample, tail]), L), L, S, note


FAMILIES = {
    "a": [lds_chain_one_group, lds_chain_four_groups],
    "b": [global_chain_sixteen_groups, global_chain_knife_edge, smallest_table_s1, smallest_table_s2],
    "c": [distinct_1023, distinct_1024, distinct_1025, top_group_1023, top_group_1024, top_group_1025,
          tie_byte0_with_zero_and_ones, tie_byte1, tie_byte2, tie_byte3, cut_in_second_count_byte, count_2_24],
    "d": [full_bucket, retry_once, retry_twice, tiny_table_1, tiny_table_2, tiny_table_3, tiny_table_4, evicted_zero],
}
BUILDERS = {f.__name__: f for fam in FAMILIES.values() for f in fam}
FAMILY_OF = {f.__name__: k for k, fam in FAMILIES.items() for f in fam}
LARGE = ("count_2_24",)                      # not kept in memory between tests
BUCKET_PLANS = {"full_bucket": bucket_plan, "retry_once": bucket_plan, "retry_twice": bucket_plan,
                "tiny_table_1": lambda _: tiny_plan(1), "tiny_table_2": lambda _: tiny_plan(2),
                "tiny_table_3": lambda _: tiny_plan(3), "tiny_table_4": lambda _: tiny_plan(4)}


@functools.lru_cache(maxsize=None)
def _built(name):
    return BUILDERS[name]()


def build(name: str):
    """(lines, L, S, note) of a case by name; the lines are read-only and, but for the large case, built once."""
    return BUILDERS[name]() if name in LARGE else _built(name)


def names(*families):
    return [f.__name__ for k in (families or FAMILIES) for f in FAMILIES[k]]
