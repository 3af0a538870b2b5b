"""The chosen-word cases of tests/sc2_keys.py without a device: the inverse hash, the restated seed sequence and
bucket layout against the library's own `mpcsc2::layout` (tests/native/sc2_layout_probe.cpp, a stand-alone program
built with the host sanitizers), every builder's premise, and that the cases discriminate: named wrong variants of
sc2_ref.SC2Ref each differ from it on at least one case of the family they target."""
import copy
import os
import subprocess

import numpy as np
import pytest

import sc2_keys
import sc2_ref
from test_native_cpu import CSRC, NATIVE, SAN, _build


# ---- the hash and the seeds ------------------------------------------------------------------------------------------
def test_inverse_hash_round_trips():
    x = np.concatenate([np.array([0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF], dtype=np.uint32),
                        np.random.default_rng(1).integers(0, 1 << 32, size=200000, dtype=np.uint64).astype(np.uint32)])
    for seed in (0, sc2_keys.GLOBAL_SEED, 0xFFFFFFFF, *sc2_keys.layout_seeds(1)[0]):
        assert (sc2_keys.sc2_hash_inv(sc2_keys.sc2_hash(x, seed), seed) == x).all()
        assert (sc2_keys.sc2_hash(sc2_keys.sc2_hash_inv(x, seed), seed) == x).all()
    # the hash written out for one word, so that hash and inverse cannot be wrong together
    k, seed = 0x12345678, 0x5C2
    h = ((k ^ seed) * 0x9E3779B1) & 0xFFFFFFFF
    h ^= h >> 15
    h = (h * 0x2C1B3C6D) & 0xFFFFFFFF
    h ^= h >> 12
    assert int(sc2_keys.sc2_hash(np.uint32(k), seed)) == h


def test_slot_populations():
    at = sc2_keys.words_at(8191, 13, 0)
    assert len(at) == 1 << 19 == len(np.unique(at)) and (sc2_keys.sc2_hash(at, 0) & np.uint32(8191) == 8191).all()
    at = sc2_keys.words_at(8190, 13, sc2_keys.GLOBAL_SEED)
    assert len(np.unique(at)) == 1 << 19 and (sc2_keys.sc2_hash(at, sc2_keys.GLOBAL_SEED) & np.uint32(8191) == 8190).all()
    assert [sc2_keys.global_mask(L, S) for L, S in ((4, 1), (4, 2), (64, 1024), (64, 4096), (36, 500))] == \
        [1, 3, (1 << 15) - 1, (1 << 17) - 1, 16383]


# ---- layout_seeds / layout_model against mpcsc2::layout ------------------------------------------------------------------
@pytest.fixture(scope="module")
def layout_probe(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("sc2_layout"))
    return _build(tmp, "sc2_layout_probe", ["g++", "-std=c++17", *SAN, "-Wall", "-Werror", "-I", CSRC,
                                            os.path.join(NATIVE, "sc2_layout_probe.cpp")])


def _run_probe(exe, tmp_path, keys, lens, queries):
    path = str(tmp_path / "keys.txt")
    with open(path, "w") as f:
        f.write(f"{len(keys)} {len(queries)}\n")
        f.writelines(f"{int(k)} {int(l)}\n" for k, l in zip(keys, lens))
        f.writelines(f"{int(q)}\n" for q in queries)
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-500:] + r.stderr[-3000:]
    out = r.stdout.strip().split("\n")
    mask, s1, s2 = (int(v) for v in out[0].split()[1:])
    image = np.array(out[1].split()[1:], dtype=np.uint64).astype(np.uint32).reshape(-1, 4)
    answers = [ln.split()[1:] for ln in out[2:]]
    assert [int(a[0]) for a in answers] == [int(q) for q in queries]
    return mask, s1, s2, image, [None if a[1] == "miss" else int(a[1]) for a in answers]


@pytest.mark.parametrize("name", list(sc2_keys.BUCKET_PLANS))
def test_layout_model_is_the_library_layout(layout_probe, tmp_path, name):
    plan = sc2_keys.BUCKET_PLANS[name](name)
    ref = sc2_ref.SC2Ref(plan["L"], plan["S"])
    ref.feed(plan["lines"])
    keys, lens = ref.table_syms, ref.table_lens
    assert keys.tolist() == plan["keys"].tolist()                   # <= 1024 distinct words: the table is the sample
    model = sc2_keys.layout_model(keys, lens)
    misses = np.concatenate(list(plan["misses"].values()))
    assert not np.isin(misses, keys).any()
    mask, s1, s2, image, answers = _run_probe(layout_probe, tmp_path, keys, lens, np.concatenate([keys, misses]))
    assert (mask, s1, s2) == (model["mask"], model["seed1"], model["seed2"])
    assert (s1, s2) == sc2_keys.layout_seeds(model["attempt"] + 1)[-1] and model["attempt"] == plan["model"]["attempt"]
    assert image.shape == model["image"].shape and (image == model["image"]).all()
    assert answers[:len(keys)] == lens.tolist()                    # every key is found with its length
    assert answers[len(keys):] == [None] * len(misses)             # every steered miss misses
    # the image holds what the note says: bucket fills, the keys in a second bucket
    fill = image[:, 3] >> 30
    assert (fill == model["fill"]).all() and int(fill.sum()) == len(keys)
    b1 = sc2_keys.sc2_hash(keys, s1) & np.uint32(mask)
    placed_first = np.array([k in image[b, :fill[b]].tolist() for k, b in zip(keys.tolist(), b1.tolist())])
    assert sorted(keys[~placed_first].tolist()) == sorted(model["second"].tolist())


def test_bucket_cases_reach_their_paths():
    for name, attempt, zero_fill in (("full_bucket", 0, 1), ("retry_once", 1, 2), ("retry_twice", 2, 0)):
        plan = sc2_keys.bucket_plan(name)
        m = plan["model"]
        mask = np.uint32(m["mask"])
        assert m["attempt"] == attempt and m["mask"] == 2047
        assert m["fill"][int(sc2_keys.sc2_hash(np.uint32(0), m["seed1"]) & mask)] == zero_fill
        first = m["fill"][(sc2_keys.sc2_hash(plan["misses"]["second_empty"], m["seed1"]) & mask).astype(int)]
        assert (first == 3).all()
        for kind, want in (("second_empty", {0}), ("second_partial", {1, 2}), ("second_full", {3})):
            w = plan["misses"][kind]
            assert (m["fill"][(sc2_keys.sc2_hash(w, m["seed1"]) & mask).astype(int)] == 3).all()
            assert set(m["fill"][(sc2_keys.sc2_hash(w, m["seed2"]) & mask).astype(int)].tolist()) <= want
        tail = plan["lines"][plan["S"]:].view("<u4")
        for w in np.concatenate([plan["keys"], *plan["misses"].values()]).tolist():
            assert w in tail
    assert len(sc2_keys.bucket_plan("full_bucket")["model"]["second"]) == 4
    assert [sc2_keys.tiny_plan(n)["model"]["mask"] + 1 for n in (1, 2, 3, 4)] == [2, 4, 8, 8]


def test_evicted_zero_misses_in_the_library_image(layout_probe, tmp_path):
    lines, L, S, _ = sc2_keys.build("evicted_zero")
    ref = sc2_ref.SC2Ref(L, S)
    ref.feed(lines)
    assert 0 in lines[:S].view("<u4") and 0 in lines[S:].view("<u4") and 0 not in ref.table_syms and len(ref.table_syms) == 1024
    _, _, _, _, answers = _run_probe(layout_probe, tmp_path, ref.table_syms, ref.table_lens, [0, 0xFFFFFFFF, int(ref.table_syms[0])])
    assert answers == [None, None, int(ref.table_lens[0])]


# ---- premises: what each case holds, counted here from its lines -----------------------------------------------------------
SMALL = [n for n in sc2_keys.names() if n not in sc2_keys.LARGE]


@pytest.fixture(scope="module")
def refs():
    """name -> (SC2Ref after the whole case, sizes, selected)."""
    out = {}
    for name in SMALL:
        lines, L, S, _ = sc2_keys.build(name)
        ref = sc2_ref.SC2Ref(L, S)
        out[name] = (ref, *ref.feed(lines))
    return out


def test_reference_runs_every_case(refs):
    for name in SMALL:
        lines, L, S, note = sc2_keys.build(name)
        ref, sizes, sel = refs[name]
        W = L // 4
        assert lines.dtype == np.uint8 and lines.shape[1] == L and 0 < len(lines) - S <= 300 and note, name
        assert 2 * S * W <= sc2_keys.global_mask(L, S) + 1                       # the load of the counting table: <= 1/2
        assert (sizes[:S] == 33 * W).all() and (sel[:S] == 0).all() and (sel[S:] == 1).all(), name
        tail = lines[S:].view("<u4")
        assert ref.found > 0 and ref.found < tail.size, name                     # hits and misses in every tail
        assert 0 in tail and 0xFFFFFFFF in tail, name


def _slot_groups(words, home):
    """The distinct words of `words` that share the most common home slot, ascending."""
    u = np.unique(words)
    slots, n = np.unique(home(u), return_counts=True)
    return u[home(u) == slots[np.argmax(n)]], int(n.max())


def test_chain_premises(refs):
    lds = lambda w: sc2_keys.sc2_hash(w, 0) & np.uint32(sc2_keys.LDS_SLOTS - 1)
    lines, L, S, _ = sc2_keys.build("lds_chain_one_group")
    words = lines[:S].view("<u4").reshape(-1)
    chain, n = _slot_groups(words, lds)
    assert len(words) == 4096 and n == 1000 == len(np.unique(words)) and lds(chain[:1])[0] == 8191
    assert len(set(np.unique(words, return_counts=True)[1].tolist())) > 5      # uneven multiplicities
    lines, L, S, _ = sc2_keys.build("lds_chain_four_groups")
    words = lines[:S].view("<u4").reshape(4, 4096)
    for g, slot in enumerate((8191, 8190, 0, 4095)):
        u = np.unique(words[g])
        assert int((lds(u) == slot).sum()) == 256 and len(u) == 384
        assert len(np.intersect1d(u, np.unique(words[(g + 1) % 4]))) >= 128     # words that recur in the next workgroup
    assert len(np.unique(words)) == 1024 == len(refs["lds_chain_four_groups"][0].table_syms)
    for name, groups, n_chain in (("global_chain_sixteen_groups", 16, 1000), ("global_chain_knife_edge", 4, 2048)):
        lines, L, S, _ = sc2_keys.build(name)
        mask = sc2_keys.global_mask(L, S)
        words = lines[:S].view("<u4").reshape(-1)
        assert -(-len(words) // 4096) == groups
        home = sc2_keys.sc2_hash(np.unique(words), sc2_keys.GLOBAL_SEED) & np.uint32(mask)
        assert (home == mask).all() and len(home) == n_chain
    words = sc2_keys.build("global_chain_sixteen_groups")[0][:4096].view("<u4").reshape(16, 4096)
    assert all(len(np.unique(words[g])) == 1000 for g in range(16))              # every word in every workgroup
    lines, L, S, _ = sc2_keys.build("global_chain_knife_edge")
    u, c = sc2_keys.warmup_counts(lines, S)
    assert (c[0:1024:2] == 8).all() and (c[1:1024:2] == 7).all() and (c[1024::2] == 7).all() and (c[1025::2] == 8).all()
    assert refs["global_chain_knife_edge"][0].table_syms.tolist() == u[c == 8].tolist() and int((c == 8).sum()) == 1024
    for S in (1, 2):
        lines, L, S_, _ = sc2_keys.build(f"smallest_table_s{S}")
        assert (L, S_) == (sc2_keys.MIN_LINE, S) and len(np.unique(lines[:S].view("<u4"))) == S


def test_selection_premises(refs):
    for n in (1023, 1024, 1025):
        lines, L, S, _ = sc2_keys.build(f"distinct_{n}")
        assert len(sc2_keys.warmup_counts(lines, S)[0]) == n and len(refs[f"distinct_{n}"][0].table_syms) == min(n, 1024)
        lines, L, S, _ = sc2_keys.build(f"top_group_{n}")
        u, c = sc2_keys.warmup_counts(lines, S)
        assert int((c == 2).sum()) == n and int((c == 1).sum()) == len(u) - n > 400
    for p, name in enumerate(("tie_byte0_with_zero_and_ones", "tie_byte1", "tie_byte2", "tie_byte3")):
        lines, L, S, _ = sc2_keys.build(name)
        u, c = sc2_keys.warmup_counts(lines, S)
        tied = u[c == 1]
        kept = np.intersect1d(tied, refs[name][0].table_syms)
        n_fill = 668 if p == 3 else 667
        assert len(tied) == 512 and int((c >= 2).sum()) == n_fill and len(kept) == 1024 - n_fill
        lost = np.setdiff1d(tied, kept)
        assert lost.max() < kept.min()
        assert int(lost.max() ^ kept.min()) >> (8 * p) != 0 and (p == 3 or int(lost.max() ^ kept.min()) >> (8 * (p + 1)) == 0)
        if p in (0, 3):
            assert lost.min() == 0 and kept.max() == 0xFFFFFFFF
    lines, L, S, _ = sc2_keys.build("cut_in_second_count_byte")
    u, c = sc2_keys.warmup_counts(lines, S)
    assert L == 256 and (c >= 256).all() and len(u) == 1100
    kept = np.isin(u, refs["cut_in_second_count_byte"][0].table_syms)
    assert kept[c >= 512].all() and int(kept[c < 512].sum()) == 424 and c[~kept].max() == c[kept & (c < 512)].min()


# ---- the cases discriminate ----------------------------------------------------------------------------------------------
class Variant(sc2_ref.SC2Ref):
    """SC2Ref with one named mistake.  `chain`: the words of the longest probe chain, ascending, and how often each
    occurs among the words that are counted through that chain."""

    def __init__(self, base, kind, chain=None):
        self.__dict__.update(copy.deepcopy(base.__dict__))
        self.kind, self.chain = kind, chain

    def _build(self):
        counts = dict(self.counts)
        if self.kind == "counts_mod_2_24":
            counts = {s: c % (1 << 24) for s, c in counts.items() if c % (1 << 24)}
        elif self.kind == "chain_last_dropped":
            (w, c) = self.chain[-1]
            counts[w] -= c
        elif self.kind == "chain_first_into_neighbour":
            (w, c), (n, _) = self.chain[0], self.chain[1]
            counts[w] -= c
            counts[n] += c
        counts = {s: c for s, c in counts.items() if c > 0}
        cut = {"cut_at_1023": 1023, "cut_at_1025": 1025}.get(self.kind, 1024)
        down = -1 if self.kind == "ties_descending" else 1
        order = sorted(counts, key=lambda s: (counts[s], down * s))
        syms = np.array(sorted(order[max(0, len(order) - cut):]), dtype=np.uint32)
        sc2_ref.ENTRIES, saved = max(cut, 1024), sc2_ref.ENTRIES
        try:
            lens = sc2_ref.code_lengths(syms, [counts[int(s)] for s in syms])
        finally:
            sc2_ref.ENTRIES = saved
        self.table_syms, self.table_lens = syms, np.array(lens, dtype=np.uint16)
        self.built = True

    def feed(self, lines):
        sizes, sel = super().feed(lines)
        if self.kind == "zero_miss_as_first_key" and self.built and len(self.table_syms) and 0 not in self.table_syms:
            zeros = (np.ascontiguousarray(lines).view("<u4").reshape(len(lines), -1) == 0).sum(axis=1) * (sel == 1)
            sizes = (sizes.astype(np.int64) + zeros * (int(self.table_lens[0]) - 33)).astype(np.uint16)
            self.comp += int(zeros.sum()) * (int(self.table_lens[0]) - 33)
            self.found += int(zeros.sum())
        return sizes, sel


def _outcome(ref, sizes):
    return (ref.table_syms.tolist(), ref.table_lens.tolist(), sizes.tolist(), ref.stats_vector().tolist())


def _chain(lines, L, S, family):
    """The longest chain of the case: in workgroup 0's LDS table (family a) or in the global table (family b)."""
    words = lines[:S].view("<u4").reshape(-1)
    if family == "a":
        words = words[:sc2_keys.GROUP_WORDS]
        home = lambda w: sc2_keys.sc2_hash(w, 0) & np.uint32(sc2_keys.LDS_SLOTS - 1)
    else:
        home = lambda w: sc2_keys.sc2_hash(w, sc2_keys.GLOBAL_SEED) & np.uint32(sc2_keys.global_mask(L, S))
    chain, _ = _slot_groups(words, home)
    u, c = np.unique(words, return_counts=True)
    return [(int(w), int(c[np.searchsorted(u, w)])) for w in chain]


def _rejected_by(name, kinds, large=False):
    """Which of the wrong variants `kinds` differ from SC2Ref on the case."""
    lines, L, S, _ = sc2_keys.build(name)
    base = sc2_ref.SC2Ref(L, S)
    base.feed(lines[:S])
    right = Variant(base, "none")
    want = _outcome(right, right.feed(lines[S:])[0])
    chain = _chain(lines, L, S, sc2_keys.FAMILY_OF[name]) if sc2_keys.FAMILY_OF[name] in "ab" else None
    out = set()
    for kind in kinds:
        if kind.startswith("chain") and len(chain) < 2:
            continue
        v = Variant(base, kind, chain)
        if _outcome(v, v.feed(lines[S:])[0]) != want:
            out.add(kind)
    return out, want, right


TARGETS = {
    "a": ["chain_last_dropped", "chain_first_into_neighbour"],
    "b": ["chain_last_dropped", "chain_first_into_neighbour", "cut_at_1023", "cut_at_1025"],
    "c": ["ties_descending", "cut_at_1023", "cut_at_1025", "counts_mod_2_24"],
    "d": ["zero_miss_as_first_key", "cut_at_1023", "cut_at_1025"],
}


@pytest.mark.parametrize("family", list(TARGETS))
def test_wrong_variants_are_rejected(refs, family):
    rejected = {}
    for name in sc2_keys.names(family):
        if name in sc2_keys.LARGE:
            continue
        rejected[name], want, right = _rejected_by(name, TARGETS[family])
        assert want == _outcome(refs[name][0], refs[name][1][sc2_keys.build(name)[2]:]), name   # the unchanged Variant is SC2Ref
    for name, kinds in rejected.items():
        print(f"{name}: rejects {sorted(kinds)}")
    for kind in TARGETS[family]:
        if kind != "counts_mod_2_24":                      # (only the large case can: test_count_2_24_case)
            assert any(kind in r for r in rejected.values()), (family, kind)
    # what particular cases are there for
    if family == "a":
        assert all(len(r) == 2 for r in rejected.values()), rejected
    if family == "b":
        assert rejected["global_chain_knife_edge"] == set(TARGETS["b"])
        assert rejected["global_chain_sixteen_groups"] >= {"chain_last_dropped", "chain_first_into_neighbour"}
        assert "chain_last_dropped" in rejected["smallest_table_s2"]
    if family == "c":
        for name in ("tie_byte0_with_zero_and_ones", "tie_byte1", "tie_byte2", "tie_byte3", "top_group_1023", "top_group_1025",
                     "distinct_1025", "cut_in_second_count_byte"):
            assert rejected[name] >= {"ties_descending", "cut_at_1023", "cut_at_1025"}, (name, rejected[name])
        assert rejected["top_group_1024"] >= {"cut_at_1023", "cut_at_1025"} and "cut_at_1023" in rejected["distinct_1024"]
    if family == "d":
        assert all("zero_miss_as_first_key" in r for r in rejected.values()), rejected
        assert rejected["evicted_zero"] == set(TARGETS["d"])


def test_count_2_24_case():
    """The one large case (about 128 MiB): its premise, SC2Ref on it, and that only exact 32-bit counts pass."""
    lines, L, S, note = sc2_keys.build("count_2_24")
    assert L == 256 and 2 * S * 64 <= sc2_keys.global_mask(L, S) + 1 == 1 << 27 and len(lines) - S <= 300
    u, c = sc2_keys.warmup_counts(lines, S)
    assert sorted(c.tolist())[-2:] == [(1 << 24) - 1, 1 << 24] and len(u) == 1502 and sorted(c.tolist())[-3] == 3
    rejected, want, right = _rejected_by("count_2_24", ["counts_mod_2_24", "ties_descending", "cut_at_1023", "cut_at_1025"])
    assert rejected == {"counts_mod_2_24", "ties_descending", "cut_at_1023", "cut_at_1025"}
    heavy = u[c >= (1 << 24) - 1]
    assert np.isin(heavy, right.table_syms).all() and len(right.table_syms) == 1024
    assert sorted(right.table_lens[np.isin(right.table_syms, heavy)].tolist()) == [1, 2]


# ---- the cases that joined the reference fixture ---------------------------------------------------------------------------
def test_fixture_cases_are_the_builders_lines():
    keyed = [c for c in sc2_ref.CASES if c["kind"] == "keys"]
    assert {c["builder"] for c in keyed} == {"distinct_1024", "distinct_1025", "top_group_1024", "tie_byte0_with_zero_and_ones",
                                             "evicted_zero", "retry_once"}
    for c in keyed:
        lines, L, S, _ = sc2_keys.build(c["builder"])
        assert (c["L"], c["S"], c["post"]) == (L, S, len(lines) - S) and c["post"] <= 300
        assert (sc2_ref.case_input(c) == lines).all()
