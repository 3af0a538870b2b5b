"""Rewrite accounting on the MI355X (csrc/mpc_rewrite.hip, include/mpc_hip_rewrite.h): the sequence of sizes per line
address -- transitions between size classes, first touches, latest and peak size and the number of observations -- for
every evaluator, through every ingestion path.  The expected table is tests/rewrite_ref.py over the sizes that a handle
or group WITHOUT the accounting returns for the same lines; every comparison is equality of whole uint64 tables.

The traces are a few thousand lines of mixed kinds (all-zero, word-same, small-integer, random), so that sizes differ
from line to line and a transition counted against the wrong predecessor shows in the matrix."""
import json
import os

import numpy as np
import pytest

from conftest import ROOT, pkg

import rewrite_ref as R

pytestmark = pytest.mark.gpu

MPC_E_INVAL = -22
KINDS = ("VPC", "BDI", "FPC", "BPC", "SC2", "CPACK", "CPACK-block", "Pattern")


@pytest.fixture(scope="module")
def mpc():
    pkg("build").build_lib()
    m = pkg()
    m.lib()
    return m


def make(mpc, configs, comp, L):
    if comp == "VPC":
        return mpc.VPC(configs.probe_config(L))
    if comp == "SC2":
        return mpc.SC2(L, 100, device=0)
    if comp == "Pattern":
        return mpc.Pattern(L)
    if comp == "CPACK-block":
        return mpc.CPACK(L, "block", block_lines=4)
    return getattr(mpc, comp)(L)


def mixed_lines(traces, L, n, seed=0):
    """n lines, each all-zero, word-same, small integers or random with equal probability."""
    rng = np.random.default_rng(1000 + L + seed)
    small = rng.integers(0, 200, (n, L // 4), dtype=np.uint32).view(np.uint8).reshape(n, L)
    kinds = np.stack([traces.zeros(n, L), traces.word_same(n, L), small, traces.random_u32(n, L, first_line=seed)])
    return np.ascontiguousarray(kinds[rng.integers(0, 4, n), np.arange(n)])


def spread_addresses(n, L, keys, seed, misaligned=True):
    """n addresses over `keys` distinct lines from a base above 2^32, and (every 7th line) an address that is no multiple of L."""
    rng = np.random.default_rng(seed)
    a = np.uint64(0x7f0000000000) + rng.integers(0, keys, n).astype(np.uint64) * np.uint64(L)
    if misaligned:
        a[::7] += rng.integers(1, L, a[::7].size).astype(np.uint64)
    return a


def plain_sizes(mpc, configs, comp, L, lines):
    ev = make(mpc, configs, comp, L)
    sizes, sel = ev.compress_lines(lines)
    stats = ev.stats_vector()
    ev.close()
    return sizes, sel, stats


def feed(ev, lines, addrs, cuts=None):
    at = 0
    for n in cuts or [len(lines)]:
        ev.compress_lines(lines[at:at + n], want_sizes=False, want_selected=False, addresses=addrs[at:at + n])
        at += n
    assert at == len(lines)


def rewrite_of(mpc, L, lines, addrs, g, capacity=8192, cuts=None, comp="BDI"):
    ev = getattr(mpc, comp)(L)
    ev.enable_rewrite_stats(g, capacity)
    feed(ev, lines, addrs, cuts)
    t = ev.rewrite_table()
    ev.close()
    return t


def refused(mpc, call, *words):
    with pytest.raises(mpc.MpcError) as e:
        call()
    assert e.value.code == MPC_E_INVAL and all(w in str(e.value) for w in words), str(e.value)


# ---- 1. every evaluator once -----------------------------------------------------------------------------------------
CASES = [(c, L, g) for c, (L, g) in zip(KINDS, [(32, 8), (64, 16), (128, 32), (64, 8), (32, 16), (128, 8), (64, 32), (128, 16)])]


@pytest.mark.parametrize("comp,L,g", CASES, ids=[f"{c}-{L}-{g}" for c, L, g in CASES])
def test_every_evaluator(mpc, configs, traces, comp, L, g):
    n = 4096
    lines = mixed_lines(traces, L, n)
    sizes, _, want_stats = plain_sizes(mpc, configs, comp, L, lines)
    assert len(set(sizes.tolist())) >= 3
    addrs = spread_addresses(n, L, 1024, seed=L)                   # about four observations per key
    ev = make(mpc, configs, comp, L)
    ev.enable_rewrite_stats(g, 2048)
    ev.enable_rewrite_stats(g, 2048)                              # idempotent
    feed(ev, lines, addrs)
    want = R.rewrite_table(addrs, sizes, L, g, 2048)
    assert int(want[2]) < int(want[0]) and int(want[3]) > 0 and int(want[5]) > 0 and int(want[6]) > 0 and int(want[11]) > int(want[10])
    R.same_table(f"{comp} L={L} g={g}", ev.rewrite_table(), want)
    assert (ev.stats_vector() == want_stats).all()
    view = ev.rewrite_stats()
    assert (view["overflow_rate"], view["image_granule_ratio"], view["peak_granule_ratio"], view["traffic_ratio"]) == R.ratios(want, L)
    G = R.classes_of(L, g)
    assert view["trans"].shape == (G + 1, G) and (view["trans"][0] == want[R.FIRST:R.FIRST + G]).all()
    assert int(view["trans"][1:].sum()) == view["rewrites"] == int(want[4]) and view["distinct_lines"] == int(want[2])
    ev.close()


def test_sizes_above_the_line_clamp(mpc, configs, traces):
    """C-Pack and BPC are uncapped: random lines cost more than 8 L bits, and such a size counts in class G."""
    L, g, n = 32, 8, 4096
    lines = mixed_lines(traces, L, n, seed=1)
    addrs = spread_addresses(n, L, 1000, seed=2)
    for comp in ("CPACK", "BPC"):
        sizes = plain_sizes(mpc, configs, comp, L, lines)[0]
        assert int(sizes.max()) > 8 * L
        want = R.rewrite_table(addrs, sizes, L, g, 1024)
        assert int(want[R.PEAK + 3]) > 0                           # peaks in the top class, G = 4
        R.same_table(comp, rewrite_of(mpc, L, lines, addrs, g, 1024, comp=comp), want)


# ---- 2. run shapes ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bdi64(mpc, traces):
    """4096 mixed lines of 64 bytes and BDI's sizes of them."""
    L, n = 64, 4096
    lines = mixed_lines(traces, L, n, seed=3)
    ev = mpc.BDI(L)
    sizes = ev.compress_lines(lines, want_selected=False)[0]
    ev.close()
    assert len(set(sizes.tolist())) >= 3
    return lines, sizes


def run_shapes(n, L):
    """name -> addresses of n lines."""
    i = np.arange(n, dtype=np.uint64)
    rng = np.random.default_rng(5)
    # runs whose lengths put their ends on both sides of a wave of 64, a workgroup of 256 and (the test library) a sub-batch
    lengths = np.array([63, 2, 64, 1, 65, 190, 256, 3, 257, 1000, 129, 511, 513], dtype=np.int64)
    straddle = np.repeat(np.arange(lengths.size, dtype=np.uint64), lengths)
    straddle = np.concatenate([straddle, np.uint64(100) + i[:n - straddle.size] // np.uint64(3)])
    return {"all distinct": i * np.uint64(L),
            "one address": np.full(n, 0x1234 * L, np.uint64),
            "twice adjacent": (i // np.uint64(2)) * np.uint64(L),
            "twice half a trace apart": (i % np.uint64(n // 2)) * np.uint64(L),
            "straddling runs": straddle * np.uint64(L),
            "interleaved": (rng.integers(0, 700, n).astype(np.uint64) * np.uint64(0x100000001)) * np.uint64(L)}


def test_run_shapes(mpc, bdi64):
    L = 64
    lines, sizes = bdi64
    n = len(lines)
    for tag, addrs in run_shapes(n, L).items():
        for g in (8, 32):
            want = R.rewrite_table(addrs, sizes, L, g, 8192)
            R.same_table(f"{tag} g={g}", rewrite_of(mpc, L, lines, addrs, g), want)
    one = R.rewrite_table(run_shapes(n, L)["one address"], sizes, L, 8, 8192)
    assert int(one[2]) == 1 and int(one[4]) == n - 1 and int(one[10]) == int(sizes[-1]) and int(one[11]) == int(sizes.max()) and int(one[R.COUNT + 12]) == 1
    distinct = R.rewrite_table(run_shapes(n, L)["all distinct"], sizes, L, 8, 8192)
    assert int(distinct[2]) == n and int(distinct[4]) == 0 and int(distinct[R.COUNT]) == n


def test_a_key_last_seen_many_calls_earlier(mpc, bdi64):
    L, g = 64, 16
    lines, sizes = bdi64
    n = len(lines)
    addrs = np.uint64(1 << 40) + np.arange(n, dtype=np.uint64) * np.uint64(L)
    addrs[n - 1] = addrs[0]                                        # seen in the first call and again in the last
    addrs[n - 700] = addrs[5]
    cuts = [100] * 40 + [96]
    ev = mpc.BDI(L)
    ev.enable_rewrite_stats(g, 8192)
    feed(ev, lines, addrs, cuts)
    want = R.rewrite_table(addrs, sizes, L, g, 8192)
    assert int(want[4]) == 2
    R.same_table("old keys", ev.rewrite_table(), want)
    ev.close()


# ---- 3. class edges --------------------------------------------------------------------------------------------------
def test_class_edges(mpc, configs, traces):
    """Sizes at 8 g c and at 8 g c + 1 lie in classes c and c + 1.  BDI's sizes are all 4 modulo 8 (a 4-bit state in front
    of whole bytes), so they cannot sit ON a multiple of 8 g: BDI lines of known size -- zero, repeated, base-delta,
    uncompressed -- give the nearest pair, 8 g c - 4 and 8 g c + 4, and FPC lines picked by their size give the exact pair.
    The same two sizes in both orders at two addresses: one grow and one shrink."""
    L, g = 64, 8
    import baseline_chosen
    pool = np.concatenate([mixed_lines(traces, L, 4096, seed=7), baseline_chosen.build("bdi_chosen_L64")[0], baseline_chosen.build("fpc_chosen_L64")[0],
                           traces.zeros(4, L), traces.word_same(4, L), traces.random_u32(4, L)])
    for comp, low_rest, high_rest in (("BDI", 8 * g - 4, 4), ("FPC", 0, 1)):
        sizes = plain_sizes(mpc, configs, comp, L, pool)[0].astype(np.int64)
        low = np.nonzero((sizes % (8 * g) == low_rest) & (sizes >= 8 * g - 4) & (sizes < 8 * L))[0]
        assert low.size, (comp, sorted(set(sizes.tolist()))[:40])
        pair = None
        for i in low:
            high = np.nonzero(sizes == sizes[i] + (high_rest if comp == "FPC" else 8))[0]
            if high.size:
                pair = (int(i), int(high[0]))
                break
        assert pair is not None, (comp, sorted(set(sizes.tolist()))[:60])
        a, b = pair
        c = R.class_of(sizes[a], L, g)
        assert R.class_of(sizes[b], L, g) == c + 1 and (comp != "FPC" or (sizes[a] == 8 * g * c and sizes[b] == 8 * g * c + 1))
        lines = pool[[a, b, b, a]]
        s = sizes[[a, b, b, a]]
        addrs = np.array([0, 0, 5 * L, 5 * L], dtype=np.uint64)    # a then b at address 0, b then a at address 5 L
        want = R.rewrite_table(addrs, s, L, g, 16)
        assert (int(want[4]), int(want[5]), int(want[6])) == (2, 1, 1)
        assert int(want[R.TRANS + (c - 1) * 32 + c]) == 1 and int(want[R.TRANS + c * 32 + c - 1]) == 1
        R.same_table(f"{comp} edge", rewrite_of(mpc, L, lines, addrs, g, 16, comp=comp), want)
        # the known sizes of zero, repeated and uncompressed lines, each in its class
        known = pool[-12:]
        ks = sizes[-12:]
        ka = np.arange(12, dtype=np.uint64) % np.uint64(3) * np.uint64(L)
        R.same_table(f"{comp} known sizes", rewrite_of(mpc, L, known, ka, g, 16, comp=comp), R.rewrite_table(ka, ks, L, g, 16))


# ---- 4. seams --------------------------------------------------------------------------------------------------------
def uneven_cuts(n, parts, seed):
    rng = np.random.default_rng(seed)
    at = np.sort(rng.choice(np.arange(1, n), parts - 1, replace=False))
    return np.diff(np.concatenate([[0], at, [n]])).tolist()


@pytest.mark.parametrize("parts", [1, 3, 37])
def test_call_seams(mpc, bdi64, parts):
    L, g = 64, 16
    lines, sizes = bdi64
    n = len(lines)
    addrs = spread_addresses(n, L, 600, seed=21)
    cuts = uneven_cuts(n, parts, parts) if parts > 1 else [n]     # in-place calls up to 512 lines, staged ones above
    ev = mpc.BDI(L)
    ev.enable_rewrite_stats(g, 1024)
    at = 0
    for c in cuts:
        feed(ev, lines[at:at + c], addrs[at:at + c])
        at += c
        R.same_table(f"after {at} lines", ev.rewrite_table(), R.rewrite_table(addrs[:at], sizes[:at], L, g, 1024))
    ev.close()


def test_stager_slots(mpc, traces):
    """1.25 Mi lines of 128 bytes in one staged call of 160 MiB: three chunks over the two staging slots, so two chunks
    are in flight on two streams.  Every chunk rewrites all 2^16 keys with other sizes: a pass that did not wait for
    the pass of the chunk before it would read latest sizes that are not there yet."""
    L, g, n = 128, 16, (1 << 20) + (1 << 18)
    pool = mixed_lines(traces, L, 4096, seed=5)
    lines = pool[np.random.default_rng(5).integers(0, len(pool), n)]
    ev = mpc.BDI(L)
    sizes = ev.compress_lines(lines, want_selected=False)[0]
    ev.close()
    addrs = (np.arange(n, dtype=np.uint64) % np.uint64(1 << 16)) * np.uint64(L)
    want = R.rewrite_table(addrs, sizes, L, g, 1 << 17)
    assert int(want[5]) > 1000 and int(want[6]) > 1000
    R.same_table("staged", rewrite_of(mpc, L, lines, addrs, g, 1 << 17), want)


def test_device_path(mpc):
    """300 000 lines of 32 bytes from mpc_synth_fill, without a sizes array (the scratch array of the accountings) and
    with the caller's."""
    import torch
    L, g, n = 32, 8, 300000
    buf = torch.empty(n * L, dtype=torch.uint8, device="cuda:0")
    mpc.synth_fill(buf.data_ptr(), n, L, "mixed")
    torch.cuda.synchronize()
    d_sizes = torch.zeros(n, dtype=torch.int16, device="cuda:0")
    plain = mpc.BDI(L)
    plain.compress_device(buf.data_ptr(), n, d_sizes.data_ptr())
    plain.sync()
    plain.close()
    sizes = d_sizes.cpu().numpy().view(np.uint16)
    assert len(set(sizes[:100000].tolist())) >= 3
    addrs = spread_addresses(n, L, 1 << 15, seed=8)
    d_addrs = torch.from_numpy(addrs.view(np.int64)).to("cuda:0")
    want = R.rewrite_table(addrs, sizes, L, g, 1 << 16)
    ev = mpc.BDI(L)
    ev.enable_rewrite_stats(g, 1 << 16)
    ev.compress_device(buf.data_ptr(), n, addresses=d_addrs.data_ptr())
    R.same_table("the scratch array", ev.rewrite_table(), want)
    ev.reset()
    out = torch.zeros(n, dtype=torch.int16, device="cuda:0")
    half = n // 2                                                  # two calls on two streams of the caller's: the passes are chained
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    ev.compress_device(buf.data_ptr(), half, out.data_ptr(), stream=s1.cuda_stream, addresses=d_addrs.data_ptr())
    ev.compress_device(buf.data_ptr() + half * L, n - half, out.data_ptr() + 2 * half, stream=s2.cuda_stream, addresses=d_addrs.data_ptr() + 8 * half)
    R.same_table("the caller's sizes array", ev.rewrite_table(), want)
    assert (out.cpu().numpy().view(np.uint16) == sizes).all()
    refused(mpc, lambda: ev.compress_device(buf.data_ptr(), 100), "every line needs an address")
    ev.close()


# ---- 5. the test library: sub-batch seams, probing, the capacity (a process of its own per setting) ------------------------
CHILD = r"""
import os
sys.path.insert(0, os.path.join(%(root)r, "tests"))
import rewrite_ref as R
L, g = 64, 16
rng = np.random.default_rng(11)
def mixed(n):
    small = rng.integers(0, 200, (n, L // 4), dtype=np.uint32).view(np.uint8).reshape(n, L)
    kinds = np.stack([T.zeros(n, L), T.word_same(n, L), small, T.random_u32(n, L)])
    return np.ascontiguousarray(kinds[rng.integers(0, 4, n), np.arange(n)])
lines = mixed(%(n)d)
n = len(lines)
plain = mpc.BDI(L); sizes = plain.compress_lines(lines, want_selected=False)[0]; plain.close()
def table(addrs, capacity, cuts=None, m=None):
    m = m or len(addrs)
    ev = mpc.BDI(L)
    ev.enable_rewrite_stats(g, capacity)
    at = 0
    for c in cuts or [m]:
        ev.compress_lines(lines[at:at + c], want_sizes=False, want_selected=False, addresses=addrs[at:at + c])
        at += c
    got = ev.rewrite_table()
    ev.close()
    return got
checked = 0
"""

BATCHES = CHILD + r"""
i = np.arange(n, dtype=np.uint64)
lengths = np.array([63, 2, 64, 1, 65, 190, 256, 3, 257], dtype=np.int64)
straddle = np.repeat(np.arange(lengths.size, dtype=np.uint64), lengths)
straddle = np.concatenate([straddle, np.uint64(100) + i // np.uint64(3)])[:n]
shapes = {"all distinct": i, "one address": np.full(n, 77, np.uint64), "twice adjacent": i // np.uint64(2), "twice apart": i %% np.uint64(n // 2),
          "straddling": straddle, "interleaved": rng.integers(0, 300, n).astype(np.uint64)}
for tag, keys in shapes.items():
    addrs = keys * np.uint64(L)
    R.same_table(tag, table(addrs, 4096), R.rewrite_table(addrs, sizes, L, g, 4096)); checked += 1
addrs = shapes["interleaved"] * np.uint64(L)
R.same_table("calls", table(addrs, 4096, [100, 1, 700, n - 801]), R.rewrite_table(addrs, sizes, L, g, 4096)); checked += 1
print("ROUTES " + json.dumps({"checked": checked}))
"""

PROBING = CHILD + r"""
def run(capacity, keys, bits):
    # n lines over these keys, every key at least once, many rewrites; exactly len(keys) distinct
    addrs = np.concatenate([keys, keys[rng.integers(0, len(keys), n - len(keys))]]) * np.uint64(L)
    addrs = addrs[rng.permutation(n)]
    got = table(addrs, capacity, [n // 3, n - n // 3])
    R.same_table(f"capacity {capacity} bits {bits}", got, R.rewrite_table(addrs, sizes, L, g, capacity))
    assert int(got[2]) == len(keys)
bits = int(os.environ["MPC_TEST_REWRITE_HASH_BITS"])
overflows = 0
for capacity in (1, 2, 3, 4, 1000):
    slots = R.slots_of(capacity)
    assert slots == {1: 2, 2: 4, 3: 8, 4: 8, 1000: 2048}[capacity]
    # every key shares one first slot (bits 0) or four (bits 2): chains through most of the table that wrap; exactly `capacity` keys succeeds
    run(capacity, np.arange(1, capacity + 1, dtype=np.uint64) * np.uint64(1000003), bits); checked += 1
    # capacity + 1 distinct keys is the error: in that call, in the next call and in the get
    ev = mpc.BDI(L)
    ev.enable_rewrite_stats(g, capacity)
    addrs = (np.arange(n, dtype=np.uint64) %% np.uint64(capacity + 1)) * np.uint64(L)
    for call in (lambda: ev.compress_lines(lines, addresses=addrs), lambda: ev.compress_lines(lines[:8], addresses=addrs[:8]), ev.rewrite_table):
        try:
            call()
            raise AssertionError("no error")
        except mpc.MpcError as e:
            assert e.code == -22 and "distinct line addresses" in str(e) and str(capacity) in str(e), str(e)
    ev.close()
    overflows += 1
print("ROUTES " + json.dumps({"checked": checked, "overflows": overflows}))
"""


@pytest.mark.parametrize("batch", [1, 63, 64, 1000])
def test_sub_batch_seams(mpc, batch):
    from testlib_child import _run_with_test_library
    pkg("build").build_lib(test=True)
    n = 600 if batch == 1 else 4096                               # (a sub-batch of one line is seven launches per line)
    res = _run_with_test_library(BATCHES % {"root": ROOT, "n": n}, grid_cap=0, timeout=600, env={"MPC_TEST_REWRITE_BATCH": str(batch)})
    assert res == {"checked": 7}


@pytest.mark.parametrize("bits", [0, 2])
def test_probing_and_the_capacity(mpc, bits):
    from testlib_child import _run_with_test_library
    pkg("build").build_lib(test=True)
    res = _run_with_test_library(PROBING % {"root": ROOT, "n": 4096}, grid_cap=0, timeout=600, env={"MPC_TEST_REWRITE_HASH_BITS": str(bits)})
    assert res == {"checked": 5, "overflows": 5}


def test_wrapping_chains(mpc, bdi64):
    """Keys whose first slot is the table's last one (found through mpc_image_hash, the map's hash): their chain wraps to
    slot 0.  Exactly `capacity` keys succeeds."""
    L, g = 64, 16
    lines, sizes = bdi64
    n = len(lines)
    rng = np.random.default_rng(4)
    for capacity in (1, 2, 3, 4, 1000):
        slots = R.slots_of(capacity)
        keys, k = [], 1
        while len(keys) < capacity:
            if mpc.image_hash(k) & (slots - 1) == slots - 1:
                keys.append(k)
            k += 1
        keys = np.array(keys, dtype=np.uint64)
        addrs = np.concatenate([keys, keys[rng.integers(0, capacity, n - capacity)]]) * np.uint64(L)
        want = R.rewrite_table(addrs, sizes, L, g, capacity)
        assert int(want[2]) == capacity
        R.same_table(f"capacity {capacity}", rewrite_of(mpc, L, lines, addrs, g, capacity, cuts=[1500, n - 1500]), want)


# ---- 6. overflow on the product library ------------------------------------------------------------------------------
def test_overflow_on_the_product_library(mpc, bdi64):
    L = 64
    lines, _ = bdi64
    ev = mpc.BDI(L)
    ev.enable_rewrite_stats(16, 100)
    addrs = np.arange(101, dtype=np.uint64) * np.uint64(L)
    feed(ev, lines[:100], addrs[:100])                            # exactly the capacity
    assert int(ev.rewrite_table()[2]) == 100
    feed(ev, lines[:100], addrs[:100])                            # ... and known keys again
    refused(mpc, lambda: feed(ev, lines[100:101], addrs[100:101]), "more than 100 distinct line addresses")
    refused(mpc, lambda: feed(ev, lines[:1], addrs[:1]), "takes no more lines")
    refused(mpc, ev.rewrite_table, "more than 100 distinct line addresses")
    ev.close()


def test_overflow_far_beyond_the_table(mpc, traces):
    """2^20 distinct lines into a capacity of 2^16 (2^17 slots): the device stops probing and claiming once it has seen
    the capacity exceeded, so the call returns at once -- a probe per new line over a table that filled up would be
    2^17 loads for each of nearly 2^20 lines -- in the staged path and in the device path, where the error surfaces at
    the sync."""
    import time
    import torch
    L, n, capacity = 32, 1 << 20, 1 << 16
    lines = mixed_lines(traces, L, 4096, seed=2)[np.arange(n) % 4096]
    addrs = np.arange(n, dtype=np.uint64) * np.uint64(L)
    d_lines, d_addrs = torch.from_numpy(lines).to("cuda:0"), torch.from_numpy(addrs.view(np.int64)).to("cuda:0")
    torch.cuda.synchronize()
    ev = mpc.BDI(L)
    ev.enable_rewrite_stats(8, capacity)
    t0 = time.perf_counter()
    refused(mpc, lambda: feed(ev, lines, addrs), f"more than {capacity} distinct line addresses")
    refused(mpc, ev.rewrite_table, f"more than {capacity} distinct line addresses")
    ev.close()
    ev = mpc.BDI(L)
    ev.enable_rewrite_stats(8, capacity)
    t1 = time.perf_counter()                                       # (the enable allocates and clears the sub-batch scratch: not the work in question)
    ev.compress_device(d_lines.data_ptr(), n, addresses=d_addrs.data_ptr())       # asynchronous: the error surfaces at the sync
    refused(mpc, ev.sync, f"more than {capacity} distinct line addresses")
    refused(mpc, lambda: ev.compress_device(d_lines.data_ptr(), n, addresses=d_addrs.data_ptr()), "takes no more lines")
    t2 = time.perf_counter()
    ev.close()
    # Bounded work is tens of milliseconds for 32 MiB of lines.  Probing a full table of 2^17 slots for each of the
    # 2^20 - 2^17 lines behind it is 1.2e11 dependent loads a path, tens of seconds: 5 s lies far from both.
    print("overflow far beyond the table: staged", t1 - t0, "device", t2 - t1)
    assert t2 - t0 < 5.0


# ---- 7. address edge values ------------------------------------------------------------------------------------------
def test_address_edges(mpc, bdi64):
    L = 64
    lines, sizes = bdi64
    top = np.uint64((1 << 64) - 1)
    edge = np.array([0, top, 5 * L, (1 << 32) + 5 * L, (1 << 40) + 5 * L, 0, 1, L - 1, top - np.uint64(L), 7 * L + 1, top], dtype=np.uint64)
    addrs = np.tile(edge, 20)
    n = addrs.size
    for g in (8, 16, 32):
        want = R.rewrite_table(addrs, sizes[:n], L, g, 64)
        assert int(want[2]) == 7 and int(want[3]) == 20 * 6       # key 0 (0, 1, L - 1), the top two, 5 and its two twins above bit 32, 7
        R.same_table(f"g={g}", rewrite_of(mpc, L, lines[:n], addrs, g, 64), want)
    R.same_table("reference against the loop", R.rewrite_table(addrs, sizes[:n], L, 8, 64), R.rewrite_table_loop(addrs, sizes[:n], L, 8, 64))


# ---- 8. together with image accounting, and switched off -------------------------------------------------------------
def test_together_with_image_accounting(mpc, bdi64):
    import image_ref
    L = 64
    lines, sizes = bdi64
    addrs = spread_addresses(len(lines), L, 900, seed=31)
    ev = mpc.BDI(L)
    ev.enable_image_stats(1, 32, 0, 1024)                          # N = 1, header 0, and g = sector_bytes
    ev.enable_rewrite_stats(32, 2048)
    feed(ev, lines, addrs, [1000, 2000, 1096])
    img, rw = ev.image_table(), ev.rewrite_table()
    ev.close()
    image_ref.same_table("image", img, image_ref.image_table(addrs, sizes, 1, L, 32, 0, 1024))
    R.same_table("rewrite", rw, R.rewrite_table(addrs, sizes, L, 32, 2048))
    assert int(rw[2]) == int(img[2]) and int(rw[10]) == int(img[3]) and int(rw[8]) == int(img[5])


@pytest.mark.parametrize("comp", ["BDI", "VPC", "SC2"])
def test_switched_off_and_interplay(mpc, configs, traces, comp):
    """A handle with the accounting on returns the statistics, per-line results and the other accountings' tables of a
    handle that never heard of it."""
    import image_ref
    import pack_ref
    L, n = 64, 3000
    lines = mixed_lines(traces, L, n, seed=6)
    sizes, sel, stats = plain_sizes(mpc, configs, comp, L, lines)
    addrs = spread_addresses(n, L, 800, seed=14)
    ev = make(mpc, configs, comp, L)
    ev.enable_size_histogram()
    ev.enable_class_stats(32)
    ev.enable_pack_stats(16, 32, 0)
    ev.enable_image_stats(4, 32, 0, 1024)
    ev.compress_lines(lines, want_sizes=False, want_selected=False, addresses=addrs)
    off = (ev.size_histogram(), ev.class_table(), ev.pack_table(), ev.image_table())
    ev.close()
    ev = make(mpc, configs, comp, L)
    ev.enable_size_histogram()
    ev.enable_class_stats(32)
    ev.enable_pack_stats(16, 32, 0)
    ev.enable_image_stats(4, 32, 0, 1024)
    ev.enable_rewrite_stats(16, 1024)
    got_sizes, got_sel = ev.compress_lines(lines, addresses=addrs)
    assert (got_sizes == sizes).all() and (got_sel == sel).all() and (ev.stats_vector() == stats).all()
    on = (ev.size_histogram(), ev.class_table(), ev.pack_table(), ev.image_table())
    for a, b in zip(off, on):
        assert (np.asarray(a) == np.asarray(b)).all()
    pack_ref.same_table("pack", on[2], pack_ref.pack_table(sizes, 16, L, 32, 0))
    image_ref.same_table("image", on[3], image_ref.image_table(addrs, sizes, 4, L, 32, 0, 1024))
    R.same_table("rewrite", ev.rewrite_table(), R.rewrite_table(addrs, sizes, L, 16, 1024))
    ev.close()


def test_get_is_not_destructive_and_reset_starts_over(mpc, bdi64):
    L, g = 64, 8
    lines, sizes = bdi64
    addrs = spread_addresses(len(lines), L, 1500, seed=13)
    ev = mpc.BDI(L)
    ev.enable_rewrite_stats(g, 2048)
    feed(ev, lines[:2000], addrs[:2000])
    first = ev.rewrite_table()
    R.same_table("first get", first, R.rewrite_table(addrs[:2000], sizes[:2000], L, g, 2048))
    R.same_table("second get", ev.rewrite_table(), first)
    feed(ev, lines[2000:], addrs[2000:])
    R.same_table("lines after a get count", ev.rewrite_table(), R.rewrite_table(addrs, sizes, L, g, 2048))
    ev.reset()
    R.same_table("after reset", ev.rewrite_table(), R.rewrite_table(addrs[:0], sizes[:0], L, g, 2048))
    feed(ev, lines[1000:3000], addrs[:2000])                      # the map and the table start over
    R.same_table("after reset and lines", ev.rewrite_table(), R.rewrite_table(addrs[:2000], sizes[1000:3000], L, g, 2048))
    ev.close()


# ---- 9. groups and the .log ------------------------------------------------------------------------------------------
GROUP = ("BDI", "FPC", "BPC", "VPC", "CPACK")


def patched_log(traces, path, lines, req_types, addrs):
    """traces.write_gpgpusim_log, then the mem_addr of record i (bytes 30 .. 38 of its header) set to addrs[i]."""
    traces.write_gpgpusim_log(path, lines, req_types)
    n, L = lines.shape
    head = 1 + 17 * 7
    raw = np.fromfile(path, dtype=np.uint8)
    rec = raw[head:head + n * (62 + L)].reshape(n, 62 + L)
    rec[:, 30:38] = np.asarray(addrs, dtype="<u8").view(np.uint8).reshape(n, 8)
    raw.tofile(path)
    return path


def test_group_members(mpc, configs, traces, tmp_path):
    import torch
    L, g, n = 64, 16, 3000
    lines = mixed_lines(traces, L, n, seed=7)
    addrs = spread_addresses(n, L, 900, seed=15)
    sizes = [plain_sizes(mpc, configs, c, L, lines)[0] for c in GROUP]
    alone = []
    for c, s in zip(GROUP, sizes):
        ev = make(mpc, configs, c, L)
        ev.enable_rewrite_stats(g, 1024)
        feed(ev, lines, addrs, [1000, 2000])
        alone.append(ev.rewrite_table())
        ev.close()
        R.same_table(f"{c} alone", alone[-1], R.rewrite_table(addrs, s, L, g, 1024))
    assert len({int(t[10]) for t in alone}) >= 3                  # the members' maps differ
    members = [make(mpc, configs, c, L) for c in GROUP]
    grp = mpc.EvaluatorSet(members)
    grp.enable_rewrite_stats(g, 1024)
    grp.enable_rewrite_stats(g, 1024)
    refused(mpc, lambda: grp.enable_rewrite_stats(8, 1024), "already on")
    grp.compress_lines(lines[:400], want_sizes=False, want_selected=False, addresses=addrs[:400])       # in place
    grp.compress_lines(lines[400:1000], want_sizes=False, want_selected=False, addresses=addrs[400:1000])   # staged
    d_lines = torch.from_numpy(lines[1000:]).to("cuda:0")
    d_addrs = torch.from_numpy(addrs[1000:].view(np.int64)).to("cuda:0")
    grp.compress_device(d_lines.data_ptr(), n - 1000, addresses=d_addrs.data_ptr())
    for i, t in enumerate(alone):
        R.same_table(f"member {i}", grp.rewrite_table(i), t)
    assert grp.rewrite_stats()[1]["latest_bits"] == int(alone[1][10])
    refused(mpc, lambda: grp.compress_lines(lines[:10]), "every line needs an address")
    # the .log delivers each evaluated record's mem_addr to all members
    for m in members:
        m.reset()
    req_types = np.where(np.arange(n) % 5 == 0, 4, np.where(np.arange(n) % 11 == 0, 3, 0))      # reads, writes, and texture reads that are not evaluated
    keep = req_types != 3
    log = patched_log(traces, str(tmp_path / "g.log"), lines, req_types, addrs)
    assert grp.compress_gpgpusim_log(log)[1] == int(keep.sum())
    kept = [plain_sizes(mpc, configs, c, L, lines[keep])[0] for c in GROUP]
    for i, s in enumerate(kept):
        R.same_table(f".log member {i}", grp.rewrite_table(i), R.rewrite_table(addrs[keep], s, L, g, 1024))
    # a member fed alone: the group refuses until the members are reset
    members[2].compress_lines(lines[:5], addresses=addrs[:5])
    refused(mpc, lambda: grp.compress_lines(lines[:10], addresses=addrs[:10]), "member 2", "fed outside the group")
    for m in members:
        m.reset()
    grp.compress_lines(lines[:10], addresses=addrs[:10])
    grp.close()
    for m in members:
        m.close()
    # a handle reads the same log
    ev = mpc.FPC(L)
    ev.enable_rewrite_stats(g, 1024)
    assert ev.compress_gpgpusim_log(log)[1] == int(keep.sum())
    R.same_table(".log, a handle", ev.rewrite_table(), R.rewrite_table(addrs[keep], kept[1], L, g, 1024))
    ev.close()


# ---- 10. refusals ----------------------------------------------------------------------------------------------------
def test_refusals(mpc, traces, tmp_path):
    L = 64
    lines = mixed_lines(traces, L, 600, seed=8)
    addrs = spread_addresses(600, L, 100, seed=16)
    ev = mpc.BDI(L)
    with pytest.raises(mpc.MpcError) as e:                          # addresses on a plain handle: the text of before
        ev.compress_lines(lines, addresses=addrs)
    assert str(e.value) == "mpc error -22: image accounting is not switched on for this handle (mpc_image_stats_enable)"
    refused(mpc, ev.rewrite_table, "not switched on", "mpc_rewrite_stats_enable")
    for bad, word in (((0, 16), "granule_bytes"), ((65, 16), "granule_bytes"), ((1, 16), "size classes"), ((16, 0), "capacity_lines"),
                      ((16, (1 << 28) + 1), "capacity_lines")):
        refused(mpc, lambda: ev.enable_rewrite_stats(*bad), word)
    ev.enable_rewrite_stats(16, 256)
    refused(mpc, lambda: ev.enable_rewrite_stats(8, 256), "already on", "granule_bytes 16")
    refused(mpc, lambda: ev.enable_rewrite_stats(16, 512), "already on", "capacity_lines 256")
    refused(mpc, lambda: ev.compress_lines(lines), "rewrite accounting is on", "every line needs an address")             # staged
    refused(mpc, lambda: ev.compress_lines(lines[:10]), "every line needs an address")        # in place
    npy = traces.save_npy(str(tmp_path / "t.npy"), lines)
    refused(mpc, lambda: ev.compress_npy(npy), "every line needs an address")
    assert int(ev.rewrite_table()[0]) == 0 and int(ev.stats_vector()[0]) == 0     # nothing of the refused calls was evaluated
    ev.compress_lines(lines, addresses=addrs)
    assert int(ev.rewrite_table()[0]) == 600
    ev.close()
    fit = mpc.FitPairs(L)
    refused(mpc, lambda: fit.enable_rewrite_stats(16), "Fit")
    fit.close()


# ---- 11. the command line --------------------------------------------------------------------------------------------
def test_cli_rewrites(mpc, configs, traces, tmp_path):
    import subprocess
    pkg("build").build_all()
    bindir = os.path.join(ROOT, "bin")
    cli = os.path.join(bindir, "compressor")
    L, n = 32, 3002
    lines = mixed_lines(traces, L, n, seed=9)
    ds = tmp_path / "ds"
    ds.mkdir()
    req_types = np.where(np.arange(n) % 5 == 0, 4, np.where(np.arange(n) % 11 == 0, 3, 0))
    keep = req_types != 3
    addrs = spread_addresses(n, L, 700, seed=17)
    log = patched_log(traces, str(ds / "t.log"), lines, req_types, addrs)
    cfg_path = str(tmp_path / "probe.json")
    with open(cfg_path, "w") as f:
        json.dump(configs.probe_config(L), f)
    names = ("VPC", "BDI", "FPC")
    sizes = [plain_sizes(mpc, configs, c, L, lines[keep])[0] for c in names]

    def run(args, out, program=cli):
        out.mkdir()
        r = subprocess.run([program, *args, "-o", str(out)], cwd=bindir, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        return r.stdout

    # one algorithm: --rewrites alone changes not one byte of the other outputs
    base = ["-a", "BDI", "-i", log]
    plain_stdout = run(base, tmp_path / "one_plain")
    assert run(base + ["--rewrites", "8", "--rewrite-capacity", "1024"], tmp_path / "one") == plain_stdout
    for name in os.listdir(tmp_path / "one_plain"):
        assert (tmp_path / "one" / name).read_bytes() == (tmp_path / "one_plain" / name).read_bytes(), name
    assert sorted(set(os.listdir(tmp_path / "one")) - set(os.listdir(tmp_path / "one_plain"))) == ["BDI_results_rewrites.csv"]
    want = R.rewrite_table(addrs[keep], sizes[1], L, 8, 1024)
    assert len(np.nonzero(want[R.TRANS:])[0]) >= 6 and int(want[2]) < int(want[0])
    assert (tmp_path / "one" / "BDI_results_rewrites.csv").read_text() == R.CSV_HEADER + R.csv_row("ds_t", want, L)
    # a list, next to the other accountings: every member gets its own file; the default capacity
    base = ["-a", ",".join(names), "-c", cfg_path, "-i", log, "--size-histogram", "--pack", "4", "--image", "4", "--by", "rw"]
    plain_stdout = run(base, tmp_path / "list_plain")
    assert run(base + ["--rewrites", "8"], tmp_path / "list") == plain_stdout
    for name in os.listdir(tmp_path / "list_plain"):
        assert (tmp_path / "list" / name).read_bytes() == (tmp_path / "list_plain" / name).read_bytes(), name
    stems = ["probe", "BDI", "FPC"]
    assert sorted(set(os.listdir(tmp_path / "list")) - set(os.listdir(tmp_path / "list_plain"))) == sorted(f"{s}_results_rewrites.csv" for s in stems)
    for stem, s in zip(stems, sizes):
        table = R.rewrite_table(addrs[keep], s, L, 8, 1 << 24)
        assert (tmp_path / "list" / f"{stem}_results_rewrites.csv").read_text() == R.CSV_HEADER + R.csv_row("ds_t", table, L), stem
    # the refusals: an input that is no .log, --snapshot, a bad value; one message, exit status 1, nothing written
    npy = traces.save_npy(str(ds / "t.npy"), lines)
    none = tmp_path / "none"
    none.mkdir()
    for args in (["-i", npy, "--rewrites", "8"], ["-i", log, "--rewrites", "8", "--snapshot", "64"], ["-i", log, "--rewrites", "64"], ["-i", log, "--rewrites", "x"]):
        r = subprocess.run([cli, "-a", "BDI", *args, "-o", str(none)], cwd=bindir, capture_output=True, text=True, timeout=600)
        assert r.returncode == 1 and len(r.stdout.strip().splitlines()) == 1 and "--rewrites" in r.stdout, (args, r.stdout, r.stderr)
    assert os.listdir(none) == []


def test_bin_run_passes_the_option_through(mpc, traces, tmp_path):
    """bin/run <algorithm> <dataset dir> <output dir> --rewrites 8: every ./compressor run gets the option."""
    import subprocess
    pkg("build").build_all()
    bindir = os.path.join(ROOT, "bin")
    L, n = 32, 1000
    lines = mixed_lines(traces, L, n, seed=10)
    addrs = spread_addresses(n, L, 200, seed=18)
    ds = tmp_path / "ds"
    (ds / "bench").mkdir(parents=True)
    patched_log(traces, str(ds / "bench" / "t.log"), lines, np.zeros(n, np.uint32), addrs)
    out = tmp_path / "out"
    out.mkdir()
    r = subprocess.run([os.path.join(bindir, "run"), "BDI", str(ds), str(out), "--rewrites", "8", "--rewrite-capacity", "512"], cwd=bindir,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout, r.stderr)
    ev = mpc.BDI(L)
    sizes = ev.compress_lines(lines, want_selected=False)[0]
    ev.close()
    want = R.rewrite_table(addrs, sizes, L, 8, 512)
    assert (out / "BDI_results_rewrites.csv").read_text() == R.CSV_HEADER + R.csv_row("bench_t", want, L), (r.stdout, r.stderr)
