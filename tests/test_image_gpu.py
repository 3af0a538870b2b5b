"""Image accounting on the MI355X (csrc/mpc_image.hip, include/mpc_hip_image.h): the latest size per line address and
the sectors that address-aligned blocks of that image occupy, for every evaluator, through every ingestion path.  The
expected table is tests/image_ref.py (numpy over addresses and per-line sizes) over the sizes that a handle or group
WITHOUT image accounting returns for the same lines; every comparison is equality of uint64 arrays.

The traces are a few thousand lines of mixed kinds (all-zero, word-same, small-integer, random), so that sizes differ
from line to line and a wrong winner at an address shows in the sum of the latest sizes."""
import json
import os

import numpy as np
import pytest

from conftest import ROOT, pkg

import image_ref as R

pytestmark = pytest.mark.gpu

MPC_E_INVAL = -22
ALL_N = (1, 4, 128, 1000)
KINDS = ("VPC", "BDI", "FPC", "BPC", "SC2", "CPACK", "Pattern")


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
    return getattr(mpc, comp)(L)


def mixed_lines(traces, L, n, seed=0):
    """n lines, each all-zero, word-same, small integers or random with equal probability."""
    rng = np.random.default_rng(1000 + L + seed)
    small = rng.integers(0, 200, (n, L // 4), dtype=np.uint32).view(np.uint8).reshape(n, L)
    kinds = np.stack([traces.zeros(n, L), traces.word_same(n, L), small, traces.random_u32(n, L, first_line=seed)])
    return np.ascontiguousarray(kinds[rng.integers(0, 4, n), np.arange(n)])


def sector_for(N, L):
    """32-byte sectors where a block then has at most 1024 of them, else the smallest power of two that keeps it so."""
    sb = 32
    while N * L > 1024 * sb:
        sb *= 2
    return sb


def spread_addresses(n, L, keys, seed, misaligned=True):
    """n addresses over `keys` distinct lines from a base above 2^32: repeats, partially touched blocks, and (every 7th
    line) an address that is no multiple of L."""
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


def image_of(mpc, L, lines, addrs, N, sb=32, hb=0, capacity=8192, cuts=None, comp="BDI"):
    ev = getattr(mpc, comp)(L)
    ev.enable_image_stats(N, sb, hb, capacity)
    feed(ev, lines, addrs, cuts)
    t = ev.image_table()
    ev.close()
    return t


def refused(mpc, call, *words):
    with pytest.raises(mpc.MpcError) as e:
        call()
    assert e.value.code == MPC_E_INVAL and all(w in str(e.value) for w in words), str(e.value)


# ---- 1. every evaluator kind -----------------------------------------------------------------------------------------
CASES = [(c, L) for c in KINDS for L in (32, 64, 128)]


@pytest.mark.parametrize("comp,L", CASES, ids=[f"{c}-{L}" for c, L in CASES])
def test_every_evaluator(mpc, configs, traces, comp, L):
    n = 3000
    lines = mixed_lines(traces, L, n)
    sizes, _, want_stats = plain_sizes(mpc, configs, comp, L, lines)
    assert len(set(sizes.tolist())) >= 3
    addrs = spread_addresses(n, L, 2500, seed=L)
    for N in ALL_N:
        sb = sector_for(N, L)
        ev = make(mpc, configs, comp, L)
        ev.enable_image_stats(N, sb, 0, 4096)
        ev.enable_image_stats(N, sb, 0, 4096)      # idempotent
        feed(ev, lines, addrs)
        want = R.image_table(addrs, sizes, N, L, sb, 0, 4096)
        assert int(want[2]) < int(want[0]) and int(want[7]) > 0 and int(want[3]) != int(want[1])
        R.same_table(f"{comp} L={L} N={N}", ev.image_table(), want)
        assert (ev.stats_vector() == want_stats).all()
        view = ev.image_stats()
        assert (view["traffic_ratio"], view["image_ratio"], view["image_sector_ratio"]) == R.ratios(want, L)
        assert (view["histogram"] == want[16:16 + view["block_sectors"]]).all() and view["distinct_lines"] == int(want[2])
        ev.close()


# ---- 2. last writer wins ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bdi64(mpc, traces):
    """4096 mixed lines of 64 bytes and BDI's sizes of them."""
    L, n = 64, 4096
    lines = mixed_lines(traces, L, n, seed=3)
    lines[-2:] = traces.random_u32(2, L)
    lines[-1] = 0                                                 # the last two lines differ in size
    ev = mpc.BDI(L)
    sizes = ev.compress_lines(lines, want_selected=False)[0]
    ev.close()
    assert len(set(sizes.tolist())) >= 3 and sizes[-1] != sizes[-2]
    return lines, sizes


def repeated_addresses(n, L, seed):
    """Each address 2 .. 70 times, in runs."""
    rng = np.random.default_rng(seed)
    reps = rng.integers(2, 71, n)
    keys = np.repeat(np.arange(n, dtype=np.uint64), reps)[:n]
    return keys * np.uint64(L)


def test_last_writer_wins(mpc, bdi64):
    L = 64
    lines, sizes = bdi64
    n = len(lines)
    one = np.full(n, 0x1234 * L, np.uint64)                       # 64 lanes of every wave on one slot
    runs = repeated_addresses(n, L, 1)
    interleaved = runs[np.random.default_rng(2).permutation(n)]
    descending = (np.arange(n, dtype=np.uint64)[::-1] // np.uint64(3)) * np.uint64(L)
    for tag, addrs in (("one address", one), ("runs", runs), ("interleaved", interleaved), ("descending", descending)):
        for N in (1, 4, 128):
            want = R.image_table(addrs, sizes, N, L, 32, 0, 8192)
            R.same_table(f"{tag} N={N}", image_of(mpc, L, lines, addrs, N), want)
    want = R.image_table(one, sizes, 4, L, 32, 0, 8192)
    assert int(want[2]) == 1 and int(want[3]) == int(sizes[-1])


def test_later_calls_overwrite(mpc, bdi64):
    L, N = 64, 4
    lines, sizes = bdi64
    third = 1300
    addrs = np.tile(spread_addresses(third, L, 900, seed=9, misaligned=False), 3)      # the same addresses in three calls, other lines
    lines, sizes = lines[:3 * third], sizes[:3 * third]
    ev = mpc.BDI(L)
    ev.enable_image_stats(N, 32, 0, 2048)
    for call in range(3):
        at = (call + 1) * third
        feed(ev, lines[at - third:at], addrs[at - third:at])
        R.same_table(f"after call {call}", ev.image_table(), R.image_table(addrs[:at], sizes[:at], N, L, 32, 0, 2048))
    ev.close()
    assert int(R.image_table(addrs[:third], sizes[:third], N, L, 32, 0, 2048)[3]) != int(R.image_table(addrs, sizes, N, L, 32, 0, 2048)[3])


# ---- 3. probing and overflow (the test library: a process of its own) --------------------------------------------------
PROBING = r"""
import os
sys.path.insert(0, os.path.join(%(root)r, "tests"))
import image_ref as R
L, N = 64, 4
rng = np.random.default_rng(11)
def mixed(n):
    small = rng.integers(0, 200, (n, L // 4), dtype=np.uint32).view(np.uint8).reshape(n, L)
    kinds = np.stack([T.zeros(n, L), T.word_same(n, L), small, T.random_u32(n, L)])
    return np.ascontiguousarray(kinds[rng.integers(0, 4, n), np.arange(n)])
lines = mixed(4096)
plain = mpc.BDI(L); sizes = plain.compress_lines(lines, want_selected=False)[0]; plain.close()
def keys_at(slot0, slots, count):
    # keys found through mpc_image_hash whose first slot is slot0
    out, k = [], 1
    while len(out) < count:
        if mpc.image_hash(k) & (slots - 1) == slot0:
            out.append(k)
        k += 1
    return np.array(out, dtype=np.uint64)
def run(capacity, keys, n, bits=None):
    # n lines over these keys, every key at least once, many overwrites; exactly len(keys) distinct
    if bits is None: os.environ.pop("MPC_TEST_IMAGE_HASH_BITS", None)
    else: os.environ["MPC_TEST_IMAGE_HASH_BITS"] = str(bits)
    addrs = np.concatenate([keys, keys[rng.integers(0, len(keys), n - len(keys))]]) * np.uint64(L)
    addrs = addrs[rng.permutation(n)]
    ev = mpc.BDI(L)
    ev.enable_image_stats(N, 32, 0, capacity)
    ev.compress_lines(lines[:n], want_sizes=False, want_selected=False, addresses=addrs)
    got = ev.image_table()
    ev.close()
    R.same_table(f"capacity {capacity} bits {bits}", got, R.image_table(addrs, sizes[:n], N, L, 32, 0, capacity))
    assert int(got[2]) == len(keys)
checked = 0
for capacity in (1, 2, 3, 4, 1000):
    slots = R.slots_of(capacity)
    assert slots == {1: 2, 2: 4, 3: 8, 4: 8, 1000: 2048}[capacity]
    # chains that start at the last slot and wrap to slot 0; exactly `capacity` distinct keys succeeds
    run(capacity, keys_at(slots - 1, slots, capacity), 4096); checked += 1
    # every key shares one first slot (bits 0) or four (bits 2): chains through most of the table
    for bits in (0, 2):
        run(capacity, np.arange(1, capacity + 1, dtype=np.uint64) * np.uint64(1000003), 4096, bits); checked += 1
# overflow: capacity + 1 distinct keys is the error; far more keys than slots returns (every probe loop terminates)
overflows = 0
for capacity, distinct, bits in ((1, 2, None), (4, 5, None), (1000, 1001, None), (4, 4000, None), (4, 4000, 0), (1000, 4096, 2)):
    if bits is None: os.environ.pop("MPC_TEST_IMAGE_HASH_BITS", None)
    else: os.environ["MPC_TEST_IMAGE_HASH_BITS"] = str(bits)
    ev = mpc.BDI(L)
    ev.enable_image_stats(N, 32, 0, capacity)
    addrs = (np.arange(4096, dtype=np.uint64) %% np.uint64(distinct)) * np.uint64(L)
    for call in (lambda: ev.compress_lines(lines, addresses=addrs), lambda: ev.compress_lines(lines[:8], addresses=addrs[:8]), ev.image_table):
        try:
            call()
            raise AssertionError("no error")
        except mpc.MpcError as e:
            assert e.code == -22 and "distinct line addresses" in str(e) and str(capacity) in str(e), str(e)
    ev.close()
    overflows += 1
print("ROUTES " + json.dumps({"checked": checked, "overflows": overflows}))
"""


def test_probing_and_overflow(mpc):
    from testlib_child import _run_with_test_library
    pkg("build").build_lib(test=True)
    res = _run_with_test_library(PROBING % {"root": ROOT}, grid_cap=0, timeout=600)
    assert res == {"checked": 15, "overflows": 6}


def test_overflow_on_the_product_library(mpc, bdi64):
    L = 64
    lines, _ = bdi64
    ev = mpc.BDI(L)
    ev.enable_image_stats(4, 32, 0, 100)
    addrs = np.arange(101, dtype=np.uint64) * np.uint64(L)
    feed(ev, lines[:100], addrs[:100])                            # exactly the capacity
    assert int(ev.image_table()[2]) == 100
    refused(mpc, lambda: feed(ev, lines[100:101], addrs[100:101]), "more than 100 distinct line addresses")
    refused(mpc, lambda: feed(ev, lines[:1], addrs[:1]), "takes no more lines")
    refused(mpc, ev.image_table, "more than 100 distinct line addresses")
    ev.close()


def test_overflow_far_beyond_the_table(mpc, traces):
    """2^20 distinct lines into a capacity of 2^16 (2^17 slots): the device stops probing and claiming once it has seen
    the capacity exceeded, so the call returns at once -- a probe per new line over a table that filled up would be
    2^17 loads for each of nearly 2^20 lines -- in the staged path (chunks behind the overflow find the flag set) and
    in the device path."""
    import time
    import torch
    L, n, capacity = 32, 1 << 20, 1 << 16
    lines = mixed_lines(traces, L, 4096, seed=2)[np.arange(n) % 4096]
    addrs = np.arange(n, dtype=np.uint64) * np.uint64(L)
    d_lines, d_addrs = torch.from_numpy(lines).to("cuda:0"), torch.from_numpy(addrs.view(np.int64)).to("cuda:0")
    torch.cuda.synchronize()
    ev = mpc.BDI(L)
    ev.enable_image_stats(4, 32, 0, capacity)
    t0 = time.perf_counter()
    refused(mpc, lambda: feed(ev, lines, addrs), f"more than {capacity} distinct line addresses")
    refused(mpc, ev.image_table, f"more than {capacity} distinct line addresses")
    ev.close()
    ev = mpc.BDI(L)
    ev.enable_image_stats(4, 32, 0, capacity)
    ev.compress_device(d_lines.data_ptr(), n, addresses=d_addrs.data_ptr())       # asynchronous: the error surfaces at the sync
    refused(mpc, ev.sync, f"more than {capacity} distinct line addresses")
    refused(mpc, lambda: ev.compress_device(d_lines.data_ptr(), n, addresses=d_addrs.data_ptr()), "takes no more lines")
    ev.close()
    # Bounded work is tens of milliseconds for 32 MiB of lines.  Probing a full table of 2^17 slots for each of the
    # 2^20 - 2^17 lines behind it is 1.2e11 dependent loads a path, tens of seconds: 5 s lies far from both.
    assert time.perf_counter() - t0 < 5.0


# ---- 4. address edge values ------------------------------------------------------------------------------------------
def test_address_edges(mpc, bdi64):
    L = 64
    lines, sizes = bdi64
    top = np.uint64((1 << 64) - 1)
    edge = np.array([0, top, 5 * L, (1 << 32) + 5 * L, (1 << 40) + 5 * L, 0, 1, L - 1, top - np.uint64(L), 7 * L + 1, top], dtype=np.uint64)
    addrs = np.tile(edge, 20)
    n = addrs.size
    for N in (1, 4, 1000):
        want = R.image_table(addrs, sizes[:n], N, L, sector_for(N, L), 0, 64)
        assert int(want[2]) == 7 and int(want[7]) == 20 * 6       # key 0 (0, 1, L - 1), the top two, 5 and its two twins above bit 32, 7
        R.same_table(f"N={N}", image_of(mpc, L, lines[:n], addrs, N, sector_for(N, L), 0, 64), want)
    loop = R.image_table_loop(addrs, sizes[:n], 4, L, 32, 0, 64)
    R.same_table("reference against the loop", R.image_table(addrs, sizes[:n], 4, L, 32, 0, 64), loop)


# ---- 5. blocks -------------------------------------------------------------------------------------------------------
def test_blocks(mpc, traces, bdi64):
    L, N = 64, 8
    lines, sizes = bdi64
    # blocks with T = 1, T = N - 1, T = N and everything between, each key written twice (the second write wins)
    keys = np.concatenate([np.arange(b * N, b * N + 1 + b % N, dtype=np.uint64) for b in range(400)])
    keys = np.concatenate([keys, keys[::-1]])[:4096]
    addrs = keys * np.uint64(L)
    n = addrs.size
    blocks, T, payload = R.blocks_of(addrs, sizes[:n], N, L)
    assert {1, N - 1, N} <= set(T.tolist())
    sec, caps = R.sectors_of(T, payload, L, 32, 0)
    assert (sec == caps).any() and (sec < caps).any() and (sec == 1).any()     # a block that reaches its cap, blocks below it
    pair = R.boundary_headers(addrs, sizes[:n], N, L, 32)
    assert pair is not None
    for hb in (0,) + pair:
        want = R.image_table(addrs, sizes[:n], N, L, 32, hb, 8192)
        R.same_table(f"header {hb}", image_of(mpc, L, lines[:n], addrs, N, 32, hb), want)
    exact, plus_one = (R.image_table(addrs, sizes[:n], N, L, 32, hb, 8192) for hb in pair)
    assert int(plus_one[5]) > int(exact[5])                       # the one bit more costs a sector
    # random lines: BDI's size is above 8 L bits, every block reaches its cap
    rnd = traces.random_u32(n, L)
    ev = mpc.BDI(L)
    rs = ev.compress_lines(rnd, want_selected=False)[0]
    ev.close()
    want = R.image_table(addrs, rs, N, L, 32, 0, 8192)
    assert int(want[5]) == int(want[6])
    R.same_table("all at the cap", image_of(mpc, L, rnd, addrs, N), want)


# ---- 6. seams --------------------------------------------------------------------------------------------------------
def test_call_seams(mpc, bdi64):
    L, N = 64, 4
    lines, sizes = bdi64
    cuts = [1, 63, 64, 65, 1, 511, 512, 513, 65, 64, 63]          # in-place calls up to 512 lines, staged ones above
    n = sum(cuts)
    addrs = spread_addresses(n, L, 600, seed=21)
    ev = mpc.BDI(L)
    ev.enable_image_stats(N, 32, 0, 1024)
    at = 0
    for c in cuts:
        feed(ev, lines[at:at + c], addrs[at:at + c])
        at += c
        R.same_table(f"after {at} lines", ev.image_table(), R.image_table(addrs[:at], sizes[:at], N, L, 32, 0, 1024))
    ev.close()


def test_stager_slots(mpc, traces):
    """1.25 Mi lines of 128 bytes in one staged call of 160 MiB: three chunks over the two staging slots."""
    L, N, n = 128, 4, (1 << 20) + (1 << 18)
    pool = mixed_lines(traces, L, 4096, seed=5)
    lines = pool[np.random.default_rng(5).integers(0, len(pool), n)]
    ev = mpc.BDI(L)
    sizes = ev.compress_lines(lines, want_selected=False)[0]
    ev.close()
    addrs = spread_addresses(n, L, 1 << 16, seed=6)               # every key many times, on both sides of the chunk seams
    want = R.image_table(addrs, sizes, N, L, 32, 0, 1 << 17)
    R.same_table("staged", image_of(mpc, L, lines, addrs, N, 32, 0, 1 << 17), want)


def test_device_path(mpc):
    """4 Mi + 12 345 lines of 32 bytes from mpc_synth_fill, without a sizes array (pieces of 4 Mi lines over the
    scratch array; positions and addresses run across the seam) and with the caller's."""
    import torch
    L, N, n = 32, 4, (4 << 20) + 12345
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
    addrs = spread_addresses(n, L, 1 << 18, seed=8)
    addrs[(4 << 20) - 50:(4 << 20) + 50] = np.uint64(77 * L)       # one key on both sides of the seam of the pieces
    d_addrs = torch.from_numpy(addrs.view(np.int64)).to("cuda:0")
    want = R.image_table(addrs, sizes, N, L, 32, 0, 1 << 19)
    ev = mpc.BDI(L)
    ev.enable_image_stats(N, 32, 0, 1 << 19)
    ev.compress_device(buf.data_ptr(), n, addresses=d_addrs.data_ptr())
    R.same_table("pieces", ev.image_table(), want)
    ev.reset()
    out = torch.zeros(n, dtype=torch.int16, device="cuda:0")
    ev.compress_device(buf.data_ptr(), n, out.data_ptr(), addresses=d_addrs.data_ptr())
    R.same_table("the caller's sizes array", ev.image_table(), want)
    assert (out.cpu().numpy().view(np.uint16) == sizes).all()
    refused(mpc, lambda: ev.compress_device(buf.data_ptr(), 100), "every line needs an address")
    ev.close()


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


def test_gpgpusim_log(mpc, traces, tmp_path):
    L, N, n = 64, 4, 3001
    lines = mixed_lines(traces, L, n, seed=4)
    ev = mpc.FPC(L)
    sizes = ev.compress_lines(lines, want_selected=False)[0]
    ev.close()
    req_types = np.where(np.arange(n) % 5 == 0, 4, np.where(np.arange(n) % 11 == 0, 3, 0))      # reads, writes, and texture reads that are not evaluated
    keep = req_types != 3
    addrs = spread_addresses(n, L, 700, seed=12)
    addrs[~keep] = np.uint64(0xdead0000)                          # an address only skipped records carry
    log = patched_log(traces, str(tmp_path / "t.log"), lines, req_types, addrs)
    want = R.image_table(addrs[keep], sizes[keep], N, L, 32, 0, 1024)
    assert int((addrs[keep] // np.uint64(L) == np.uint64(0xdead0000 // L)).sum()) == 0
    ev = mpc.FPC(L)
    ev.enable_image_stats(N, 32, 0, 1024)
    ev.enable_class_stats(32)
    ev.class_log_field("rw")                                      # class fields of the same log keep working next to it
    assert ev.compress_gpgpusim_log(log)[1] == int(keep.sum())
    R.same_table(".log", ev.image_table(), want)
    cls = ev.class_stats()
    assert int(cls["lines"][0]) == int((req_types == 0).sum()) and int(cls["lines"][1]) == int((req_types == 4).sum())
    ev.close()


# ---- 7. get, reset and the off state ---------------------------------------------------------------------------------
def test_get_is_not_destructive_and_reset_starts_over(mpc, bdi64):
    L, N = 64, 4
    lines, sizes = bdi64
    addrs = spread_addresses(len(lines), L, 1500, seed=13)
    ev = mpc.BDI(L)
    ev.enable_image_stats(N, 32, 0, 2048)
    feed(ev, lines[:2000], addrs[:2000])
    first = ev.image_table()
    R.same_table("first get", first, R.image_table(addrs[:2000], sizes[:2000], N, L, 32, 0, 2048))
    R.same_table("second get", ev.image_table(), first)
    feed(ev, lines[2000:], addrs[2000:])
    R.same_table("lines after a get count", ev.image_table(), R.image_table(addrs, sizes, N, L, 32, 0, 2048))
    ev.reset()
    R.same_table("after reset", ev.image_table(), R.image_table(addrs[:0], sizes[:0], N, L, 32, 0, 2048))
    feed(ev, lines[1000:3000], addrs[:2000])                      # positions and the image start over
    R.same_table("after reset and lines", ev.image_table(), R.image_table(addrs[:2000], sizes[1000:3000], N, L, 32, 0, 2048))
    ev.close()


# (That a handle with image accounting OFF computes what the parent commit computes is what the suite's existing tests
# hold, unchanged, for every evaluator and path; here the same handle is compared with the accounting on and off.)
@pytest.mark.parametrize("comp", ["BDI", "VPC", "SC2"])
def test_interplay_and_the_off_state(mpc, configs, traces, comp):
    import pack_ref
    L, n = 64, 3000
    lines = mixed_lines(traces, L, n, seed=6)
    sizes, sel, stats = plain_sizes(mpc, configs, comp, L, lines)
    addrs = spread_addresses(n, L, 800, seed=14)
    # class and pack accounting without image accounting
    ev = make(mpc, configs, comp, L)
    ev.enable_class_stats(32)
    ev.enable_pack_stats(16, 32, 0)
    ev.compress_lines(lines, want_sizes=False, want_selected=False)
    cls_table, pack_table = ev.class_table(), ev.pack_table()
    ev.close()
    pack_ref.same_table("pack", pack_table, pack_ref.pack_table(sizes, 16, L, 32, 0))
    # ... and with it: those tables are what they were, sizes and selected too; addressed lines count in class 0
    ev = make(mpc, configs, comp, L)
    ev.enable_class_stats(32)
    ev.enable_pack_stats(16, 32, 0)
    ev.enable_image_stats(4, 32, 0, 1024)
    got_sizes, got_sel = ev.compress_lines(lines, addresses=addrs)
    assert (got_sizes == sizes).all() and (got_sel == sel).all() and (ev.stats_vector() == stats).all()
    assert (ev.class_table() == cls_table).all() and (ev.pack_table() == pack_table).all()
    R.same_table("image", ev.image_table(), R.image_table(addrs, sizes, 4, L, 32, 0, 1024))
    ev.close()


# ---- 8. groups -------------------------------------------------------------------------------------------------------
GROUP = ("BDI", "FPC", "BPC", "VPC", "CPACK")


def test_group_members(mpc, configs, traces, tmp_path):
    import torch
    L, N, n = 64, 4, 3000
    lines = mixed_lines(traces, L, n, seed=7)
    addrs = spread_addresses(n, L, 900, seed=15)
    alone = []
    for c in GROUP:
        ev = make(mpc, configs, c, L)
        ev.enable_image_stats(N, 32, 64, 1024)
        feed(ev, lines, addrs, [1000, 2000])
        alone.append(ev.image_table())
        ev.close()
    sizes = [plain_sizes(mpc, configs, c, L, lines)[0] for c in GROUP]
    for t, s in zip(alone, sizes):
        R.same_table("alone", t, R.image_table(addrs, s, N, L, 32, 64, 1024))
    assert len({int(t[3]) for t in alone}) >= 3                   # the members' images differ
    members = [make(mpc, configs, c, L) for c in GROUP]
    grp = mpc.EvaluatorSet(members)
    grp.enable_image_stats(N, 32, 64, 1024)
    grp.enable_image_stats(N, 32, 64, 1024)
    refused(mpc, lambda: grp.enable_image_stats(N, 64, 64, 1024), "already on")
    grp.compress_lines(lines[:400], want_sizes=False, want_selected=False, addresses=addrs[:400])       # in place
    grp.compress_lines(lines[400:1000], want_sizes=False, want_selected=False, addresses=addrs[400:1000])   # staged
    d_lines = torch.from_numpy(lines[1000:]).to("cuda:0")
    d_addrs = torch.from_numpy(addrs[1000:].view(np.int64)).to("cuda:0")
    grp.compress_device(d_lines.data_ptr(), n - 1000, addresses=d_addrs.data_ptr())
    for i, t in enumerate(alone):
        R.same_table(f"member {i}", grp.image_table(i), t)
    assert grp.image_stats()[1]["image_bits"] == int(alone[1][3])
    refused(mpc, lambda: grp.compress_lines(lines[:10]), "every line needs an address")
    # the .log delivers each record's mem_addr to all members
    for m in members:
        m.reset()
    log = patched_log(traces, str(tmp_path / "g.log"), lines, np.zeros(n, np.uint32), addrs)
    assert grp.compress_gpgpusim_log(log)[1] == n
    for i, s in enumerate(sizes):
        R.same_table(f".log member {i}", grp.image_table(i), R.image_table(addrs, s, N, L, 32, 64, 1024))
    # a member fed alone: the group refuses until the members are reset
    members[2].compress_lines(lines[:5], addresses=addrs[:5])
    refused(mpc, lambda: grp.compress_lines(lines[:10], addresses=addrs[:10]), "member 2", "fed outside the group")
    for m in members:
        m.reset()
    grp.compress_lines(lines[:10], addresses=addrs[:10])
    grp.close()
    for m in members:
        m.close()


# ---- 9. refusals -----------------------------------------------------------------------------------------------------
def test_refusals(mpc, traces, tmp_path):
    L = 64
    lines = mixed_lines(traces, L, 600, seed=8)
    addrs = spread_addresses(600, L, 100, seed=16)
    ev = mpc.BDI(L)
    refused(mpc, lambda: ev.compress_lines(lines, addresses=addrs), "not switched on")
    refused(mpc, ev.image_table, "not switched on")
    for bad, word in (((0, 32, 0, 16), "block_lines"), ((4, 0, 0, 16), "sector_bytes"), ((4, 32, 70000, 16), "header_bits"), ((4, 32, 0, 0), "capacity_lines"),
                      ((4, 32, 0, (1 << 28) + 1), "capacity_lines"), ((1 << 20, 4096, 0, 16), "block_lines")):
        refused(mpc, lambda: ev.enable_image_stats(*bad), word)
    ev.enable_image_stats(4, 32, 0, 256)
    refused(mpc, lambda: ev.enable_image_stats(8, 32, 0, 256), "already on", "block_lines 4")
    refused(mpc, lambda: ev.enable_image_stats(4, 32, 0, 512), "already on", "capacity_lines 256")
    refused(mpc, lambda: ev.compress_lines(lines), "every line needs an address")             # staged
    refused(mpc, lambda: ev.compress_lines(lines[:10]), "every line needs an address")        # in place
    ev.enable_class_stats(32)
    refused(mpc, lambda: ev.compress_lines(lines, classes=np.zeros(600, np.uint8)), "every line needs an address")
    npy = traces.save_npy(str(tmp_path / "t.npy"), lines)
    refused(mpc, lambda: ev.compress_npy(npy), "every line needs an address")
    assert int(ev.image_table()[0]) == 0 and int(ev.stats_vector()[0]) == 0     # nothing of the refused calls was evaluated
    ev.compress_lines(lines, addresses=addrs)
    assert int(ev.image_table()[0]) == 600
    ev.close()
    fit = mpc.FitPairs(L)
    refused(mpc, lambda: fit.enable_image_stats(4), "Fit")
    fit.close()


# ---- 10. the command line --------------------------------------------------------------------------------------------
def test_cli_image(mpc, configs, traces, tmp_path):
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

    def run(args, out):
        out.mkdir()
        r = subprocess.run([cli, *args, "-o", str(out)], cwd=bindir, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        return r.stdout

    # one algorithm: --image alone changes not one byte of the other outputs and does not switch the size histogram on
    base = ["-a", "BDI", "-i", log]
    plain_stdout = run(base, tmp_path / "one_plain")
    assert run(base + ["--image", "4", "--sector", "32", "--image-capacity", "1024"], tmp_path / "one") == plain_stdout
    for name in os.listdir(tmp_path / "one_plain"):
        assert (tmp_path / "one" / name).read_bytes() == (tmp_path / "one_plain" / name).read_bytes(), name
    assert sorted(set(os.listdir(tmp_path / "one")) - set(os.listdir(tmp_path / "one_plain"))) == ["BDI_results_image.csv"]
    want = R.image_table(addrs[keep], sizes[1], 4, L, 32, 0, 1024)
    assert len(np.nonzero(want[16:20])[0]) >= 3 and int(want[2]) < int(want[0])
    assert (tmp_path / "one" / "BDI_results_image.csv").read_text() == R.CSV_HEADER + R.csv_row("ds_t", want, L)
    # a list: every member gets its own file; the default capacity
    base = ["-a", ",".join(names), "-c", cfg_path, "-i", log]
    plain_stdout = run(base, tmp_path / "list_plain")
    assert run(base + ["--image", "128", "--image-header", "256"], tmp_path / "list") == plain_stdout
    for name in os.listdir(tmp_path / "list_plain"):
        assert (tmp_path / "list" / name).read_bytes() == (tmp_path / "list_plain" / name).read_bytes(), name
    stems = ["probe", "BDI", "FPC"]
    assert sorted(set(os.listdir(tmp_path / "list")) - set(os.listdir(tmp_path / "list_plain"))) == sorted(f"{s}_results_image.csv" for s in stems)
    for stem, s in zip(stems, sizes):
        table = R.image_table(addrs[keep], s, 128, L, 32, 256, 1 << 24)
        assert (tmp_path / "list" / f"{stem}_results_image.csv").read_text() == R.CSV_HEADER + R.csv_row("ds_t", table, L), stem
