"""Snapshots on the MI355X (csrc/mpc_snapshot.hip, include/mpc_hip_snapshot.h): the bytes of the latest unit per address,
written out as address-aligned lines of any line size and evaluated by handles and groups.  The expected bytes, plans and
statistics are tests/snapshot_ref.py over everything that was added; every comparison is equality of integer or byte
arrays.  Units are random bytes, so a wrong winner at an address, a misplaced unit or a gap that is not zero shows."""
import json
import os

import numpy as np
import pytest

from conftest import ROOT, pkg

import image_ref
import snapshot_ref as R

pytestmark = pytest.mark.gpu

MPC_E_INVAL = -22
SIZES = {32: (32, 64, 128, 256), 64: (128,), 128: (128, 256)}          # U: the line sizes tested with it
BASE = 0x7f0000000000                                                     # above 2^32


@pytest.fixture(scope="module")
def mpc():
    pkg("build").build_lib()
    m = pkg()
    m.lib()
    return m


@pytest.fixture(scope="module")
def cli():
    pkg("build").build_all()
    return os.path.join(ROOT, "bin", "compressor")


def refused(mpc, call, *words):
    with pytest.raises(mpc.MpcError) as e:
        call()
    assert e.value.code == MPC_E_INVAL and all(w in str(e.value) for w in words), str(e.value)


def drawn(U, n, keys, seed, misaligned=True, base=BASE):
    """n random units over `keys` unit addresses from `base`: repeats, lines with units missing, and (every 7th unit) an
    address that is no multiple of U."""
    rng = np.random.default_rng(seed)
    units = rng.integers(0, 256, (n, U), dtype=np.uint8)
    addrs = np.uint64(base) + rng.integers(0, keys, n).astype(np.uint64) * np.uint64(U)
    if misaligned:
        addrs[::7] += rng.integers(1, U, addrs[::7].size).astype(np.uint64)
    return units, addrs


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


def cut(units, addrs, cuts):
    out, at = [], 0
    for n in list(cuts) + [len(addrs) - sum(cuts)]:
        out.append((units[at:at + n], addrs[at:at + n]))
        at += n
    assert at == len(addrs)
    return out


def add_host(snap, calls):
    for u, a in calls:
        snap.add(u, a)


def add_device(snap, calls):
    import torch
    keep = []
    for u, a in calls:
        if len(a) == 0:
            snap.add_device(0, 0, 0)
            continue
        du, da = torch.from_numpy(np.ascontiguousarray(u)).to("cuda:0"), torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to("cuda:0")
        torch.cuda.synchronize()
        snap.add_device(du.data_ptr(), len(a), da.data_ptr())
        keep.append((du, da))
    snap.stats()                                                    # waits: the tensors may go
    return keep


def same(tag, snap, units, addrs, U, capacity, sizes=None):
    """stats, and per line size and partial mode the plan with its identities and the emitted bytes, addresses and masks"""
    want = R.stats(units, addrs, U, capacity)
    assert snap.stats() == want, (tag, snap.stats(), want)
    out = {}
    for L in sizes or SIZES[U]:
        for partial in ("skip", "zero"):
            p = snap.plan(L, partial)
            assert p == R.plan(units, addrs, U, L, partial, capacity), (tag, L, partial, p)
            R.plan_identities(p, L // U, want["distinct_units"], partial)
            got, ref = snap.read_lines(L, partial), R.read(units, addrs, U, L, partial, capacity)
            for name, g, r in zip(("lines", "addresses", "presence"), got, ref):
                assert g.dtype == r.dtype and g.shape == r.shape and (g == r).all(), (tag, L, partial, name)
            out[L, partial] = got
    return out


# ---- 1. sizes and paths ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("U", sorted(SIZES))
def test_sizes_and_paths(mpc, traces, tmp_path, U):
    n, capacity = 3000, 4096
    units, addrs = drawn(U, n, 2200, seed=U)
    ref = R.plan(units, addrs, U, SIZES[U][-1], "zero", capacity)
    assert ref["partial"] > 0 and ref["complete"] > 0 and R.stats(units, addrs, U)["distinct_units"] < n
    results = []
    for how in ("host", "device", "log"):
        snap = mpc.Snapshot(U, capacity)
        if how == "host":
            add_host(snap, [(units, addrs)])
        elif how == "device":
            add_device(snap, [(units, addrs)])
        else:
            # the records that are not evaluated (texture reads) sit between the others and carry addresses of their own
            m = n + n // 10
            rng = np.random.default_rng(77)
            skip = np.zeros(m, dtype=bool)
            skip[rng.choice(m, m - n, replace=False)] = True
            lu = rng.integers(0, 256, (m, U), dtype=np.uint8)
            la = np.full(m, 0xdead0000, dtype=np.uint64)
            lu[~skip], la[~skip] = units, addrs
            req_types = np.where(skip, 3, np.where(np.arange(m) % 3 == 0, 4, 0))
            log = patched_log(traces, str(tmp_path / "t.log"), lu, req_types, la)
            assert snap.add_gpgpusim_log(log) == n
        results.append(same(how, snap, units, addrs, U, capacity))
        snap.close()
    for key in results[0]:                                          # identical bytes through the three paths
        for other in results[1:]:
            assert all((a == b).all() for a, b in zip(results[0][key], other[key])), key


def test_log_refusals(mpc, traces, tmp_path):
    rng = np.random.default_rng(3)
    u32, u64 = rng.integers(0, 256, (10, 32), dtype=np.uint8), rng.integers(0, 256, (10, 64), dtype=np.uint8)
    log32 = traces.write_gpgpusim_log(str(tmp_path / "a.log"), u32)
    snap = mpc.Snapshot(64, 64)
    refused(mpc, lambda: snap.add_gpgpusim_log(log32), "trace line size 32", "unit size 64")
    with pytest.raises(mpc.MpcError, match="Failed to open a file"):
        snap.add_gpgpusim_log(str(tmp_path / "missing.log"))
    # evaluated records of two sizes: the loaders' message
    a, b = open(log32, "rb").read(), open(traces.write_gpgpusim_log(str(tmp_path / "b.log"), u64), "rb").read()
    with open(tmp_path / "mixed.log", "wb") as f:
        f.write(a + b[1 + 17 * 7:])
    snap32 = mpc.Snapshot(32, 64)
    refused(mpc, lambda: snap32.add_gpgpusim_log(str(tmp_path / "mixed.log")), "mixes request sizes", "64 after 32")
    assert snap.stats()["units"] == 0
    snap.close()
    snap32.close()


# ---- 2. unit counts --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (0, 1, 63, 64, 65, 255, 256, 257))
def test_unit_counts(mpc, n):
    for U in (32, 128):
        units, addrs = drawn(U, n, max(1, (2 * n) // 3), seed=100 + n)
        for how in (add_host, add_device):
            snap = mpc.Snapshot(U, 512)
            how(snap, [(units, addrs)])
            same(f"n={n} U={U}", snap, units, addrs, U, 512)
            snap.close()


def test_calls_cut_at_odd_places(mpc):
    U, n = 32, 5000
    units, addrs = drawn(U, n, 3000, seed=9)
    whole = mpc.Snapshot(U, 4096)
    add_host(whole, [(units, addrs)])
    a = same("one call", whole, units, addrs, U, 4096)
    for how in (add_host, add_device):
        parts = mpc.Snapshot(U, 4096)
        how(parts, cut(units, addrs, (1, 63, 0, 700, 1237, 65)))
        b = same("several calls", parts, units, addrs, U, 4096)
        assert all((x == y).all() for key in a for x, y in zip(a[key], b[key]))
        parts.close()
    whole.close()


# ---- 3. the latest unit wins -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", (65, 257))
def test_latest_wins_at_one_address(mpc, run):
    """`run` consecutive units of one address with different data, straddling a wave (65) and a workgroup (257), between
    units of other addresses; then the same run across two calls."""
    U = 32
    rng = np.random.default_rng(run)
    for lead in (0, 30, 200):
        units = rng.integers(0, 256, (lead + run + 10, U), dtype=np.uint8)
        addrs = np.uint64(BASE) + np.arange(1, lead + run + 11, dtype=np.uint64) * np.uint64(U)
        addrs[lead:lead + run] = np.uint64(BASE)
        for how in (add_host, add_device):
            for cuts in ((), (lead + run // 2,), (lead + run - 1,)):
                snap = mpc.Snapshot(U, 512)
                how(snap, cut(units, addrs, cuts))
                same(f"run {run} lead {lead} cuts {cuts}", snap, units, addrs, U, 512, sizes=(32, 64))
                lines, la, _ = snap.read_lines(32)
                assert int(la[0]) == BASE and (lines[0] == units[lead + run - 1]).all()
                snap.close()


def test_stale_versions_before_the_final_one(mpc):
    U, keys = 64, 1500
    rng = np.random.default_rng(21)
    final = rng.integers(0, 256, (keys, U), dtype=np.uint8)
    fa = np.uint64(BASE) + rng.permutation(4000)[:keys].astype(np.uint64) * np.uint64(U)
    stale_of = rng.integers(0, keys, 4000)
    stale = rng.integers(0, 256, (4000, U), dtype=np.uint8)
    order = rng.permutation(keys)
    units, addrs = np.concatenate([stale, final[order]]), np.concatenate([fa[stale_of], fa[order]])
    for how in (add_host, add_device):
        snap = mpc.Snapshot(U, 2048)
        how(snap, cut(units, addrs, (333, 3000)))
        same("stale", snap, units, addrs, U, 2048)
        lines, la, _ = snap.read_lines(64)
        by = np.argsort(fa)
        assert (la == fa[by]).all() and (lines == final[by]).all()
        snap.close()


# ---- 4. presence masks -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("U,k", ((32, 2), (32, 4), (64, 2), (32, 8), (128, 2)))
def test_every_presence_mask(mpc, U, k):
    L = U * k
    rng = np.random.default_rng(k * 1000 + U)
    masks = list(range(1, 1 << k)) if k < 8 else [1, 2, 128, 255, 254, 127, 0x55, 0xaa, 0x81, 0x18] + rng.integers(1, 256, 40).tolist()
    masks = [masks[i] for i in rng.permutation(len(masks))] * 3
    keys = [line * 2 * k + j for line, m in enumerate(masks) for j in range(k) if m >> j & 1]      # every other line is touched
    keys = np.array(keys, dtype=np.uint64)[rng.permutation(len(keys))]
    units, addrs = rng.integers(0, 256, (len(keys), U), dtype=np.uint8), keys * np.uint64(U)
    snap = mpc.Snapshot(U, 4096)
    snap.add(units, addrs)
    same(f"masks k={k}", snap, units, addrs, U, 4096, sizes=(L,))
    lines, la, pres = snap.read_lines(L, "zero")
    assert pres.tolist() == masks and la.tolist() == [i * 2 * L for i in range(len(masks))]
    for row, m in zip(lines.reshape(len(masks), k, U), masks):
        for j in range(k):
            assert (row[j] != 0).any() if m >> j & 1 else not row[j].any()
    _, _, pres = snap.read_lines(L, "skip")
    assert pres.tolist() == [m for m in masks if m == (1 << k) - 1] and len(pres) >= 3
    snap.close()


# ---- 5. addresses ----------------------------------------------------------------------------------------------------
def test_address_edges(mpc):
    """key 0, addresses above 2^32 and just below 2^63 -- emitted lines are in ascending order of the whole 64-bit
    address -- and addresses that are no multiple of U."""
    U = 32
    top = (1 << 63) - 256
    bases = [0, 32, 64 + 5, 4096, (1 << 32) - 32, 1 << 32, (1 << 32) + 32 + 31, (1 << 40) + 96, top, top + 64, top + 224 + 31]
    rng = np.random.default_rng(12)
    order = rng.permutation(len(bases) * 2) % len(bases)
    addrs = np.array(bases, dtype=np.uint64)[order]
    units = rng.integers(0, 256, (len(addrs), U), dtype=np.uint8)
    for how in (add_host, add_device):
        snap = mpc.Snapshot(U, 64)
        how(snap, [(units, addrs)])
        out = same("edges", snap, units, addrs, U, 64)
        assert snap.stats()["misaligned"] == 2 * 3 and snap.stats()["distinct_units"] == len(bases)
        la = out[256, "zero"][1]
        assert la.tolist() == [0, 4096, (1 << 32) - 256, 1 << 32, 1 << 40, top] and out[256, "zero"][2].tolist() == [7, 1, 128, 3, 8, 1 | 4 | 128]
        snap.close()


# ---- 6. probing, striding and the capacity under the test library -----------------------------------------------------
TESTLIB = r"""
import os
sys.path.insert(0, os.path.join(%(root)r, "tests"))
import snapshot_ref as R
rng = np.random.default_rng(31)
def check(tag, snap, units, addrs, U, capacity, sizes):
    assert snap.stats() == R.stats(units, addrs, U, capacity), (tag, snap.stats())
    for L in sizes:
        for partial in ("skip", "zero"):
            assert snap.plan(L, partial) == R.plan(units, addrs, U, L, partial, capacity), (tag, L, partial)
            for g, r in zip(snap.read_lines(L, partial), R.read(units, addrs, U, L, partial, capacity)):
                assert g.shape == r.shape and (g == r).all(), (tag, L, partial)
def keys_at(slot0, slots, count):
    # keys whose first slot is slot0 (the snapshot's hash is image accounting's)
    out, k = [], 1
    while len(out) < count:
        if mpc.image_hash(k) & (slots - 1) == slot0:
            out.append(k)
        k += 1
    return np.array(out, dtype=np.uint64)
def run(U, capacity, keys, n, bits, cuts=()):
    if bits is None: os.environ.pop("MPC_TEST_SNAPSHOT_HASH_BITS", None)
    else: os.environ["MPC_TEST_SNAPSHOT_HASH_BITS"] = str(bits)
    # n units over these keys, every key at least once, many overwrites; exactly len(keys) distinct
    addrs = np.concatenate([keys, keys[rng.integers(0, len(keys), n - len(keys))]])[rng.permutation(n)] * np.uint64(U)
    units = rng.integers(0, 256, (n, U), dtype=np.uint8)
    snap = mpc.Snapshot(U, capacity)
    at = 0
    for c in list(cuts) + [n - sum(cuts)]:
        snap.add(units[at:at + c], addrs[at:at + c]); at += c
    check((U, capacity, bits), snap, units, addrs, U, capacity, (U, 4 * U) if U == 32 else (2 * U,))
    assert snap.stats()["distinct_units"] == len(keys)
    snap.close()
checked = 0
# the grid is capped at two workgroups: 5000 units are ten rounds of every kernel's loop
for U in (32, 64, 128):
    run(U, 4096, np.arange(3000, dtype=np.uint64) * np.uint64(3) + np.uint64(1 << 33), 5000, None); checked += 1
run(32, 4096, np.arange(3000, dtype=np.uint64) + np.uint64(7), 5000, None, cuts=(1, 511, 513, 1237)); checked += 1
# one address for 257 and 1100 consecutive units: across the rounds of the two workgroups
for rep in (257, 1100):
    units = rng.integers(0, 256, (rep + 40, 32), dtype=np.uint8)
    addrs = np.arange(rep + 40, dtype=np.uint64) * np.uint64(32); addrs[20:20 + rep] = np.uint64(1 << 35)
    snap = mpc.Snapshot(32, 2048); snap.add(units, addrs)
    check(("run", rep), snap, units, addrs, 32, 2048, (32, 128)); snap.close(); checked += 1
for capacity in (1, 2, 3, 8, 1000):
    slots = R.slots_of(capacity)
    assert slots == {1: 2, 2: 4, 3: 8, 8: 16, 1000: 2048}[capacity]
    # chains that start at the last slot and wrap to slot 0; exactly `capacity` distinct keys succeeds
    run(32, capacity, keys_at(slots - 1, slots, capacity), 3000, None); checked += 1
    # every key shares one first slot (bits 0) or four (bits 2): chains through most of the table
    for bits in (0, 2):
        run(64 if bits else 32, capacity, np.arange(1, capacity + 1, dtype=np.uint64) * np.uint64(1000003), 3000, bits); checked += 1
# overflow: capacity + 1 distinct keys is the error; far more keys than slots returns (every probe loop terminates)
overflows = 0
for capacity, distinct, bits in ((1, 2, None), (8, 9, None), (1000, 1001, None), (8, 4000, None), (8, 4000, 0), (1000, 4096, 2)):
    if bits is None: os.environ.pop("MPC_TEST_SNAPSHOT_HASH_BITS", None)
    else: os.environ["MPC_TEST_SNAPSHOT_HASH_BITS"] = str(bits)
    snap = mpc.Snapshot(32, capacity)
    units = rng.integers(0, 256, (4096, 32), dtype=np.uint8)
    addrs = (np.arange(4096, dtype=np.uint64) %% np.uint64(distinct)) * np.uint64(32)
    for call in (lambda: snap.add(units, addrs), lambda: snap.add(units[:8], addrs[:8]), snap.stats, lambda: snap.plan(32), lambda: snap.read_lines(32)):
        try:
            call()
            raise AssertionError("no error")
        except mpc.MpcError as e:
            assert e.code == -22 and "distinct unit addresses" in str(e) and str(capacity) in str(e), str(e)
    snap.reset()
    snap.add(units[:capacity], addrs[:capacity])
    check(("revived", capacity), snap, units[:capacity], addrs[:capacity], 32, capacity, (32,))
    snap.close()
    overflows += 1
print("ROUTES " + json.dumps({"checked": checked, "overflows": overflows}))
"""


def test_probing_striding_and_overflow(mpc):
    from testlib_child import _run_with_test_library
    pkg("build").build_lib(test=True)
    res = _run_with_test_library(TESTLIB % {"root": ROOT}, grid_cap=2, timeout=600)
    assert res == {"checked": 21, "overflows": 6}


# ---- 7. the capacity on the product library ---------------------------------------------------------------------------
def test_capacity(mpc):
    import torch
    U, capacity = 32, 100
    units, addrs = drawn(U, 101, 1, seed=5, misaligned=False)
    addrs = np.uint64(BASE) + np.arange(101, dtype=np.uint64) * np.uint64(U)
    snap = mpc.Snapshot(U, capacity)
    snap.add(units[:100], addrs[:100])                              # exactly the capacity
    snap.add(units[:100], addrs[:100])                              # ... and known keys again
    assert snap.stats()["distinct_units"] == 100 and snap.plan(32)["n_out"] == 100
    refused(mpc, lambda: snap.add(units[100:], addrs[100:]), "more than 100 distinct unit addresses")
    refused(mpc, lambda: snap.add(units[:1], addrs[:1]), "takes no more units")
    refused(mpc, snap.stats, "more than 100 distinct unit addresses")
    refused(mpc, lambda: snap.plan(32), "more than 100 distinct unit addresses")
    refused(mpc, lambda: snap.read_lines(32), "more than 100 distinct unit addresses")
    bdi = mpc.BDI(32)
    refused(mpc, lambda: snap.evaluate(bdi, 32), "more than 100 distinct unit addresses")
    assert int(bdi.stats_vector()[0]) == 0
    snap.reset()                                                    # revives it
    assert snap.stats() == {"units": 0, "distinct_units": 0, "misaligned": 0, "capacity": 100, "unit_bytes": 32}
    assert snap.plan(64, "zero") == dict.fromkeys(R.PLAN_KEYS, 0) and snap.read_lines(64)[0].shape == (0, 64)
    snap.add(units[1:], addrs[1:])
    same("revived", snap, units[1:], addrs[1:], U, capacity)
    # the device add does not wait: the error surfaces at the next synchronising call
    du, da = torch.from_numpy(units).to("cuda:0"), torch.from_numpy(addrs.view(np.int64)).to("cuda:0")
    torch.cuda.synchronize()
    snap.add_device(du.data_ptr(), 1, da.data_ptr())
    refused(mpc, snap.stats, "more than 100 distinct unit addresses")
    refused(mpc, lambda: snap.add_device(du.data_ptr(), 1, da.data_ptr()), "takes no more units")
    snap.close()
    bdi.close()


# ---- 8. written into the caller's device memory ------------------------------------------------------------------------
def test_write_lines(mpc):
    import torch
    U, L, capacity = 32, 128, 4096
    units, addrs = drawn(U, 8000, 3000, seed=44)
    snap = mpc.Snapshot(U, capacity)
    snap.add(units, addrs)
    for partial in ("skip", "zero"):
        lines, la, pres = R.read(units, addrs, U, L, partial, capacity)
        n_out = len(la)
        assert n_out > 300
        for first, n in ((0, n_out), (0, 1), (n_out - 1, 1), (17, 259), (n_out, 0), (5, 0)):
            d_lines = torch.full((n * L + 16,), 0xee, dtype=torch.uint8, device="cuda:0")
            d_addrs = torch.zeros(n + 1, dtype=torch.int64, device="cuda:0")
            d_pres = torch.full((n + 1,), 0xee, dtype=torch.uint8, device="cuda:0")
            snap.write_lines(L, partial, first, n, d_lines.data_ptr(), d_addrs.data_ptr(), d_pres.data_ptr())
            torch.cuda.synchronize()
            got = d_lines.cpu().numpy()
            assert (got[:n * L].reshape(n, L) == lines[first:first + n]).all() and (got[n * L:] == 0xee).all()      # nothing behind the last line
            assert (d_addrs.cpu().numpy().view(np.uint64)[:n] == la[first:first + n]).all() and int(d_addrs[n]) == 0
            assert (d_pres.cpu().numpy()[:n] == pres[first:first + n]).all() and int(d_pres[n]) == 0xee
        d_lines = torch.zeros(n_out * L, dtype=torch.uint8, device="cuda:0")
        snap.write_lines(L, partial, 0, n_out, d_lines.data_ptr())  # the two last arrays are optional
        torch.cuda.synchronize()
        assert (d_lines.cpu().numpy().reshape(n_out, L) == lines).all()
        refused(mpc, lambda: snap.write_lines(L, partial, 1, n_out, d_lines.data_ptr()), "beyond", str(n_out))
        refused(mpc, lambda: snap.write_lines(L, partial, n_out + 1, 0, d_lines.data_ptr()), "beyond")
        refused(mpc, lambda: snap.write_lines(L, partial, 0, 2, d_lines.data_ptr() + 8), "16-byte aligned")
    refused(mpc, lambda: snap.plan(96), "is not 1, 2, 4 or 8 units")
    refused(mpc, lambda: snap.plan(512), "above 256")
    refused(mpc, lambda: snap.plan(0), "line_size")
    snap.close()


# ---- 9. the round trip into the evaluators -----------------------------------------------------------------------------
def mixed_lines(traces, L, n, seed=0):
    """n lines, each all-zero, word-same, small integers or random with equal probability."""
    rng = np.random.default_rng(1000 + L + seed)
    small = rng.integers(0, 200, (n, L // 4), dtype=np.uint32).view(np.uint8).reshape(n, L)
    kinds = np.stack([traces.zeros(n, L), traces.word_same(n, L), small, traces.random_u32(n, L, first_line=seed)])
    return np.ascontiguousarray(kinds[rng.integers(0, 4, n), np.arange(n)])


@pytest.fixture(scope="module")
def memory(traces):
    """2000 lines X of 128 bytes at distinct addresses, ordered by address, and the 32-byte units that rebuild them: stale
    versions of every unit, shuffled, then the final ones, shuffled."""
    L, U, n = 128, 32, 2000
    rng = np.random.default_rng(61)
    X = mixed_lines(traces, L, n, seed=6)
    la = np.sort(np.uint64(BASE) + rng.permutation(6000)[:n].astype(np.uint64) * np.uint64(L))
    fu = X.reshape(n * 4, U)
    fa = (la[:, None] + np.arange(4, dtype=np.uint64)[None, :] * np.uint64(U)).reshape(-1)
    stale_of = np.concatenate([np.arange(n * 4), rng.integers(0, n * 4, n)])[rng.permutation(n * 5)]
    stale = rng.integers(0, 256, (len(stale_of), U), dtype=np.uint8)
    order = rng.permutation(n * 4)
    units, addrs = np.concatenate([stale, fu[order]]), np.concatenate([fa[stale_of], fa[order]])
    return {"L": L, "U": U, "X": X, "la": la, "units": units, "addrs": addrs, "final_order": order, "fu": fu, "fa": fa}


@pytest.fixture(scope="module")
def snapshot_of_memory(mpc, memory):
    snap = mpc.Snapshot(memory["U"], 8192)
    add_host(snap, cut(memory["units"], memory["addrs"], (4097, 5000)))
    yield snap
    snap.close()


def test_round_trip_reads_the_lines_back(mpc, memory, snapshot_of_memory):
    lines, la, pres = snapshot_of_memory.read_lines(128, "skip")
    assert (lines == memory["X"]).all() and (la == memory["la"]).all() and (pres == 15).all()
    assert snapshot_of_memory.plan(128) == dict(zip(R.PLAN_KEYS, (2000, 2000, 0, 0, 0, 2000)))


def test_round_trip_into_an_evaluator_a_set_and_an_image(mpc, configs, memory, snapshot_of_memory):
    L, X, la, snap = memory["L"], memory["X"], memory["la"], snapshot_of_memory
    make = lambda: [mpc.VPC(configs.probe_config(L)), mpc.BDI(L), mpc.FPC(L), mpc.BPC(L)]
    plain = make()
    want, sizes = [], []
    for ev in plain:
        sizes.append(ev.compress_lines(X, want_selected=False)[0])
        want.append(ev.stats_vector())
        ev.close()
    assert len(set(sizes[1].tolist())) >= 3
    # one evaluator
    bdi = mpc.BDI(L)
    assert snap.evaluate(bdi, L) == len(X)
    assert (bdi.stats_vector() == want[1]).all()
    assert snap.evaluate(bdi, L, "zero") == len(X)                  # every line is complete: the same lines again
    assert int(bdi.stats_vector()[0]) == 2 * len(X)
    bdi.close()
    # a set
    members = make()
    group = mpc.EvaluatorSet(members)
    assert snap.evaluate(group, L) == len(X)
    for ev, w in zip(members, want):
        assert (ev.stats_vector() == w).all(), type(ev).__name__
    group.close()
    for ev in members:
        ev.close()
    # a handle with image accounting: the lines' own addresses
    for N in (1, 4):
        bdi = mpc.BDI(L)
        bdi.enable_image_stats(N, 32, 0, 4096)
        bdi.enable_size_histogram()
        snap.evaluate(bdi, L)
        image_ref.same_table(f"image N={N}", bdi.image_table(), image_ref.image_table(la, sizes[1], N, L, 32, 0, 4096))
        assert (bdi.stats_vector() == want[1]).all()
        assert (bdi.size_histogram()[:2048] == np.bincount(sizes[1], minlength=2048)[:2048]).all()
        bdi.close()
    # ... and a set with it
    members = [mpc.BDI(L), mpc.FPC(L)]
    group = mpc.EvaluatorSet(members)
    group.enable_image_stats(4, 32, 0, 4096)
    snap.evaluate(group, L)
    for i, s in ((0, sizes[1]), (1, sizes[2])):
        image_ref.same_table(f"member {i}", group.image_table(i), image_ref.image_table(la, s, 4, L, 32, 0, 4096))
    group.close()
    for ev in members:
        ev.close()
    # what an evaluation refuses
    fpc64 = mpc.FPC(64)
    refused(mpc, lambda: snap.evaluate(fpc64, 128), "line size 64", "128")
    refused(mpc, lambda: snap.evaluate(fpc64, 96), "line size 64")
    fpc64.close()
    with pytest.raises(ValueError):
        snap.evaluate(None, 128)


def test_round_trip_by_presence(mpc, memory):
    """Units left out of the feed: with partial="zero" and by_presence the class table has one row per presence mask, with
    the lines and bits that the plain evaluator gives for the zero-filled lines of that mask."""
    L, U = memory["L"], memory["U"]
    rng = np.random.default_rng(62)
    mask_of_line = np.concatenate([np.arange(1, 16), rng.integers(1, 16, len(memory["la"]) - 15)])
    keep = (mask_of_line[:, None] >> np.arange(4)[None, :] & 1).astype(bool).reshape(-1)        # of the final units, in address order
    keep_fed = keep[memory["final_order"]]
    units, addrs = memory["fu"][memory["final_order"]][keep_fed], memory["fa"][memory["final_order"]][keep_fed]
    snap = mpc.Snapshot(U, 8192)
    snap.add(units, addrs)
    Z, la, pres = R.read(units, addrs, U, L, "zero")
    assert (pres == mask_of_line).all() and set(pres.tolist()) == set(range(1, 16))
    out = same("holes", snap, units, addrs, U, 8192, sizes=(L,))
    assert (out[L, "zero"][0] == Z).all()
    plain = mpc.BDI(L)
    sizes = plain.compress_lines(Z, want_selected=False)[0]
    plain.close()
    want_lines = np.bincount(pres, minlength=256)
    want_bits = np.bincount(pres, weights=sizes.astype(np.float64), minlength=256).astype(np.uint64)
    bdi = mpc.BDI(L)
    bdi.enable_class_stats(32)
    assert snap.evaluate(bdi, L, "zero", by_presence=True) == len(Z)
    cls = bdi.class_stats()
    assert (cls["lines"] == want_lines).all() and (cls["bits"] == want_bits).all() and int((cls["lines"] > 0).sum()) == 15
    bdi.reset()
    snap.evaluate(bdi, L, "zero")                                   # without by_presence: class 0
    cls = bdi.class_stats()
    assert int(cls["lines"][0]) == len(Z) and int(cls["lines"][1:].sum()) == 0
    bdi.reset()
    snap.evaluate(bdi, L, "skip", by_presence=True)                 # complete lines only: one row, mask 15
    cls = bdi.class_stats()
    assert int(cls["lines"][15]) == int((pres == 15).sum()) == int(cls["lines"].sum())
    bdi.close()
    members = [mpc.BDI(L), mpc.FPC(L)]
    group = mpc.EvaluatorSet(members)
    group.enable_class_stats(32)
    snap.evaluate(group, L, "zero", by_presence=True)
    cls = members[0].class_stats()
    assert (cls["lines"] == want_lines).all() and (cls["bits"] == want_bits).all()
    assert (members[1].class_stats()["lines"] == want_lines).all()
    group.close()
    for ev in members:
        ev.close()
    snap.close()


# ---- 10. the command line ---------------------------------------------------------------------------------------------
def test_cli_snapshot(mpc, cli, configs, traces, memory, tmp_path):
    import subprocess
    bindir = os.path.join(ROOT, "bin")
    L, U, X, la = memory["L"], memory["U"], memory["X"], memory["la"]
    ds = tmp_path / "ds"
    ds.mkdir()
    n = len(memory["addrs"])
    req_types = np.where(np.arange(n) % 5 == 0, 4, 0)
    log = patched_log(traces, str(ds / "t.log"), memory["units"], req_types, memory["addrs"])
    npy = traces.save_npy(str(ds / "x.npy"), np.concatenate([X, np.zeros((1, L), np.uint8)]))      # (the .npy loader drops the last row)
    cfg_path = str(tmp_path / "probe.json")
    with open(cfg_path, "w") as f:
        json.dump(configs.probe_config(L), f)
    cfg32 = str(tmp_path / "probe32.json")
    with open(cfg32, "w") as f:
        json.dump(configs.probe_config(32), f)

    def run(args, out, code=0):
        out.mkdir()
        r = subprocess.run([cli, *args, "-o", str(out)], cwd=bindir, capture_output=True, text=True, timeout=600)
        assert r.returncode == code, r.stdout + r.stderr
        return r.stdout

    def same_files(snap_dir, plain_dir, extra):
        for name in os.listdir(plain_dir):
            assert (snap_dir / name).read_text() == (plain_dir / name).read_text().replace("ds_x,", f"ds_t@snapshot{L},"), name
        assert sorted(set(os.listdir(snap_dir)) - set(os.listdir(plain_dir))) == sorted(extra)

    st = R.stats(memory["units"], memory["addrs"], U)
    row = R.csv_row(f"ds_t@snapshot{L}", U, L, "skip", st, R.plan(memory["units"], memory["addrs"], U, L))
    # one algorithm: the plain run over the ordered lines
    assert run(["-a", "BDI", "-i", log, "--snapshot", str(L)], tmp_path / "one") == run(["-a", "BDI", "-i", npy], tmp_path / "one_plain")
    same_files(tmp_path / "one", tmp_path / "one_plain", ["BDI_results_snapshot.csv"])
    assert (tmp_path / "one" / "BDI_results_snapshot.csv").read_text() == R.CSV_HEADER + row
    assert "BDI_results.csv" in os.listdir(tmp_path / "one_plain")
    # a list with every accounting next to it; the image takes the lines' own addresses
    names, stems = ("VPC", "BDI", "FPC"), ("probe", "BDI", "FPC")
    base = ["-a", ",".join(names), "-c", cfg_path]
    accounts = ["--size-histogram", "--sector", "32", "--pack", "4", "--by", "cluster"]
    stdout = run(base + ["-i", log, "--snapshot", str(L), "--snapshot-partial", "zero", "--snapshot-capacity", "8192", "--image", "4"] + accounts, tmp_path / "list")
    assert stdout == run(base + ["-i", npy] + accounts, tmp_path / "list_plain")
    same_files(tmp_path / "list", tmp_path / "list_plain", [f"{s}_results_{kind}.csv" for s in stems for kind in ("snapshot", "image")])
    assert all(f"{s}_results_{kind}.csv" in os.listdir(tmp_path / "list_plain") for s in stems + ("BEST",) for kind in ("sizes", "classes", "pack"))
    zero_row = row.replace(",skip,", ",zero,")                      # every line is complete: the same lines
    for name, stem in zip(names, stems):
        ev = mpc.VPC(configs.probe_config(L)) if name == "VPC" else getattr(mpc, name)(L)
        sizes = ev.compress_lines(X, want_selected=False)[0]
        ev.close()
        table = image_ref.image_table(la, sizes, 4, L, 32, 0, 1 << 24)
        assert (tmp_path / "list" / f"{stem}_results_image.csv").read_text() == image_ref.CSV_HEADER + image_ref.csv_row(f"ds_t@snapshot{L}", table, L), stem
        assert (tmp_path / "list" / f"{stem}_results_snapshot.csv").read_text() == R.CSV_HEADER + zero_row
    # the driver script hands the options on
    (tmp_path / "tree").mkdir()
    (tmp_path / "tree" / "split").mkdir()
    os.link(log, tmp_path / "tree" / "split" / "t.log")
    (tmp_path / "driven").mkdir()
    r = subprocess.run(["./run", "BDI", str(tmp_path / "tree"), str(tmp_path / "driven"), "--snapshot", str(L)], cwd=bindir, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert (tmp_path / "driven" / "BDI_results_snapshot.csv").read_text() == R.CSV_HEADER + row.replace("ds_t@", "split_t@")
    # refusals that need the evaluator or the snapshot: one message, exit status 1
    out = run(["-a", "VPC", "-c", cfg32, "-i", log, "--snapshot", str(L)], tmp_path / "bad_vpc", code=1)
    assert len(out.strip().splitlines()) == 1 and "--snapshot 128" in out and "32-byte lines" in out
    out = run(["-a", "BDI,VPC", "-c", cfg32, "-i", log, "--snapshot", str(L)], tmp_path / "bad_list", code=1)
    assert len(out.strip().splitlines()) == 1 and "32-byte lines" in out
    out = run(["-a", "BDI", "-i", log, "--snapshot", str(L), "--snapshot-capacity", "100"], tmp_path / "full", code=1)
    assert len(out.strip().splitlines()) == 1 and "more than 100 distinct unit addresses" in out
    assert os.listdir(tmp_path / "bad_vpc") == os.listdir(tmp_path / "bad_list") == os.listdir(tmp_path / "full") == []
