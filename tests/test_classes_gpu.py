"""Per-class accounting on the MI355X (csrc/mpc_classes.hip, include/mpc_hip_classes.h): every evaluator's lines, bits
and sector counts grouped by a class byte per line.  The expected table is tests/classes_ref.py (np.bincount and the
sector formula) over the sizes that a handle which never heard of classes returns for the same lines; every comparison
is equality of uint64 arrays."""
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, pkg

import classes_ref as R
import footprint as F

pytestmark = pytest.mark.gpu

MPC_E_INVAL = -22
NS = (1, 2, 63, 64, 65, 127, 128, 129, 511, 512, 513, 1025)      # up to 512 lines: in place; above: staged
# sectors so that several counts occur at every line size (32-byte lines: two sectors of 16 bytes; 8-byte lines: two of 4)
SECTOR = {8: 4, 32: 16, 64: 32, 128: 32, 256: 32}


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
        return mpc.SC2(L, 100, device=0)      # the table is built inside the sweep
    if comp == "Pattern":
        return mpc.Pattern(L)
    return getattr(mpc, comp)(L)


def line_mix(traces, L, n, seed=0):
    """Zeros, word-same, structured and random lines, permuted: several sector counts occur."""
    def gen(g, k, **kw):
        if L in (32, 64, 128):
            return g(k, L, **kw)
        wide = g(k, 128, **kw)
        return np.ascontiguousarray(wide[:, :L]) if L < 128 else np.ascontiguousarray(np.hstack([wide, wide[::-1]]))
    k = -(-n // 10)
    pool = np.concatenate([gen(traces.zeros, k), gen(traces.word_same, k), gen(traces.structured, 5 * k, seed=5), gen(traces.random_u32, 3 * k)])
    return np.ascontiguousarray(pool[np.random.default_rng(L + seed).permutation(len(pool))][:n])


def same(tag, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (tag, got.shape, want.shape, got.dtype, want.dtype)
    bad = np.nonzero(got.reshape(-1) != want.reshape(-1))[0]
    assert bad.size == 0, f"{tag}: {bad.size} of {got.size} differ, first at {bad[:6].tolist()}"


# ---- 1. sizes and patterns -------------------------------------------------------------------------------------------
CASES = [(c, L) for c in ("BDI", "FPC", "BPC", "CPACK", "SC2", "Pattern", "VPC") for L in (32, 64, 128)] + [("BDI", 8), ("BDI", 256)]


@pytest.mark.parametrize("comp,L", CASES, ids=[f"{c}-{L}" for c, L in CASES])
def test_sizes_and_patterns(mpc, configs, traces, comp, L):
    sb = SECTOR[L]
    plain, ev = make(mpc, configs, comp, L), make(mpc, configs, comp, L)
    ev.enable_class_stats(sb)
    ev.enable_class_stats(sb)      # idempotent
    assert ev.class_sector_bytes() == sb
    pool = line_mix(traces, L, 2 * max(NS))
    want = np.zeros((R.CLASSES, R.ROW), np.uint64)
    seen_sectors = set()
    for n in NS:
        lines = pool[n % 7: n % 7 + n]
        for name, classes in R.class_patterns(n).items():
            s0, k0 = plain.compress_lines(lines)
            s1, k1 = ev.compress_lines(lines, classes=classes)
            same(f"{comp} L={L} n={n} {name}: sizes", s1, s0)
            same(f"{comp} L={L} n={n} {name}: selected", k1, k0)
            want += R.class_table(classes, s0, L, sb)
            R.same_table(f"{comp} L={L} n={n} {name}", ev.class_table(), want)
            seen_sectors |= set(R.sectors_of(s0, L, sb).tolist())
    assert len(seen_sectors) >= 2, seen_sectors
    same("statistics", ev.stats_vector(), plain.stats_vector())
    stats = ev.class_stats()
    S = -(-L // sb)
    same("lines", stats["lines"], want[:, 0])
    same("bits", stats["bits"], want[:, 1])
    same("sectors", stats["sectors"], want[:, 2:2 + S])
    plain.close()
    ev.close()


# ---- 2. many workgroups ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,n", [(32, 100003), (128, 20001)])
def test_many_workgroups(mpc, traces, L, n):
    sb = SECTOR[L]
    pool = line_mix(traces, L, 4096)
    lines = np.ascontiguousarray(pool[np.random.default_rng(9).integers(0, len(pool), n)])
    plain, ev = mpc.BDI(L), mpc.BDI(L)
    ev.enable_class_stats(sb)
    s0, _ = plain.compress_lines(lines, want_selected=False)
    want = np.zeros((R.CLASSES, R.ROW), np.uint64)
    for name, classes in (("random", np.random.default_rng(n).integers(0, 256, n, dtype=np.uint8)), ("one class", np.full(n, 5, np.uint8))):
        s1, _ = ev.compress_lines(lines, want_selected=False, classes=classes)
        same(name, s1, s0)
        want += R.class_table(classes, s0, L, sb)
        R.same_table(f"L={L} n={n} {name}", ev.class_table(), want)
    # the stager provides the sizes when the caller does not ask for them
    ev.compress_lines(lines, want_sizes=False, want_selected=False, classes=np.full(n, 5, np.uint8))
    want += R.class_table(np.full(n, 5), s0, L, sb)
    R.same_table(f"L={L} n={n} not asked", ev.class_table(), want)
    plain.close()
    ev.close()


# ---- 3. the device path's footprint ----------------------------------------------------------------------------------
class Classed:
    """An evaluator whose device calls carry the class array at `p_classes` (what footprint.check_call drives)."""

    def __init__(self, ev, p_classes):
        self.ev, self.p_classes, self.line_size = ev, p_classes, ev.line_size

    def compress_device(self, d_lines, n, d_sizes=0, d_selected=0, stream=0):
        self.ev.compress_device(d_lines, n, d_sizes, d_selected, stream, classes=self.p_classes)

    def sync(self):
        self.ev.sync()

    def stats_vector(self):
        return self.ev.stats_vector()


CLASS_CANARY = 0x77


@pytest.mark.parametrize("L", [32, 64])
def test_device_path_footprint(mpc, oracle, traces, L):
    """Lines 16 bytes into their buffer, with and without the caller's sizes array; the class array at an odd and at an
    8-byte aligned address inside a tensor of canaries: a class byte read outside the n asked for would count in row
    0x77, a line or a size outside shows in the checks of tests/footprint.py."""
    import torch
    sb = SECTOR[L]
    ev = mpc.BDI(L)
    ev.enable_class_stats(sb)
    ref = F.OracleRef(oracle.BdiOracle(L))
    pool = F.line_pool(traces, L)
    want = np.zeros((R.CLASSES, R.ROW), np.uint64)
    for n in (1, 7, 8, 63, 65, 129, 513, 1025):
        lines = pool[:n]
        sizes = oracle.BdiOracle(L).compress(lines)[0]
        for start in (F.OUT_START, F.OUT_MARGIN):
            classes = np.random.default_rng(n + start).integers(0, 256, n, dtype=np.uint8)
            classes[classes == CLASS_CANARY] = 0
            host = np.full(F.OUT_MARGIN + 1 + n + F.OUT_MARGIN, CLASS_CANARY, np.uint8)
            host[start:start + n] = classes
            d_cls = torch.from_numpy(host).to("cuda:0")
            assert d_cls.data_ptr() % 256 == 0
            target = Classed(ev, d_cls.data_ptr() + start)
            for mode in ("both", "sel only", "none", "sizes only"):
                F.check_call(target, [ref], lines, off=16, mode=mode, poison=0xF007, tag=f"classed start={start}")
                want += R.class_table(classes, sizes, L, sb)
                R.same_table(f"L={L} n={n} start={start} {mode}", ev.class_table(), want)
            same("the class tensor", d_cls.cpu().numpy(), host)
    assert int(want[CLASS_CANARY].sum()) == 0
    ev.close()


def test_device_path_pieces_share_the_sizes_scratch(mpc, traces):
    """More than 4 Mi lines without the caller's sizes array: pieces of 4 Mi lines, classes offset per piece; the size
    histogram and the class table come from the same pieces."""
    import torch
    L, sb = 32, 16
    n = (4 << 20) + 777
    pool = line_mix(traces, L, 4096)
    idx = torch.randint(0, len(pool), (n,), device="cuda:0", generator=torch.Generator(device="cuda:0").manual_seed(1))
    d_lines = torch.from_numpy(pool).to("cuda:0")[idx].contiguous()
    d_cls = ((torch.arange(n, device="cuda:0") >> 12) & 255).to(torch.uint8)
    d_sizes = torch.zeros(n, dtype=torch.int16, device="cuda:0")
    plain, ev = mpc.BDI(L), mpc.BDI(L)
    plain.compress_device(d_lines.data_ptr(), n, d_sizes.data_ptr())
    plain.sync()
    sizes = d_sizes.cpu().numpy().view(np.uint16)
    ev.enable_class_stats(sb)
    ev.enable_size_histogram()
    ev.compress_device(d_lines.data_ptr(), n, classes=d_cls.data_ptr())
    R.same_table("pieces", ev.class_table(), R.class_table(d_cls.cpu().numpy(), sizes, L, sb))
    same("histogram", ev.size_histogram(), np.bincount(sizes, minlength=4096).astype(np.uint64))
    same("statistics", ev.stats_vector(), plain.stats_vector())
    plain.close()
    ev.close()


# ---- 4. groups -------------------------------------------------------------------------------------------------------
GROUP = ("VPC", "BDI", "FPC", "BPC", "CPACK")


def test_group_members_and_best(mpc, configs, traces):
    L, sb = 64, 32
    plain = [make(mpc, configs, c, L) for c in GROUP]
    members = [make(mpc, configs, c, L) for c in GROUP]
    group = mpc.EvaluatorSet(members)
    group.enable_class_stats(sb)
    group.enable_best()            # after the class accounting: the best-of's table appears with it
    pool = line_mix(traces, L, 6000)
    want = [np.zeros((R.CLASSES, R.ROW), np.uint64) for _ in range(len(GROUP) + 1)]
    for n, name in ((3000, "random"), (300, "runs of 65"), (513, "i % 256")):
        lines = pool[n:2 * n]
        classes = R.class_patterns(n)[name]
        sizes0 = [p.compress_lines(lines)[0] for p in plain]
        out = group.compress_lines(lines, classes=classes)
        for i in range(len(GROUP)):
            same(f"{GROUP[i]} sizes", out[i][0], sizes0[i])
            want[i] += R.class_table(classes, sizes0[i], L, sb)
        want[-1] += R.class_table(classes, np.min(np.stack(sizes0), axis=0), L, sb)
        stats = group.class_stats()
        assert sorted(stats, key=str) == [0, 1, 2, 3, 4, "best"]
        for i in range(len(GROUP)):
            R.same_table(f"{GROUP[i]} n={n}", group.class_table(i), want[i])
            R.same_table(f"{GROUP[i]} n={n}, the member's own get", members[i].class_table(), want[i])
            same("lines", stats[i]["lines"], want[i][:, 0])
        R.same_table(f"best n={n}", group.class_table(mpc.MPC_CLASS_BEST), want[-1])
        same("best bits", stats["best"]["bits"], want[-1][:, 1])
    # a call without classes: class 0
    lines = pool[:700]
    sizes0 = [p.compress_lines(lines)[0] for p in plain]
    group.compress_lines(lines, want_sizes=False, want_selected=False)
    for i in range(len(GROUP)):
        want[i] += R.class_table(np.zeros(700, np.uint8), sizes0[i], L, sb)
        R.same_table(f"{GROUP[i]} un-classed", group.class_table(i), want[i])
    for i, p in enumerate(plain):
        same(f"{GROUP[i]} statistics", members[i].stats_vector(), p.stats_vector())
    group.close()
    for e in plain + members:
        e.close()


def test_group_class_from_member(mpc, configs, traces):
    import torch
    L, sb = 64, 32
    plain = [make(mpc, configs, c, L) for c in GROUP]
    members = [make(mpc, configs, c, L) for c in GROUP]
    group = mpc.EvaluatorSet(members)
    group.enable_best()
    group.enable_class_stats(sb)   # after the best-of
    group.class_from_member(0)
    pool = line_mix(traces, L, 6000, seed=3)
    want = [np.zeros((R.CLASSES, R.ROW), np.uint64) for _ in range(len(GROUP) + 1)]

    def expect(lines):
        res = [p.compress_lines(lines) for p in plain]
        classes = R.classes_of_selected(res[0][1])
        for i in range(len(GROUP)):
            want[i] += R.class_table(classes, res[i][0], L, sb)
        want[-1] += R.class_table(classes, np.min(np.stack([r[0] for r in res]), axis=0), L, sb)

    def check(tag):
        for i in range(len(GROUP)):
            R.same_table(f"{tag}: {GROUP[i]}", group.class_table(i), want[i])
        R.same_table(f"{tag}: best", group.class_table(mpc.MPC_CLASS_BEST), want[-1])
        v, K = members[0].stats_vector(), members[0].num_modules + 1
        clusters = np.array([v[3 + 6 * k] for k in range(K)], np.uint64)
        for i in range(len(GROUP)):
            same(f"{tag}: {GROUP[i]} column 0 against the VPC cluster counts", group.class_table(i)[:K, 0], clusters)
            assert int(group.class_table(i)[K:, 0].sum()) == 0

    for n, asked in ((3000, True), (2000, False), (400, False), (512, True)):      # staged and in place, selected asked for or not
        lines = pool[n:2 * n]
        expect(lines)
        group.compress_lines(lines, want_sizes=asked, want_selected=asked)
        check(f"host n={n} asked={asked}")
    assert len(np.nonzero(want[0][:, 0])[0]) >= 3      # several clusters took lines
    # device path: nobody's arrays (scratch sizes and a scratch selected), then the VPC member's own selected array
    n = 5000
    lines = pool[:n]
    d_lines = torch.from_numpy(lines).to("cuda:0")
    expect(lines)
    group.compress_device(d_lines.data_ptr(), n)
    check("device, no arrays")
    d_sel = torch.full((n,), 90, dtype=torch.int8, device="cuda:0")
    expect(lines)
    group.compress_device(d_lines.data_ptr(), n, None, [d_sel.data_ptr(), 0, 0, 0, 0])
    check("device, the member's selected array")
    same("selected", d_sel.cpu().numpy(), plain[0].compress_lines(lines)[1])
    plain[0].reset()
    # the classes come from the member: a call must not bring its own
    with pytest.raises(mpc.MpcError) as e:
        group.compress_lines(lines, classes=np.zeros(n, np.uint8))
    assert e.value.code == MPC_E_INVAL and "member 0" in str(e.value)
    # and off again
    group.class_from_member(None)
    before = group.class_table(1)
    group.compress_lines(lines[:100], classes=np.full(100, 9, np.uint8))
    assert int(group.class_table(1)[9, 0]) == int(before[9, 0]) + 100
    group.close()
    for e in plain + members:
        e.close()


# ---- 5. classes from a .log -------------------------------------------------------------------------------------------
def test_log_fields_more_than_one_slot(mpc, traces, tmp_path):
    """BDI at 32 bytes over a .log of more kept records than one staging slot holds (2 Mi lines of 32 bytes), with
    request types other than GLOBAL_ACC_R / GLOBAL_ACC_W mixed in."""
    L, sb = 32, 16
    stage_lines = (64 << 20) // L
    n = stage_lines + 200_000
    rng = np.random.default_rng(11)
    pool = line_mix(traces, L, 4096)
    lines = pool[rng.integers(0, len(pool), n)]
    req_types = rng.choice(np.array([0, 4, 1, 2, 5, 8], np.uint32), n, p=[0.5, 0.44, 0.02, 0.02, 0.01, 0.01])
    log = traces.write_gpgpusim_log(str(tmp_path / "t.log"), lines, req_types)
    kid, mftype, rt, payload = R.log_fields(log, L)
    keep = (rt == 0) | (rt == 4)
    assert keep.sum() > stage_lines and (~keep).sum() > 1000 and len(np.unique(kid[keep])) > 1
    plain = mpc.BDI(L)
    sizes = plain.compress_lines(payload[keep], want_selected=False)[0]
    plain.close()
    ev = mpc.BDI(L)
    ev.enable_class_stats(sb)
    for field, classes in (("kernel", kid[keep]), ("rw", (rt[keep] == 4).astype(np.uint8)), ("mftype", mftype[keep]), (None, np.zeros(keep.sum(), np.uint8))):
        ev.class_log_field(field)
        assert ev.compress_gpgpusim_log(log) == (n, int(keep.sum()))
        R.same_table(f".log by {field}", ev.class_table(), R.class_table(classes, sizes, L, sb))
        ev.reset()
    ev.close()


def test_log_fields_group(mpc, traces, tmp_path):
    L, sb, n = 64, 32, 3000
    lines = line_mix(traces, L, n)
    req_types = np.where(np.arange(n) % 5 == 0, 4, np.where(np.arange(n) % 11 == 0, 3, 0))
    log = traces.write_gpgpusim_log(str(tmp_path / "g.log"), lines, req_types)
    kid, mftype, rt, payload = R.log_fields(log, L)
    keep = (rt == 0) | (rt == 4)
    members = [mpc.BDI(L), mpc.FPC(L)]
    group = mpc.EvaluatorSet(members)
    group.enable_class_stats(sb)
    group.class_log_field("kernel")
    assert group.compress_gpgpusim_log(log) == (n, int(keep.sum()))
    for i, p in enumerate((mpc.BDI(L), mpc.FPC(L))):
        sizes = p.compress_lines(payload[keep], want_selected=False)[0]
        R.same_table(f"member {i}", group.class_table(i), R.class_table(kid[keep], sizes, L, sb))
        p.close()
    group.close()
    for e in members:
        e.close()


# ---- 6. additivity and the off state ---------------------------------------------------------------------------------
@pytest.mark.parametrize("comp", ["VPC", "BDI", "FPC", "BPC", "CPACK", "SC2", "Pattern"])
def test_additivity_and_the_off_state(mpc, configs, traces, comp):
    L, sb = 64, 32
    a, b = make(mpc, configs, comp, L), make(mpc, configs, comp, L)
    pool = line_mix(traces, L, 4000)
    first, second = pool[:700], pool[700:1300]
    # off: b is a handle like any other
    ra, rb = a.compress_lines(first), b.compress_lines(first)
    same("off: sizes", rb[0], ra[0]); same("off: selected", rb[1], ra[1]); same("off: statistics", b.stats_vector(), a.stats_vector())
    with pytest.raises(mpc.MpcError):
        b.class_table()
    # enabling changes neither
    b.enable_class_stats(sb)
    same("enabled: statistics", b.stats_vector(), a.stats_vector())
    assert int(b.class_table().sum()) == 0          # only lines from now on
    ra, rb = a.compress_lines(second), b.compress_lines(second)          # un-classed: class 0
    same("on: sizes", rb[0], ra[0]); same("on: selected", rb[1], ra[1]); same("on: statistics", b.stats_vector(), a.stats_vector())
    t1 = R.class_table(np.zeros(600, np.uint8), ra[0], L, sb)
    R.same_table("un-classed calls land in class 0", b.class_table(), t1)
    # two calls add
    classes = R.class_patterns(500)["random"]
    third = pool[1300:1800]
    ra, rb = a.compress_lines(third), b.compress_lines(third, classes=classes)
    t2 = t1 + R.class_table(classes, ra[0], L, sb)
    R.same_table("two calls add", b.class_table(), t2)
    # merge adds, and the device table stays what it was
    b.class_stats_merge(t2)
    R.same_table("merge adds", b.class_table(), 2 * t2)
    same("merge: statistics", b.stats_vector(), a.stats_vector())
    # reset clears the table, the merged part included
    b.reset()
    a.reset()
    assert int(b.class_table().sum()) == 0
    ra, rb = a.compress_lines(first[:50]), b.compress_lines(first[:50], classes=np.full(50, 77, np.uint8))
    R.same_table("after reset", b.class_table(), R.class_table(np.full(50, 77), ra[0], L, sb))
    a.close()
    b.close()


# ---- 7. refusals -----------------------------------------------------------------------------------------------------
def refused(mpc, call, *words):
    with pytest.raises(mpc.MpcError) as e:
        call()
    assert e.value.code == MPC_E_INVAL and all(w in str(e.value) for w in words), str(e.value)


def test_refusals(mpc, traces):
    L = 64
    lines = line_mix(traces, L, 100)
    for fit in (mpc.FitPairs(L), mpc.FitResidues(L, list(range(L)))):
        refused(mpc, lambda: fit.enable_class_stats(32), "Fit")
        fit.close()
    ev = mpc.BDI(L)
    refused(mpc, lambda: ev.compress_lines(lines, classes=np.zeros(100, np.uint8)), "mpc_class_stats_enable")
    refused(mpc, lambda: ev.class_log_field("rw"), "mpc_class_stats_enable")
    refused(mpc, lambda: ev.class_stats())
    refused(mpc, lambda: ev.class_stats_merge(np.zeros(2560, np.uint64)), "mpc_class_stats_enable")
    assert ev.stats_vector()[0] == 0                       # a refused call evaluates nothing
    for sb in (0, L + 1, 7):                               # 0, above the line, ceil(64 / 7) = 10 sectors
        refused(mpc, lambda: ev.enable_class_stats(sb), "sector")
    wide = mpc.BDI(128)
    refused(mpc, lambda: wide.enable_class_stats(8), "8 sectors")
    wide.enable_class_stats(16)                            # exactly 8
    wide.close()
    ev.enable_class_stats(32)
    refused(mpc, lambda: ev.enable_class_stats(16), "32")   # another sector size on a handle that counts
    t = np.zeros(2559, np.uint64)
    assert mpc.lib().mpc_class_stats_get(ev._h, t.ctypes.data, 2559) == MPC_E_INVAL
    assert mpc.lib().mpc_class_stats_merge(ev._h, t.ctypes.data, 2559) == MPC_E_INVAL
    assert mpc.lib().mpc_class_log_field(ev._h, 4) == MPC_E_INVAL
    members = [mpc.VPC(pkg("configs").probe_config(L)), mpc.FPC(L), mpc.BDI(L)]
    group = mpc.EvaluatorSet(members)
    refused(mpc, lambda: group.compress_lines(lines, classes=np.zeros(100, np.uint8)), "mpc_group_class_stats_enable")
    refused(mpc, lambda: group.class_from_member(0), "mpc_group_class_stats_enable")
    refused(mpc, lambda: group.class_stats())
    refused(mpc, lambda: group.enable_class_stats(0), "sector")
    group.enable_class_stats(32)
    refused(mpc, lambda: group.class_from_member(1), "FPC")
    refused(mpc, lambda: group.class_from_member(3), "member")
    refused(mpc, lambda: group.class_table(mpc.MPC_CLASS_BEST), "mpc_group_best_enable")
    assert mpc.lib().mpc_group_class_stats_get(group._g, 0, t.ctypes.data, 2559) == MPC_E_INVAL
    group.class_from_member(2)                             # a BDI member: its state + 1
    out = group.compress_lines(lines)
    R.same_table("BDI states as classes", group.class_table(1), R.class_table(R.classes_of_selected(out[2][1]), out[1][0], L, 32))
    group.close()
    for e in members + [ev]:
        e.close()


# ---- 8. one large case -----------------------------------------------------------------------------------------------
def test_large_device_batch(mpc):
    """2^27 + 12 345 lines of 32 bytes (more than 2^32 bytes) from mpc_synth_fill, BDI, classes (i >> 20) & 255 made on
    the device; against a torch reduction, on the device, of the sizes the same call returned."""
    import torch
    L, sb = 32, 16
    n = (1 << 27) + 12345
    dev = "cuda:0"
    try:
        buf = torch.empty(n * L, dtype=torch.uint8, device=dev)
        d_sizes = torch.zeros(n, dtype=torch.int16, device=dev)
    except RuntimeError as e:
        pytest.fail(f"cannot allocate the {n * L} byte buffer: {e}")
    mpc.synth_fill(buf.data_ptr(), n, L, "mixed")
    d_cls = ((torch.arange(n, device=dev, dtype=torch.int32) >> 20) & 255).to(torch.uint8)
    torch.cuda.synchronize()
    ev = mpc.BDI(L)
    ev.enable_class_stats(sb)
    ev.compress_device(buf.data_ptr(), n, d_sizes.data_ptr(), classes=d_cls.data_ptr())
    got = ev.class_table()
    sizes = d_sizes.to(torch.int32) & 0xffff
    cls = d_cls.to(torch.int64)
    sec = torch.clamp((sizes + (8 * sb - 1)) // (8 * sb), 1, L // sb).to(torch.int64)
    want = np.zeros((R.CLASSES, R.ROW), np.uint64)
    want[:, 0] = torch.bincount(cls, minlength=256).cpu().numpy()
    want[:, 1] = torch.zeros(256, dtype=torch.int64, device=dev).index_add_(0, cls, sizes.to(torch.int64)).cpu().numpy()
    want[:, 2:2 + L // sb] = torch.bincount(cls * (L // sb) + sec - 1, minlength=256 * (L // sb)).reshape(256, L // sb).cpu().numpy()
    R.same_table("2^27 + 12345 lines", got, want)
    assert int(got[:, 0].sum()) == n == int(ev.stats_vector()[0]) and int(got[:, 1].sum()) == int(ev.stats_vector()[2])
    assert (got[:128, 0] == 1 << 20).all() and int(got[128, 0]) == 12345
    ev.close()
    del buf, d_sizes, d_cls, sizes, cls, sec
    torch.cuda.empty_cache()


# ---- 9. the command line ---------------------------------------------------------------------------------------------
def fmt_double(x):
    r = repr(float(x))
    return r[:-2] if r.endswith(".0") else r


def csv_text(workload, table, L, sb):
    most = -(-L // sb)
    text = "Workload,Class,Lines,Original Bits,Compressed Bits,Ratio,Sector Ratio,\n"
    for c in range(256):
        lines, bits = int(table[c, 0]), int(table[c, 1])
        if not lines:
            continue
        occupied = sum(k * int(table[c, 1 + k]) for k in range(1, most + 1))
        text += (f"{workload},{c},{lines},{lines * 8 * L},{bits},{fmt_double(lines * 8 * L / bits) if bits else '0'},"
                 f"{fmt_double(lines * most / occupied)},\n")
    return text


def test_cli_by(mpc, configs, traces, tmp_path):
    pkg("build").build_all()
    bindir = os.path.join(ROOT, "bin")
    cli = os.path.join(bindir, "compressor")
    L, n = 64, 3001
    lines = line_mix(traces, L, n, seed=8)
    ds = tmp_path / "ds"
    ds.mkdir()
    req_types = np.where(np.arange(n) % 3 == 0, 4, np.where(np.arange(n) % 17 == 0, 2, 0))
    log = traces.write_gpgpusim_log(str(ds / "t.log"), lines, req_types)
    npy = traces.save_npy(str(ds / "t.npy"), lines)
    cfg_path = str(tmp_path / "probe.json")
    with open(cfg_path, "w") as f:
        json.dump(configs.probe_config(L), f)

    def run(args, out):
        out.mkdir()
        r = subprocess.run([cli, *args, "-o", str(out)], cwd=bindir, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        return r.stdout

    def group_tables(feed, setup):
        members = [mpc.VPC(configs.probe_config(L)), mpc.BDI(L)]
        group = mpc.EvaluatorSet(members)
        group.enable_best()
        group.enable_class_stats(32)
        setup(group)
        feed(group)
        tables = [group.class_table(0), group.class_table(1), group.class_table(mpc.MPC_CLASS_BEST)]
        group.close()
        for e in members:
            e.close()
        return tables

    # a list over a .log, by read / write, with the size histogram: every member's file and the best of the list
    base = ["-a", "VPC,BDI", "-c", cfg_path, "-i", log]
    plain_stdout = run(base + ["--size-histogram"], tmp_path / "rw_plain")
    stdout = run(base + ["--by", "rw", "--size-histogram"], tmp_path / "rw")
    assert stdout == plain_stdout
    for name in os.listdir(tmp_path / "rw_plain"):
        assert (tmp_path / "rw" / name).read_bytes() == (tmp_path / "rw_plain" / name).read_bytes(), name
    stems = ["probe", "BDI", "BEST"]
    assert sorted(set(os.listdir(tmp_path / "rw")) - set(os.listdir(tmp_path / "rw_plain"))) == sorted(f"{s}_results_classes.csv" for s in stems)
    tables = group_tables(lambda g: g.compress_gpgpusim_log(log), lambda g: g.class_log_field("rw"))
    assert int(tables[1][0, 0]) > 0 and int(tables[1][1, 0]) > 0 and int(tables[1][2:, 0].sum()) == 0
    for stem, table in zip(stems, tables):
        assert (tmp_path / "rw" / f"{stem}_results_classes.csv").read_text() == csv_text("ds_t", table, L, 32), stem
    # without the size histogram: no best of the list
    run(base + ["--by", "kernel"], tmp_path / "kernel")
    assert sorted(f for f in os.listdir(tmp_path / "kernel") if f.endswith("_classes.csv")) == ["BDI_results_classes.csv", "probe_results_classes.csv"]
    # one algorithm, another sector size
    run(["-a", "BDI", "-i", log, "--by", "mftype", "--sector", "16"], tmp_path / "one")
    ev = mpc.BDI(L)
    ev.enable_class_stats(16)
    ev.class_log_field("mftype")
    ev.compress_gpgpusim_log(log)
    assert (tmp_path / "one" / "BDI_results_classes.csv").read_text() == csv_text("ds_t", ev.class_table(), L, 16)
    ev.close()
    # by cluster on an .npy (the driver drops the final row)
    base = ["-a", "VPC,BDI", "-c", cfg_path, "-i", npy]
    plain_stdout = run(base, tmp_path / "cluster_plain")
    assert run(base + ["--by", "cluster"], tmp_path / "cluster") == plain_stdout
    for name in os.listdir(tmp_path / "cluster_plain"):
        assert (tmp_path / "cluster" / name).read_bytes() == (tmp_path / "cluster_plain" / name).read_bytes(), name
    tables = group_tables(lambda g: g.compress_lines(lines[:-1], want_sizes=False, want_selected=False), lambda g: g.class_from_member(0))
    assert len(np.nonzero(tables[1][:, 0])[0]) >= 3
    for stem, table in zip(stems[:2], tables[:2]):
        assert (tmp_path / "cluster" / f"{stem}_results_classes.csv").read_text() == csv_text("ds_t", table, L, 32), stem

