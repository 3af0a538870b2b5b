"""Pack accounting on the MI355X (csrc/mpc_pack.hip, include/mpc_hip_pack.h): the sectors that blocks of N consecutive
lines occupy, for every evaluator, through every ingestion path.  The expected table is tests/pack_ref.py (numpy over
per-line sizes) over the sizes that a handle or group WITHOUT pack accounting returns for the same lines; every
comparison is equality of uint64 arrays.

The traces are runs of all-zero lines and of random lines, each longer than two of the largest blocks, followed by a
mix of all-zero, word-same, small-integer and random lines in which the share of all-zero lines falls from all to none
along the trace: blocks differ, long ones too, and before it compares each test
asserts on the reference's numbers that its closed blocks cover at least three distinct sector counts, the count 1,
the cap S_B with an uncapped count above it, and -- over a sweep of header_bits chosen from the reference sizes -- a
block of exactly 8 sector_bytes k bits and one of that + 1."""
import numpy as np
import pytest

from conftest import pkg

import pack_ref as R

pytestmark = pytest.mark.gpu

MPC_E_INVAL = -22
ALL_N = (1, 2, 3, 5, 16, 31, 32, 33, 63, 64, 65, 100, 1000)
# ... and where the kernel takes another form: a lane up to 32 lines, a wave up to 511, a workgroup above
FORM_N = (511, 512)
RUN = 2100          # lines of the all-zero and of the random run: two blocks of 1000 lines and more
EXCEED_8L = ("BDI", "FPC", "BPC", "CPACK")      # on random lines their size is above 8 L bits


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


def small_ints(n, L, seed):
    return np.random.default_rng(seed).integers(0, 200, (n, L // 4), dtype=np.uint32).view(np.uint8).reshape(n, L)


def trace(traces, L, n, seed=0):
    """[RUN zeros | RUN random | a mix of zeros, word-same, small-integer and random lines], n lines.  In the mix line i
    of m is all-zero with probability 1 - i / m and else one of the other three kinds, so that blocks of 1000 lines
    differ as blocks of a few lines do."""
    m = n - 2 * RUN
    rng = np.random.default_rng(100 + L + seed)
    kinds = np.stack([traces.word_same(m, L), small_ints(m, L, seed + 1), traces.random_u32(m, L, first_line=RUN)])
    mix = kinds[rng.integers(0, 3, m), np.arange(m)]
    mix[rng.random(m) >= np.arange(m) / m] = 0
    return np.ascontiguousarray(np.concatenate([traces.zeros(RUN, L), traces.random_u32(RUN, L), mix]))


def coarse_sector(N, L, parts=4):
    """S_B = parts: with 4 an all-zero block is one sector for every evaluator but Pattern (its value for an all-zero
    line is above 2 L bits at 32 and 64 bytes, and below 4 L: 2 parts); no power of two in general."""
    return N * L // parts


def fine_sector(N, L):
    """The smallest power of two (from 4 bytes) that keeps S_B <= 1024."""
    sb = 4
    while N * L > 1024 * sb:
        sb *= 2
    return sb


def runs_for(sizes, N, L, parts=4):
    """The (sector_bytes, header_bits) a test counts these sizes with: `parts` sectors a block without a header, and
    many sectors a block with two header_bits chosen from the reference sizes, the second one more than the first."""
    fine = fine_sector(N, L)
    pair = R.boundary_headers(sizes, N, L, fine)
    assert pair is not None, (N, L, fine)
    return [(coarse_sector(N, L, parts), 0), (fine, pair[0]), (fine, pair[1])]


def assert_coverage(tag, sizes, N, L, runs, exceeds=True):
    """On the reference's numbers: what the closed blocks of the test's runs cover between them."""
    cov = [(R.block_sectors(N, L, sb), R.coverage(sizes, N, L, sb, hb)) for sb, hb in runs]
    assert any(len(c["counts"]) >= 3 for _, c in cov), (tag, "three distinct sector counts")
    assert any(1 in c["counts"] for _, c in cov), (tag, "the count 1")
    assert any(S in c["counts"] and (c["capped_above"] or not exceeds) for S, c in cov), (tag, "the cap, with an uncapped count above it")
    assert any(c["exact"] for _, c in cov) and any(c["plus_one"] for _, c in cov), (tag, "8 sector_bytes k bits exactly, and one more", runs)


def run_packed(mpc, configs, comp, L, lines, N, sb, hb):
    ev = make(mpc, configs, comp, L)
    ev.enable_pack_stats(N, sb, hb)
    ev.enable_pack_stats(N, sb, hb)      # idempotent
    ev.compress_lines(lines, want_sizes=False, want_selected=False)
    t = ev.pack_table()
    stats = ev.stats_vector()
    ev.close()
    return t, stats


# ---- 1. every N on every evaluator -----------------------------------------------------------------------------------
CASES = [(c, L) for c in ("BDI", "FPC", "BPC", "CPACK", "SC2", "Pattern", "VPC") for L in (32, 64, 128)]


@pytest.mark.parametrize("comp,L", CASES, ids=[f"{c}-{L}" for c, L in CASES])
def test_every_block_size(mpc, configs, traces, comp, L):
    lines = trace(traces, L, 20000)
    plain = make(mpc, configs, comp, L)
    sizes = plain.compress_lines(lines, want_selected=False)[0]
    want_stats = plain.stats_vector()
    plain.close()
    for N in ALL_N + (FORM_N if L == 32 else ()):
        runs = runs_for(sizes, N, L, 2 if comp == "Pattern" else 4)
        assert_coverage(f"{comp} L={L} N={N}", sizes, N, L, runs, comp in EXCEED_8L)
        for sb, hb in runs:
            got, stats = run_packed(mpc, configs, comp, L, lines, N, sb, hb)
            R.same_table(f"{comp} L={L} N={N} sector={sb} header={hb}", got, R.pack_table(sizes, N, L, sb, hb))
            assert (stats == want_stats).all()


def test_one_line_blocks_are_the_size_histogram(mpc, traces):
    L = 64
    lines = trace(traces, L, 6000)
    for sb in (16, 32, 64):
        ev = mpc.FPC(L)
        ev.enable_pack_stats(1, sb, 0)
        ev.enable_size_histogram()
        ev.compress_lines(lines, want_sizes=False, want_selected=False)
        sectors = mpc.size_sectors(ev.size_histogram(), L, sb)
        stats = ev.pack_stats()
        assert (stats["histogram"] == sectors["classes"]).all() and stats["sectors"] == sectors["total_sectors"]
        assert stats["blocks"] == 6000 and stats["open_lines"] == 0 and stats["sector_ratio"] == sectors["ratio"]
        ev.close()


# ---- 2. call seams ---------------------------------------------------------------------------------------------------
def feed_and_check(tag, ev, lines, sizes, cuts, N, L, sb, hb):
    at = 0
    for n in cuts:
        ev.compress_lines(lines[at:at + n], want_sizes=False, want_selected=False)
        at += n
        R.same_table(f"{tag}: after {at} lines", ev.pack_table(), R.pack_table(sizes[:at], N, L, sb, hb))
    assert at == len(lines)


def cuts_of(total, lengths):
    out, at, i = [], 0, 0
    while at < total:
        out.append(min(lengths[i % len(lengths)], total - at))
        at += out[-1]
        i += 1
    return out


@pytest.mark.parametrize("N", [7, 1000])
def test_call_seams(mpc, traces, N):
    L = 64
    lines = trace(traces, L, 20000, seed=2)
    plain = mpc.BPC(L)
    sizes = plain.compress_lines(lines, want_selected=False)[0]
    plain.close()
    runs = runs_for(sizes, N, L)
    assert_coverage(f"N={N}", sizes, N, L, runs)
    rng = np.random.default_rng(N)
    feeds = {"one call": [20000], "511, 512, 513": cuts_of(20000, [511, 512, 513]),
             "drawn lengths": cuts_of(20000, rng.integers(1, 1500, 400).tolist())}
    for sb, hb in runs:
        for name, cuts in feeds.items():
            ev = mpc.BPC(L)
            ev.enable_pack_stats(N, sb, hb)
            feed_and_check(f"N={N} sector={sb} header={hb} {name}", ev, lines, sizes, cuts, N, L, sb, hb)
            ev.close()


def test_call_seams_line_by_line(mpc, traces):
    """Calls of one line with N = 1000: almost every launch lies inside a block."""
    L, N, n = 64, 1000, 2600
    lines = trace(traces, L, 20000, seed=2)[RUN - 1200:RUN - 1200 + n]      # zeros, then random lines
    plain = mpc.BPC(L)
    sizes = plain.compress_lines(lines, want_selected=False)[0]
    plain.close()
    sb, hb = coarse_sector(N, L), 9
    assert len(set(R.sectors_of(R.payloads(sizes, N)[0] + hb, sb, 4).tolist())) == 2
    ev = mpc.BPC(L)
    ev.enable_pack_stats(N, sb, hb)
    feed_and_check("line by line", ev, lines, sizes, [1] * n, N, L, sb, hb)
    ev.close()


# ---- 3. the stager's slot switch -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big_trace(mpc, traces):
    """3 Mi lines of 32 bytes: one staged call of 96 MiB, the slot switch after 2 Mi lines; with the sizes of BDI."""
    L, n = 32, 3 << 20
    pool = trace(traces, L, 2 * RUN + 4096)[2 * RUN:]
    idx = np.random.default_rng(5).integers(0, len(pool), n)
    lines = pool[idx]
    lines[1 << 20:(1 << 20) + RUN] = 0
    lines[(2 << 20) - RUN // 2:(2 << 20) + RUN // 2] = traces.random_u32(RUN, L)[:2 * (RUN // 2)]
    plain = mpc.BDI(L)
    sizes = plain.compress_lines(lines, want_selected=False)[0]
    plain.close()
    return lines, sizes


@pytest.mark.parametrize("N", [3, 1000])
def test_stager_seam(mpc, big_trace, N):
    L = 32
    lines, sizes = big_trace
    assert (2 << 20) % N != 0                      # a block straddles the slot switch
    runs = runs_for(sizes, N, L)
    assert_coverage(f"N={N}", sizes, N, L, runs)
    for sb, hb in runs:
        ev = mpc.BDI(L)
        ev.enable_pack_stats(N, sb, hb)
        ev.compress_lines(lines, want_sizes=False, want_selected=False)
        R.same_table(f"N={N} sector={sb} header={hb}", ev.pack_table(), R.pack_table(sizes, N, L, sb, hb))
        ev.close()


# ---- 4. the device path ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def device_trace(mpc):
    """4 Mi + 12 345 lines of 32 bytes from mpc_synth_fill (zeros, random words, then mixed), and BDI's sizes of them
    from a handle that was given a sizes array."""
    import torch
    L, n = 32, (4 << 20) + 12345
    buf = torch.empty(n * L, dtype=torch.uint8, device="cuda:0")
    mpc.synth_fill(buf.data_ptr(), n, L, "mixed")
    mpc.synth_fill(buf.data_ptr() + 5000 * L, 2 * RUN, L, "zeros")
    mpc.synth_fill(buf.data_ptr() + ((4 << 20) - RUN) * L, 2 * RUN, L, "random_u32")      # across the seam of the 4 Mi-line pieces
    torch.cuda.synchronize()
    d_sizes = torch.zeros(n, dtype=torch.int16, device="cuda:0")
    plain = mpc.BDI(L)
    plain.compress_device(buf.data_ptr(), n, d_sizes.data_ptr())
    plain.sync()
    plain.close()
    return buf, n, d_sizes.cpu().numpy().view(np.uint16)


@pytest.mark.parametrize("N", [3, 1000])
def test_device_path(mpc, device_trace, N):
    import torch
    L = 32
    buf, n, sizes = device_trace
    assert (4 << 20) % N != 0                      # a block straddles the seam of the pieces
    runs = runs_for(sizes, N, L)
    assert_coverage(f"N={N}", sizes, N, L, runs)
    for sb, hb in runs:
        want = R.pack_table(sizes, N, L, sb, hb)
        ev = mpc.BDI(L)
        ev.enable_pack_stats(N, sb, hb)
        ev.compress_device(buf.data_ptr(), n)      # no sizes array: pieces of 4 Mi lines over the scratch array
        R.same_table(f"N={N} sector={sb} header={hb}, pieces", ev.pack_table(), want)
        ev.reset()
        d_sizes = torch.zeros(n, dtype=torch.int16, device="cuda:0")
        ev.compress_device(buf.data_ptr(), n, d_sizes.data_ptr())
        R.same_table(f"N={N} sector={sb} header={hb}, the caller's sizes array", ev.pack_table(), want)
        assert (d_sizes.cpu().numpy().view(np.uint16) == sizes).all()
        ev.close()


# ---- 5. files --------------------------------------------------------------------------------------------------------
def test_files(mpc, traces, tmp_path):
    L, N, n = 64, 16, 2 * RUN + 3001
    lines = trace(traces, L, n, seed=4)
    plain = mpc.FPC(L)
    sizes = plain.compress_lines(lines, want_selected=False)[0]
    plain.close()
    runs = runs_for(sizes[:-1], N, L)
    assert_coverage("files", sizes[:-1], N, L, runs)
    npy = traces.save_npy(str(tmp_path / "t.npy"), lines)
    req_types = np.where(np.arange(n) % 5 == 0, 4, np.where(np.arange(n) % 11 == 0, 3, 0))
    log = traces.write_gpgpusim_log(str(tmp_path / "t.log"), lines, req_types)
    keep = req_types != 3
    for sb, hb in runs:
        ev = mpc.FPC(L)
        ev.enable_pack_stats(N, sb, hb)
        assert ev.compress_npy(npy) == n - 1       # the driver drops the final row
        R.same_table(f".npy sector={sb} header={hb}", ev.pack_table(), R.pack_table(sizes[:-1], N, L, sb, hb))
        ev.reset()
        assert ev.compress_gpgpusim_log(log)[1] == int(keep.sum())
        R.same_table(f".log sector={sb} header={hb}", ev.pack_table(), R.pack_table(sizes[keep], N, L, sb, hb))
        ev.close()


# ---- 6. groups -------------------------------------------------------------------------------------------------------
GROUP = ("BDI", "FPC", "BPC", "VPC", "CPACK")


def refused(mpc, call, *words):
    with pytest.raises(mpc.MpcError) as e:
        call()
    assert e.value.code == MPC_E_INVAL and all(w in str(e.value) for w in words), str(e.value)


@pytest.mark.parametrize("N", [5, 100, 1000])
def test_group_members_and_best(mpc, configs, traces, N):
    L = 64
    lines = trace(traces, L, 9000, seed=6)
    plain = [make(mpc, configs, c, L) for c in GROUP]
    sizes = [p.compress_lines(lines, want_selected=False)[0] for p in plain]
    for p in plain:
        p.close()
    best = np.min(np.stack(sizes), axis=0)
    tag_bits = 3                                   # ceil(log2(5 participants))
    runs = runs_for(sizes[0], N, L)
    assert_coverage(f"N={N} BDI", sizes[0], N, L, runs)
    for sb, hb in runs:
        group_run(mpc, configs, lines, sizes, best, N, L, sb, hb, tag_bits)
    cov = R.coverage(best, N, L, runs[0][0], N * tag_bits)
    assert len(cov["counts"]) >= 2 and 4 in cov["counts"], cov      # (the minimum's blocks differ too, and reach the cap)


def group_run(mpc, configs, lines, sizes, best, N, L, sb, hb, tag_bits):
    members = [make(mpc, configs, c, L) for c in GROUP]
    group = mpc.EvaluatorSet(members)
    group.enable_best()
    group.enable_pack_stats(N, sb, hb)
    group.enable_pack_stats(N, sb, hb)             # idempotent
    at = 0
    for n in (3000, 300, 513, 5187):               # staged and in place
        out = group.compress_lines(lines[at:at + n])
        at += n
        stats = group.pack_stats()
        assert sorted(stats, key=str) == [0, 1, 2, 3, 4, "best"]
        for i, c in enumerate(GROUP):
            assert (out[i][0] == sizes[i][at - n:at]).all()
            want = R.pack_table(sizes[i][:at], N, L, sb, hb)
            R.same_table(f"{c} after {at}", group.pack_table(i), want)
            R.same_table(f"{c} after {at}, the member's own get", members[i].pack_table(), want)
            assert stats[i]["blocks"] == int(want[0]) and stats[i]["sectors"] == int(want[2])
        R.same_table(f"best after {at}", group.pack_table(mpc.MPC_PACK_BEST), R.pack_table(best[:at], N, L, sb, hb + N * tag_bits))
    # each member's table equals the table of the handle run alone
    for i, c in enumerate(GROUP):
        alone = make(mpc, configs, c, L)
        alone.enable_pack_stats(N, sb, hb)
        alone.compress_lines(lines, want_sizes=False, want_selected=False)
        R.same_table(f"{c} alone", alone.pack_table(), group.pack_table(i))
        alone.close()
    group.close()
    for e in members:
        e.close()


def test_group_refusals(mpc, configs, traces):
    L, N = 64, 10
    lines = trace(traces, L, 2 * RUN + 500)[2 * RUN:]
    members = [mpc.BDI(L), mpc.FPC(L), mpc.BPC(L)]
    group = mpc.EvaluatorSet(members)
    refused(mpc, lambda: group.pack_table(0), "mpc_group_pack_stats_enable")
    refused(mpc, lambda: group.enable_pack_stats(0), "block_lines")
    group.enable_pack_stats(N, 32, 0)              # the best-of is off
    refused(mpc, lambda: group.enable_pack_stats(N, 64, 0), "already on")
    refused(mpc, lambda: group.pack_table(mpc.MPC_PACK_BEST), "best-of")
    refused(mpc, lambda: group.pack_table(3), "member")
    assert "best" not in group.pack_stats()
    group.compress_lines(lines[:105])
    before = [group.pack_table(i) for i in range(3)]
    assert int(before[0][0]) == 10 and int(before[0][3]) == 5
    members[1].compress_lines(lines[105:112])      # a member fed alone between two group calls
    refused(mpc, lambda: group.compress_lines(lines[112:200]), "member 1", "fed outside the group")
    refused(mpc, lambda: group.compress_npy("/nonexistent.npy"), "member 1", "fed outside the group")
    assert members[0].stats_vector()[0] == 105     # the refused calls evaluated nothing
    R.same_table("member 0 is where it was", members[0].pack_table(), before[0])
    # reset the members: the group counts from line 0 again
    for e in members:
        e.reset()
    out = group.compress_lines(lines[:37])
    R.same_table("after the reset", group.pack_table(2), R.pack_table(out[2][0], N, L, 32, 0))
    group.close()
    # a member that already counts with other values, or stands at another line
    refused(mpc, lambda: mpc.EvaluatorSet(members).enable_pack_stats(N, 64, 0), "member 0", "already counts")
    members[2].compress_lines(lines[:3])
    refused(mpc, lambda: mpc.EvaluatorSet(members).enable_pack_stats(N, 32, 0), "member 2", "line 40")
    for e in members:
        e.close()


# ---- 7. reset and merge ----------------------------------------------------------------------------------------------
def test_reset_starts_over(mpc, traces):
    L, N, sb, hb = 32, 33, 64, 17
    lines = trace(traces, L, 2 * RUN + 2000)[RUN:]
    plain = mpc.CPACK(L)
    sizes = plain.compress_lines(lines, want_selected=False)[0]
    plain.close()
    ev = mpc.CPACK(L)
    ev.enable_pack_stats(N, sb, hb)
    ev.compress_lines(lines[:1000], want_sizes=False, want_selected=False)
    assert int(ev.pack_table()[3]) == 1000 % N != 0
    ev.reset()
    t = ev.pack_table()
    assert t[:5].tolist() == [0, 0, 0, 0, 0] and t[5:8].tolist() == [N, sb, hb] and int(t[8:].sum()) == 0
    ev.compress_lines(lines[500:2500], want_sizes=False, want_selected=False)
    R.same_table("after reset", ev.pack_table(), R.pack_table(sizes[500:2500], N, L, sb, hb))
    ev.close()


@pytest.mark.parametrize("N", [3, 64, 1000])
def test_shards_merge(mpc, traces, N):
    sharded = pkg("sharded")
    L, n = 32, 2 * RUN + 3334
    lines = trace(traces, L, n, seed=7)
    plain = mpc.BDI(L)
    sizes = plain.compress_lines(lines, want_selected=False)[0]
    plain.close()
    runs = runs_for(sizes, N, L)
    assert_coverage(f"N={N}", sizes, N, L, runs)
    for sb, hb in runs:
        merge_run(mpc, sharded, lines, sizes, n, N, L, sb, hb)


def merge_run(mpc, sharded, lines, sizes, n, N, L, sb, hb):
    want = R.pack_table(sizes, N, L, sb, hb)
    assert int(want[3]) != 0                       # the trace has a tail
    shards = []
    for rank in range(2):
        b, e = sharded.shard_range(n, rank, 2, align=N)
        assert b % N == 0
        ev = mpc.BDI(L)
        ev.enable_pack_stats(N, sb, hb)
        ev.compress_lines(lines[b:e], want_sizes=False, want_selected=False)
        shards.append(ev)
    t1 = shards[1].pack_table()
    shards[0].pack_stats_merge(t1)
    R.same_table("merged", shards[0].pack_table(), want)
    R.same_table("merged, the reference's merge", R.merge(R.pack_table(sizes[:b], N, L, sb, hb), t1), want)
    stats = shards[0].pack_stats()
    assert (stats["tail_sectors"], stats["tail_cap"]) == R.tail(want, L) and stats["sector_ratio"] == R.sector_ratio(want, L)
    assert shards[0].pack_stats(close_tail=False)["sector_ratio"] == R.sector_ratio(want, L, close_tail=False) == stats["sector_ratio_closed"]
    # the merged handle continues the open block
    shards[0].compress_lines(lines[:N], want_sizes=False, want_selected=False)
    R.same_table("continued", shards[0].pack_table(), R.pack_table(np.concatenate([sizes, sizes[:N]]), N, L, sb, hb))
    # both sides open, other values
    refused(mpc, lambda: shards[0].pack_stats_merge(t1), "both sides")
    other = t1.copy()
    other[7] += 1
    refused(mpc, lambda: shards[1].pack_stats_merge(other), "other values")
    for ev in shards:
        ev.close()


# ---- 8. with the other two accountings, and the off state ------------------------------------------------------------
@pytest.mark.parametrize("comp", ["VPC", "BDI", "SC2", "Pattern"])
def test_interplay_and_the_off_state(mpc, configs, traces, comp):
    L, N, sb, hb = 64, 31, 128, 40
    lines = trace(traces, L, 2 * RUN + 3000, seed=8)[RUN:]
    n = len(lines)
    classes = (np.arange(n) // 97 % 256).astype(np.uint8)
    alone = {}
    for which in ("pack", "hist", "classes", "all"):
        ev = make(mpc, configs, comp, L)
        refused(mpc, lambda: ev.pack_table(), "mpc_pack_stats_enable")
        if which in ("pack", "all"):
            ev.enable_pack_stats(N, sb, hb)
        if which in ("hist", "all"):
            ev.enable_size_histogram()
        if which in ("classes", "all"):
            ev.enable_class_stats(32)
        at = 0
        for k in (700, 400, n - 1100):
            ev.compress_lines(lines[at:at + k], want_sizes=False, want_selected=False, classes=classes[at:at + k] if which in ("classes", "all") else None)
            at += k
        got = {"stats": ev.stats_vector()}
        if which in ("pack", "all"):
            got["pack"] = ev.pack_table()
        if which in ("hist", "all"):
            got["hist"] = ev.size_histogram()
        if which in ("classes", "all"):
            got["classes"] = ev.class_table()
        alone[which] = got
        ev.close()
    plain = make(mpc, configs, comp, L)      # (the same calls: SC2 and Pattern keep state from line to line)
    sizes = np.concatenate([plain.compress_lines(part, want_selected=False)[0] for part in (lines[:700], lines[700:1100], lines[1100:])])
    R.same_table("pack alone", alone["pack"]["pack"], R.pack_table(sizes, N, L, sb, hb))
    R.same_table("pack with the others", alone["all"]["pack"], alone["pack"]["pack"])
    assert (alone["all"]["hist"] == alone["hist"]["hist"]).all() and (alone["all"]["classes"] == alone["classes"]["classes"]).all()
    for which in alone:
        assert (alone[which]["stats"] == plain.stats_vector()).all(), which
    plain.close()


def test_refusals(mpc, traces):
    L = 64
    for fit in (mpc.FitPairs(L), mpc.FitResidues(L, list(range(L)))):
        refused(mpc, lambda: fit.enable_pack_stats(4), "Fit")
        fit.close()
    ev = mpc.BDI(L)
    refused(mpc, lambda: ev.pack_stats(), "mpc_pack_stats_enable")
    refused(mpc, lambda: ev.pack_stats_merge(np.zeros(R.TABLE_LEN, np.uint64)), "mpc_pack_stats_enable")
    for args, word in (((0,), "block_lines"), ((4, 0), "sector_bytes"), ((4, 257), "sector_bytes"), ((64, 2), "1024 sectors"),
                       ((4, 32, 65536), "header_bits"), (((1 << 19) + 1, 1 << 16), "block_lines")):
        refused(mpc, lambda: ev.enable_pack_stats(*args), word)
    ev.enable_pack_stats(64, 4, 65535)             # exactly 1024 sectors, the largest header
    refused(mpc, lambda: ev.enable_pack_stats(64, 4, 0), "already on", "65535")
    t = np.zeros(R.TABLE_LEN - 1, np.uint64)
    assert mpc.lib().mpc_pack_stats_get(ev._h, t.ctypes.data, t.size) == MPC_E_INVAL
    assert mpc.lib().mpc_pack_stats_merge(ev._h, t.ctypes.data, t.size) == MPC_E_INVAL
    assert ev.stats_vector()[0] == 0
    ev.close()


# ---- 9. the command line ---------------------------------------------------------------------------------------------
def fmt_double(x):
    """The host code's text of a double: shortest round-trip, no trailing ".0"."""
    r = repr(float(x))
    return r[:-2] if r.endswith(".0") else r


CSV_HEADER = "Workload,Line Size,Block Lines,Sector Bytes,Header Bits,Blocks,Tail Lines,Sector Ratio,Histogram,\n"


def csv_text(workload, table, L):
    """The row of <stem>_results_pack.csv, restated from a reference table."""
    S = R.block_sectors(table[5], L, table[6])
    hist = ";".join(f"{k}:{int(table[8 + k - 1])}" for k in range(1, S + 1) if int(table[8 + k - 1]))
    return CSV_HEADER + (f"{workload},{L},{int(table[5])},{int(table[6])},{int(table[7])},{int(table[0])},{int(table[3])},"
                         f"{fmt_double(R.sector_ratio(table, L))},{hist},\n")


def test_cli_pack(mpc, configs, traces, tmp_path):
    import json
    import os
    import subprocess
    from conftest import ROOT
    pkg("build").build_all()
    bindir = os.path.join(ROOT, "bin")
    cli = os.path.join(bindir, "compressor")
    L, n = 32, 2 * RUN + 3002
    lines = trace(traces, L, n, seed=9)
    ds = tmp_path / "ds"
    ds.mkdir()
    npy = traces.save_npy(str(ds / "t.npy"), lines)
    cfg_path = str(tmp_path / "probe.json")
    with open(cfg_path, "w") as f:
        json.dump(configs.probe_config(L), f)
    fed = lines[:-1]                               # the driver drops the final row of an .npy
    names = ("VPC", "BDI", "FPC")
    plain = [make(mpc, configs, c, L) for c in names]
    sizes = [p.compress_lines(fed, want_selected=False)[0] for p in plain]
    for p in plain:
        p.close()

    def run(args, out):
        out.mkdir()
        r = subprocess.run([cli, *args, "-o", str(out)], cwd=bindir, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        return r.stdout

    # one algorithm, four 32-byte lines a block of four 32-byte sectors; --pack alone does not switch the size histogram on
    base = ["-a", "BDI", "-i", npy]
    plain_stdout = run(base, tmp_path / "one_plain")
    assert run(base + ["--pack", "4"], tmp_path / "one") == plain_stdout
    for name in os.listdir(tmp_path / "one_plain"):
        assert (tmp_path / "one" / name).read_bytes() == (tmp_path / "one_plain" / name).read_bytes(), name
    assert sorted(set(os.listdir(tmp_path / "one")) - set(os.listdir(tmp_path / "one_plain"))) == ["BDI_results_pack.csv"]
    want = R.pack_table(sizes[1], 4, L, 32, 0)
    assert len(np.nonzero(want[8:12])[0]) >= 3 and int(want[8]) > 0 and int(want[11]) > 0 and int(want[3]) != 0
    assert (tmp_path / "one" / "BDI_results_pack.csv").read_text() == csv_text("ds_t", want, L)
    # a list with the size histogram: every member's file and the best of the list, whose blocks carry the tag bits too
    base = ["-a", ",".join(names), "-c", cfg_path, "-i", npy, "--size-histogram"]
    plain_stdout = run(base, tmp_path / "list_plain")
    assert run(base + ["--pack", "128", "--sector", "32", "--pack-header", "256"], tmp_path / "list") == plain_stdout
    for name in os.listdir(tmp_path / "list_plain"):
        assert (tmp_path / "list" / name).read_bytes() == (tmp_path / "list_plain" / name).read_bytes(), name
    stems = ["probe", "BDI", "FPC", "BEST"]
    assert sorted(set(os.listdir(tmp_path / "list")) - set(os.listdir(tmp_path / "list_plain"))) == sorted(f"{s}_results_pack.csv" for s in stems)
    tables = [R.pack_table(s, 128, L, 32, 256) for s in sizes] + [R.pack_table(np.min(np.stack(sizes), axis=0), 128, L, 32, 256 + 128 * 2)]
    assert len(np.nonzero(tables[1][8:])[0]) >= 3 and int(tables[1][8 + 127]) > 0      # several counts, the cap of 128 sectors
    for stem, table in zip(stems, tables):
        assert (tmp_path / "list" / f"{stem}_results_pack.csv").read_text() == csv_text("ds_t", table, L), stem
    # without the size histogram: no best of the list, and --sector next to --pack does not switch it on
    run(["-a", "BDI,FPC", "-i", npy, "--pack", "16", "--sector", "64"], tmp_path / "no_best")
    assert sorted(f for f in os.listdir(tmp_path / "no_best") if not f.endswith(("_results.csv", "_results_detail.csv"))) == \
        ["BDI_results_pack.csv", "FPC_results_pack.csv"]
    assert (tmp_path / "no_best" / "FPC_results_pack.csv").read_text() == csv_text("ds_t", R.pack_table(sizes[2], 16, L, 64, 0), L)
