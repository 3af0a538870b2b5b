"""Groups of evaluators on the MI355X (mpc_group / EvaluatorSet / `compressor -a A,B,...`): every member of a group sees
every line exactly as if it had been called alone.  All comparisons are exact: integers, and CSV text byte for byte.

- the reference's own BDI / FPC / BPC numbers (tests/golden/ref_baseline_vectors.npz) through groups of all the
  baselines that accept the case's line size: the shared kernel at 32 / 64 / 128 bytes, the members' own elsewhere;
- VPC (built in and compiled at creation), SC2, BDI, FPC, BPC in one group against fresh solo handles, on every
  ingestion path;
- more than two staging chunks with SC2's table build early in the second one;
- ragged calls across the in-place / staged seam; rejected sets; the command line."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, pkg

import baseline_ref
import sc2_ref

pytestmark = pytest.mark.gpu

BIN = os.path.join(ROOT, "bin")


@pytest.fixture(scope="module")
def mpc():
    m = pkg()
    m.lib()
    return m


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return baseline_ref.load_fixture(os.path.join(golden_dir, "ref_baseline_vectors.npz"))


def accepts(comp, L):
    """Line sizes the create calls take (include/mpc_hip.h)."""
    return {"BDI": L % 8 == 0 and 8 <= L <= 256, "FPC": L % 4 == 0 and 4 <= L <= 256, "BPC": L % 4 == 0 and 8 <= L <= 128}[comp]


def expected_form(comps, L):
    if len(comps) >= 2 and L in (32, 64, 128):
        return "+".join(comps) + ": one kernel"
    return "; ".join(f"{c}: own kernel" for c in comps)


def same_lines(tag, got, want):
    for what, g, w in (("sizes", got[0], want[0]), ("selected", got[1], want[1])):
        bad = np.nonzero(g != w)[0]
        assert bad.size == 0, f"{tag}: {bad.size} {what} differ, first at {bad[:5]}: {g[bad[:5]]} vs {w[bad[:5]]}"


# ---- reference parity through the group ---------------------------------------------------------------------------
def test_reference_fixture_through_groups(mpc, fixture):
    meta, arrays = fixture
    compared, single_member_groups, shared_groups = 0, 0, 0
    for case in meta["cases"]:
        name, comp, L = case["name"], case["comp"], case["L"]
        lines = baseline_ref.case_input(case)
        all_comps = [c for c in ("BDI", "FPC", "BPC") if accepts(c, L)]
        assert comp in all_comps
        sets = [all_comps]
        if L == 64:
            sets += [["BDI", "FPC"], ["BDI", "BPC"], ["FPC", "BPC"]]
        for comps in sets:
            if comp not in comps:
                continue
            members = [getattr(mpc, c)(L) for c in comps]
            group = mpc.EvaluatorSet(members)
            assert group.form == expected_form(comps, L), (name, comps, group.form)
            single_member_groups += len(comps) == 1
            shared_groups += "one kernel" in group.form
            outs = group.compress_lines(lines)
            for c, ev, out in zip(comps, members, outs):
                tag = f"{name} in {'+'.join(comps)}: {c}"
                if c == comp:      # the case's own compressor: the reference's numbers
                    want_sel = arrays[name + ".states"] if c == "BDI" else np.zeros(case["n"], np.int8)
                    same_lines(tag, out, (arrays[name + ".sizes"], want_sel))
                    stats = arrays[name + ".stats"]
                    assert (ev.stats_vector() == baseline_ref.stats_vector(c, case["n"], stats)).all(), tag
                    assert ev.result()["comp_ratio"] == float(arrays[name + ".ratio"][0]), tag
                else:              # the others: a fresh handle fed alone
                    solo = getattr(mpc, c)(L)
                    same_lines(tag, out, solo.compress_lines(lines))
                    assert (ev.stats_vector() == solo.stats_vector()).all(), tag
                    solo.close()
            group.close()
            for ev in members:
                ev.close()
        compared += 1
    assert compared == 33 == len(baseline_ref.CASES)
    assert single_member_groups >= 1       # FPC alone at 4, 100, 132, 252 bytes: behaves as the solo handle
    assert shared_groups == 9 + 3 * 2      # 32 / 64 / 128 bytes x three compressors, and two pairs per 64-byte case


# ---- group equals solo ------------------------------------------------------------------------------------------
def second_vpc_config(configs, L):
    """A module sequence without a built-in kernel: compiled when the handle is created."""
    prev1 = [max(i - 1, 0) for i in range(L)]
    prev4 = [max(i - 4, 0) for i in range(L)]
    return configs.make_config(L, [{"name": "AllZero"}, configs.consecutive_base(L, 0, True), configs.diff_base(L, prev1, [2] * L, 3, False),
                                   configs.weight_base(L, prev4, [[1.0, 0.5][i % 2] for i in range(L)], 0, True),
                                   configs.one_base(L, 7, True)])


SC2_S = 1500


def make_members(mpc, configs, L):
    return [mpc.VPC(configs.probe_config(L)), mpc.VPC(second_vpc_config(configs, L)), mpc.SC2(L, SC2_S), mpc.BDI(L), mpc.FPC(L), mpc.BPC(L)]


def close_all(group, members):
    if group is not None:
        group.close()
    for ev in members:
        ev.close()


def trace_lines(traces, kind):
    n = 7000
    if kind == "mixed":
        return traces.mixed(n, 64)
    if kind == "sine":
        return traces.sine_f32(n, 64)
    if kind == "structured":
        return traces.structured(n, 64)
    return traces.pointers_u64(n, 128)


@pytest.mark.parametrize("kind", ["mixed", "sine", "structured", "pointers128"])
def test_group_equals_solo_on_every_path(mpc, configs, traces, tmp_path, kind):
    import torch
    lines = trace_lines(traces, kind)
    n, L = lines.shape
    # what fresh solo handles give, with per-line outputs
    solo = make_members(mpc, configs, L)
    assert solo[0].kernel_form == "unrolled" and solo[1].kernel_form.startswith("unrolled, compiled at creation")
    want = [ev.compress_lines(lines) for ev in solo]
    want_stats = [ev.stats_vector() for ev in solo]
    close_all(None, solo)
    solo = make_members(mpc, configs, L)
    for ev in solo:
        ev.compress_lines(lines[:-1], want_sizes=False, want_selected=False)
    want_stats_short = [ev.stats_vector() for ev in solo]
    close_all(None, solo)

    def check_stats(members, ws, tag):
        for i, (ev, w) in enumerate(zip(members, ws)):
            assert (ev.stats_vector() == w).all(), f"{kind} {tag}: member {i}"

    # host path, per-line outputs
    members = make_members(mpc, configs, L)
    group = mpc.EvaluatorSet(members)
    form = group.form
    assert form == ("VPC: unrolled; VPC: " + members[1].kernel_form + "; SC2: own kernel; BDI+FPC+BPC: one kernel"), form
    outs = group.compress_lines(lines)
    for i in range(len(members)):
        same_lines(f"{kind} host: member {i}", outs[i], want[i])
    check_stats(members, want_stats, "host")
    close_all(group, members)

    # host path, no per-line outputs
    members = make_members(mpc, configs, L)
    group = mpc.EvaluatorSet(members)
    outs = group.compress_lines(lines, want_sizes=False, want_selected=False)
    assert all(o == (None, None) for o in outs)
    check_stats(members, want_stats, "host, statistics only")
    close_all(group, members)

    # device path on a caller's stream, with outputs for some members only
    members = make_members(mpc, configs, L)
    group = mpc.EvaluatorSet(members)
    stream = torch.cuda.Stream()
    d_lines = torch.from_numpy(lines).to("cuda:0")
    d_sizes = [torch.zeros(n, dtype=torch.int16, device="cuda:0") for _ in members]
    d_sel = [torch.full((n,), -7, dtype=torch.int8, device="cuda:0") for _ in members]
    torch.cuda.synchronize()
    cut = 3000                                # SC2's line S lies in the first call
    for a, b in ((0, cut), (cut, n)):
        group.compress_device(d_lines[a:].data_ptr(), b - a, [t[a:].data_ptr() for t in d_sizes],
                              [t[a:].data_ptr() if i != 4 else 0 for i, t in enumerate(d_sel)], stream=stream.cuda_stream)
    group.sync()
    torch.cuda.synchronize()
    for i in range(len(members)):
        got_sel = d_sel[i].cpu().numpy()
        if i == 4:                            # not asked for: untouched
            assert (got_sel == -7).all()
            got_sel = want[i][1]
        same_lines(f"{kind} device: member {i}", (d_sizes[i].cpu().numpy().view(np.uint16), got_sel), want[i])
    check_stats(members, want_stats, "device")
    close_all(group, members)

    # .npy, with and without the dropped last row
    npy = traces.save_npy(str(tmp_path / "t.npy"), lines)
    for skip, ws in ((True, want_stats_short), (False, want_stats)):
        members = make_members(mpc, configs, L)
        group = mpc.EvaluatorSet(members)
        assert group.compress_npy(npy, skip_last_row=skip) == n - (1 if skip else 0)
        check_stats(members, ws, f".npy skip_last_row={skip}")
        close_all(group, members)

    # GPGPU-Sim .log: every request a global read or write, so the same lines
    log = traces.write_gpgpusim_log(str(tmp_path / "t.log"), lines, np.where(np.arange(n) % 3 == 0, 4, 0))
    members = make_members(mpc, configs, L)
    group = mpc.EvaluatorSet(members)
    assert group.compress_gpgpusim_log(log) == (n, n)
    check_stats(members, want_stats, ".log")
    close_all(group, members)


def test_several_vpc_configurations_and_two_handles_of_one_algorithm(mpc, configs, traces):
    """Configuration authoring: several VPC configurations in one group; a second BDI handle runs its own kernel."""
    L = 64
    lines = traces.structured(5000, L, seed=11)
    cfgs = [configs.probe_config(L), configs.probe_config_u64(L), second_vpc_config(configs, L)]
    members = [mpc.VPC(c) for c in cfgs] + [mpc.BDI(L), mpc.BDI(L), mpc.FPC(L)]
    group = mpc.EvaluatorSet(members)
    assert group.form.endswith("BDI+FPC: one kernel; BDI: own kernel"), group.form
    outs = group.compress_lines(lines)
    solo = [mpc.VPC(c) for c in cfgs] + [mpc.BDI(L), mpc.BDI(L), mpc.FPC(L)]
    for i, (ev, s) in enumerate(zip(members, solo)):
        same_lines(f"member {i}", outs[i], s.compress_lines(lines))
        assert (ev.stats_vector() == s.stats_vector()).all(), i
    close_all(group, members)
    close_all(None, solo)


# ---- more than two chunks, SC2's table build early in the second one ----------------------------------------------
def _zipf_lines(n, L, seed):
    rng = np.random.default_rng(seed)
    pool = rng.integers(0, 1 << 32, size=4000, dtype=np.uint64).astype(np.uint32)
    p = 1.0 / np.arange(1, len(pool) + 1) ** 1.05
    p /= p.sum()
    words = pool[rng.choice(len(pool), size=n * (L // 4), p=p)]
    noise = rng.random(words.size) < 0.1
    words = np.where(noise, rng.integers(0, 1 << 32, size=words.size, dtype=np.uint64).astype(np.uint32), words)
    return words.astype("<u4").view(np.uint8).reshape(n, L)


def test_three_chunks_with_the_table_build_behind_a_counting_chunk(mpc):
    """64-byte lines: a staging slot holds 2^20 of them.  2.5 slots and a bit, so both slots are reused; S = 2^20 + 1000, so
    the table is built early in the second chunk (the group's second slot) while the first chunk, all warm-up lines, may
    still be counting on the group's first slot."""
    L, slot = 64, (64 << 20) // 64
    n, S = 5 * slot // 2 + 777, slot + 1000
    lines = _zipf_lines(n, L, seed=21)
    members = [mpc.BDI(L), mpc.SC2(L, S), mpc.FPC(L), mpc.BPC(L)]
    group = mpc.EvaluatorSet(members)
    assert group.form == "BDI+FPC+BPC: one kernel; SC2: own kernel"
    outs = group.compress_lines(lines)
    ref = sc2_ref.SC2Ref(L, S)
    rs, rk = ref.feed(lines)
    same_lines("SC2 against sc2_ref", outs[1], (rs, rk))
    assert members[1].stats_vector().tolist() == ref.stats_vector().tolist()
    sym, lens = members[1].table()
    assert sym.tolist() == ref.table_syms.tolist() and lens.tolist() == ref.table_lens.tolist()
    solo = [mpc.BDI(L), mpc.SC2(L, S), mpc.FPC(L), mpc.BPC(L)]
    for i, (ev, s) in enumerate(zip(members, solo)):
        same_lines(f"member {i}", outs[i], s.compress_lines(lines))
        assert (ev.stats_vector() == s.stats_vector()).all(), i
    close_all(group, members)
    close_all(None, solo)


# ---- ragged calls -------------------------------------------------------------------------------------------------
def test_ragged_calls(mpc, configs, traces):
    L = 64
    lines = np.concatenate([traces.mixed(1500, L), traces.structured(1500, L), traces.sine_f32(1000, L)])
    members = make_members(mpc, configs, L)
    group = mpc.EvaluatorSet(members)
    cuts = np.cumsum([1, 511, 512, 513])      # in place, in place, the last in-place size, the first staged one; then the rest
    assert cuts[-1] + 513 < len(lines)
    parts = [group.compress_lines(p) for p in np.split(lines, cuts)]
    solo = make_members(mpc, configs, L)
    for i, (ev, s) in enumerate(zip(members, solo)):
        got = (np.concatenate([p[i][0] for p in parts]), np.concatenate([p[i][1] for p in parts]))
        same_lines(f"member {i}", got, s.compress_lines(lines))
        assert (ev.stats_vector() == s.stats_vector()).all(), i
    close_all(group, members)
    close_all(None, solo)


# ---- errors -------------------------------------------------------------------------------------------------------
def test_rejected_sets_and_members_after_a_failed_call(mpc, traces, tmp_path):
    a, b, c = mpc.BDI(64), mpc.FPC(64), mpc.FPC(32)
    for bad, text in (([a, c], "different line sizes"), ([a, b, a], "repeats member 0"), ([], "at least one member")):
        with pytest.raises(mpc.MpcError) as e:
            mpc.EvaluatorSet(bad)
        assert e.value.code == -22 and text in str(e.value), str(e.value)
    group = mpc.EvaluatorSet([a, b])
    lines = traces.mixed(2000, 64)
    wrong = traces.save_npy(str(tmp_path / "w.npy"), traces.mixed(100, 32))
    with pytest.raises(mpc.MpcError) as e:
        group.compress_npy(wrong)
    assert e.value.code == -22 and "trace line size 32 differs" in str(e.value)
    with pytest.raises(mpc.MpcError) as e:
        group.compress_npy(str(tmp_path / "missing.npy"))
    assert e.value.code == -2
    # the members alone, then the group again, then alone again: one running total each
    sa, _ = a.compress_lines(lines[:700])
    outs = group.compress_lines(lines[700:1400])
    sb, _ = b.compress_lines(lines[1400:])
    a.compress_lines(lines[1400:])
    b.compress_lines(lines[:700])
    solo_a, solo_b = mpc.BDI(64), mpc.FPC(64)
    wa, wb = solo_a.compress_lines(lines), solo_b.compress_lines(lines)
    assert (sa == wa[0][:700]).all() and (outs[0][0] == wa[0][700:1400]).all()
    assert (sb == wb[0][1400:]).all() and (outs[1][0] == wb[0][700:1400]).all()
    assert (a.stats_vector() == solo_a.stats_vector()).all() and (b.stats_vector() == solo_b.stats_vector()).all()
    close_all(group, [a, b, c, solo_a, solo_b])


# ---- the command line -----------------------------------------------------------------------------------------------
def test_cli_list_writes_what_the_solo_runs_write(configs, traces, tmp_path):
    pkg("build").build_all()
    cli = os.path.join(BIN, "compressor")
    L = 64
    lines = np.concatenate([traces.structured(3000, L, seed=9), traces.mixed(1500, L), traces.random_u32(500, L)])
    d = tmp_path / "ds"
    d.mkdir()
    npy = traces.save_npy(str(d / "t.npy"), lines)
    types = np.random.default_rng(8).choice([0, 4, 1, 2], size=len(lines), p=[0.45, 0.45, 0.05, 0.05])
    log = traces.write_gpgpusim_log(str(d / "u.log"), lines, types)
    cfg = configs.write_config(configs.probe_config(L), str(tmp_path / "probe.json"))
    names = ["VPC", "BDI", "FPC", "BPC"]

    def run(algo, trace, out):
        out.mkdir()
        r = subprocess.run([cli, "-a", algo, "-i", trace, "-c", cfg, "-o", str(out)], cwd=BIN, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        return r.stdout.strip().split("\n")

    for k, trace in enumerate((npy, log)):
        together = tmp_path / f"together{k}"
        got = run(",".join(names), trace, together)
        files = {}
        for name in names:
            alone = tmp_path / f"{name}{k}"
            line = run(name, trace, alone)
            assert got[names.index(name)] == f"{name} {line[-1]}" and line[-1].startswith("comp.ratio: ")
            for f in sorted(os.listdir(alone)):
                assert f not in files
                files[f] = (alone / f).read_bytes()
        assert len(got) == len(names)
        assert {"probe_results.csv", "probe_results_detail.csv", "BDI_results.csv", "FPC_results.csv", "BPC_results.csv"} <= set(files)
        assert sorted(os.listdir(together)) == sorted(files)
        for f, text in files.items():
            assert (together / f).read_bytes() == text, f
