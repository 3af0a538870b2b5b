"""Size accounting on the MI355X (csrc/mpc_sizes.hip): per-evaluator histograms of the per-line sizes and the per-line
best-of of a group.  Every comparison is exact integer equality.  The expected values come from the committed reference
fixtures (the reference's own per-line sizes) or, where several compressors must see the same lines, from the CPU
oracle and the numpy restatements -- never from per-line output of the library under test."""
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, pkg

import baseline_ref
import pattern_ref
import sc2_ref
import vpc_ref

pytestmark = pytest.mark.gpu

BINS = 4096
K_ACCOUNT_LINES = 4 << 20          # kAccountLines of csrc/mpc_capi.hip
MPC_E_INVAL = -22


@pytest.fixture(scope="module")
def mpc():
    m = pkg()
    m.lib()
    assert m.MPC_SIZE_BINS == BINS
    return m


@pytest.fixture(scope="module")
def baselines(golden_dir):
    return baseline_ref.load_fixture(os.path.join(golden_dir, "ref_baseline_vectors.npz"))


def bincount(sizes):
    return np.bincount(np.asarray(sizes).astype(np.int64), minlength=BINS).astype(np.uint64)


def same_hist(tag, got, want):
    assert got.dtype == np.uint64 and got.shape == (BINS,), tag
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{tag}: {bad.size} bins differ, first {bad[:6]}: {got[bad[:6]]} vs {want[bad[:6]]}"


def baseline_case(baselines, name):
    meta, arrays = baselines
    case = next(c for c in meta["cases"] if c["name"] == name)
    return case, baseline_ref.case_input(case), arrays[name + ".sizes"]


# ---- 1. fixture parity for the baselines -----------------------------------------------------------------------------
FIXTURE_CASES = ["bdi_L32", "bdi_L64", "bdi_L128", "bdi_L40", "fpc_L32", "fpc_L64", "fpc_L128", "fpc_L252",
                 "bpc_L8", "bpc_L32", "bpc_L64", "bpc_L128"]


@pytest.mark.parametrize("name", FIXTURE_CASES)
def test_baseline_fixture_histograms(mpc, baselines, name):
    case, lines, want_sizes = baseline_case(baselines, name)
    if name == "bpc_L8":
        assert want_sizes.max() == 217 > 8 * case["L"]      # the case that breaks a histogram sized by 8 L
    ev = getattr(mpc, case["comp"])(case["L"])
    ev.enable_size_histogram()
    ev.compress_lines(lines, want_sizes=False, want_selected=False)
    same_hist(name, ev.size_histogram(), bincount(want_sizes))
    assert (ev.stats_vector() == baseline_ref.stats_vector(case["comp"], case["n"], baselines[1][name + ".stats"])).all(), name
    ev.close()


# ---- 2. SC2 and Pattern ----------------------------------------------------------------------------------------------
def test_sc2_fixture_histogram(mpc, golden_dir):
    with open(os.path.join(golden_dir, "ref_sc2_vectors.json")) as f:
        case = next(c for c in json.load(f)["cases"] if c["name"] == "zipf_L64")
    lines = sc2_ref.case_input(case)
    assert sc2_ref.digest(lines) == case["sha256"]
    W = case["L"] // 4
    want_sizes = np.array([33 * W] * case["sizes_from"] + case["sizes"])      # warm-up lines cost W x 33, then the recorded sizes
    assert len(want_sizes) == len(lines)
    ev = mpc.SC2(case["L"], case["S"], device=0)
    ev.enable_size_histogram()
    ev.compress_lines(lines, want_sizes=False, want_selected=False)
    same_hist("zipf_L64", ev.size_histogram(), bincount(want_sizes))
    r = ev.result()
    assert (r["original_bits"], r["compressed_bits"]) == (case["original"], case["compressed"])
    ev.close()


def test_pattern_fixture_histogram(mpc, golden_dir):
    z = np.load(os.path.join(golden_dir, "ref_pattern_vectors.npz"))
    case = next(c for c in json.loads(bytes(z["meta"]).decode())["cases"] if c["name"] == "menu_L64")
    lines = pattern_ref.case_input(case)
    assert pattern_ref.digest(lines) == case["sha256"]
    ev = mpc.Pattern(64)
    ev.enable_size_histogram()
    ev.compress_lines(lines, want_sizes=False, want_selected=False)
    same_hist("menu_L64", ev.size_histogram(), bincount(z["menu_L64/sizes"]))      # the smallest scan + 4
    assert (ev.stats_vector() == z["menu_L64/stats"]).all()
    ev.close()


# ---- 3. VPC: no pass, the histogram of the statistics ----------------------------------------------------------------
def test_vpc_fixture_histogram(mpc, golden_dir):
    fixture = vpc_ref.load_fixture(os.path.join(golden_dir, "ref_vpc_vectors.npz"))
    case = vpc_ref.fixture_case(fixture, "probe_L64")
    lines = vpc_ref.case_input(case)
    ev = mpc.VPC(vpc_ref.case_config(case))
    ev.enable_size_histogram()
    ev.compress_lines(lines, want_sizes=False, want_selected=False)
    got = ev.size_histogram()
    same_hist("probe_L64", got, bincount(fixture[1]["probe_L64.sizes"]))
    v, K, B = ev.stats_vector(), ev.num_modules + 1, ev.hist_bins
    summed = v[3 + 6 * K:].reshape(K, B).sum(axis=0)
    want = np.zeros(BINS, np.uint64)
    np.add.at(want, np.minimum(np.arange(B), BINS - 1), summed)
    same_hist("probe_L64 (statistics)", got, want)
    ev.close()


# ---- 4. every ingestion path -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[64, 32])
def bdi(request, baselines):
    """BDI at one line size: the fixture's lines and the reference's sizes for them, to be tiled."""
    L = request.param
    case, lines, sizes = baseline_case(baselines, f"bdi_L{L}")
    return L, lines, sizes


def tiled(bdi, n, first=0):
    """n lines (fixture line (first + i) % len) and the histogram of the reference's sizes for them."""
    L, lines, sizes = bdi
    idx = (first + np.arange(n)) % len(lines)
    return np.ascontiguousarray(lines[idx]), bincount(sizes[idx])


@pytest.mark.parametrize("n", [1, 63, 64, 65, 512, 513])
def test_host_calls_in_place_and_smallest_staged(mpc, bdi, n):
    """Up to 512 lines are evaluated in place (wave and load tails: 1, 63, 64, 65); 513 is the smallest staged call."""
    ev = mpc.BDI(bdi[0])
    ev.enable_size_histogram()
    lines, want = tiled(bdi, n, first=7)
    ev.compress_lines(lines, want_sizes=False, want_selected=False)
    same_hist(f"{n} lines", ev.size_histogram(), want)
    sizes, _ = ev.compress_lines(lines, want_sizes=True, want_selected=False)      # the caller asks as well
    same_hist(f"{n} lines twice", ev.size_histogram(), 2 * want)
    assert (bincount(sizes) == want).all()
    ev.close()


def test_three_chunks_through_both_slots(mpc, bdi):
    L = bdi[0]
    stage_lines = (64 << 20) // L
    n = 2 * stage_lines + 12345
    lines, want = tiled(bdi, n)
    ev = mpc.BDI(L)
    ev.enable_size_histogram()
    ev.compress_lines(lines, want_sizes=False, want_selected=False)
    same_hist("three chunks", ev.size_histogram(), want)
    assert int(ev.stats_vector()[0]) == n
    ev.close()


def test_npy_and_log_files(mpc, bdi, traces, tmp_path):
    L = bdi[0]
    n = 3000
    lines, want = tiled(bdi, n, first=100)
    npy = traces.save_npy(str(tmp_path / "t.npy"), lines)
    ev = mpc.BDI(L)
    ev.enable_size_histogram()
    assert ev.compress_npy(npy, skip_last_row=False) == n
    same_hist(".npy", ev.size_histogram(), want)
    ev.reset()
    assert ev.compress_npy(npy, skip_last_row=True) == n - 1
    same_hist(".npy without its last row", ev.size_histogram(), tiled(bdi, n - 1, first=100)[1])
    ev.reset()
    log = traces.write_gpgpusim_log(str(tmp_path / "t.log"), lines, np.where(np.arange(n) % 3 == 0, 4, 0))
    assert ev.compress_gpgpusim_log(log) == (n, n)
    same_hist(".log", ev.size_histogram(), want)
    ev.close()


def test_device_batch_with_the_callers_sizes_array(mpc, bdi):
    import torch
    L, n = bdi[0], 20011
    lines, want = tiled(bdi, n, first=3)
    d_lines = torch.from_numpy(lines).to("cuda:0")
    d_sizes = torch.zeros(n + 8, dtype=torch.int16, device="cuda:0")
    ev = mpc.BDI(L)
    ev.enable_size_histogram()
    stream = torch.cuda.current_stream().cuda_stream
    ev.compress_device(d_lines.data_ptr(), n, d_sizes.data_ptr(), stream=stream)
    same_hist("caller's array", ev.size_histogram(), want)
    # an array that is only 2-byte aligned: the pass takes 2-byte loads
    ev.compress_device(d_lines.data_ptr(), n, d_sizes[1:].data_ptr(), stream=stream)
    same_hist("caller's array, not 16-byte aligned", ev.size_histogram(), 2 * want)
    assert (bincount(d_sizes[1:n + 1].cpu().numpy().view(np.uint16)) == want).all()
    ev.close()


def test_device_batch_without_a_sizes_array_crosses_a_piece_boundary(mpc, baselines):
    """kAccountLines + 4097 lines of 32 bytes (128 MiB): two pieces over the handle's scratch array."""
    import torch
    bdi = (32,) + baseline_case(baselines, "bdi_L32")[1:]
    n = K_ACCOUNT_LINES + 4097
    lines, want = tiled(bdi, n)
    d_lines = torch.from_numpy(lines).to("cuda:0")
    ev = mpc.BDI(32)
    ev.enable_size_histogram()
    ev.compress_device(d_lines.data_ptr(), n, stream=torch.cuda.current_stream().cuda_stream)
    same_hist("two pieces", ev.size_histogram(), want)
    assert int(ev.stats_vector()[0]) == n
    ev.close()


# ---- 5. one-bin pile-ups ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["zeros", "incompressible"])
def test_one_bin_pile_up(mpc, oracle, kind):
    L, n = 64, 1 << 20
    line = np.zeros(L, np.uint8) if kind == "zeros" else np.random.default_rng(5).integers(0x10, 0xF0, L).astype(np.uint8)
    size = int(oracle.BdiOracle(L).compress(line[None, :])[0][0])
    ev = mpc.BDI(L)
    ev.enable_size_histogram()
    ev.compress_lines(np.broadcast_to(line, (n, L)), want_sizes=False, want_selected=False)
    got = ev.size_histogram()
    assert int(got[size]) == n and int(got.sum()) == n, (kind, size, np.nonzero(got)[0])
    ev.close()


# ---- 6. groups -------------------------------------------------------------------------------------------------------
SC2_S = 1500


def tie_lines(oracle, L, want=40):
    """Lines on which FPC and BPC give the same size, smaller than BDI's: picked with the oracle on the CPU."""
    rng = np.random.default_rng(1000 + L)
    n, W = 200000, L // 4
    k = rng.integers(1, 33, (n, 1)).astype(np.uint64)
    w = rng.integers(0, 1 << 32, (n, W), dtype=np.uint64) & ((np.uint64(1) << k) - np.uint64(1))
    w[rng.random((n, W)) < rng.random((n, 1))] = 0
    base = rng.integers(0, 1 << 32, (n, 1), dtype=np.uint64) * (rng.random((n, 1)) < 0.3)
    pool = ((w + base) & np.uint64(0xFFFFFFFF)).astype("<u4").view(np.uint8).reshape(n, L)
    b = oracle.BdiOracle(L).compress(pool)[0].astype(np.int64)
    f = oracle.FpcOracle(L).compress(pool).astype(np.int64)
    p = oracle.BpcOracle(L).compress(pool).astype(np.int64)
    pick = np.nonzero((f == p) & (f < b))[0][:want]
    assert len(pick) >= 3, f"L={L}: the candidate pool has {len(pick)} FPC/BPC ties"
    return np.ascontiguousarray(pool[pick])


def group_lines(oracle, L):
    """5 000 lines: the fixture generators' lines, zero lines, random lines and FPC/BPC ties, shuffled."""
    rng = np.random.default_rng(77 + L)
    ties = tie_lines(oracle, L)
    parts = [baseline_ref.case_lines({"name": f"group_{c}_L{L}", "comp": c, "L": L, "seed": 9000 + L + i})[:1300]
             for i, c in enumerate(("BDI", "FPC", "BPC"))]
    parts += [np.zeros((300, L), np.uint8), ties]
    rest = 5000 - sum(len(p) for p in parts)
    parts.append(rng.integers(0, 256, (rest, L), dtype=np.uint8))
    lines = np.concatenate(parts)
    assert lines.shape == (5000, L)
    return np.ascontiguousarray(lines[rng.permutation(len(lines))])


def oracle_sizes(oracle, configs, name, L, lines):
    if name == "BDI":
        return oracle.BdiOracle(L).compress(lines)[0].astype(np.int64)
    if name == "FPC":
        return oracle.FpcOracle(L).compress(lines).astype(np.int64)
    if name == "BPC":
        return oracle.BpcOracle(L).compress(lines).astype(np.int64)
    if name == "VPC":
        return oracle.VpcOracle(configs.probe_config(L)).compress(lines)[0].astype(np.int64)
    if name == "SC2":
        return sc2_ref.SC2Ref(L, SC2_S).feed(lines)[0].astype(np.int64)
    return pattern_ref.analyse(lines)[0].astype(np.int64)


def make(mpc, configs, name, L):
    if name == "VPC":
        return mpc.VPC(configs.probe_config(L))
    if name == "SC2":
        return mpc.SC2(L, SC2_S)
    return getattr(mpc, {"PATTERN": "Pattern"}.get(name, name))(L)


@pytest.mark.parametrize("names,L,form", [
    (["BDI", "FPC", "BPC"], 64, "BDI+FPC+BPC: one kernel"),
    (["BDI", "FPC", "BPC"], 40, "BDI: own kernel; FPC: own kernel; BPC: own kernel"),
    (["VPC", "BDI", "FPC", "BPC", "SC2", "PATTERN"], 64, "VPC: unrolled; BDI+FPC+BPC: one kernel; SC2: own kernel; PATTERN: own kernels"),
])
def test_group_histograms_and_best_of(mpc, configs, oracle, names, L, form):
    lines = group_lines(oracle, L)
    n = len(lines)
    want = {name: oracle_sizes(oracle, configs, name, L, lines) for name in names}
    taking_part = [name for name in names if name != "PATTERN"]
    M = np.stack([want[name] for name in taking_part])
    best, winner = M.min(axis=0), M.argmin(axis=0)              # argmin: the first minimal member
    tied = (M == best).sum(axis=0) > 1
    f, p = taking_part.index("FPC"), taking_part.index("BPC")
    assert int(((M[f] == best) & (M[p] == best) & (winner == f)).sum()) >= 3      # real ties that FPC must win
    assert int(tied.sum()) >= 3

    # the same handles fed alone
    solo_hist = []
    for name in names:
        ev = make(mpc, configs, name, L)
        ev.enable_size_histogram()
        ev.compress_lines(lines, want_sizes=False, want_selected=False)
        solo_hist.append(ev.size_histogram())
        same_hist(f"{name} alone against the oracle", solo_hist[-1], bincount(want[name]))
        ev.close()

    members = [make(mpc, configs, name, L) for name in names]
    for ev in members:
        ev.enable_size_histogram()
    group = mpc.EvaluatorSet(members)
    assert group.form == form
    group.enable_best()
    group.enable_best()                                          # idempotent
    cut = 300                                                    # an in-place call, then a staged one
    group.compress_lines(lines[:cut], want_sizes=False, want_selected=False)
    group.compress_lines(lines[cut:], want_sizes=False, want_selected=False)
    for name, ev, alone in zip(names, members, solo_hist):
        same_hist(f"{name} in the group", ev.size_histogram(), alone)
    got = group.best()
    same_hist("best-of", got["bins"], bincount(best))
    want_wins = np.zeros(len(names), np.uint64)
    for k, name in enumerate(taking_part):
        want_wins[names.index(name)] = int((winner == k).sum())
    assert got["wins"].tolist() == want_wins.tolist()
    if "PATTERN" in names:
        assert int(got["wins"][names.index("PATTERN")]) == 0
    assert got["best_bits"] == int(best.sum()) and got["lines"] == n
    assert got["tag_bits"] == {3: 2, 5: 3}[len(taking_part)]

    # the device path on a caller's stream, sizes arrays for some members only (the others: the group's scratch)
    import torch
    group.reset_best()
    for ev in members:
        ev.reset()
    d_lines = torch.from_numpy(lines).to("cuda:0")
    d_sizes = [torch.zeros(n, dtype=torch.int16, device="cuda:0") if i % 2 == 0 else None for i in range(len(names))]
    if "SC2" in names:       # a fresh trace for SC2's line counter: new members
        group.close()
        for ev in members:
            ev.close()
        members = [make(mpc, configs, name, L) for name in names]
        for ev in members:
            ev.enable_size_histogram()
        group = mpc.EvaluatorSet(members)
        group.enable_best()
    group.compress_device(d_lines.data_ptr(), n, [t.data_ptr() if t is not None else 0 for t in d_sizes],
                          stream=torch.cuda.current_stream().cuda_stream)
    for name, ev, alone in zip(names, members, solo_hist):
        same_hist(f"{name} in the group, device path", ev.size_histogram(), alone)
    got = group.best()
    same_hist("best-of, device path", got["bins"], bincount(best))
    assert got["wins"].tolist() == want_wins.tolist() and got["best_bits"] == int(best.sum())
    group.close()
    for ev in members:
        ev.close()


def test_best_of_needs_two_members_that_take_part(mpc):
    members = [mpc.BDI(64), mpc.Pattern(64)]
    group = mpc.EvaluatorSet(members)
    with pytest.raises(mpc.MpcError) as e:
        group.enable_best()
    assert e.value.code == MPC_E_INVAL and "at least two members" in str(e.value)
    with pytest.raises(mpc.MpcError) as e:
        group.best()
    assert e.value.code == MPC_E_INVAL
    group.close()
    for ev in members:
        ev.close()


# ---- 7. life cycle ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["BDI", "VPC"])
def test_life_cycle(mpc, configs, baselines, oracle, name):
    L = 64
    _, lines, _ = baseline_case(baselines, "bdi_L64")
    sizes = oracle_sizes(oracle, configs, name, L, lines)
    plain = make(mpc, configs, name, L)
    form_before = (mpc.lib().mpc_kernel_form(plain._h) or b"").decode()
    ev = make(mpc, configs, name, L)
    with pytest.raises(mpc.MpcError) as e:
        ev.size_histogram()
    assert e.value.code == MPC_E_INVAL and "mpc_size_hist_enable" in str(e.value)
    ev.compress_lines(lines[:1000], want_sizes=False, want_selected=False)
    ev.enable_size_histogram()                                   # only later lines count
    assert int(ev.size_histogram().sum()) == 0
    ev.compress_lines(lines[1000:], want_sizes=False, want_selected=False)
    same_hist("after enabling", ev.size_histogram(), bincount(sizes[1000:]))
    ev.enable_size_histogram()                                   # harmless
    same_hist("after a second enable", ev.size_histogram(), bincount(sizes[1000:]))
    assert int(ev.stats_vector()[0]) == len(lines)
    ev.reset()
    assert int(ev.size_histogram().sum()) == 0 and int(ev.stats_vector()[0]) == 0
    ev.compress_lines(lines[:700], want_sizes=False, want_selected=False)
    same_hist("after a reset", ev.size_histogram(), bincount(sizes[:700]))
    # accounting changes neither the kernel the handle reports nor a group's form
    assert (mpc.lib().mpc_kernel_form(ev._h) or b"").decode() == form_before
    other = mpc.FPC(L)
    g1, g2 = mpc.EvaluatorSet([plain, other]), mpc.EvaluatorSet([ev, other])
    assert g1.form == g2.form
    g1.close()
    g2.close()
    other.close()
    plain.close()
    ev.close()                                                   # destroy with accounting on


# ---- 8. the command line ---------------------------------------------------------------------------------------------
def _csv_rows(path):
    text = open(path).read().split("\n")
    assert text[0] == "Workload,Line Size,Lines,Sector Bytes,Sector Ratio,Sector Classes,Histogram," and text[-1] == "" and len(text) == 3, text[:2]
    return text[1].split(",")


def _check_row(mpc, row, workload, L, sector, bins):
    nz = np.nonzero(bins)[0]
    sec = mpc.size_sectors(bins, L, sector)
    assert row[0] == workload and row[1:4] == [str(L), str(int(bins.sum())), str(sector)]
    assert float(row[4]) == sec["ratio"]
    assert row[5] == ";".join(str(int(c)) for c in sec["classes"])
    assert row[6] == ";".join(f"{int(s)}:{int(bins[s])}" for s in nz)
    assert row[7] == ""


def test_cli_size_files(mpc, configs, baselines, traces, tmp_path):
    pkg("build").build_all()
    cli, bindir = os.path.join(ROOT, "bin", "compressor"), os.path.join(ROOT, "bin")
    L = 64
    _, lines, _ = baseline_case(baselines, "bdi_L64")
    lines = np.ascontiguousarray(lines[np.arange(3000) % len(lines)])
    ds = tmp_path / "ds"
    ds.mkdir()
    npy = traces.save_npy(str(ds / "t.npy"), lines)
    cfg_path = str(tmp_path / "probe.json")
    with open(cfg_path, "w") as f:
        json.dump(configs.probe_config(L), f)
    fed = lines[:-1]                                             # the driver drops the final row

    def run(args, out):
        out.mkdir()
        r = subprocess.run([cli, *args, "-i", npy, "-o", str(out)], cwd=bindir, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        return r.stdout

    def python_hist(name):
        ev = make(mpc, configs, name, L)
        ev.enable_size_histogram()
        ev.compress_lines(fed, want_sizes=False, want_selected=False)
        h = ev.size_histogram()
        ev.close()
        return h

    # one algorithm
    plain_out, out = tmp_path / "bdi_plain", tmp_path / "bdi"
    plain_stdout = run(["-a", "BDI"], plain_out)
    stdout = run(["-a", "BDI", "--size-histogram"], out)
    assert stdout == plain_stdout
    assert "BDI_results.csv" in os.listdir(plain_out)
    for name in os.listdir(plain_out):
        assert (out / name).read_bytes() == (plain_out / name).read_bytes(), name
    assert sorted(os.listdir(plain_out)) == sorted(set(os.listdir(out)) - {"BDI_results_sizes.csv"})
    _check_row(mpc, _csv_rows(out / "BDI_results_sizes.csv"), "ds_t", L, 32, python_hist("BDI"))

    # a list: one file per member, the best of the list, one more line
    names = ["VPC", "BDI", "FPC", "BPC"]
    plain_out, out = tmp_path / "list_plain", tmp_path / "list"
    plain_stdout = run(["-a", ",".join(names), "-c", cfg_path], plain_out)
    stdout = run(["-a", ",".join(names), "-c", cfg_path, "--sector", "32"], out)
    for name in os.listdir(plain_out):
        assert (out / name).read_bytes() == (plain_out / name).read_bytes(), name
    stems = ["probe", "BDI", "FPC", "BPC", "BEST"]
    assert sorted(set(os.listdir(out)) - set(os.listdir(plain_out))) == sorted(f"{s}_results_sizes.csv" for s in stems)
    members = [make(mpc, configs, name, L) for name in names]
    for ev in members:
        ev.enable_size_histogram()
    group = mpc.EvaluatorSet(members)
    group.enable_best()
    group.compress_lines(fed, want_sizes=False, want_selected=False)
    for stem, ev in zip(stems, members):
        _check_row(mpc, _csv_rows(out / f"{stem}_results_sizes.csv"), "ds_t", L, 32, ev.size_histogram())
    best = group.best()
    _check_row(mpc, _csv_rows(out / "BEST_results_sizes.csv"), "ds_t", L, 32, best["bins"])
    out_lines, plain_lines = stdout.strip().split("\n"), plain_stdout.strip().split("\n")
    assert out_lines[:-1] == plain_lines and len(plain_lines) == 4
    label, value = out_lines[-1].split(": ")
    assert label == "BEST comp.ratio"
    assert float(value) == (best["lines"] * 8 * L) / (best["best_bits"] + best["lines"] * best["tag_bits"]) and best["tag_bits"] == 2
    group.close()
    for ev in members:
        ev.close()

    # a sector larger than the line is refused before anything is written
    refused = tmp_path / "refused"
    refused.mkdir()
    r = subprocess.run([cli, "-a", "BDI", "--sector", "128", "-i", npy, "-o", str(refused)], cwd=bindir, capture_output=True, text=True, timeout=600)
    assert r.returncode == 1 and "--sector 128" in r.stdout and os.listdir(refused) == []


# ---- 9. the accounting pass at its full width --------------------------------------------------------------------------
# MPC_SIZES_MAX = 8 arrays a launch; with eight histograms and the best-of one a workgroup keeps nine LDS histograms
# (144 KiB, beyond the 64 KiB a kernel gets by default).
def make_spec(mpc, spec, L):
    """"BDI" / "FPC" / "BPC" / "PATTERN", or ("SC2", S)."""
    if isinstance(spec, tuple):
        return mpc.SC2(L, spec[1])
    return getattr(mpc, {"PATTERN": "Pattern"}.get(spec, spec))(L)


def spec_sizes(oracle, spec, L, lines):
    if isinstance(spec, tuple):
        return sc2_ref.SC2Ref(L, spec[1]).feed(lines)[0].astype(np.int64)
    return oracle_sizes(oracle, None, spec, L, lines)


def open_group(mpc, specs, L, best):
    members = [make_spec(mpc, s, L) for s in specs]
    for ev in members:
        ev.enable_size_histogram()
    group = mpc.EvaluatorSet(members)
    if best:
        group.enable_best()
    return group, members


def close_group(group, members):
    group.close()
    for ev in members:
        ev.close()


def check_wide_group(group, members, specs, want, best_expected, tag):
    for i, (spec, ev) in enumerate(zip(specs, members)):
        same_hist(f"{tag}: member {i} {spec}", ev.size_histogram(), bincount(want[i]))
    if best_expected is None:
        return None
    best, winner, part = best_expected
    got = group.best()
    same_hist(f"{tag}: best-of", got["bins"], bincount(best))
    want_wins = np.zeros(len(specs), np.uint64)
    for k, i in enumerate(part):
        want_wins[i] = int((winner == k).sum())
    assert got["wins"].tolist() == want_wins.tolist(), tag
    assert got["best_bits"] == int(best.sum()) and got["lines"] == len(best), tag
    return got


EIGHT = ["BDI", "FPC", "BPC", ("SC2", 1500), "BDI", "FPC", "BPC", ("SC2", 700)]


def best_of(want, specs):
    part = [i for i, s in enumerate(specs) if s != "PATTERN"]
    M = np.stack([want[i] for i in part])
    return M.min(axis=0), M.argmin(axis=0), part          # argmin: the first minimal member


def test_eight_members_with_best_of(mpc, oracle):
    """Eight arrays and nine LDS histograms in one launch.  Members 4-6 are copies of members 0-2: they tie on every line
    and the first minimal member wins, so they win nothing."""
    import torch
    L = 64
    lines = group_lines(oracle, L)
    n = len(lines)
    want = [spec_sizes(oracle, s, L, lines) for s in EIGHT]
    expected = best_of(want, EIGHT)
    assert len(expected[2]) == 8 and len(set(expected[1].tolist())) >= 3          # several members win somewhere
    # host path: an in-place call, then a staged one
    group, members = open_group(mpc, EIGHT, L, best=True)
    group.compress_lines(lines[:300], want_sizes=False, want_selected=False)
    group.compress_lines(lines[300:], want_sizes=False, want_selected=False)
    got = check_wide_group(group, members, EIGHT, want, expected, "host")
    assert got["wins"][4:7].tolist() == [0, 0, 0] and int(got["wins"].sum()) == n
    assert got["tag_bits"] == 3
    close_group(group, members)
    # device path: fresh members (SC2 counts its lines), the caller's sizes arrays for every other member
    group, members = open_group(mpc, EIGHT, L, best=True)
    d_lines = torch.from_numpy(lines).to("cuda:0")
    d_sizes = [torch.zeros(n, dtype=torch.int16, device="cuda:0") if i % 2 == 0 else None for i in range(len(EIGHT))]
    group.compress_device(d_lines.data_ptr(), n, [t.data_ptr() if t is not None else 0 for t in d_sizes],
                          stream=torch.cuda.current_stream().cuda_stream)
    got = check_wide_group(group, members, EIGHT, want, expected, "device")
    assert got["wins"][4:7].tolist() == [0, 0, 0] and got["tag_bits"] == 3
    for i, t in enumerate(d_sizes):
        if t is not None:
            assert (t.cpu().numpy().view(np.uint16) == want[i]).all(), i
    close_group(group, members)


def test_nine_members_take_two_launches_and_no_best_of(mpc, oracle):
    """More members than one launch takes: best-of is refused, and without it the nine histograms come from two
    launches of the pass (eight arrays, then one)."""
    import torch
    L = 64
    specs = EIGHT + [("SC2", 300)]
    lines = group_lines(oracle, L)
    n = len(lines)
    want = [spec_sizes(oracle, s, L, lines) for s in specs]
    group, members = open_group(mpc, specs, L, best=False)
    with pytest.raises(mpc.MpcError) as e:
        group.enable_best()
    assert e.value.code == MPC_E_INVAL and "at most 8" in str(e.value)
    with pytest.raises(mpc.MpcError) as e:
        group.best()
    assert e.value.code == MPC_E_INVAL
    group.compress_lines(lines[:300], want_sizes=False, want_selected=False)
    group.compress_lines(lines[300:], want_sizes=False, want_selected=False)
    check_wide_group(group, members, specs, want, None, "host")
    close_group(group, members)
    group, members = open_group(mpc, specs, L, best=False)
    d_lines = torch.from_numpy(lines).to("cuda:0")
    group.compress_device(d_lines.data_ptr(), n, stream=torch.cuda.current_stream().cuda_stream)
    check_wide_group(group, members, specs, want, None, "device")
    close_group(group, members)


def test_eight_members_and_a_pattern_member(mpc, oracle):
    """A Pattern member does not take part: best-of over the other eight is accepted, Pattern wins nothing, and its
    histogram comes from a launch of its own."""
    L = 64
    specs = EIGHT[:3] + ["PATTERN"] + EIGHT[3:]
    lines = group_lines(oracle, L)
    want = [spec_sizes(oracle, s, L, lines) for s in specs]
    expected = best_of(want, specs)
    assert expected[2] == [0, 1, 2, 4, 5, 6, 7, 8]
    group, members = open_group(mpc, specs, L, best=True)
    group.compress_lines(lines[:300], want_sizes=False, want_selected=False)
    group.compress_lines(lines[300:], want_sizes=False, want_selected=False)
    got = check_wide_group(group, members, specs, want, expected, "host")
    assert int(got["wins"][3]) == 0 and got["wins"][5:8].tolist() == [0, 0, 0] and got["tag_bits"] == 3
    close_group(group, members)


# ---- 10. the pass alone, on synthetic sizes ----------------------------------------------------------------------------
# mpc_launch_sizes and mpc_sizes_wg_per_cu (csrc/mpc_sizes.hip) are extern "C" and exported by libmpc_hip.so: called through
# ctypes on torch-owned arrays, against numpy.
SIZES_MAX = 8
BEST_LEN = BINS + SIZES_MAX + 1
SPECIAL_SIZES = np.array([0, 1, 4094, 4095, 4096, 0x7FFF, 0x8000, 0xFFFF], dtype=np.uint16)


def sizes_abi(mpc):
    import ctypes as C

    class MpcSizesArgs(C.Structure):          # csrc/mpc_sizes.h
        _fields_ = [("sizes", C.c_void_p * SIZES_MAX), ("hist", C.c_void_p * SIZES_MAX), ("best", C.c_void_p), ("m", C.c_int)]
    lib = mpc.lib()
    lib.mpc_launch_sizes.argtypes = [C.POINTER(MpcSizesArgs), C.c_uint64, C.c_int, C.c_void_p]
    lib.mpc_launch_sizes.restype = C.c_int
    lib.mpc_sizes_wg_per_cu.argtypes = [C.POINTER(MpcSizesArgs)]
    lib.mpc_sizes_wg_per_cu.restype = C.c_int
    return lib, MpcSizesArgs


def synthetic_sizes(rng, n, kind):
    """kind 0: the special sizes and random ones, line by line.  kind 1: per 512 lines (what a wave takes per loop
    step: 64 lanes x 8 lines) one, two, three and 64 distinct values across the lanes -- the two aggregation rounds and
    the lane-by-lane remainder of wave_hist_add."""
    palette = np.concatenate([SPECIAL_SIZES, rng.integers(0, 1 << 16, 56).astype(np.uint16)])
    if kind == 0:
        draw = palette[rng.integers(0, len(palette), n)]
        return np.where(rng.random(n) < 0.5, draw, rng.integers(0, 2300, n).astype(np.uint16)).astype(np.uint16)
    i = np.arange(n)
    lane, segment = (i // 8) % 64, i // 512
    distinct = np.array([1, 2, 3, 64])[segment % 4]
    return rng.permutation(palette)[lane % distinct].astype(np.uint16)


def test_the_pass_alone_on_synthetic_sizes(mpc):
    import ctypes as C
    import torch
    lib, MpcSizesArgs = sizes_abi(mpc)
    rng = np.random.default_rng(4096)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    case = 0
    for m in range(1, SIZES_MAX + 1):
        for n in (1, 7, 8, 9, 511, 512, 513, 2051):
            for one_workgroup in (True, False):
                case += 1
                with_best = m >= 2 and case % 4 != 0
                no_hist = [(i + case) % 3 == 0 for i in range(m)]
                shifted = case % m if case % 2 else -1        # this member's array starts one element in: 2-byte loads for all
                host = [synthetic_sizes(rng, n, (i + case) % 2) for i in range(m)]
                dev = [torch.from_numpy(np.concatenate([np.full(8, 0x1111, np.uint16), a, np.full(8, 0x2222, np.uint16)]).view(np.int16)).to("cuda:0")
                       for a in host]
                d_hist = [None if no_hist[i] else torch.zeros(BINS, dtype=torch.int64, device="cuda:0") for i in range(m)]
                d_best = torch.zeros(BEST_LEN, dtype=torch.int64, device="cuda:0") if with_best else None
                A = MpcSizesArgs()
                A.m = m
                for i in range(m):
                    A.sizes[i] = dev[i].data_ptr() + 2 * (8 + (1 if i == shifted else 0))
                    A.hist[i] = None if no_hist[i] else d_hist[i].data_ptr()
                A.best = d_best.data_ptr() if with_best else None
                n_hist = sum(not x for x in no_hist) + (1 if with_best else 0)
                per_cu = lib.mpc_sizes_wg_per_cu(C.byref(A))          # (pinned to its documented formula: a regression pin, not a second opinion)
                assert per_cu == (0 if n_hist == 0 else min(8, (160 * 1024) // (n_hist * BINS * 4 + 128))), (m, n_hist, per_cu)
                grid = 1 if one_workgroup else max(1, per_cu * cus)
                torch.cuda.synchronize()
                assert lib.mpc_launch_sizes(C.byref(A), n, grid, None) == 0, (m, n, grid)
                torch.cuda.synchronize()
                tag = f"m={m} n={n} grid={grid} best={with_best} no_hist={no_hist} shifted={shifted}"
                # the member whose array is shifted reads elements 1 .. n of its data (the last one is the 0x2222 behind it)
                seen = [np.concatenate([a[1:], [0x2222]]).astype(np.uint16) if i == shifted else a for i, a in enumerate(host)]
                for i in range(m):
                    if not no_hist[i]:
                        same_hist(f"{tag}: member {i}", d_hist[i].cpu().numpy().view(np.uint64),
                                  bincount(np.minimum(seen[i].astype(np.int64), BINS - 1)))
                if with_best:
                    M = np.stack([a.astype(np.int64) for a in seen])
                    best, winner = M.min(axis=0), M.argmin(axis=0)
                    got = d_best.cpu().numpy().view(np.uint64)
                    same_hist(f"{tag}: best-of", got[:BINS].copy(), bincount(np.minimum(best, BINS - 1)))
                    assert got[BINS:BINS + SIZES_MAX].tolist() == np.bincount(winner, minlength=SIZES_MAX).tolist(), tag
                    assert int(got[BINS + SIZES_MAX]) == int(best.sum()), tag          # the unclipped sizes
    # refused: no array, more than eight, a best-of over one member
    A = MpcSizesArgs()
    for m in (0, SIZES_MAX + 1):
        A.m = m
        assert lib.mpc_launch_sizes(C.byref(A), 8, 1, None) != 0
    A.m = 1
    scratch = torch.zeros(BEST_LEN, dtype=torch.int64, device="cuda:0")
    A.sizes[0], A.best = scratch.data_ptr(), scratch.data_ptr()
    assert lib.mpc_launch_sizes(C.byref(A), 8, 1, None) != 0
    torch.cuda.synchronize()
    assert not scratch.any()
