"""The two Fit analyses on the GPU.  Every comparison is exact integer equality against tests/fit_ref.py (the definitions
in numpy, checked against a plain loop by tests/test_fit_cpu.py)."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, pkg

import fit_ref
import footprint as F

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1025)
with open(os.path.join(ROOT, "cal_22-mpc_amd", "csrc", "mpc_fit.h")) as _f:
    S = int(re.search(r"#define MPC_FIT_SPILL_LINES\s+(\d+)\b", _f.read()).group(1))


@pytest.fixture(scope="module")
def mpc():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("these tests need an MI355X")
    m = pkg()
    m.lib()
    return m


def _same(tag, got, want):
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{tag}: {bad.size} of {got.size} differ, first at {bad[:6].tolist()}: {got[bad[:6]].tolist()} vs {want[bad[:6]].tolist()}"


def random_lines(n, L, seed=11):
    return np.random.default_rng(seed + L).integers(0, 256, size=(n, L), dtype=np.uint8)


def base_tables(L):
    """The three base tables of the residue tests: one word back, all 0, any byte of the line (forward references and
    base[i] == i included: the handle takes any table, only the fit restricts itself)."""
    rnd = [int(b) for b in np.random.default_rng(100 + L).integers(0, L, L)]
    assert any(b > i for i, b in enumerate(rnd))
    return {"prev word": [max(i - 4, 0) for i in range(L)], "zero": [0] * L, "random": rnd}


def constant_lines(kind, n, L):
    if kind == "zero":
        return np.zeros((n, L), dtype=np.uint8)
    if kind == "index":
        return np.ascontiguousarray(np.tile(np.arange(L, dtype=np.uint8), (n, 1)))
    return np.ascontiguousarray(np.tile(np.array([0x00, 0xFF] * (L // 2), dtype=np.uint8), (n, 1)))


# ---- the pair table ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [32, 64, 128])
def test_pairs_sizes(mpc, L):
    pool = random_lines(max(SIZES), L)
    full = fit_ref.pair_table(pool)
    off_diagonal = full[~np.eye(L, dtype=bool)]
    # every bin is populated in nearly every pair i != j (bins 0 and 1 take one line in 256: (255/256)^1025 = 0.018 stay empty)
    assert (off_diagonal > 0).mean(axis=0).min() > 0.95 and (off_diagonal[:, 3:] > 0).all()
    for n in SIZES:
        ev = mpc.FitPairs(L)
        assert ev.compress_lines(pool[:n]) == (None, None)
        _same(f"pairs L={L} n={n}", ev.stats_vector(), fit_ref.pairs_vector(pool[:n]))
        assert ev.lines() == n and ev.table().shape == (L, L, 9)
        ev.close()


@pytest.mark.parametrize("kind", ["zero", "index", "alternating"])
@pytest.mark.parametrize("L", [32, 64, 128])
def test_pairs_constant_lines_at_the_spill_interval(mpc, L, kind):
    """Every increment of a pair lands in ONE counter: a field that wrapped, or a carry out of the top bin, shows."""
    for n in (S - 1, S, S + 1, 2 * S + 1):
        lines = constant_lines(kind, n, L)
        want = fit_ref.pair_table(lines)
        assert set(np.unique(want).tolist()) <= {0, n}
        if kind == "alternating":
            assert int(want[1, 0, 8]) == n and int(want[0, 2, 0]) == n and int(want[0, 1, 1]) == n      # 255 - 0, 0 - 0, 0 - 255 = 1: bins 8, 0 and 1
        if kind == "index":
            assert [int(np.argmax(want[d, 0])) for d in (0, 1, 2, 4, 8, 16, 31)] == [0, 1, 2, 3, 4, 5, 5] and int(want[0, 1, 8]) == n
        for via in ("host", "device"):
            ev = mpc.FitPairs(L)
            if via == "host":
                ev.compress_lines(lines)
            else:
                import torch
                d = torch.from_numpy(lines).to("cuda:0")
                ev.compress_device(d.data_ptr(), n)
                ev.sync()
            _same(f"pairs {kind} L={L} n={n} {via}", ev.table(), want)
            assert ev.lines() == n
            ev.close()


@pytest.mark.parametrize("L,n", [(32, 100003), (128, 20001)])
def test_pairs_many_workgroups(mpc, L, n):
    import torch
    lines = fit_ref.records16(n, L, 5)
    want = fit_ref.pairs_vector(lines)
    ev = mpc.FitPairs(L)
    assert ev.info.algorithm == 7 and ev.kernel_path == mpc.MPC_PATH_FIT_PAIRS == 11 and ev.stats_len == 3 + 9 * L * L
    assert ev.kernel_form == "one lane per byte pair"
    d = torch.from_numpy(lines).to("cuda:0")
    ev.compress_device(d.data_ptr(), n)
    _same(f"pairs device L={L} n={n}", ev.stats_vector(), want)
    ev.reset()
    ev.compress_lines(lines)      # the staged path: chunks on two streams
    _same(f"pairs staged L={L} n={n}", ev.stats_vector(), want)
    ev.close()


@pytest.mark.parametrize("L", [32, 64, 128])
def test_calls_add_reset_clears_merge_adds_and_raw_exchange(mpc, L):
    import torch
    a, b = fit_ref.stride_u32(300, L, 3), random_lines(77, L)
    va, vb = fit_ref.pairs_vector(a), fit_ref.pairs_vector(b)
    ev, other = mpc.FitPairs(L), mpc.FitPairs(L)
    ev.compress_lines(a)
    ev.compress_lines(b)
    _same("two calls", ev.stats_vector(), va + vb)
    other.compress_lines(b)
    ev.stats_merge(other.stats_vector())
    _same("merge", ev.stats_vector(), va + vb + vb)
    # the raw accumulators, as a device-side all-reduce would move them (merged-in statistics are not part of them)
    n_raw = ev.stats_raw_len()
    assert n_raw == 1 + 8 * L * L
    d_raw = torch.zeros(n_raw, dtype=torch.int64, device="cuda:0")
    ev.sync()
    ev.stats_copy_raw_device(d_raw.data_ptr())
    torch.cuda.synchronize()
    _same("from raw", ev.stats_from_raw(d_raw.cpu().numpy().view(np.uint64)), va + vb)
    ev.stats_set(va)
    _same("set", ev.stats_vector(), va)
    ev.reset()
    assert not ev.stats_vector().any()
    ev.compress_lines(b)
    _same("after reset", ev.stats_vector(), vb)
    d_raw.zero_()
    ev.sync()
    ev.stats_copy_raw_device(d_raw.data_ptr())
    torch.cuda.synchronize()
    _same("from raw == stats_vector", ev.stats_from_raw(d_raw.cpu().numpy().view(np.uint64)), ev.stats_vector())
    # the same for the residue histogram
    base = base_tables(L)["random"]
    rv, ro = mpc.FitResidues(L, base), mpc.FitResidues(L, base)
    wa, wb = fit_ref.residues_vector(a, base), fit_ref.residues_vector(b, base)
    rv.compress_lines(a)
    rv.compress_lines(b)
    _same("residues two calls", rv.stats_vector(), wa + wb)
    assert rv.stats_raw_len() == 1 + 256 * L
    d_raw = torch.zeros(rv.stats_raw_len(), dtype=torch.int64, device="cuda:0")
    rv.sync()
    rv.stats_copy_raw_device(d_raw.data_ptr())
    torch.cuda.synchronize()
    _same("residues from raw", rv.stats_from_raw(d_raw.cpu().numpy().view(np.uint64)), rv.stats_vector())
    ro.compress_lines(a)
    rv.stats_merge(ro.stats_vector())
    _same("residues merge", rv.stats_vector(), wa + wb + wa)
    rv.reset()
    assert not rv.stats_vector().any()
    for e in (ev, other, rv, ro):
        e.close()


def _footprint_call(ev, want_vector, lines, off, poison, tag):
    """tests/footprint.py's input side for a handle without per-line outputs: the lines inside a larger tensor of the
    test's own, poison around them; the statistics are the reference's for exactly these lines and the tensor is unchanged."""
    import torch
    n, L = lines.shape
    host = F._poison(F.IN_MARGIN + off + n * L + F.IN_MARGIN, poison)
    host[F.IN_MARGIN + off:F.IN_MARGIN + off + n * L] = lines.reshape(-1)
    d_in = torch.from_numpy(host).to("cuda:0")
    p = d_in.data_ptr() + F.IN_MARGIN + off
    assert p % 16 == 0
    torch.cuda.synchronize()
    ev.reset()
    ev.compress_device(p, n)
    ev.sync()
    torch.cuda.synchronize()
    tag = f"{tag} L={L} n={n} off={off} poison={'zero' if poison == 0 else 'random'}"
    _same(tag, ev.stats_vector(), want_vector)
    back = d_in.cpu().numpy()
    changed = np.nonzero(back != host)[0]
    assert changed.size == 0, f"{tag}: the input tensor changed at {changed.size} bytes"


@pytest.mark.parametrize("L", [32, 64, 128])
def test_pairs_footprint(mpc, L):
    pool = F.line_pool(pkg("traces"), L, max(SIZES))
    ev = mpc.FitPairs(L)
    for n in SIZES:
        want = fit_ref.pairs_vector(pool[:n])
        for off in (0, 16):
            for poison in F.POISON_SEEDS:
                _footprint_call(ev, want, pool[:n], off, poison, "pairs")
    ev.close()


# ---- the residue histogram ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [32, 64, 128])
def test_residues_sizes_offsets_and_base_tables(mpc, L):
    pool = F.line_pool(pkg("traces"), L, max(SIZES))
    for name, base in base_tables(L).items():
        ev = mpc.FitResidues(L, base)
        assert ev.base_table == base and ev.kernel_path == mpc.MPC_PATH_FIT_RESIDUES == 12 and ev.info.algorithm == 7
        assert ev.stats_len == 3 + 256 * L and ev.kernel_form == "one lane per byte"
        out = np.zeros(L, dtype=np.uint8)      # mpc_fit_base_table round-trips
        assert mpc.lib().mpc_fit_base_table(ev._h, out.ctypes.data, L) == 0 and out.tolist() == base
        assert mpc.lib().mpc_fit_base_table(ev._h, out.ctypes.data, L - 1) == -22
        for n in SIZES:
            want = fit_ref.residues_vector(pool[:n], base)
            for off in (0, 16):
                for poison in F.POISON_SEEDS:
                    _footprint_call(ev, want, pool[:n], off, poison, f"residues {name}")
            ev.reset()
            assert ev.compress_lines(pool[:n]) == (None, None)
            _same(f"residues {name} host L={L} n={n}", ev.stats_vector(), want)
            assert ev.table().shape == (L, 256) and ev.lines() == n
        ev.close()
    pairs = mpc.FitPairs(L)
    out = np.zeros(L, dtype=np.uint8)
    assert mpc.lib().mpc_fit_base_table(pairs._h, out.ctypes.data, L) == -22      # a handle of another kind
    bdi = mpc.BDI(L)
    assert mpc.lib().mpc_fit_base_table(bdi._h, out.ctypes.data, L) == -22
    bdi.close()
    pairs.close()


@pytest.mark.parametrize("L,n", [(32, 100003), (128, 20001)])
def test_residues_many_workgroups(mpc, L, n):
    import torch
    lines = fit_ref.records16(n, L, 5)
    base = base_tables(L)["prev word"]
    ev = mpc.FitResidues(L, base)
    d = torch.from_numpy(lines).to("cuda:0")
    ev.compress_device(d.data_ptr(), n)
    _same(f"residues L={L} n={n}", ev.stats_vector(), fit_ref.residues_vector(lines, base))
    ev.close()


# ---- files ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [32, 128])
def test_trace_files_equal_the_array_path(mpc, traces, tmp_path, L):
    lines = fit_ref.records16(3000, L, 9)
    npy = traces.save_npy(str(tmp_path / "t.npy"), lines)
    log = traces.write_gpgpusim_log(str(tmp_path / "t.log"), lines)
    base = base_tables(L)["prev word"]
    for make, vector in ((lambda: mpc.FitPairs(L), fit_ref.pairs_vector), (lambda: mpc.FitResidues(L, base), lambda x: fit_ref.residues_vector(x, base))):
        ev = make()
        assert ev.compress_npy(npy, skip_last_row=False) == 3000
        _same("npy", ev.stats_vector(), vector(lines))
        ev.reset()
        assert ev.compress_npy(npy) == 2999      # the reference driver never compresses the last row
        _same("npy, skip_last_row", ev.stats_vector(), vector(lines[:2999]))
        ev.reset()
        assert ev.compress_gpgpusim_log(log) == (3000, 3000)
        _same("log", ev.stats_vector(), vector(lines))
        ev.close()
    # requests of every type: only global reads (0) and writes (4) are lines
    types = np.arange(3000) % 9
    log = traces.write_gpgpusim_log(str(tmp_path / "m.log"), lines, req_types=types)
    kept = lines[(types == 0) | (types == 4)]
    ev = mpc.FitPairs(L)
    assert ev.compress_gpgpusim_log(log) == (3000, len(kept))
    _same("log, mixed request types", ev.stats_vector(), fit_ref.pairs_vector(kept))
    ev.close()


# ---- refusals ------------------------------------------------------------------------------------------------------------
def test_refusals(mpc):
    def refused(call):
        with pytest.raises(mpc.MpcError) as e:
            call()
        assert e.value.code == -22 and str(e.value).split(": ", 1)[1].startswith("Fit"), str(e.value)

    refused(lambda: mpc.FitPairs(48))
    refused(lambda: mpc.FitResidues(48, [0] * 48))
    refused(lambda: mpc.FitResidues(64, [0] * 63 + [64]))
    lines = random_lines(10, 64)
    for ev in (mpc.FitPairs(64), mpc.FitResidues(64, [0] * 64)):
        refused(lambda: ev.compress_lines(lines, want_sizes=True, want_selected=False))
        refused(lambda: ev.compress_lines(lines, want_sizes=False, want_selected=True))
        import torch
        d = torch.from_numpy(lines).to("cuda:0")
        out = torch.zeros(64, dtype=torch.int16, device="cuda:0")
        refused(lambda: ev.compress_device(d.data_ptr(), 10, d_sizes=out.data_ptr()))
        refused(lambda: ev.compress_device(d.data_ptr(), 10, d_selected=out.data_ptr()))
        refused(ev.enable_size_histogram)
        assert not ev.stats_vector().any()      # nothing was counted by a refused call
        bdi = mpc.BDI(64)
        refused(lambda: mpc.EvaluatorSet([bdi, ev]))
        ev.compress_lines(lines)                 # and the handle is still good
        assert ev.lines() == 10
        bdi.close()
        ev.close()


# ---- fit end to end ------------------------------------------------------------------------------------------------------
def test_fit_config_end_to_end(mpc, traces, tmp_path):
    fit = pkg("fit")
    lines = fit_ref.records16(4096, 64, 1)
    r = fit.fit_config(lines, with_models="mpc")
    assert set(r) == {"config", "base", "diff", "lines", "ratio_fitted", "ratio_without", "kernel_form", "path_reason"}
    base = fit.fit_base_table(fit_ref.pair_table(lines))
    diff = fit.fit_diff_table(fit_ref.residue_table(lines, base))
    assert r["base"] == base and r["diff"] == diff and r["lines"] == 4096
    print(f"ratio_fitted {r['ratio_fitted']:.4f} ratio_without {r['ratio_without']:.4f} form {r['kernel_form']!r} reason {r['path_reason']!r}")
    assert r["ratio_fitted"] > r["ratio_without"]
    assert r["config"]["overview"]["num_modules"] == 8 and r["kernel_form"]
    # the script form writes a file that VPC(path) loads
    npy = traces.save_npy(str(tmp_path / "t.npy"), lines)
    cfg_path = str(tmp_path / "cfg.json")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "cal_22-mpc_amd", "fit.py"), "--trace", npy, "--with", "mpc", "-o", cfg_path],
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    printed = json.loads(p.stdout.strip().splitlines()[-1])
    assert "config" not in printed and printed["base"] == base and printed["diff"] == diff and printed["lines"] == 4096
    assert printed["ratio_fitted"] == r["ratio_fitted"] and printed["ratio_without"] == r["ratio_without"]
    with open(cfg_path) as f:
        assert json.load(f) == r["config"]
    v = mpc.VPC(cfg_path)
    v.compress_lines(lines, False, False)
    assert v.num_modules == 8 and v.result()["comp_ratio"] == r["ratio_fitted"]
    v.close()
    # windowed: the tables land on an unrolled form
    w = fit.fit_config(lines, with_models="none", windowed=True, lines=1000)
    assert w["lines"] == 1000 and all(b >= max(0, 4 * (i // 4) - 4) for i, b in enumerate(w["base"]))
    assert w["kernel_form"].startswith("unrolled") and w["path_reason"] == ""
