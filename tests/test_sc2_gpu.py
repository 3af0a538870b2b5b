"""SC2 on the MI355X: per-line sizes, `selected`, the statistics vector and the table against the reference's own
outputs (tests/golden/ref_sc2_vectors.json) and the numpy restatement (tests/sc2_ref.py), with line S (where the
table is built) at every kind of boundary of every ingestion path."""
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, pkg

import sc2_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mpc():
    return pkg()


@pytest.fixture(scope="module")
def fixture(golden_dir):
    with open(os.path.join(golden_dir, "ref_sc2_vectors.json")) as f:
        return json.load(f)["cases"]


def _check_against_ref(ev, ref, sizes, sel, want_sizes, want_sel):
    assert (sizes == want_sizes).all(), np.nonzero(sizes != want_sizes)[0][:10]
    assert (sel == want_sel).all()
    assert ev.stats_vector().tolist() == ref.stats_vector().tolist()
    sym, lens = ev.table()
    assert sym.tolist() == ref.table_syms.tolist() and lens.tolist() == ref.table_lens.tolist()


def test_reference_fixture(mpc, fixture):
    for case in fixture:
        lines = sc2_ref.case_input(case)
        assert sc2_ref.digest(lines) == case["sha256"]
        W = case["L"] // 4
        ev = mpc.SC2(case["L"], case["S"], device=0)
        assert ev.kernel_path == mpc.MPC_PATH_SC2 and ev.kernel_form == "warm-up counting"
        sizes, sel = ev.compress_lines(lines)
        frm = case["sizes_from"]
        assert (sizes[:frm] == 33 * W).all(), case["name"]
        assert sizes[frm:].tolist() == case["sizes"], case["name"]
        S = min(case["S"], len(lines))
        assert (sel[:S] == 0).all() and (sel[S:] == 1).all()
        sym, lens = ev.table()
        assert [[int(s), int(l)] for s, l in zip(sym, lens)] == case["table"], case["name"]
        r = ev.result()
        assert (r["original_bits"], r["compressed_bits"], r["name"]) == (case["original"], case["compressed"], "SC2-Huffman")
        ref = sc2_ref.SC2Ref(case["L"], case["S"])
        ref.feed(lines)
        assert ev.stats_vector().tolist() == ref.stats_vector().tolist(), case["name"]
        assert ev.kernel_form == ("table sizing" if len(lines) > case["S"] else "warm-up counting")
        ev.close()


def _zipf_lines(n, L, seed):
    rng = np.random.default_rng(seed)
    pool = rng.integers(0, 1 << 32, size=4000, dtype=np.uint64).astype(np.uint32)
    p = 1.0 / np.arange(1, len(pool) + 1) ** 1.05
    p /= p.sum()
    words = pool[rng.choice(len(pool), size=n * (L // 4), p=p)]
    noise = rng.random(words.size) < 0.1
    words = np.where(noise, rng.integers(0, 1 << 32, size=words.size, dtype=np.uint64).astype(np.uint32), words)
    return words.astype("<u4").view(np.uint8).reshape(n, L)


@pytest.mark.parametrize("L,S,chunks", [
    (64, 250, [100, 100, 100, 100]),         # line S inside a <= 512-line call
    (64, 300, [100, 200, 100, 50]),          # line S at a call boundary
    (32, 700, [2000]),                       # inside one staged call
    (128, 900, [300, 300, 300, 1, 499]),     # the build triggered by a one-line call
    (36, 500, [256, 600]),                   # a line size that is not a multiple of 16 bytes
])
def test_line_s_inside_and_at_call_boundaries(mpc, L, S, chunks):
    lines = _zipf_lines(sum(chunks), L, seed=L + S)
    ev, ref = mpc.SC2(L, S, device=0), sc2_ref.SC2Ref(L, S)
    at = 0
    for c in chunks:
        s, k = ev.compress_lines(lines[at:at + c])
        rs, rk = ref.feed(lines[at:at + c])
        assert (s == rs).all() and (k == rk).all(), (at, c)
        at += c
    _check_against_ref(ev, ref, s, k, rs, rk)


@pytest.mark.parametrize("S", [1 << 20, (1 << 20) + 12345, (1 << 20) - 1])
def test_line_s_at_and_inside_staging_slots(mpc, S):
    """64-byte lines: a 64 MiB staging slot holds exactly 2^20 of them, so S = 2^20 falls on a slot boundary."""
    L, n = 64, 3_000_000
    lines = _zipf_lines(n, L, seed=S & 0xffff)
    ev, ref = mpc.SC2(L, S, device=0), sc2_ref.SC2Ref(L, S)
    s, k = ev.compress_lines(lines)
    rs, rk = ref.feed(lines)
    _check_against_ref(ev, ref, s, k, rs, rk)
    assert ev.result()["table_symbols"] == 1024


def test_device_path_across_calls(mpc):
    import torch
    L, S = 64, 5000
    lines = _zipf_lines(20000, L, seed=5)
    ref = sc2_ref.SC2Ref(L, S)
    rs, rk = ref.feed(lines)
    ev = mpc.SC2(L, S, device=0)
    d = torch.from_numpy(lines).to("cuda:0")
    ds = torch.zeros(len(lines), dtype=torch.int16, device="cuda:0")
    dk = torch.full((len(lines),), -1, dtype=torch.int8, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    for a, b in ((0, 3000), (3000, 7000), (7000, 7001), (7001, 20000)):     # line S inside the second call
        ev.compress_device(d[a:].data_ptr(), b - a, ds[a:].data_ptr(), dk[a:].data_ptr(), stream=stream)
    ev.sync()
    torch.cuda.synchronize()
    _check_against_ref(ev, ref, ds.cpu().numpy().view(np.uint16), dk.cpu().numpy(), rs, rk)


def test_npy_with_s_from_all_rows(mpc, traces, tmp_path):
    L = 64
    lines = _zipf_lines(30001, L, seed=6)
    path = traces.save_npy(str(tmp_path / "t.npy"), lines)
    S = mpc.sc2_sampling_lines(len(lines))                      # numLines counts the row the driver never evaluates
    assert S == 10000
    ev, ref = mpc.SC2(L, S, device=0), sc2_ref.SC2Ref(L, S)
    assert ev.compress_npy(path) == len(lines) - 1
    ref.feed(lines[:-1])
    assert ev.stats_vector().tolist() == ref.stats_vector().tolist()
    assert ev.table()[0].tolist() == ref.table_syms.tolist() and ev.table()[1].tolist() == ref.table_lens.tolist()


def test_gpgpusim_log_counts_filtered_lines(mpc, traces, tmp_path):
    L = 64
    lines = _zipf_lines(30000, L, seed=7)
    types = np.random.default_rng(8).choice([0, 4, 1, 2], size=len(lines), p=[0.45, 0.45, 0.05, 0.05])
    path = traces.write_gpgpusim_log(str(tmp_path / "t.log"), lines, types)
    S = mpc.sc2_sampling_lines(len(lines))                      # from every record, as GetNumLines() counts them
    kept = lines[(types == 0) | (types == 4)]
    assert len(kept) > S
    ev, ref = mpc.SC2(L, S, device=0), sc2_ref.SC2Ref(L, S)
    req, done = ev.compress_gpgpusim_log(path)
    assert (req, done) == (len(lines), len(kept))
    ref.feed(kept)
    assert ev.stats_vector().tolist() == ref.stats_vector().tolist()
    assert ev.table()[0].tolist() == ref.table_syms.tolist()


def test_all_zero_million_line_warmup(mpc):
    L, S = 64, 1_000_000
    lines = np.zeros((S + 1000, L), dtype=np.uint8)
    lines[S + 500:, :4] = 7                                      # one word per line that is not in the table
    ev = mpc.SC2(L, S, device=0)
    s, k = ev.compress_lines(lines)
    assert (s[:S] == 16 * 33).all() and (s[S:S + 500] == 0).all() and (s[S + 500:] == 33).all()
    assert (k[:S] == 0).all() and (k[S:] == 1).all()
    assert ev.table()[0].tolist() == [0] and ev.table()[1].tolist() == [0]
    v = ev.stats_vector().tolist()
    assert v == [S + 1000, (S + 1000) * 512, S * 16 * 33 + 500 * 33, S, 1, 1000 * 16 - 500]


def test_stats_reset_keeps_table_and_line_counter(mpc):
    L, S = 32, 400
    lines = _zipf_lines(1000, L, seed=9)
    ev, ref = mpc.SC2(L, S, device=0), sc2_ref.SC2Ref(L, S)
    ev.compress_lines(lines[:300])
    ref.feed(lines[:300])
    ev.reset()
    s, _ = ev.compress_lines(lines[300:])
    rs, _ = ref.feed(lines[300:])
    assert (s == rs).all()
    v = ev.stats_vector()
    assert v[0] == 700 and v[3] == 100 and v[2] == int(rs.sum()) and v[4] == len(ref.table_syms)


def test_rejected_arguments(mpc):
    with pytest.raises(mpc.MpcError) as e:
        mpc.SC2(64, 0, device=0)
    assert e.value.code == -22
    with pytest.raises(mpc.MpcError) as e:
        mpc.SC2(30, 100, device=0)
    assert e.value.code == -22


@pytest.mark.parametrize("L", [32, 64, 128])
def test_sample_beyond_2_28_words_is_refused(mpc, L):
    """A warm-up count and a slot index are 32 bits wide: S * W <= 2^28 keeps both in range.  One line more than that is
    refused before anything is allocated, and so is a line count whose product with W wraps a 64-bit word."""
    W = L // 4
    for S in ((1 << 28) // W + 1, (1 << 28) + 1, (1 << 64) // W):
        with pytest.raises(mpc.MpcError) as e:
            mpc.SC2(L, S, device=0)
        assert e.value.code == -22 and "2^28 words" in str(e.value), (L, S, str(e.value))


def test_cpp_mirror_runs_the_reference_loop(mpc, traces, tmp_path):
    host = os.path.join(ROOT, "cal_22-mpc_amd", "host")
    libdir = os.path.join(ROOT, "cal_22-mpc_amd")
    exe = str(tmp_path / "sc2_probe")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", host, "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "native", "sc2_probe.cpp"), os.path.join(host, "SC2.cpp"), os.path.join(host, "DeviceCompressor.cpp"),
                    os.path.join(host, "Compressor.cpp"), os.path.join(host, "CompResult.cpp"), os.path.join(host, "LoaderNPY.cpp"),
                    os.path.join(host, "LoaderGPGPU.cpp"), os.path.join(host, "LoaderAPSim.cpp"), os.path.join(host, "utils.cpp"),
                    "-L", libdir, "-lmpc_hip", f"-Wl,-rpath,{libdir}", "-o", exe], check=True, capture_output=True, text=True)
    L, S = 64, 1500
    lines = _zipf_lines(4001, L, seed=10)
    binf = str(tmp_path / "lines.bin")
    lines[:-1].tofile(binf)
    npy = traces.save_npy(str(tmp_path / "t.npy"), lines)
    r = subprocess.run([exe, binf, npy, str(L), str(S)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    ref = sc2_ref.SC2Ref(L, S)
    ref.feed(lines[:-1])
    want = f"{ref.lines * 8 * L} {ref.comp} SC2-Huffman"
    assert r.stdout.strip().split("\n") == [f"line {want}", f"batch {want}", f"file {want}"], r.stdout
