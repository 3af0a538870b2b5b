"""Every device-path kernel on one device batch of more than 2^32 bytes, in the product library.

One buffer per line size L in {32, 64, 128}: n = (2^32 + 2^27) / L + 37 lines (4.13 GiB), the smallest ragged batch whose
last lines lie beyond byte offset 2^32; it crosses 2^31 on the way.  The buffer is a tile of T = 16 411 lines repeated,
so every expected value comes from the CPU references on one tile: per-line outputs are the tile's, repeated (compared on
the device), and every statistic is an integer sum, reps x v(tile) + v(tile[:n mod T]).

T is prime.  A kernel that read or wrote line i at a byte offset or index taken modulo 2^31 or 2^32 would land at
another phase of the tile: (2^k / L) mod T lines away.  Each case first asserts, on the CPU, that at least half of the
reference's per-line sizes of the tile differ from the same sizes rolled by each of those shifts (`_assert_sensitive`):
that is what makes a wrapped access visible, and it is a condition on the test's input, not a measurement.

A case that cannot allocate its buffer fails; none skips."""
import math
import time

import numpy as np
import pytest

from conftest import pkg

import cpack_ref
import pattern_evict_ref
import pattern_ref
import sc2_ref

pytestmark = pytest.mark.gpu

T = 16411                                                  # lines of the tile: prime
# ((2^31 / L) mod T, (2^32 / L) mod T): the lines of the tile between a line and the one 2^31 or 2^32 bytes before it
PHASE_SHIFTS = {32: (4285, 8570), 64: (10348, 4285), 128: (5174, 10348)}


def _shifts(L):
    """Lines, modulo the tile, between a line and the one a wrapped access would reach instead.  Four wraps:
    a byte offset taken modulo 2^31 or 2^32 (PHASE_SHIFTS[L]); a 16-byte-unit index taken modulo 2^32, which is 2^36
    bytes ((2^36 / L) mod T: 5832, 2916 and 1458 lines); and a line index taken modulo 2^28 (2^28 mod T = 729 lines at
    every line size).  The buffer is too short for the last two to happen, which costs nothing to guard against: they make
    the condition on the tile stricter."""
    s = {(1 << 31) // L % T, (1 << 32) // L % T, (1 << 36) // L % T, (1 << 28) % T}
    assert set(PHASE_SHIFTS[L]) <= s and 729 in s and 0 not in s
    return sorted(s)


def _assert_sensitive(what, sizes, shifts):
    """The condition on the tile: rolled by any of the shifts, at least half of the reference's sizes change."""
    sizes = np.asarray(sizes)
    for sh in shifts:
        frac = float((sizes != np.roll(sizes, -sh)).mean())
        assert frac >= 0.5, f"{what}: only {frac:.3f} of the tile's sizes differ from themselves {sh} lines on"


def _assert_sensitive_bytes(what, tile, sizes_of, period_bytes):
    """The same for a line size that does not divide 2^31: a wrapped access lands inside a line, so the reference sizes
    the tile's bytes rolled by (2^k mod the period) instead (the first 20 000 lines are enough to tell)."""
    L, m = tile.shape[1], min(len(tile), 20000)
    want = np.asarray(sizes_of(tile[:m]))
    flat = tile.reshape(-1)
    for k in (31, 32):
        rolled = np.roll(flat, -((1 << k) % period_bytes))[:m * L].reshape(m, L)
        frac = float((np.asarray(sizes_of(np.ascontiguousarray(rolled))) != want).mean())
        assert frac >= 0.5, f"{what}: only {frac:.3f} of the sizes differ 2^{k} bytes on"


def make_tile(traces, L):
    t = np.concatenate([traces.structured(6000, L, seed=5), traces.mixed(4000, L), traces.sine_f32(2000, L),
                        traces.counters_u32(1500, L), traces.pointers_u64(1000, L), traces.bdi_stress(900, L),
                        traces.random_u32(800, L), traces.zeros(100, L), traces.word_same(111, L)])
    assert len(t) == T
    return np.ascontiguousarray(t[np.random.default_rng(2024 + L).permutation(T)])


class Batch:
    """The device buffer of one line size and what a case needs to know about it.  `view(L2)` reads the same bytes as
    lines of another size: the period is then lcm(T L, L2) bytes."""

    def __init__(self, torch, buf, L, n, tile):
        self.torch, self.buf, self.L, self.n, self.tile = torch, buf, L, n, tile
        self.T = len(tile)
        self.reps, self.tail = divmod(n, self.T)
        self.ptr = buf.data_ptr()
        self.refs = {}                                      # references of the tile, computed once per buffer

    def view(self, L2):
        nbytes, period = self.n * self.L, math.lcm(self.T * self.L, L2)
        tile = np.ascontiguousarray(np.tile(self.tile.reshape(-1), period // (self.T * self.L)).reshape(-1, L2))
        return Batch(self.torch, self.buf, L2, nbytes // L2, tile)

    def ref(self, key, make):
        if key not in self.refs:
            self.refs[key] = make()
        return self.refs[key]

    def outputs(self):
        """Per-line output arrays, filled with what no evaluator writes."""
        t = self.torch
        return (t.full((self.n,), -2, dtype=t.int16, device="cuda:0"), t.full((self.n,), 77, dtype=t.int8, device="cuda:0"))

    def scale(self, v_tile, v_tail):
        return np.uint64(self.reps) * np.asarray(v_tile, dtype=np.uint64) + np.asarray(v_tail, dtype=np.uint64)

    def same_tiled(self, what, d_out, want_first, want_rest=None):
        """d_out (n elements on the device) is want_first for the first repetition, want_rest (default: the same) for every
        later one and the head of want_rest in the tail; on a mismatch the first ten line indices."""
        t, T_, reps = self.torch, self.T, self.reps
        want_rest = want_first if want_rest is None else want_rest
        kind = {np.dtype(np.uint16): np.int16, np.dtype(np.int8): np.int8}[np.asarray(want_first).dtype]
        w0 = t.from_numpy(np.ascontiguousarray(want_first).view(kind)).to("cuda:0")
        w1 = t.from_numpy(np.ascontiguousarray(want_rest).view(kind)).to("cuda:0")
        bad = t.cat([d_out[:T_] != w0, (d_out[T_:reps * T_].view(reps - 1, T_) != w1[None, :]).view(-1), d_out[reps * T_:] != w1[:self.tail]])
        if bool(bad.any()):
            idx = t.nonzero(bad).view(-1)
            first = idx[:10].cpu().tolist()
            raise AssertionError(f"{what}: {int(idx.numel())} of {self.n} lines differ from the tile's reference, the first at lines "
                                 f"{first} (tile positions {[i % T_ for i in first]}): got {d_out[idx[:10]].cpu().tolist()}")


@pytest.fixture(scope="module")
def mpc():
    return pkg()


@pytest.fixture(scope="module")
def batch(request, traces):
    """The 4.13 GiB buffer of line size request.param: the tile uploaded once, repeated by a broadcast copy on the device,
    the n mod T tail lines from the head of the tile; freed at teardown."""
    import torch
    L = request.param
    n = ((1 << 32) + (1 << 27)) // L + 37
    assert n == {32: 138412069, 64: 69206053, 128: 34603045}[L] and n % 64 == 37 and (n - 1) * L > 1 << 32
    tile = make_tile(traces, L)
    try:
        buf = torch.empty(n * L, dtype=torch.uint8, device="cuda:0")
    except RuntimeError as e:                               # (torch.cuda.OutOfMemoryError is one)
        free, total = torch.cuda.mem_get_info(0)
        pytest.fail(f"cannot allocate the {n * L} byte buffer: {free} of {total} bytes free on the device ({e})")
    d_tile = torch.from_numpy(tile.reshape(-1)).to("cuda:0")
    reps, tail = divmod(n, T)
    buf[:reps * T * L].view(reps, T * L).copy_(d_tile[None, :].expand(reps, T * L))
    buf[reps * T * L:].copy_(d_tile[:tail * L])
    torch.cuda.synchronize()
    b = Batch(torch, buf, L, n, tile)
    yield b
    b.buf = b.ptr = None
    del buf, d_tile
    torch.cuda.empty_cache()


ALL_SIZES = pytest.mark.parametrize("batch", [32, 64, 128], indirect=True)
AT_64 = pytest.mark.parametrize("batch", [64], indirect=True)


def _timed(what, run, sync):
    t0 = time.perf_counter()
    run()
    sync()
    print(f"\n[large batch] {what}: {1e3 * (time.perf_counter() - t0):.1f} ms", end="")


def _run_stateless(b, what, ev, want_s, want_k, v_tile, v_tail, shifts=None, twice=True):
    """One handle over the whole buffer: per-line outputs against the tile's, the statistics vector against the scaled
    one, and (twice) again without per-line outputs, after which the vector has doubled."""
    if shifts is None:
        shifts = _shifts(b.L)
    _assert_sensitive(what, want_s, shifts)
    d_s, d_k = b.outputs()
    _timed(what, lambda: ev.compress_device(b.ptr, b.n, d_s.data_ptr(), d_k.data_ptr()), ev.sync)
    b.same_tiled(what + ", sizes", d_s, want_s)
    b.same_tiled(what + ", selected", d_k, want_k)
    want_v = b.scale(v_tile, v_tail)
    got = ev.stats_vector()
    assert (got == want_v).all(), (what, "statistics", np.nonzero(got != want_v)[0][:10].tolist(), got[:12].tolist(), want_v[:12].tolist())
    if twice:
        _timed(what + ", statistics only", lambda: ev.compress_device(b.ptr, b.n), ev.sync)
        got = ev.stats_vector()
        assert (got == np.uint64(2) * want_v).all(), (what, "statistics after a second run without per-line outputs",
                                                       np.nonzero(got != np.uint64(2) * want_v)[0][:10].tolist())


def _vpc_ref(b, oracle, key, cfg):
    def make():
        o = oracle.VpcOracle(cfg)
        s, k = o.compress(b.tile)
        v = o.stats_vector()
        o2 = oracle.VpcOracle(cfg)
        o2.compress(b.tile[:b.tail])
        return s, k, v, o2.stats_vector()
    return b.ref(("vpc", key), make)


def _baseline_ref(b, oracle, name):
    def make():
        zeros = np.zeros(b.T, np.int8)
        if name == "CPACK":
            s, c = cpack_ref.compress(b.tile)
            return s, zeros, cpack_ref.stats_vector(b.L, s, c), cpack_ref.stats_vector(b.L, s[:b.tail], c[:b.tail])
        make_o = {"BDI": oracle.BdiOracle, "FPC": oracle.FpcOracle, "BPC": oracle.BpcOracle}[name]
        o, o2 = make_o(b.L), make_o(b.L)
        out = o.compress(b.tile)
        s, k = out if name == "BDI" else (out, zeros)
        o2.compress(b.tile[:b.tail])
        return s, k, o.stats_vector(), o2.stats_vector()
    return b.ref(("baseline", name), make)


def _make(mpc, name, L):
    return {"BDI": mpc.BDI, "FPC": mpc.FPC, "BPC": mpc.BPC, "CPACK": mpc.CPACK}[name](L)


# ---- 32, 64 and 128 bytes ----------------------------------------------------------------------------------------------
@ALL_SIZES
def test_vpc_probe_configuration(mpc, oracle, configs, batch):
    cfg = configs.probe_config(batch.L)
    ev = mpc.VPC(cfg)
    assert ev.kernel_path == mpc.MPC_PATH_VPC_FAST and ev.kernel_form == "unrolled", ev.kernel_form
    _run_stateless(batch, f"VPC probe, {batch.L} B", ev, *_vpc_ref(batch, oracle, "probe", cfg))
    ev.close()


@ALL_SIZES
@pytest.mark.parametrize("name", ["BDI", "FPC", "BPC", "CPACK"])
def test_baseline_alone(mpc, oracle, batch, name):
    ev = _make(mpc, name, batch.L)
    _run_stateless(batch, f"{name}, {batch.L} B", ev, *_baseline_ref(batch, oracle, name))
    ev.close()


@ALL_SIZES
def test_bdi_fpc_bpc_group(mpc, oracle, batch):
    """baselines_kernel: the ring feed at 32 and 64 bytes, the staged feed at 128."""
    b, names = batch, ("BDI", "FPC", "BPC")
    refs = [_baseline_ref(b, oracle, c) for c in names]
    for c, r in zip(names, refs):
        _assert_sensitive(f"group member {c}, {b.L} B", r[0], _shifts(b.L))
    members = [_make(mpc, c, b.L) for c in names]
    group = mpc.EvaluatorSet(members)
    assert group.form == "BDI+FPC+BPC: one kernel", group.form
    outs = [b.outputs() for _ in names]
    _timed(f"BDI+FPC+BPC group, {b.L} B", lambda: group.compress_device(b.ptr, b.n, d_sizes=[o[0].data_ptr() for o in outs],
                                                                         d_selected=[o[1].data_ptr() for o in outs]), group.sync)
    for c, ev, (d_s, d_k), (s, k, v, v_tail) in zip(names, members, outs, refs):
        b.same_tiled(f"group member {c}, {b.L} B, sizes", d_s, s)
        b.same_tiled(f"group member {c}, {b.L} B, selected", d_k, k)
        assert (ev.stats_vector() == b.scale(v, v_tail)).all(), (c, "statistics")
    _timed(f"BDI+FPC+BPC group, {b.L} B, statistics only", lambda: group.compress_device(b.ptr, b.n), group.sync)
    for c, ev, (s, k, v, v_tail) in zip(names, members, refs):
        assert (ev.stats_vector() == np.uint64(2) * b.scale(v, v_tail)).all(), (c, "statistics after a second run")
    group.close()
    for ev in members:
        ev.close()


# ---- the other VPC kernel forms, on the 64-byte buffer -----------------------------------------------------------------
def _probe_like(configs, L, roots):
    prev4 = [max(i - 4, 0) for i in range(L)]
    w2 = [[1.0, 0.5][i % 2] for i in range(L)]
    d1 = [1 if i % 4 == 0 else 0 for i in range(L)]
    return configs.make_config(L, [{"name": "AllZero"}, {"name": "AllWordSame"}, configs.one_base(L, roots[0], True),
                                   configs.consecutive_base(L, 0, True), configs.diff_base(L, prev4, d1, roots[1], False),
                                   configs.weight_base(L, prev4, w2, roots[2], True)])


def _ob_df_wt_ob(configs, L):
    """"OB DF WT OB" of test_vpc_sequences_compiled_at_creation: a sequence without a built-in instantiation."""
    prev1, prev4 = [max(i - 1, 0) for i in range(L)], [max(i - 4, 0) for i in range(L)]
    diff, w2 = [(-2 + (i % 5)) for i in range(L)], [[1.0, 0.5][i % 2] for i in range(L)]
    return configs.make_config(L, [{"name": "AllZero"}, {"name": "AllWordSame"}, configs.one_base(L, 0, True),
                                   configs.diff_base(L, prev1, diff, 0, False), configs.weight_base(L, prev4, w2, 0, True),
                                   configs.one_base(L, 0, False)])


def _permuted_scan(configs, L):
    """The configuration of test_vpc_generic_path: a permuted, truncated scan table and random predictor tables."""
    rng = np.random.default_rng(L)
    n = 8 * L
    perm = rng.permutation(n)
    scan = {"TableSize": n - 16, "Rows": [int(p) // L for p in perm[: n - 16]], "Cols": [int(p) % L for p in perm[: n - 16]]}
    rb = [int(x) for x in rng.integers(0, L, L)]
    rd = [int(x) for x in rng.integers(-300, 300, L)]
    rw = [float(2.0 ** int(x)) for x in rng.integers(-9, 10, L)]
    return configs.make_config(L, [{"name": "AllZero"}, {"name": "AllWordSame"}, configs.one_base(L, root=5, consecutive_xor=True),
                                   configs.consecutive_base(L, 0, False, scan=scan), configs.diff_base(L, rb, rd, root=3, consecutive_xor=True),
                                   configs.weight_base(L, rb, rw, root=L - 1, consecutive_xor=False, scan=scan)])


@AT_64
def test_vpc_general_layout_twin(mpc, oracle, configs, batch):
    cfg = _probe_like(configs, 64, (5, 3, 2))
    ev = mpc.VPC(cfg)
    assert ev.kernel_form == "unrolled, general layout", ev.kernel_form
    _run_stateless(batch, "VPC general-layout twin (5, 3, 2), 64 B", ev, *_vpc_ref(batch, oracle, "twin", cfg))
    ev.close()


@AT_64
def test_vpc_sequence_compiled_at_creation(mpc, oracle, configs, batch, monkeypatch):
    monkeypatch.delenv("MPC_JIT", raising=False)
    cfg = _ob_df_wt_ob(configs, 64)
    ev = mpc.VPC(cfg)
    assert ev.kernel_form.startswith("unrolled, compiled at creation"), ev.kernel_form
    _run_stateless(batch, "VPC OB DF WT OB compiled at creation, 64 B", ev, *_vpc_ref(batch, oracle, "seq", cfg))
    ev.close()


@AT_64
def test_vpc_run_time_loop(mpc, oracle, configs, batch, monkeypatch):
    monkeypatch.setenv("MPC_JIT", "0")
    cfg = _ob_df_wt_ob(configs, 64)
    ev = mpc.VPC(cfg)
    assert ev.kernel_path == mpc.MPC_PATH_VPC_FAST and ev.kernel_form == "run-time loop", ev.kernel_form
    _run_stateless(batch, "VPC OB DF WT OB run-time loop, 64 B", ev, *_vpc_ref(batch, oracle, "seq", cfg))
    ev.close()


@AT_64
@pytest.mark.parametrize("L", [64, 48])
def test_vpc_generic_kernel(mpc, oracle, configs, batch, monkeypatch, L):
    """vpc_generic_kernel indexes bytes (`lines + line * L`).  It has one form, with or without per-line outputs, and runs
    at some 45 GB/s (0.1 s for the buffer): one pass."""
    monkeypatch.setenv("MPC_JIT", "0")
    b = batch if L == 64 else batch.view(L)
    cfg = _permuted_scan(configs, L)
    ev = mpc.VPC(cfg)
    assert ev.kernel_path == mpc.MPC_PATH_VPC_GENERIC, ev.kernel_form
    s, k, v, v_tail = _vpc_ref(b, oracle, "generic", cfg)
    if L == 64:
        shifts = _shifts(64)
    else:
        _assert_sensitive_bytes("VPC generic, 48 B", b.tile, lambda x: oracle.VpcOracle(cfg).compress(x)[0], batch.T * 64)
        shifts = []
    _run_stateless(b, f"VPC generic kernel, {L} B", ev, s, k, v, v_tail, shifts=shifts, twice=False)
    ev.close()


# ---- the any-line-size kernels: the 64-byte buffer read at another line size ------------------------------------------
@AT_64
@pytest.mark.parametrize("name", ["BDI", "FPC", "BPC"])
def test_baseline_generic_kernel_at_24_bytes(mpc, oracle, batch, name):
    b = batch.view(24)
    s, k, v, v_tail = _baseline_ref(b, oracle, name)
    make_o = {"BDI": oracle.BdiOracle, "FPC": oracle.FpcOracle, "BPC": oracle.BpcOracle}[name]
    _assert_sensitive_bytes(f"{name}, 24 B", b.tile, lambda x: (make_o(24).compress(x)[0] if name == "BDI" else make_o(24).compress(x)), batch.T * 64)
    ev = _make(mpc, name, 24)
    _run_stateless(b, f"{name} any-line-size kernel, 24 B", ev, s, k, v, v_tail, shifts=[], twice=False)
    ev.close()


@AT_64
def test_cpack_any_kernel_at_36_bytes(mpc, oracle, batch):
    b = batch.view(36)
    s, k, v, v_tail = _baseline_ref(b, oracle, "CPACK")
    _assert_sensitive_bytes("C-Pack, 36 B", b.tile, lambda x: cpack_ref.compress(x)[0], batch.T * 64)
    ev = mpc.CPACK(36)
    _run_stateless(b, "C-Pack any-line-size kernel, 36 B", ev, s, k, v, v_tail, shifts=[], twice=False)
    ev.close()


# ---- SC2 ----------------------------------------------------------------------------------------------------------------
def _run_sc2(mpc, b, what, shifts):
    """S = 5000: the table is built inside the first tile.  The reference takes the tile twice: the first pass is
    repetition 0, the second (table frozen) every later one; a third feed of the tail's lines gives the tail."""
    S = 5000
    ref = sc2_ref.SC2Ref(b.L, S)
    s0, k0 = ref.feed(b.tile)
    v1 = ref.stats_vector().astype(np.int64)
    s1, k1 = ref.feed(b.tile)
    v2 = ref.stats_vector().astype(np.int64)
    ref.feed(b.tile[:b.tail])
    v3 = ref.stats_vector().astype(np.int64)
    _assert_sensitive(what + ", warm-up tile", s0, shifts)
    _assert_sensitive(what + ", later tiles", s1, shifts)
    want_v = v2 + (b.reps - 2) * (v2 - v1) + (v3 - v2)
    ev = mpc.SC2(b.L, S, device=0)
    d_s, d_k = b.outputs()
    _timed(what, lambda: ev.compress_device(b.ptr, b.n, d_s.data_ptr(), d_k.data_ptr()), ev.sync)
    assert ev.kernel_form == "table sizing"
    b.same_tiled(what + ", sizes", d_s, s0, s1)
    b.same_tiled(what + ", selected", d_k, k0, k1)
    assert ev.stats_vector().astype(np.int64).tolist() == want_v.tolist(), (what, "statistics")
    sym, lens = ev.table()
    assert sym.tolist() == ref.table_syms.tolist() and lens.tolist() == ref.table_lens.tolist(), (what, "table")
    # again, without per-line outputs: every line is sized against the table now
    _timed(what + ", statistics only", lambda: ev.compress_device(b.ptr, b.n), ev.sync)
    want_v = want_v + b.reps * (v2 - v1) + (v3 - v2)
    assert ev.stats_vector().astype(np.int64).tolist() == want_v.tolist(), (what, "statistics after a second run")
    ev.close()
    return s1


@AT_64
def test_sc2(mpc, batch):
    _run_sc2(mpc, batch, "SC2, 64 B", _shifts(64))


@AT_64
def test_sc2_size_any_kernel_at_36_bytes(mpc, batch):
    b = batch.view(36)

    def sizes_of(x):                                        # table sizing of x against the table of the tile's first 5000 lines
        r = sc2_ref.SC2Ref(36, 5000)
        r.feed(b.tile[:5000])
        return r.feed(x)[0]
    _assert_sensitive_bytes("SC2, 36 B", b.tile, sizes_of, batch.T * 64)
    _run_sc2(mpc, b, "SC2 any-line-size kernels, 36 B", [])


# ---- Pattern ------------------------------------------------------------------------------------------------------------
@AT_64
def test_pattern(mpc, batch):
    """The default handle: every line after the first tile has been seen before.  The reference analyses one tile, two
    tiles, and two tiles and the tail; the counts of a further tile are the difference of the first two.  17 launches of
    4 Mi lines: launch_pattern's offsets into the lines, the sizes and the selected array."""
    b, L = batch, 64
    s, k, S1 = pattern_ref.analyse(b.tile)
    S2 = pattern_ref.analyse(np.concatenate([b.tile, b.tile]))[2]
    S3 = pattern_ref.analyse(np.concatenate([b.tile, b.tile, b.tile[:b.tail]]))[2]
    S1, S2, S3 = (x.astype(np.int64) for x in (S1, S2, S3))
    _assert_sensitive("Pattern, 64 B", s, _shifts(L))
    assert b.n > 16 * (1 << 22)                             # 17 launches
    ev = mpc.Pattern(L, device=0)
    d_s, d_k = b.outputs()
    _timed("Pattern, 64 B", lambda: ev.compress_device(b.ptr, b.n, d_s.data_ptr(), d_k.data_ptr()), ev.sync)
    b.same_tiled("Pattern, sizes", d_s, s)
    b.same_tiled("Pattern, selected", d_k, k)
    want = S2 + (b.reps - 2) * (S2 - S1) + (S3 - S2)
    got = ev.stats_vector().astype(np.int64)
    assert got.tolist() == want.tolist(), ("Pattern statistics", np.nonzero(got != want)[0][:10].tolist())
    assert ev.distinct_lines() == pattern_ref.distinct(b.tile) == int(S1[21])
    _timed("Pattern, 64 B, statistics only", lambda: ev.compress_device(b.ptr, b.n), ev.sync)
    want = want + b.reps * (S2 - S1) + (S3 - S2)            # every line of the second run is a duplicate
    assert ev.stats_vector().astype(np.int64).tolist() == want.tolist(), "Pattern statistics after a second run"
    assert ev.distinct_lines() == int(S1[21])
    ev.close()


@AT_64
def test_pattern_evicting(mpc, batch):
    """capacity = 1000: launches of 1000 lines (69 207 of them, ten small kernels each -- the case's time is launch
    latency).  What the reference's cache holds at the end of a tile depends on what it held at its start, so a further
    tile does not always add the same counts: the cache is fed tile by tile until its state at the end of a tile is one
    it had before (after tile 7 that of tile 1: a cycle of 6 tiles), then one cycle more to assert that the tiles of a
    cycle hit and miss as those of the cycle before did."""
    b, L, capacity = batch, 64, 1000
    keys = pattern_evict_ref.keys_of(b.tile)
    fifo, flags, seen, cycle = pattern_evict_ref.Fifo(capacity), [], {}, None
    for j in range(64):
        flags.append(fifo.feed(keys))
        state = tuple(fifo.items)
        if state in seen:
            cycle = (seen[state] + 1, j - seen[state])      # tiles from `first` on repeat with this period
            break
        seen[state] = j
    assert cycle is not None, "the reference's cache has not returned to an earlier state within 64 tiles"
    first, period = cycle

    def flags_of(j):
        return flags[j] if j < first else flags[first + (j - first) % period]
    for j in range(len(flags), len(flags) + period):
        assert (fifo.feed(keys) == flags_of(j)).all(), f"tile {j} does not repeat tile {first + (j - first) % period}"
    assert b.reps > first + period
    hits = sum(int(flags_of(j).sum()) for j in range(b.reps)) + int(flags_of(b.reps)[:b.tail].sum())
    (s, _, A), (_, _, A_tail) = (pattern_ref.analyse(x, with_set=False) for x in (b.tile, b.tile[:b.tail]))
    _assert_sensitive("Pattern with an evicting set, 64 B", s, _shifts(L))
    want = b.scale(A, A_tail)
    want[6], want[21] = L * hits, b.n - hits
    ev = mpc.Pattern(L, device=0, on_full="evict", capacity=capacity)
    assert ev.kernel_path == mpc.MPC_PATH_PATTERN_EVICTING
    _timed("Pattern, evicting set of 1000 lines, 64 B", lambda: ev.compress_device(b.ptr, b.n), ev.sync)
    got = ev.stats_vector()
    assert got.tolist() == want.tolist(), ("statistics", np.nonzero(got != want)[0][:10].tolist(), (int(got[6]), int(want[6])), (int(got[21]), int(want[21])))
    assert ev.distinct_lines() == b.n - hits
    ev.close()


# ---- size accounting ----------------------------------------------------------------------------------------------------
def _hist(mpc, sizes):
    return np.bincount(np.minimum(np.asarray(sizes).astype(np.int64), mpc.MPC_SIZE_BINS - 1), minlength=mpc.MPC_SIZE_BINS).astype(np.uint64)


def _report_sectors(mpc, what, bins, L):
    r = mpc.size_sectors(bins, L)
    print(f"\n[large batch] {what}: sector ratio {r['ratio']:.6f} ({r['total_sectors']} sectors of 32 bytes)", end="")
    assert r["total_sectors"] > 0 and int(r["classes"].sum()) == int(bins.sum())


@AT_64
def test_size_histogram_with_the_callers_array(mpc, oracle, batch):
    """One sizes_account_kernel launch over 69 M sizes."""
    b = batch
    s = _baseline_ref(b, oracle, "BDI")[0]
    _assert_sensitive("BDI, 64 B", s, _shifts(64))
    want = b.scale(_hist(mpc, s), _hist(mpc, s[:b.tail]))
    ev = mpc.BDI(64)
    ev.enable_size_histogram()
    d_s, _ = b.outputs()
    _timed("BDI size histogram over the caller's array, 64 B", lambda: ev.compress_device(b.ptr, b.n, d_s.data_ptr()), ev.sync)
    b.same_tiled("BDI sizes", d_s, s)
    got = ev.size_histogram()
    assert (got == want).all(), ("histogram bins", np.nonzero(got != want)[0][:10].tolist())
    _report_sectors(mpc, "BDI, the caller's array", got, 64)
    ev.close()


@AT_64
def test_size_histogram_without_an_array(mpc, oracle, batch):
    """17 pieces of 4 Mi lines over the handle's scratch array."""
    b = batch
    s = _baseline_ref(b, oracle, "BDI")[0]
    _assert_sensitive("BDI, 64 B", s, _shifts(64))
    want = b.scale(_hist(mpc, s), _hist(mpc, s[:b.tail]))
    ev = mpc.BDI(64)
    ev.enable_size_histogram()
    _timed("BDI size histogram in 17 pieces, 64 B", lambda: ev.compress_device(b.ptr, b.n), ev.sync)
    got = ev.size_histogram()
    assert (got == want).all(), ("histogram bins", np.nonzero(got != want)[0][:10].tolist())
    assert int(ev.stats_vector()[0]) == b.n
    _report_sectors(mpc, "BDI, 17 pieces", got, 64)
    ev.close()


@AT_64
def test_group_best_of(mpc, oracle, batch):
    """BDI + FPC + BPC + C-Pack with the best-of: with every member's array (one accounting launch over 4 x 69 M sizes),
    then without any (17 pieces over scratch arrays), after which everything has doubled."""
    b, names = batch, ("BDI", "FPC", "BPC", "CPACK")
    sizes = [_baseline_ref(b, oracle, c)[0] for c in names]
    M = np.stack([x.astype(np.int64) for x in sizes])
    best, winner = np.minimum.reduce(M), M.argmin(axis=0)   # argmin: the first minimal member wins a tie
    for c, x in zip(names + ("best-of",), sizes + [best]):
        _assert_sensitive(f"{c}, 64 B", x, _shifts(64))
    tail = b.tail
    want_hist = [b.scale(_hist(mpc, x), _hist(mpc, x[:tail])) for x in sizes]
    want_best = b.scale(_hist(mpc, best), _hist(mpc, best[:tail]))
    want_wins = [b.reps * int((winner == i).sum()) + int((winner[:tail] == i).sum()) for i in range(4)]
    want_bits = b.reps * int(best.sum()) + int(best[:tail].sum())
    members = [_make(mpc, c, 64) for c in names]
    group = mpc.EvaluatorSet(members)
    for ev in members:
        ev.enable_size_histogram()
    group.enable_best()
    outs = [b.outputs()[0] for _ in names]
    _timed("BDI+FPC+BPC+C-Pack best-of with the callers' arrays, 64 B",
           lambda: group.compress_device(b.ptr, b.n, d_sizes=[o.data_ptr() for o in outs]), group.sync)
    for times in (1, 2):
        got = group.best()
        for c, ev, w in zip(names, members, want_hist):
            assert (ev.size_histogram() == np.uint64(times) * w).all(), (c, "histogram", times)
        assert (got["bins"] == np.uint64(times) * want_best).all(), ("best-of histogram", times)
        assert got["wins"].tolist() == [times * w for w in want_wins], ("wins", times, got["wins"].tolist())
        assert got["best_bits"] == times * want_bits and got["lines"] == times * b.n, ("best bits, lines", times)
        if times == 1:
            for c, o, x in zip(names, outs, sizes):
                b.same_tiled(f"best-of member {c}, sizes", o, x)
            _timed("BDI+FPC+BPC+C-Pack best-of in 17 pieces, 64 B", lambda: group.compress_device(b.ptr, b.n), group.sync)
    _report_sectors(mpc, "best of BDI, FPC, BPC and C-Pack (two runs)", got["bins"], 64)
    group.close()
    for ev in members:
        ev.close()
