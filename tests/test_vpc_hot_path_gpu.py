"""The lane kernel's path for incompressible groups, against the CPU oracle.

`vpc_lane_kernel` leaves a group of 64 lines early when every line of it stays uncompressed: it keeps the per-line
predicates as wave masks, evaluates the last module alone after a first-stage prefilter on residue words 0..2, and
adds to the per-lane run statistics without looking at per-line selectors or sizes.  These traces make each of those
shortcuts flip inside a wave and between the two consecutive groups of a wave's block (128 lines), for the probe
configuration at 32-, 64- and 128-byte lines, through both instantiations: the one with per-line outputs and the
statistics-only one (what bench.py runs), whose statistics vector alone is compared with the oracle's aggregate.

Shapes are a few hundred lines, 128 k + r: whole blocks come through the line ring, the r lines behind the last whole
block through the plain-load copy of the group code."""
import numpy as np
import pytest

from conftest import pkg

pytestmark = pytest.mark.gpu

SHAPES = [128 * k + r for k in (1, 3) for r in (0, 1, 63, 64, 65)]
EDGE_BYTES = (0x00, 0x7F, 0x80, 0xFF)
PLANT_LANES = (0, 63, 31)


@pytest.fixture(scope="module")
def mpc():
    pkg("build").build_lib()
    return pkg()


# ---- lines with a known fate under the probe configuration -------------------------------------------------------
def weight_ramp(L, rng):
    """WeightBase predicts it exactly from word 1 on: even bytes repeat the previous word, odd bytes halve."""
    w = rng.integers(1, 256, 4, dtype=np.uint8)
    w[1] |= 0x81                      # odd bytes that differ from their halves, word after word
    line = np.empty(L, dtype=np.uint8)
    for e in range(L // 4):
        line[4 * e:4 * e + 4] = w
        w = np.array([w[0], w[1] >> 1, w[2], w[3] >> 1], dtype=np.uint8)
    return line


def diff_ramp(L, rng):
    """DiffBase predicts it exactly: a 32-bit counter from 0 (least significant byte + 1 per word).  The root byte is 0:
    a set bit of the raw root would bound every module's leading zero rows alike, and ties go to the last module."""
    return np.arange(L // 4, dtype=np.uint32).view(np.uint8)[:L].copy()


def diff_line_with_msb(L, rng, msb_at):
    """DiffBase residues (line[i] - line[i - 4] - (i % 4 == 0)) below 0x80 everywhere but at byte `msb_at` (None: nowhere):
    the row-0 prefilter of DiffBase passes or fails on that byte alone."""
    res = rng.integers(0, 4, L, dtype=np.int64)
    if msb_at is not None:
        res[msb_at] = 0x80 + int(rng.integers(0, 0x40))
    line = np.zeros(L, dtype=np.int64)
    line[0] = 0                       # (root byte 0: see diff_ramp)
    for i in range(1, L):
        line[i] = (line[max(i - 4, 0)] + (1 if i % 4 == 0 else 0) + res[i]) & 0xFF
    return line.astype(np.uint8)


def random_lines(traces, n, L, seed):
    return traces.random_u32(n, L, seed=seed).copy()


def trace_planted(traces, n, L, rot):
    """Random lines; every group of 64 gets exactly one all-zero line, one all-words-same line and one compressible line
    (a WeightBase ramp in even groups, a DiffBase ramp in odd ones) at lanes 0 / 63 / 31, rotated by `rot`."""
    rng = np.random.default_rng(100 + rot)
    lines = random_lines(traces, n, L, seed=1000 + rot)
    for g in range((n + 63) // 64):
        lanes = [PLANT_LANES[(j + rot + g) % 3] for j in range(3)]
        same = np.tile(rng.integers(1, 256, 4, dtype=np.uint8), L // 4)
        planted = (np.zeros(L, dtype=np.uint8), same, weight_ramp(L, rng) if g % 2 == 0 else diff_ramp(L, rng))
        for lane, line in zip(lanes, planted):
            if 64 * g + lane < n:
                lines[64 * g + lane] = line
    return lines


def trace_after_kept(traces, n, L, first_kept):
    """Groups of compressible lines (every line keeps its encoding) alternating with groups of only random lines, so that
    the encoder-is-hot flag and the run key change from one group of a wave to the next; which of a block's two groups
    is the compressible one alternates from block to block."""
    lines = random_lines(traces, n, L, seed=77)
    rng = np.random.default_rng(3)
    comp = np.concatenate([traces.counters_u32(n, L), np.stack([weight_ramp(L, rng) for _ in range(n)]),
                           np.stack([diff_line_with_msb(L, rng, None) for _ in range(n)])])[rng.permutation(3 * n)]
    for g in range((n + 63) // 64):
        block, half = divmod(g, 2)
        if (half == 0) == ((block % 2 == 0) == first_kept):
            lo, hi = 64 * g, min(64 * g + 64, n)
            lines[lo:hi] = comp[lo:hi]
    return lines


def trace_head_bytes(traces, n, L, compressible):
    """Lines that differ from one base line only in bytes 0..7 (the root byte and the first two words): each of the byte
    values 0x00, 0x7f, 0x80, 0xff at each of the eight positions.  The base line is random (incompressible), or a
    WeightBase / DiffBase ramp when `compressible`, so that the residues of words 0 and 1 decide the size."""
    rng = np.random.default_rng(9 + compressible)
    lines = np.empty((n, L), dtype=np.uint8)
    base = None
    for i in range(n):
        if i % 32 == 0:
            if not compressible:
                base = random_lines(traces, 1, L, seed=500 + i)[0]
            else:
                base = weight_ramp(L, rng) if (i // 32) % 2 == 0 else diff_ramp(L, rng)
        lines[i] = base
        lines[i, (i % 32) // 4] = EDGE_BYTES[i % 4]
    return lines


def trace_diff_msb(traces, n, L, background):
    """Lines whose DiffBase residue has its only MSB in byte 11 (the last byte of the prefilter's first stage), in byte 15
    (the last byte of its second stage) or nowhere, one kind after the other: alone (`background` False) or planted
    at lanes 0 / 63 / 31 of groups of random lines."""
    rng = np.random.default_rng(21)
    kinds = (11, 15, None)
    if not background:
        return np.stack([diff_line_with_msb(L, rng, kinds[i % 3]) for i in range(n)])
    lines = random_lines(traces, n, L, seed=88)
    for g in range((n + 63) // 64):
        for j, lane in enumerate(PLANT_LANES):
            if 64 * g + lane < n:
                lines[64 * g + lane] = diff_line_with_msb(L, rng, kinds[(g + j) % 3])
    return lines


TRACES = {
    "planted_rot0": lambda t, n, L: trace_planted(t, n, L, 0),
    "planted_rot1": lambda t, n, L: trace_planted(t, n, L, 1),
    "planted_rot2": lambda t, n, L: trace_planted(t, n, L, 2),
    "kept_then_random": lambda t, n, L: trace_after_kept(t, n, L, True),
    "random_then_kept": lambda t, n, L: trace_after_kept(t, n, L, False),
    "head_bytes_random": lambda t, n, L: trace_head_bytes(t, n, L, False),
    "head_bytes_ramps": lambda t, n, L: trace_head_bytes(t, n, L, True),
    "diff_msb_alone": lambda t, n, L: trace_diff_msb(t, n, L, False),
    "diff_msb_planted": lambda t, n, L: trace_diff_msb(t, n, L, True),
}


@pytest.fixture(scope="module")
def reference(oracle, configs, traces):
    """(lines, per-line sizes, per-line selectors, statistics vector) of the oracle per (L, trace, n): computed once."""
    cache = {}

    def get(L, name, n):
        key = (L, name, n)
        if key not in cache:
            lines = TRACES[name](traces, n, L)
            assert lines.shape == (n, L) and lines.dtype == np.uint8
            o = oracle.VpcOracle(configs.probe_config(L))
            s_ref, sel_ref = o.compress(lines)
            v_ref = o.stats_vector().copy()
            for a in (lines, s_ref, sel_ref, v_ref):
                a.setflags(write=False)
            cache[key] = (lines, s_ref, sel_ref, v_ref)
        return cache[key]

    return get


def test_traces_are_what_they_claim(oracle, configs, traces):
    """The planted lines meet the fate their names promise under the probe configuration (clusters: 0 AllZero,
    1 AllWordSame, 2 OneBase, 3 ConsecutiveBase, 4 DiffBase, 5 WeightBase; -1 uncompressed)."""
    for L in (32, 64, 128):
        rng = np.random.default_rng(0)
        o = oracle.VpcOracle(configs.probe_config(L))
        lines = np.stack([weight_ramp(L, rng), diff_ramp(L, rng), diff_line_with_msb(L, rng, None),
                          diff_line_with_msb(L, rng, 11), diff_line_with_msb(L, rng, 15), random_lines(traces, 1, L, 5)[0]])
        _, sel = o.compress(lines)
        assert sel[0] == 5 and sel[1] == 4 and sel[2] == 4, sel
        assert sel[3] != 4 and sel[4] != 4 and sel[5] == -1, sel
        for first in (True, False):
            _, sel = oracle.VpcOracle(configs.probe_config(L)).compress(trace_after_kept(traces, 256, L, first))
            kept = (sel.reshape(4, 64) >= 0).all(axis=1)
            unc = (sel.reshape(4, 64) == -1).all(axis=1)
            assert (kept | unc).all() and kept.tolist() == [first, not first, not first, first], (kept, unc)


@pytest.mark.parametrize("name", sorted(TRACES))
@pytest.mark.parametrize("L", [32, 64, 128])
def test_hot_path_against_oracle(mpc, configs, reference, L, name):
    cfg = configs.probe_config(L)
    for n in SHAPES:
        lines, s_ref, sel_ref, v_ref = reference(L, name, n)
        # per-line outputs
        ev = mpc.VPC(cfg)
        assert ev.kernel_path == mpc.MPC_PATH_VPC_FAST
        s, sel = ev.compress_lines(lines)
        bad = np.nonzero((s != s_ref) | (sel != sel_ref))[0]
        assert bad.size == 0, (f"n={n}: {bad.size} mismatching lines, first {bad[:5]}: size {s[bad[:5]]} vs {s_ref[bad[:5]]}, "
                               f"sel {sel[bad[:5]]} vs {sel_ref[bad[:5]]}")
        v = ev.stats_vector()
        assert (v == v_ref).all(), f"n={n}: statistics (per-line-output kernel) differ at {np.nonzero(v != v_ref)[0][:10]}"
        ev.close()
        # statistics only: another instantiation, the one with the early exit that bench.py times
        ev = mpc.VPC(cfg)
        ev.compress_lines(lines, want_sizes=False, want_selected=False)
        v = ev.stats_vector()
        assert (v == v_ref).all(), f"n={n}: statistics (statistics-only kernel) differ at {np.nonzero(v != v_ref)[0][:10]}"
        ev.close()
