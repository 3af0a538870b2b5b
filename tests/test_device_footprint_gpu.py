"""Every device-path kernel's footprint at tails and odd alignments (tests/footprint.py has the harness and says what a
call is checked for): each evaluator form at the line counts around the wave, 64-line group, 128-line block and
256-thread workgroup edges, with the line buffer at base + 0 / + 16 / + L/2 + 16, output arrays that are only 2-byte
(sizes) and 1-byte (selected) aligned, and every combination of the two optional output arrays.  One test id is one
evaluator form; each asserts the kernel form it claims, so a routing change cannot quietly empty a row."""
import numpy as np
import pytest

from conftest import pkg

import footprint as F
import sc2_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mpc():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("these tests need an MI355X")
    pkg("build").build_lib()
    m = pkg()
    m.lib()
    return m


# ---- VPC ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [32, 64, 128])
def test_vpc_built_in_unrolled(mpc, oracle, configs, traces, L):
    cfg = configs.probe_config(L)
    ev = mpc.VPC(cfg)
    assert ev.kernel_path == mpc.MPC_PATH_VPC_FAST and ev.kernel_form == "unrolled"
    F.sweep(ev, [F.OracleRef(oracle.VpcOracle(cfg))], F.line_pool(traces, L), tag="probe")
    ev.close()
    if L == 64:          # the paper figure's five models: the longest built-in sequence
        cfg = configs.mpc_config(64)
        assert mpc.describe_config(cfg)["compiled"] == "built in"
        ev = mpc.VPC(cfg)
        assert ev.kernel_form == "unrolled"
        F.sweep(ev, [F.OracleRef(oracle.VpcOracle(cfg))], F.line_pool(traces, L), tag="mpc_config")
        ev.close()


@pytest.mark.parametrize("L", [32, 64, 128])
def test_vpc_general_layout_twin(mpc, oracle, configs, traces, L):
    """vpc_lane_gen_kernel: roots inside word 0, and a table truncated to whole bit planes."""
    for name, cfg in (("roots (5, 3, 2)", F.probe_layout_config(configs, L, (5, 3, 2))),
                      ("6 planes", F.probe_layout_config(configs, L, (0, 0, 0), F.plane_major(L, 6 * L)))):
        d = mpc.describe_config(cfg)
        assert d["path"] == "fast" and d["general_layout"] == "yes" and d["sequence"] == "unrolled", d
        ev = mpc.VPC(cfg)
        assert ev.kernel_path == mpc.MPC_PATH_VPC_FAST and ev.kernel_form == "unrolled, general layout", ev.kernel_form
        F.sweep(ev, [F.OracleRef(oracle.VpcOracle(cfg))], F.line_pool(traces, L), tag="twin " + name)
        ev.close()


def test_vpc_compiled_at_creation(mpc, oracle, configs, traces, tmp_path, monkeypatch):
    """A module sequence without a built-in instantiation, and the byte-major scan order: both compiled when the handle
    is created."""
    monkeypatch.setenv("MPC_JIT_CACHE", str(tmp_path / "jit"))
    monkeypatch.delenv("MPC_JIT", raising=False)
    L = 64
    for name, cfg in (("new sequence", F.new_sequence_config(configs, L)),
                      ("byte-major", F.probe_layout_config(configs, L, (0, 0, 0), F.byte_major(L)))):
        d = mpc.describe_config(cfg)
        assert d["path"] == "fast" and d["sequence"] == "unrolled" and d["compiled"] == "at creation", d
        ev = mpc.VPC(cfg)
        assert ev.kernel_path == mpc.MPC_PATH_VPC_FAST and ev.kernel_form.startswith("unrolled, compiled at creation"), ev.kernel_form
        F.sweep(ev, [F.OracleRef(oracle.VpcOracle(cfg))], F.line_pool(traces, L), tag=name)
        ev.close()


def test_vpc_run_time_loop(mpc, oracle, configs, traces, monkeypatch):
    """The run-time module loop: the new sequence without the run-time compiler, and a scan table shorter than a row."""
    L = 64
    short = F.probe_layout_config(configs, L, (0, 0, 0), F.plane_major(L, 8))
    assert mpc.describe_config(short)["sequence"] == "run-time loop"
    monkeypatch.setenv("MPC_JIT", "0")
    seq = F.new_sequence_config(configs, L)
    assert mpc.describe_config(seq)["sequence"] == "run-time loop"
    for name, cfg in (("new sequence, MPC_JIT=0", seq), ("TableSize 8", short)):
        ev = mpc.VPC(cfg)
        assert ev.kernel_path == mpc.MPC_PATH_VPC_FAST and ev.kernel_form == "run-time loop", (name, ev.kernel_form)
        F.sweep(ev, [F.OracleRef(oracle.VpcOracle(cfg))], F.line_pool(traces, L), tag=name)
        ev.close()


@pytest.mark.parametrize("L", [64, 48])
def test_vpc_generic_kernel(mpc, oracle, configs, traces, L):
    cfg = F.mixed_scan_orders_config(configs, L) if L == 64 else F.permuted_scan_config(configs, L)
    assert mpc.describe_config(cfg)["path"] == "generic"
    ev = mpc.VPC(cfg)
    assert ev.kernel_path == mpc.MPC_PATH_VPC_GENERIC and ev.kernel_form == "generic" and ev.path_reason, ev.kernel_form
    F.sweep(ev, [F.OracleRef(oracle.VpcOracle(cfg))], F.line_pool(traces, L), tag="generic")
    ev.close()


# ---- BDI, FPC, BPC -----------------------------------------------------------------------------------------------------
BASELINES = {"BDI": "MPC_PATH_BDI", "FPC": "MPC_PATH_FPC", "BPC": "MPC_PATH_BPC"}


@pytest.mark.parametrize("L", [32, 64, 128, 24, 40])
@pytest.mark.parametrize("comp", ["BDI", "FPC", "BPC"])
def test_baseline(mpc, oracle, traces, comp, L):
    """32 / 64 / 128 bytes: the unrolled kernels; 24 and 40 bytes: the any-line-size loop kernels (lines that do not
    start on a 16-byte boundary).  Which of the two a handle launches follows from its line size alone (the launchers
    switch on L; mpc_kernel_form says "unrolled" for every baseline handle), so the row asserts kernel_path and
    line_size: the kernel is inferred from L, not read back."""
    ev = getattr(mpc, comp)(L)
    assert ev.kernel_path == getattr(mpc, BASELINES[comp]) and ev.line_size == L
    ref = F.OracleRef(getattr(oracle, comp.capitalize() + "Oracle")(L))
    F.sweep(ev, [ref], F.line_pool(traces, L), tag=comp)
    ev.close()


@pytest.mark.parametrize("L", [32, 128])
def test_group_of_baselines_one_kernel(mpc, oracle, traces, L):
    """baselines_kernel: the ring feed at 32 bytes, the staged feed at 128 (the feed follows from L and is not read
    back; the group's form is asserted); every member its own canaried arrays, then arrays for members 0 and 2 only."""
    def make():
        members = [mpc.BDI(L), mpc.FPC(L), mpc.BPC(L)]
        group = mpc.EvaluatorSet(members)
        assert group.form == "BDI+FPC+BPC: one kernel", group.form
        return group, members, [F.OracleRef(oracle.BdiOracle(L)), F.OracleRef(oracle.FpcOracle(L)), F.OracleRef(oracle.BpcOracle(L))]
    pool = F.line_pool(traces, L)
    group, members, refs = make()
    F.sweep(group, refs, pool, tag="group")
    F.sweep(group, refs, pool, counts=(1, 65, 129, 257, 1025), ask=(0, 2), tag="group, members 0 and 2 asked")
    group.close()
    for ev in members:
        ev.close()


# ---- SC2 ---------------------------------------------------------------------------------------------------------------
SC2_S = 100


@pytest.mark.parametrize("L", [64, 32, 128, 36])
def test_sc2(mpc, L):
    """S = 100.  On one handle: 63 lines (the counting kernel only), 257 lines (they straddle line S: the C ABI splits
    the call into a counting launch and a sizing launch at an offset into the caller's arrays), 129 lines (sizing
    only) -- for every offset, output mode and poison.  Then the sizing kernel (sc2_size_kernel, sc2_size_any_kernel at
    36 bytes) and the counting kernel alone over the line counts, the counting kernel also at 4097 lines: its
    workgroup covers 4096 words."""
    lines = F.zipf_lines(4097 + 449, L, seed=L)
    for off in F.offsets_for(L):
        for mode in F.MODES:
            for poison in F.POISON_SEEDS:
                ev, ref = mpc.SC2(L, SC2_S, device=0), sc2_ref.SC2Ref(L, SC2_S)
                assert ev.kernel_path == mpc.MPC_PATH_SC2 and ev.kernel_form == "warm-up counting"
                F.check_call(ev, [ref], lines[:63], off, mode, poison, tag="SC2 call 1")
                assert ev.kernel_form == "warm-up counting"
                F.check_call(ev, [ref], lines[63:320], off, mode, poison, tag="SC2 call 2")
                assert ev.kernel_form == "table sizing"
                F.check_call(ev, [ref], lines[320:449], off, mode, poison, tag="SC2 call 3")
                sym, lens = ev.table()
                assert sym.tolist() == ref.table_syms.tolist() and lens.tolist() == ref.table_lens.tolist()
                ev.close()
    # sizing only: the table from the first 100 lines, then the sweep
    ev, ref = mpc.SC2(L, SC2_S, device=0), sc2_ref.SC2Ref(L, SC2_S)
    F.check_call(ev, [ref], lines[:SC2_S], tag="SC2 warm-up")
    F.check_call(ev, [ref], lines[SC2_S:SC2_S + 1], tag="SC2 line S")
    assert ev.kernel_form == "table sizing"
    F.sweep(ev, [ref], lines[449:], tag="SC2 sizing")
    ev.close()
    # counting only: S beyond everything the sweep feeds
    counts = F.LINE_COUNTS + (4097,)
    fed = 2 * len(F.offsets_for(L)) * (sum(counts) + 3 * sum(F.MODE_COUNTS))
    ev, ref = mpc.SC2(L, fed + 1, device=0), sc2_ref.SC2Ref(L, fed + 1)
    F.sweep(ev, [ref], lines[449:], counts=counts, tag="SC2 counting")
    assert ev.kernel_form == "warm-up counting" and int(ev.stats_vector()[3]) == fed
    ev.close()


# ---- Pattern -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [64, 128, 40])
def test_pattern(mpc, traces, L):
    """The analysis kernel and the set's claim / compare / tail passes: consecutive calls on one handle, alternating
    between two streams, so every call but the first meets lines that are already in the set."""
    import torch
    ev, ref = mpc.Pattern(L), F.PatternRef(L)
    assert ev.kernel_path == mpc.MPC_PATH_PATTERN
    form = (mpc.lib().mpc_kernel_form(ev._h) or b"").decode()
    assert form == ("unrolled, then the set passes" if L in (64, 128) else "run-time loop, then the set passes")
    side = torch.cuda.Stream()
    streams = (torch.cuda.current_stream().cuda_stream, side.cuda_stream)
    pool = F.pattern_pool(traces, L)
    # three consecutive calls with lines of their own, repeats inside and across them
    for k, (a, b) in enumerate(((0, 63), (63, 320), (320, 449))):
        F.check_call(ev, [ref], pool[a:b], 16, "both", F.POISON_SEEDS[k % 2], stream=streams[k % 2], tag=f"Pattern call {k + 1}")
    assert 0 < ev.distinct_lines() == len(ref.set) < 449
    F.sweep(ev, [ref], pool, streams=streams, tag="Pattern")
    assert (ev.stats_vector() == ref.whole()).all()
    assert ev.distinct_lines() == len(ref.set)
    ev.close()


# ---- all six in one group ------------------------------------------------------------------------------------------------
def test_six_member_group(mpc, oracle, configs, traces):
    """VPC, BDI, FPC, BPC, SC2 and Pattern in one set: every member its own canaried arrays; then arrays for members 0, 2
    and 4 only (the others get null pointers)."""
    L = 64
    cfg = configs.probe_config(L)
    members = [mpc.VPC(cfg), mpc.BDI(L), mpc.FPC(L), mpc.BPC(L), mpc.SC2(L, SC2_S, device=0), mpc.Pattern(L)]
    group = mpc.EvaluatorSet(members)
    assert group.form == "VPC: unrolled; BDI+FPC+BPC: one kernel; SC2: own kernel; PATTERN: own kernels", group.form
    refs = [F.OracleRef(oracle.VpcOracle(cfg)), F.OracleRef(oracle.BdiOracle(L)), F.OracleRef(oracle.FpcOracle(L)),
            F.OracleRef(oracle.BpcOracle(L)), sc2_ref.SC2Ref(L, SC2_S), F.PatternRef(L)]
    pool = F.pattern_pool(traces, L)
    F.sweep(group, refs, pool, counts=(63, 257, 129, 1, 64, 65, 128, 1023, 1025), tag="six")       # (SC2: the second 63-line call, lines 63 .. 125, straddles S = 100)
    F.sweep(group, refs, pool, counts=(1, 65, 129, 257, 1025), ask=(0, 2, 4), tag="six, members 0, 2 and 4 asked")
    assert (members[5].stats_vector() == refs[5].whole()).all()
    group.close()
    for ev in members:
        ev.close()


# ---- under a capped grid ---------------------------------------------------------------------------------------------------
def test_footprint_under_a_capped_grid(oracle):
    """VPC built in at 64 and 32 bytes, the general-layout twin and BDI at 64, the BDI + FPC + BPC group at 32: 20 001 and
    16 384 + 65 lines at offset 16, both arrays and sizes only, in ONE workgroup (the test library's MPC_TEST_GRID=1, a
    fresh process: the cap is read once).  The route counters say that lines really were set aside and drained."""
    from test_gpu_parity import _run_with_test_library
    code = r"""
sys.path.insert(0, "tests")
import footprint
print("ROUTES " + json.dumps(footprint.capped_grid_rows(mpc, C, T, O, routes)))
"""
    res = _run_with_test_library(code, grid_cap=1)
    assert set(res) == {"vpc 64", "vpc 32", "twin 64", "bdi 64", "group 32"}
    for name in ("vpc 64", "vpc 32", "twin 64"):
        assert res[name]["vpc_deferred"] > 0 and res[name]["vpc_drains"] > 0, (name, res[name])
    assert res["bdi 64"]["bdi_deferred"] > 0 and res["bdi 64"]["bdi_drains"] > 0, res["bdi 64"]
