"""The launchers' cuts and the BDI kernels' inline-scan path, at sizes a test can afford.

A launcher cuts a device batch so that a kernel's 32-bit quantities stay in range: the VPC lane launchers every 2^30
lines (the kernel's line index; the piece's number of the first line goes in as `first_line`), mpc_launch_sizes every
2^31 sizes (a uint32 LDS bin).  bdi_kernel and baselines_kernel defer a line's exact scans into a queue of 32-bit line
indices only while the launch has at most 2^32 - 1 lines; beyond that bdi_line runs them inline.  In the product all of
this starts at 32 GiB and more.  The test library (libmpc_hip_test.so) lowers the cuts to MPC_TEST_LAUNCH_LINES
(csrc/mpc_kernel_common.h: mpc_launch_cap) and the deferral limit to 2^20 - 1 lines (csrc/mpc_baselines.h:
kBdiDeferMaxLines); the kernels and their signatures are the product's.  That a cut was taken is asserted, not
assumed: the test library counts the launches of the three cutting launchers (mpc_test_launches), and every call here
must make 25 of them, so a variable that the library did not take would fail the tests.  Every comparison is integer equality against
the CPU oracle, in a fresh process bound to the test library (tests/testlib_child.py)."""
import pytest

from testlib_child import _run_with_test_library

pytestmark = pytest.mark.gpu

CUT = 4096                       # MPC_TEST_LAUNCH_LINES: a positive multiple of 64
N_LINES = 100037                 # 24 whole launches of CUT lines and a ragged one of 1733 (1733 mod 64 = 5)
assert -(-N_LINES // CUT) == 25 and (N_LINES % CUT) % 64 != 0

# two traces of N lines: the interleaved one, and one whose neighbouring launches hold different kinds of line
TRACES = r"""
N, PIECES = %d, %d                                 # PIECES launches for a batch of N lines under the lowered cut
def two_traces(L):
    rich = np.concatenate([T.mixed(40000, L), T.structured(30000, L, seed=3), T.sine_f32(12000, L), T.random_u32(9000, L),
                           T.counters_u32(5000, L), T.pointers_u64(4000, L), T.zeros(20, L), T.word_same(17, L)])
    assert len(rich) == N
    return (("mixed", T.mixed(N, L)), ("rich", rich[np.random.default_rng(40 + L).permutation(N)]))
def check_vpc(tag, cfg, L, form, traces=("mixed", "rich")):
    ev, o = mpc.VPC(cfg), O.VpcOracle(cfg)
    assert ev.kernel_path == mpc.MPC_PATH_VPC_FAST and ev.kernel_form.startswith(form), (tag, ev.kernel_form)
    for tname, lines in two_traces(L):
        if tname not in traces:
            continue
        ev.reset(); o.reset()
        s_ref, k_ref = o.compress(lines)
        before = launches()
        s, k = ev.compress_lines(lines)
        assert launches() - before == PIECES, (tag, tname, "launches", launches() - before)       # the cut was taken
        bad = np.nonzero((s != s_ref) | (k != k_ref))[0]
        assert bad.size == 0, (tag, tname, "per-line results differ at lines", bad[:10].tolist())
        assert (ev.stats_vector() == o.stats_vector()).all(), (tag, tname, "statistics")
        ev.reset()                                               # the statistics-only kernel takes the same cuts
        before = launches()
        ev.compress_lines(lines, want_sizes=False, want_selected=False)
        assert launches() - before == PIECES, (tag, tname, "launches without per-line outputs", launches() - before)
        assert (ev.stats_vector() == o.stats_vector()).all(), (tag, tname, "statistics without per-line outputs")
    ev.close()
""" % (N_LINES, -(-N_LINES // CUT))


def _run(code):
    return _run_with_test_library(TRACES + code, grid_cap=0, env={"MPC_TEST_LAUNCH_LINES": str(CUT)})


@pytest.mark.parametrize("L", [32, 64, 128])
def test_vpc_probe_configuration_in_25_launches(L):
    """mpc_launch_vpc_lane, the built-in unrolled kernel: `first_line` and the offset of the lines of launches 1 .. 24."""
    res = _run(r"""
L = %d
check_vpc("probe", C.probe_config(L), L, "unrolled")
ev = mpc.VPC(C.probe_config(L)); form = ev.kernel_form; ev.close()
print("ROUTES " + json.dumps({"form": form}))
""" % L)
    assert res["form"] == "unrolled"


def test_vpc_general_layout_twin_in_25_launches():
    res = _run(r"""
L = 64
az, aws = {"name": "AllZero"}, {"name": "AllWordSame"}
prev4 = [max(i - 4, 0) for i in range(L)]; w2 = [[1.0, 0.5][i % 2] for i in range(L)]; d1 = [1 if i % 4 == 0 else 0 for i in range(L)]
cfg = C.make_config(L, [az, aws, C.one_base(L, 5, True), C.consecutive_base(L, 0, True), C.diff_base(L, prev4, d1, 3, False),
                        C.weight_base(L, prev4, w2, 2, True)])
d = mpc.describe_config(cfg)
assert d["sequence"] == "unrolled" and d["general_layout"] == "yes" and d["compiled"] == "built in", d
check_vpc("twin (5, 3, 2)", cfg, L, "unrolled, general layout")
print("ROUTES " + json.dumps({"ok": 1}))
""")
    assert res["ok"] == 1


SEQUENCE = r"""
L = 64
az, aws = {"name": "AllZero"}, {"name": "AllWordSame"}
prev1 = [max(i - 1, 0) for i in range(L)]; prev4 = [max(i - 4, 0) for i in range(L)]
diff = [(-2 + (i % 5)) for i in range(L)]; w2 = [[1.0, 0.5][i % 2] for i in range(L)]
cfg = C.make_config(L, [az, aws, C.one_base(L, 0, True), C.diff_base(L, prev1, diff, 0, False), C.weight_base(L, prev4, w2, 0, True),
                        C.one_base(L, 0, False)])                 # "OB DF WT OB": no built-in instantiation
"""


def test_vpc_sequence_compiled_at_creation_in_25_launches():
    """mpc_launch_vpc_lane_jit has a loop of its own."""
    res = _run(SEQUENCE + r"""
assert mpc.describe_config(cfg)["compiled"] == "at creation"
check_vpc("OB DF WT OB", cfg, L, "unrolled, compiled at creation")
print("ROUTES " + json.dumps({"ok": 1}))
""")
    assert res["ok"] == 1


def test_vpc_run_time_loop_in_25_launches():
    res = _run("import os\nos.environ['MPC_JIT'] = '0'\n" + SEQUENCE + r"""
assert mpc.describe_config(cfg)["sequence"] == "run-time loop"
check_vpc("OB DF WT OB, MPC_JIT=0", cfg, L, "run-time loop")
print("ROUTES " + json.dumps({"ok": 1}))
""")
    assert res["ok"] == 1


def test_vpc_five_models_at_128_bytes_in_25_launches():
    """The paper figure's five models at 128-byte lines: compiled at creation for a workgroup of 7 waves, so the
    launcher's grid arithmetic per piece differs from the built-in kernels'."""
    res = _run(r"""
L = 128
cfg = C.mpc_config(L)
assert mpc.describe_config(cfg)["compiled"] == "at creation"
check_vpc("five models", cfg, L, "unrolled, compiled at creation", traces=("mixed",))      # (the oracle takes 4 s per trace here)
print("ROUTES " + json.dumps({"ok": 1}))
""")
    assert res["ok"] == 1


def test_size_accounting_in_25_launches():
    """mpc_launch_sizes under the same cut: the sizes pointers of pieces 1 .. 24 (`A->sizes[i] + at`), for a BDI handle's
    histogram over the caller's array and for a best-of over four members (BDI, FPC, BPC and the VPC probe
    configuration)."""
    res = _run(r"""
import torch
L, BINS = 64, mpc.MPC_SIZE_BINS
lines = two_traces(L)[1][1]
d_lines = torch.from_numpy(lines).to("cuda:0")
bo, fo, po, vo = O.BdiOracle(L), O.FpcOracle(L), O.BpcOracle(L), O.VpcOracle(C.probe_config(L))
want = [bo.compress(lines)[0], fo.compress(lines), po.compress(lines), vo.compress(lines)[0]]
hist = lambda s: np.bincount(np.minimum(s.astype(np.int64), BINS - 1), minlength=BINS)
# a BDI handle, the caller's sizes array
ev = mpc.BDI(L)
ev.enable_size_histogram()
d_s = torch.zeros(N, dtype=torch.int16, device="cuda:0")
before = launches()
ev.compress_device(d_lines.data_ptr(), N, d_s.data_ptr())
got = ev.size_histogram()
assert launches() - before == PIECES, ("launches of the size pass", launches() - before)           # (bdi_kernel's launch is not cut)
assert (d_s.cpu().numpy().view(np.uint16) == want[0]).all(), "BDI sizes"
assert (got == hist(want[0])).all(), ("BDI histogram", np.nonzero(got != hist(want[0]))[0][:10].tolist())
ev.close()
# best-of over four members
members = [mpc.BDI(L), mpc.FPC(L), mpc.BPC(L), mpc.VPC(C.probe_config(L))]
group = mpc.EvaluatorSet(members)
for m in members: m.enable_size_histogram()
group.enable_best()
d_sizes = [torch.zeros(N, dtype=torch.int16, device="cuda:0") for _ in members]
before = launches()
group.compress_device(d_lines.data_ptr(), N, d_sizes=[t.data_ptr() for t in d_sizes])
group.sync()
# the VPC member's kernel and the one size pass over the best-of set, PIECES launches each
assert launches() - before == 2 * PIECES, ("launches of the group", launches() - before)
M = np.stack([w.astype(np.int64) for w in want])
best, winner = M.min(axis=0), M.argmin(axis=0)                  # argmin: the first minimal member
b = group.best()
for k, m in enumerate(members):
    assert (d_sizes[k].cpu().numpy().view(np.uint16) == want[k]).all(), ("sizes of member", k)
    assert (m.size_histogram() == hist(want[k])).all(), ("histogram of member", k)
assert (b["bins"] == hist(best)).all(), "best-of histogram"
assert b["wins"].tolist() == [int((winner == k).sum()) for k in range(4)], ("wins", b["wins"].tolist())
assert b["best_bits"] == int(best.sum()) and b["lines"] == N
group.close()
for m in members: m.close()
print("ROUTES " + json.dumps({"wins": b["wins"].tolist()}))
""")
    assert sum(res["wins"]) == N_LINES and min(res["wins"]) > 0          # every member's wins took part in the sums


DEFER_LIMIT = (1 << 20) - 1      # kBdiDeferMaxLines of the test library (the product's: 2^32 - 1)


@pytest.mark.parametrize("L", [32, 64])
def test_bdi_deferral_limit(L):
    """One launch of 2^20 - 1 - 64 lines defers (the queue fills and drains); one of 2^20 + 64 + 37 lines may not, and
    bdi_line<NW, true> runs its exact scans inline with the queue empty: the path a product launch of more than 2^32
    lines takes.  bdi_kernel (BDI alone) and baselines_kernel (the BDI + FPC + BPC group) on device batches, so that each is
    one launch; lines around the screening thresholds (bdi_screen_stress) between interleaved ones, drawn from a pool
    with replacement.  Per-line results and statistics against the oracle; the route counters say which path ran."""
    res = _run_with_test_library(r"""
import torch
L, LIMIT = %d, %d
pool = np.concatenate([T.bdi_screen_stress(24000, L), T.mixed(16000, L), T.bdi_stress(2800, L), T.structured(2400, L, seed=3)])
n_hi = LIMIT + 1 + 64 + 37
lines = np.ascontiguousarray(pool[np.random.default_rng(60 + L).integers(0, len(pool), n_hi)])
d_lines = torch.from_numpy(lines).to("cuda:0")
res = {}
for tag, n in (("below", LIMIT - 64), ("above", n_hi)):
    part = lines[:n]
    bo, fo, po = O.BdiOracle(L), O.FpcOracle(L), O.BpcOracle(L)
    s_ref, k_ref = bo.compress(part)
    def check(what, ev, d_s, d_k):
        s, k = d_s.cpu().numpy().view(np.uint16), d_k.cpu().numpy()
        bad = np.nonzero((s != s_ref) | (k != k_ref))[0]
        assert bad.size == 0, (tag, what, "BDI results differ at lines", bad[:10].tolist())
        assert (ev.stats_vector() == bo.stats_vector()).all(), (tag, what, "BDI statistics")
    # BDI alone
    ev = mpc.BDI(L)
    d_s = torch.zeros(n, dtype=torch.int16, device="cuda:0"); d_k = torch.full((n,), -1, dtype=torch.int8, device="cuda:0")
    ev.compress_device(d_lines.data_ptr(), n, d_s.data_ptr(), d_k.data_ptr())
    check("solo", ev, d_s, d_k)
    res[tag + "/solo"] = routes(ev)
    ev.reset()
    ev.compress_device(d_lines.data_ptr(), n)                      # without per-line outputs
    assert (ev.stats_vector() == bo.stats_vector()).all(), (tag, "solo, statistics only")
    ev.close()
    # the group's kernel
    members = [mpc.BDI(L), mpc.FPC(L), mpc.BPC(L)]
    group = mpc.EvaluatorSet(members)
    assert group.form == "BDI+FPC+BPC: one kernel", group.form
    d_sz = [torch.zeros(n, dtype=torch.int16, device="cuda:0") for _ in members]
    d_sl = [torch.full((n,), -1, dtype=torch.int8, device="cuda:0") for _ in members]
    group.compress_device(d_lines.data_ptr(), n, d_sizes=[t.data_ptr() for t in d_sz], d_selected=[t.data_ptr() for t in d_sl])
    group.sync()
    check("group", members[0], d_sz[0], d_sl[0])
    for m, o, d in ((members[1], fo, d_sz[1]), (members[2], po, d_sz[2])):
        assert (d.cpu().numpy().view(np.uint16) == o.compress(part)).all() and (m.stats_vector() == o.stats_vector()).all(), (tag, "group", type(m).__name__)
    res[tag + "/group"] = routes(members[0])
    group.close()
    for m in members: m.close()
print("ROUTES " + json.dumps(res))
""" % (L, DEFER_LIMIT), grid_cap=0)
    for what in ("solo", "group"):
        lo, hi = res["below/" + what], res["above/" + what]
        assert lo["bdi_deferred"] > 0 and lo["bdi_drains"] > 0, (what, lo)          # the deferring path ran ...
        assert hi["bdi_deferred"] == 0 and hi["bdi_drains"] == 0, (what, hi)        # ... and here the inline one did
