"""The VPC lane kernel's work distribution at its edges and its two-tier certificate, against the CPU oracle
(csrc/mpc_vpc_lane.hip: the block ticket in vpc_lane_body, the grid in lane_launch, lane_certified_fast / lane_certified_exact).

Scheduling.  A workgroup owns a range of 128-line blocks and its waves draw them from a ticket in LDS; the lines behind
the last whole block go to one wave of the launch.  The test library caps the grid (MPC_TEST_GRID=96: at most six
workgroups of 16 waves, twelve of 8), so a few thousand lines give every wave several blocks.  Shapes: fewer blocks than
workgroups, than waves, 31 / 32 / 33 blocks and 32 k + 1 blocks up to 225, each with a tail of 0, 1, 63, 64 or 127 lines
behind the last whole block, and line counts below 128.  (31 / 32 / 33 and 32 k + 1 are no edges of the range-and-ticket
scheduler in the tree; they are kept as regression shapes for it -- counts that are and are not multiples of the waves of a
workgroup and of the workgroups -- from a hand-out by 32-block chunks that was measured and not kept.)  Every case
compares the per-line sizes, the selectors and the statistics vector with the oracle, and the route counters must say that plain + paired blocks == n_lines >> 7 exactly (no block twice, none left out) and that the
tail took its groups.  Traces: random; the mixed trace (paired groups and deferral); random lines whose last 32 blocks
and tail are compressible lines.  Launch scenarios: three launches back to back on one handle without a reset, and two
handles interleaved on two streams.

Certificate.  Lines built from a chosen scanned array of the last prediction module (tests/vpc_synth.py), 64 of a kind
behind 64 lines that the fast tier closes: exactly 29 and exactly 28 rows that cost 17 bits, a row whose front half is
non-zero only in column 7 (a 17-bit row that only the exact tier can count), a zero row.  Sizes and selectors must equal
the oracle's, and the route counters must show which tier ran and whether the encoder did."""
import numpy as np
import pytest

from testlib_child import ROUTE_NAMES, _run_with_test_library

pytestmark = pytest.mark.gpu

# what every child process defines: the route counters by name (MPC_RT_* of csrc/mpc_kernel_common.h) and one checked run
# (the names of testlib_child and, behind them, the three counters of the certificate's tiers)
COMMON = r"""
NAMES = @NAMES@
def routes2(ev):
    f = mpc.lib().mpc_test_routes
    f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]; f.restype = ctypes.c_int
    out = (ctypes.c_uint64 * 16)()
    assert f(ev._h, out, 16) == 0
    return dict(zip(NAMES, [int(x) for x in out]))
def check(cfg, lines, what, out=True):
    L, n = lines.shape[1], len(lines)
    ev, o = mpc.VPC(cfg), O.VpcOracle(cfg)
    s_ref, k_ref = o.compress(lines)
    if out:
        s, k = ev.compress_lines(lines)
        assert (s == s_ref).all(), (what, "sizes", np.nonzero(s != s_ref)[0][:8])
        assert (k == k_ref).all(), (what, "selectors", np.nonzero(k != k_ref)[0][:8])
    else:
        ev.compress_lines(lines, want_sizes=False, want_selected=False)
    v, v_ref = ev.stats_vector(), o.stats_vector()
    assert (v == v_ref).all(), (what, "statistics", np.nonzero(v != v_ref)[0][:8])
    r = routes2(ev)
    blocks = n >> 7
    assert r["vpc_plain_blocks"] + r["vpc_paired_blocks"] == blocks, (what, r, blocks)
    assert r["vpc_tail_groups"] == ((n & 127) + 63) // 64, (what, r)
    ev.close()
    return r
""".replace("@NAMES@", repr(ROUTE_NAMES + ["vpc_cert_groups", "vpc_cert_exact", "vpc_encoder"]))

TAILS = (0, 1, 63, 64, 127)
# blocks: fewer than workgroups / waves | 32 and its neighbours | 32 k + 1 with two, four and six workgroups
SHAPES = (1, 2, 15, 16, 31, 32, 33, 65, 97, 129, 193, 225)


def _trace_code(trace):
    return {
        "random": "T.random_u32(n, L, seed=11)",
        "mixed": "T.mixed(n, L, first_line=3)",
        # random lines; the last 32 blocks (fewer: all of them) and the tail are compressible lines
        "compressible_end": "compressible_end(n, L)",
    }[trace]


@pytest.mark.parametrize("trace", ["random", "mixed", "compressible_end"])
def test_shapes_64(trace):
    """64-byte lines: every shape with every tail -- 0, 1, 63, 64, 127 on the random trace, 1, 63, 64, 127 on the other two.
    Per-line outputs; the statistics-only kernel too on two of the 32 k + 1 shapes."""
    code = COMMON + r"""
def compressible_end(n, L):
    a = T.random_u32(n, L, seed=12).copy()
    first = max((n >> 7) - 32, 0) * 128
    a[first:] = T.structured(n - first, L)
    return a
cfg, L, res = C.probe_config(64), 64, {}
for blocks, tail in %r:
    n = 128 * blocks + tail
    lines = np.ascontiguousarray(%s)
    res[f"{blocks}+{tail}"] = check(cfg, lines, (blocks, tail))
    if blocks in (65, 193) and tail == 63:
        check(cfg, lines, (blocks, tail, "statistics only"), out=False)
for n in (1, 64, 127):
    check(cfg, np.ascontiguousarray(%s), ("below a block", n))
print("ROUTES " + json.dumps(res))
"""
    full = trace == "random"
    cases = [(b, t) for b in SHAPES for t in TAILS if full or t != 0]
    expr = _trace_code(trace)
    res = _run_with_test_library(code % (cases, expr, expr), grid_cap=96, timeout=600)
    assert len(res) == len(cases)
    if trace == "mixed":
        assert res["193+63"]["vpc_paired_blocks"] > 0, res["193+63"]


@pytest.mark.parametrize("L", [32, 128])
def test_shapes_other_line_sizes(L):
    """32- and 128-byte lines (workgroups of 16 and of 8 waves): 32 +- 1 blocks and 32 k + 1 blocks, tails of 1 and 127
    lines, random and mixed."""
    code = COMMON + r"""
L, res = %d, {}
cfg = C.probe_config(L)
for blocks in %r:
    for tail in (1, 127):
        n = 128 * blocks + tail
        for name, lines in (("random", T.random_u32(n, L, seed=13)), ("mixed", T.mixed(n, L, first_line=1))):
            res[f"{name} {blocks}+{tail}"] = check(cfg, np.ascontiguousarray(lines), (name, blocks, tail))
print("ROUTES " + json.dumps(res))
"""
    shapes = (7, 31, 32, 33, 97, 193) if L == 32 else (7, 32, 33, 97)
    res = _run_with_test_library(code % (L, shapes), grid_cap=96, timeout=600)
    assert len(res) == 4 * len(shapes)


def test_launches_back_to_back_and_two_handles_on_two_streams():
    """Device-resident launches.  Three launches on one handle and one stream without a reset: the statistics are the
    oracle's of the three traces in order, each launch handed out its own blocks once.  Then two handles, each on a stream
    of its own, launches interleaved: neither disturbs the other."""
    code = COMMON + r"""
import torch
cfg = C.probe_config(64)
parts = [T.random_u32(128 * 97 + 5, 64, seed=21), T.mixed(128 * 65 + 64, 64), T.random_u32(128 * 193, 64, seed=22)]
st = torch.cuda.Stream()
ev, o = mpc.VPC(cfg), O.VpcOracle(cfg)
dev = [torch.from_numpy(np.ascontiguousarray(p)).to("cuda:0") for p in parts]
torch.cuda.synchronize()
for p, d in zip(parts, dev):
    o.compress(p)
    ev.compress_device(d.data_ptr(), len(p), stream=st.cuda_stream)
torch.cuda.synchronize()
assert (ev.stats_vector() == o.stats_vector()).all(), "three launches back to back"
r = routes2(ev)
assert r["vpc_plain_blocks"] + r["vpc_paired_blocks"] == sum(len(p) >> 7 for p in parts), r
ev.close()
# two handles, two streams
s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
e1, e2, o1, o2 = mpc.VPC(cfg), mpc.VPC(cfg), O.VpcOracle(cfg), O.VpcOracle(cfg)
for rnd in range(3):
    for ev_, o_, s_, k in ((e1, o1, s1, rnd), (e2, o2, s2, 2 - rnd)):
        o_.compress(parts[k])
        ev_.compress_device(dev[k].data_ptr(), len(parts[k]), stream=s_.cuda_stream)
torch.cuda.synchronize()
assert (e1.stats_vector() == o1.stats_vector()).all(), "handle 1 of two"
assert (e2.stats_vector() == o2.stats_vector()).all(), "handle 2 of two"
res = {"one": r, "a": routes2(e1), "b": routes2(e2)}
e1.close(); e2.close()
print("ROUTES " + json.dumps(res))
"""
    res = _run_with_test_library(code, grid_cap=96, timeout=600)
    blocks = 97 + 65 + 193
    for k in ("a", "b"):
        assert res[k]["vpc_plain_blocks"] + res[k]["vpc_paired_blocks"] == blocks, res[k]


def test_certificate_tiers_on_chosen_scanned_arrays():
    """Four blocks per case, one per wave of one workgroup: 64 lines that the fast tier closes (32 rows with bits in
    columns 0 and 15), then 64 lines of the case.  -> (fast-tier groups, exact-tier groups, encoder groups):
      29 seventeen-bit rows + 3 single ones       fast tier closes them: (8, 0, 0)
      the same, one single one in column 8        that row has no fold, the fast tier cannot call it non-zero; the exact
                                                  one closes the lines: (8, 4, 0)
      28 seventeen-bit rows + 4 single ones       10 * 28 + 7 * 32 = 504 < 512: both tiers leave them open, the encoder
                                                  runs and finds 28 * 17 + 4 * 7 = 504 bits: compressed, (8, 4, 4)
      28 + a row with bits in columns 7 and 15    the fast tier counts 28, the exact one 29: closed there, (8, 4, 0)
         only + 3 single ones
      31 seventeen-bit rows + a zero row          the fast tier wants every row non-zero; the exact one: 310 + 217 + 4: (8, 4, 0)"""
    code = COMMON + r"""
sys.path.insert(0, "tests")
import vpc_synth as S
cfg = C.probe_config(64)
k = S.pred_modules(cfg)[-1]
rng = np.random.default_rng(7)
def rows17(n):
    return S.row_17(rng, n)
def single():
    return S.row_of("single", rng)
def arrays(kind):
    out = []
    for _ in range(64):
        a = rows17(32)
        if kind == "n29": a[[3, 17, 30]] = [0x4000, 0x0800, 0x0002]            # single ones the folds see (columns 1, 4, 14)
        elif kind == "n29_col8": a[[3, 17, 30]] = [0x4000, 0x0080, 0x0002]     # ... one of them in column 8: a row without a fold
        elif kind == "n28": a[[3, 9, 17, 30]] = [single() for _ in range(4)]
        elif kind == "col7": a[[3, 17, 30]] = [single() for _ in range(3)]; a[9] = 0x0101
        elif kind == "zero": a[12] = 0
        out.append(a)
    return np.array(out, np.uint16)
def build(kind):
    lines, ok, why = S.lines_for_scanned(cfg, k, arrays(kind))
    assert ok.all(), (kind, [w for w in why if w is not None][:3])
    return lines
base = build("base")
res = {}
for kind in ("n29", "n29_col8", "n28", "col7", "zero"):
    case = build(kind)
    lines = np.ascontiguousarray(np.concatenate([base, case] * 4))
    r = check(cfg, lines, kind)
    o = O.VpcOracle(cfg); s_ref, k_ref = o.compress(case)
    res[kind] = dict(r, compressed=int((k_ref != -1).sum()), last_module=int((k_ref == k).sum()))
print("ROUTES " + json.dumps(res))
"""
    res = _run_with_test_library(code, grid_cap=1, timeout=600)
    got = {kind: (r["vpc_cert_groups"], r["vpc_cert_exact"], r["vpc_encoder"]) for kind, r in res.items()}
    assert got == {"n29": (8, 0, 0), "n29_col8": (8, 4, 0), "n28": (8, 4, 4), "col7": (8, 4, 0), "zero": (8, 4, 0)}, got
    assert res["n28"]["compressed"] == 64 and res["n28"]["last_module"] == 64, res["n28"]
    for kind in ("n29", "n29_col8", "col7", "zero"):
        assert res[kind]["compressed"] == 0, (kind, res[kind])
