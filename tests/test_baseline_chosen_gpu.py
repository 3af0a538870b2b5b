"""The BDI, FPC and BPC kernels on the chosen lines of tests/baseline_chosen.py against the reference's recorded numbers
(tests/golden/ref_baseline_chosen_vectors.npz): per-line sizes, `selected`, the statistics vector and `comp_ratio`, all
for equality.  Every case through the host stager, through the device path and statistics-only; the three compressors as a
group with all four member sets (baselines_kernel's masks 3, 5, 6, 7) at 32, 64 and 128 bytes; and BDI's lines in four
arrangements that send them down bdi_line's inline scans or into the wave's queue of deferred lines (test library: the
route counters say which).  tests/test_baseline_chosen_cpu.py shows what the cases reach and which mistakes they reject."""
import functools
import os

import numpy as np
import pytest

from conftest import pkg

import baseline_chosen as bc
import baseline_ref
from testlib_child import _run_with_test_library

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def mpc():
    m = pkg()
    m.lib()
    return m


@functools.lru_cache(maxsize=None)
def fixture():
    return bc.load_fixture(os.path.join(GOLDEN, "ref_baseline_chosen_vectors.npz"))


def _recorded(name, lines):
    meta, arrays = fixture()
    case = next(c for c in meta["cases"] if c["name"] == name)
    assert len(lines) == case["n"] and bc.digest(lines) == case["sha256"], f"{name}: the builders drifted"
    sel = arrays[name + ".states"] if case["comp"] == "BDI" else np.zeros(case["n"], np.int8)
    return case, arrays[name + ".sizes"], sel


def _check_lines(name, sizes, sel, want_sizes, want_sel):
    bad = np.nonzero((sizes != want_sizes) | (sel != want_sel))[0]
    assert bad.size == 0, (f"{name}: {bad.size} lines differ, first {bad[:5]}: sizes {sizes[bad[:5]]} vs "
                           f"{want_sizes[bad[:5]]}, selected {sel[bad[:5]]} vs {want_sel[bad[:5]]}")


def _check_totals(name, ev, case):
    arrays = fixture()[1]
    stats = arrays[name + ".stats"]
    assert (ev.stats_vector() == baseline_ref.stats_vector(case["comp"], case["n"], stats)).all(), name
    res = ev.result()
    assert res["comp_ratio"] == float(arrays[name + ".ratio"][0]), name            # the same double
    if case["comp"] != "BDI":
        assert res["total_words"] == int(stats[2]), name


@pytest.mark.parametrize("name", bc.NAMES)
def test_host_stager(mpc, name):
    lines, _ = bc.build(name)
    case, want_sizes, want_sel = _recorded(name, lines)
    ev = getattr(mpc, case["comp"])(case["L"])
    sizes, sel = ev.compress_lines(lines)
    _check_lines(name, sizes, sel, want_sizes, want_sel)
    _check_totals(name, ev, case)
    ev.close()


@pytest.mark.parametrize("name", bc.NAMES)
def test_device_path(mpc, name):
    import torch
    lines, _ = bc.build(name)
    case, want_sizes, want_sel = _recorded(name, lines)
    ev = getattr(mpc, case["comp"])(case["L"])
    d_lines = torch.from_numpy(np.array(lines)).to("cuda:0")
    d_sizes = torch.empty(len(lines), dtype=torch.int16, device="cuda:0")
    d_sel = torch.full((len(lines),), -1, dtype=torch.int8, device="cuda:0")
    ev.compress_device(d_lines.data_ptr(), len(lines), d_sizes.data_ptr(), d_sel.data_ptr(),
                       stream=torch.cuda.current_stream().cuda_stream)
    ev.sync()
    torch.cuda.synchronize()
    _check_lines(name, d_sizes.cpu().numpy().view(np.uint16), d_sel.cpu().numpy(), want_sizes, want_sel)
    _check_totals(name, ev, case)
    ev.close()


@pytest.mark.parametrize("name", bc.NAMES)
def test_statistics_only(mpc, name):
    lines, _ = bc.build(name)
    case, _, _ = _recorded(name, lines)
    ev = getattr(mpc, case["comp"])(case["L"])
    assert ev.compress_lines(lines, want_sizes=False, want_selected=False) == (None, None)
    _check_totals(name, ev, case)
    ev.close()


@pytest.mark.parametrize("comps", [("BDI", "FPC"), ("BDI", "BPC"), ("FPC", "BPC"), ("BDI", "FPC", "BPC")], ids="+".join)
@pytest.mark.parametrize("L", bc.GROUP_SIZES)
def test_group(mpc, L, comps):
    lines = bc.group_lines(L)
    members = [getattr(mpc, c)(L) for c in comps]
    group = mpc.EvaluatorSet(members)
    assert group.form == "+".join(comps) + ": one kernel", group.form
    outs = group.compress_lines(lines)
    for c, ev, (sizes, sel) in zip(comps, members, outs):
        name = f"group_L{L}.{c}"
        case, want_sizes, want_sel = _recorded(name, lines)
        _check_lines(f"{name} in {'+'.join(comps)}", sizes, sel, want_sizes, want_sel)
        _check_totals(name, ev, case)
    group.close()
    for ev in members:
        ev.close()


# ---- BDI: the same lines inline and deferred --------------------------------------------------------------------------
ARRANGEMENTS = r"""
import os
sys.path.insert(0, os.path.join(%(root)r, "tests"))
import baseline_chosen as bc
L = %(L)d
meta, arrays = bc.load_fixture(os.path.join(%(root)r, "tests", "golden", "ref_baseline_chosen_vectors.npz"))
name = "bdi_chosen_L%%d" %% L
chosen, layout = bc.build(name)
pool = bc.random_pool(L)
for n, l in ((name, chosen), ("pool_L%%d" %% L, pool)):
    case = next(c for c in meta["cases"] if c["name"] == n)
    assert len(l) == case["n"] and bc.digest(l) == case["sha256"], n
c_sizes, c_states = arrays[name + ".sizes"], arrays[name + ".states"]
p_sizes, p_states = arrays["pool_L%%d.sizes" %% L], arrays["pool_L%%d.states" %% L]
res = {}
def run(tag, pieces):
    # pieces: (lines, recorded sizes, recorded states) per call, a whole number of groups of 64 but for the last
    ev = mpc.BDI(L)
    n, tot_sizes, tot_states = 0, [], []
    for lines, want_sizes, want_states in pieces:
        sizes, sel = ev.compress_lines(lines)
        bad = np.nonzero((sizes != want_sizes) | (sel != want_states))[0]
        assert bad.size == 0, (tag, n, bad.size, bad[:5].tolist(), sizes[bad[:5]].tolist(), want_sizes[bad[:5]].tolist(),
                               sel[bad[:5]].tolist(), want_states[bad[:5]].tolist())
        n += len(lines)
        tot_sizes.append(want_sizes)
        tot_states.append(want_states)
    assert (ev.stats_vector() == bc.bdi_stats_vector(L, np.concatenate(tot_sizes), np.concatenate(tot_states))).all(), tag
    res[tag] = dict(routes(ev), lines=n)
    ev.close()
# dense: 64 lines of one family per wave
for fam in bc.BDI_FAMILIES:
    rows = bc.family_rows(layout, fam)
    run("dense " + fam, [(chosen[rows], c_sizes[rows], c_states[rows])])
rows = bc.dense_b8d1_rows(L)
run("dense B8D1 fits", [(chosen[rows], c_sizes[rows], c_states[rows])])
# planted: k chosen lines among random ones in every group of 64 (1; 12 and 13, either side of MPC_BDI_DEFER_MAX),
# 4096 groups per call
def planted(k):
    for a in range(0, len(chosen), 4096 * k):
        rows = slice(a, a + 4096 * k)
        src = bc.planted(len(chosen[rows]), k)
        yield bc.take(src, chosen[rows], pool), bc.take(src, c_sizes[rows], p_sizes), bc.take(src, c_states[rows], p_states)
for k in (1, 12, 13):
    run("planted %%d" %% k, planted(k))
print("ROUTES " + json.dumps(res))
"""


@pytest.mark.parametrize("L", bc.BDI_SIZES)
def test_bdi_arrangements(L):
    """The chosen BDI lines dense (a wave's 64 lines from one family: most scans are wanted by many lanes and run inline),
    one planted among 63 random lines (its scans are wanted by one lane: deferred and run from the queue), and 12 and 13
    per group of 64 (at most MPC_BDI_DEFER_MAX = 12 wanting lanes defer).  Every arrangement gives every chosen line the
    recorded size and state and every random line its own; the child compares, the route counters come back.  Lines are
    deferred at 32 and 64 bytes (bdi_kernel<NW <= 16>); at 128 bytes and in baseline_generic_kernel nothing is."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = _run_with_test_library(ARRANGEMENTS % {"root": root, "L": L}, grid_cap=0, timeout=300)
    assert set(res) == {"dense " + f for f in bc.BDI_FAMILIES} | {"dense B8D1 fits", "planted 1", "planted 12", "planted 13"}
    assert res["dense B8D1 fits"]["bdi_deferred"] == 0 and res["dense B8D1 fits"]["bdi_drains"] == 0, res
    if L in (32, 64):
        for tag in ("planted 1", "planted 12"):
            assert res[tag]["bdi_deferred"] > 0 and res[tag]["bdi_drains"] > 0, (tag, res[tag])
        # 13 wanting lanes run inline: what is still deferred there are scans that fewer of the 13 lines want
        assert res["planted 13"]["bdi_deferred"] < res["planted 12"]["bdi_deferred"], res
    else:
        assert all(r["bdi_deferred"] == 0 and r["bdi_drains"] == 0 for r in res.values()), res
