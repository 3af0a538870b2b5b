"""Every VPC kernel form on lines built from chosen scanned arrays (tests/vpc_synth.py), against the CPU oracle.

The parity tests elsewhere feed natural traces and take whatever scanned arrays come out; here the array is chosen:
a walking one at every scan position, walking pairs (adjacent, and at distances 2 and 8 inside a row), every count of
leading zero rows, the encoder's row classes around zero runs, and a ladder of 17-bit rows that puts the encoder size on
both sides of 8 L.  A mask that is wrong at one column of one plane, a certificate that miscounts one row class or an
encoder that prices one class wrongly shows as a per-line mismatch whose message names the family, the module and the
scan position or row.

Configurations: the ten built-in unrolled ones, the five general-layout twins, the eight compiled at creation (one
compilation each, cached for the module), the four run-time-loop cases with prediction modules, four for the generic
kernel, and the companions of tests/vpc_synth_cases.py (a free last module where the original's is ConsecutiveBase or
has a forced byte).  Each runs dense (built lines one after the other: every lane passes the target's prefilter),
planted (built lines at lanes 0 / 31 / 63 of groups of random lines, rotated per group: few lanes pass, lines are set
aside) and cold (a group of random lines before every group of built lines: the unrolled kernels consult the
incompressibility certificate only behind a group that kept no line, which dense and planted lines rarely are -- a
certificate that miscounted columns 7 / 8 in a scratch copy of the source passed both and failed here), in four calls
of 128 k + r lines, r = 0, 1, 63, 65 (whole blocks through the line ring, the rest through the plain-load tail), with
per-line outputs and through the statistics-only instantiation.  Dense and cold run every built line, and so does
planted up to 64-byte lines (the line sizes at which the kernels set lines aside); at 128 and 256 bytes planted takes
a seeded sample of at most 16384 / L lines of every (family, module), so that a case stays at a few seconds."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from conftest import pkg

import vpc_ref
import vpc_synth as S
from vpc_synth_cases import COMPANIONS, built, config_of, filler, form_of, planted_per_family

pytestmark = pytest.mark.gpu

CONFIGS = (vpc_ref._FORM["unrolled"] + vpc_ref._FORM["unrolled, general layout"] + vpc_ref._FORM["unrolled, compiled at creation"]
           + ["loop_bm_root_L64", "loop_many_L32", "loop_k8_L128", "loop_trunc12_L32"] + ["perm_L64", "L12", "L48", "L256"]
           + sorted(COMPANIONS))
DEVICE_PASS = ["probe_L64", "root1_L64", "jit_bytemajor_L64", "loop_k8_L128", "L48"]       # one per form


@pytest.fixture(scope="module")
def mpc():
    m = pkg()
    m.lib()
    return m


@pytest.fixture(scope="module")
def jit_cache(tmp_path_factory):
    return str(tmp_path_factory.mktemp("jit"))


def oracle_in_pieces(oracle, cfg, lines, pieces=8):
    """The oracle's per-line sizes, selectors and statistics vector, the lines split over threads (the C oracle runs
    without the interpreter lock; every count of the vector is a sum over lines, so the pieces' vectors add up)."""
    parts = [p for p in np.array_split(lines, pieces) if len(p)]

    def one(part):
        o = oracle.VpcOracle(cfg)
        s, k = o.compress(part)
        return s, k, o.stats_vector()
    with ThreadPoolExecutor(len(parts)) as pool:
        out = list(pool.map(one, parts))
    return np.concatenate([o[0] for o in out]), np.concatenate([o[1] for o in out]), sum(o[2] for o in out[1:]) + out[0][2]


@pytest.fixture(scope="module")
def reference(oracle):
    """Per (configuration, arrangement): the four calls' lines and origins, the oracle's per-line sizes and selectors
    over all of them and its statistics vector -- computed once, read-only."""
    cache = {}

    def get(name, arrangement):
        key = (name, arrangement)
        if key not in cache:
            cfg = config_of(name)
            L = int(cfg["overview"]["lineSize"])
            calls = S.arrange(built(name), L, arrangement, filler,
                              per_family=planted_per_family(L) if arrangement == "planted" else None)
            assert [len(c[0]) % 128 for c in calls] == list(S.TAILS)
            s_ref, k_ref, v_ref = oracle_in_pieces(oracle, cfg, np.concatenate([c[0] for c in calls]))
            origin = np.concatenate([c[1] for c in calls])
            for a in [s_ref, k_ref, v_ref, origin] + [c[0] for c in calls]:
                a.setflags(write=False)
            cache[key] = (calls, origin, s_ref, k_ref, v_ref)
        return cache[key]

    return get


def _handle(mpc, name):
    ev = mpc.VPC(config_of(name))
    assert vpc_ref.form_of(ev.kernel_form) == form_of(name), (name, ev.kernel_form, ev.path_reason)
    return ev


def _explain(name, arrangement, origin, s, k, s_ref, k_ref):
    bad = np.nonzero((s != s_ref) | (k != k_ref))[0]
    if bad.size == 0:
        return None
    idx = S.index(built(name))
    what = []
    for i in bad[:5]:
        fam = "a filler line (random)" if origin[i] < 0 else "family %s, module %d, %s" % idx[origin[i]]
        what.append(f"line {i} [{fam}]: size {s[i]} vs {s_ref[i]}, selector {k[i]} vs {k_ref[i]}")
    families = sorted({idx[origin[i]][0] + f" (module {idx[origin[i]][1]})" for i in bad if origin[i] >= 0})
    return f"{name} ({arrangement}): {bad.size} lines differ from the oracle, in {families}; " + "; ".join(what)


@pytest.mark.parametrize("arrangement", ["dense", "planted", "cold"])
@pytest.mark.parametrize("name", CONFIGS)
def test_families_against_oracle(mpc, reference, jit_cache, monkeypatch, name, arrangement):
    monkeypatch.setenv("MPC_JIT_CACHE", jit_cache)
    monkeypatch.delenv("MPC_JIT", raising=False)
    calls, origin, s_ref, k_ref, v_ref = reference(name, arrangement)
    # per-line outputs
    ev = _handle(mpc, name)
    out = [ev.compress_lines(lines) for lines, _ in calls]
    s, k = np.concatenate([o[0] for o in out]), np.concatenate([o[1] for o in out])
    msg = _explain(name, arrangement, origin, s, k, s_ref, k_ref)
    assert msg is None, msg
    v = ev.stats_vector()
    assert (v == v_ref).all(), f"{name} ({arrangement}): statistics (per-line-output kernel) differ at {np.nonzero(v != v_ref)[0][:10]}"
    ev.close()
    # statistics only: another instantiation
    ev = _handle(mpc, name)
    for lines, _ in calls:
        ev.compress_lines(lines, want_sizes=False, want_selected=False)
    v = ev.stats_vector()
    assert (v == v_ref).all(), f"{name} ({arrangement}): statistics (statistics-only kernel) differ at {np.nonzero(v != v_ref)[0][:10]}"
    ev.close()


@pytest.mark.parametrize("name", DEVICE_PASS)
def test_walking_one_device_resident(mpc, oracle, jit_cache, monkeypatch, name):
    """The dense walking-one family of every prediction module in one device-resident call (no staging: the built-in
    kernel's deferral behaves differently)."""
    import torch
    monkeypatch.setenv("MPC_JIT_CACHE", jit_cache)
    monkeypatch.delenv("MPC_JIT", raising=False)
    fam = [b for b in built(name) if b["family"] == "walking_one"]
    lines = np.ascontiguousarray(np.concatenate([b["lines"] for b in fam]))
    o = oracle.VpcOracle(config_of(name))
    s_ref, k_ref = o.compress(lines)
    ev = _handle(mpc, name)
    d_lines = torch.from_numpy(lines).to("cuda:0")
    d_sizes = torch.empty(len(lines), dtype=torch.int16, device="cuda:0")
    d_sel = torch.full((len(lines),), -2, dtype=torch.int8, device="cuda:0")
    ev.compress_device(d_lines.data_ptr(), len(lines), d_sizes.data_ptr(), d_sel.data_ptr(),
                       stream=torch.cuda.current_stream().cuda_stream)
    ev.sync()
    torch.cuda.synchronize()
    s, k = d_sizes.cpu().numpy().view(np.uint16), d_sel.cpu().numpy()
    bad = np.nonzero((s != s_ref) | (k != k_ref))[0]
    idx = S.index(fam)
    assert bad.size == 0, (f"{name}: {bad.size} walking-one lines differ, first " +
                           "; ".join("module %d, %s" % idx[i][1:] + f": size {s[i]} vs {s_ref[i]}, selector {k[i]} vs {k_ref[i]}"
                                     for i in bad[:5]))
    assert (ev.stats_vector() == o.stats_vector()).all(), name
    ev.close()


def test_planted_lines_are_set_aside_and_alternating_lines_pair_up():
    """The route counters of the test library (a fresh process, the grid capped to one workgroup) for the probe
    configuration at 64 bytes.  Planted: three built lines in 64 pass a module's prefilter, so they are set aside into the
    wave's queue and drained.  Paired blocks need at least 16 lines of ONE parity to pass a module's prefilter
    (lane_prefilters, csrc/mpc_vpc_lane.hip) -- three planted lines never do -- so a third arrangement is run for them:
    OneBase's walking-one lines on the even lines, random lines on the odd ones.  Results against the oracle in all."""
    from testlib_child import _run_with_test_library
    code = r"""
sys.path.insert(0, "tests")
import vpc_synth as S
from vpc_synth_cases import built, config_of, filler
cfg, b = config_of("probe_L64"), built("probe_L64")
planted = np.concatenate([c[0] for c in S.arrange(b, 64, "planted", filler)])
one = np.concatenate([x["lines"] for x in b if x["module"] == 2 and x["family"] in ("walking_one", "walking_pairs")])
alternating = T.random_u32(2 * len(one), 64, seed=5).copy()
alternating[0::2] = one
res = {}
for name, lines in (("planted", planted), ("alternating", alternating)):
    ev, o = mpc.VPC(cfg), O.VpcOracle(cfg)
    s, k = ev.compress_lines(lines)
    s_ref, k_ref = o.compress(lines)
    assert (s == s_ref).all() and (k == k_ref).all() and (ev.stats_vector() == o.stats_vector()).all(), name
    res[name] = routes(ev)
    ev.close()
print("ROUTES " + json.dumps(res))
"""
    res = _run_with_test_library(code, grid_cap=1, timeout=600)
    p, a = res["planted"], res["alternating"]
    assert p["vpc_deferred"] > 0 and p["vpc_drains"] > 0 and p["vpc_deferred"] <= 64 * p["vpc_drains"], p
    assert a["vpc_paired_blocks"] > 0 and a["vpc_to_paired"] > 0, a
