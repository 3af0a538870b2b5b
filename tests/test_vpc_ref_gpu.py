"""VPC kernels against the reference's own VPC (tests/golden/ref_vpc_vectors.npz, written by
tests/golden/make_ref_vpc_vectors.py from VPC.cpp, VPCmodules/*.cpp and utils.cpp compiled unmodified), not against
the oracle.  Every fixture case on the kernel form it is meant for (unrolled, general layout, compiled at creation,
run-time loop, generic), in one call, in ragged calls, through the device path and split over two handles whose
statistics are merged; the cases compiled at creation again without the run-time compiler; the command line's two CSV
files byte for byte; two long cases under a grid capped to one workgroup."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, pkg

import vpc_ref

pytestmark = pytest.mark.gpu

NAMES = [c["name"] for c in vpc_ref.CASES]
AT_CREATION = [c["name"] for c in vpc_ref.CASES if c["form"] == "unrolled, compiled at creation"]


@pytest.fixture(scope="module")
def mpc():
    m = pkg()
    m.lib()
    return m


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return vpc_ref.load_fixture(os.path.join(golden_dir, "ref_vpc_vectors.npz"))


def _setup(mpc, fixture, name, forms=None):
    case = vpc_ref.fixture_case(fixture, name)
    ev = mpc.VPC(vpc_ref.case_config(case))
    assert vpc_ref.form_of(ev.kernel_form) in (forms or (case["form"],)), (name, ev.kernel_form, ev.path_reason)
    arrays = fixture[1]
    return case, ev, vpc_ref.case_input(case), arrays[name + ".sizes"], arrays[name + ".clusters"]


def _check_totals(ev, case, fixture):
    name, L = case["name"], case["L"]
    want, got = vpc_ref.stats_vector(case, fixture[1], ev.hist_bins), ev.stats_vector()
    bad = np.nonzero(got != want)[0]
    assert got.shape == want.shape and bad.size == 0, f"{name}: statistics differ at {bad[:10]}"
    res, d = ev.result(), vpc_ref.doubles(case, fixture[1])
    assert res["comp_ratio"] == d["ratio"], name
    for k in range(-1, case["M"]):
        c, w = res["clusters"][k], d["clusters"][k]
        assert c["comp_ratio"] == w["comp_ratio"], (name, k)
        if L & (L - 1) == 0:
            assert (c["mae"], c["mse"]) == (w["mae"], w["mse"]), (name, k)
        else:
            # DESIGN.md section 7, "MAE / MSE for line sizes that are not powers of two": the reference adds a rounded
            # (sum r) / L per line to a running double, the library divides the integer sums once
            assert c["mae"] == pytest.approx(w["mae"], rel=1e-12, abs=0), (name, k)
            assert c["mse"] == pytest.approx(w["mse"], rel=1e-12, abs=0), (name, k)


@pytest.mark.parametrize("name", NAMES)
def test_one_call(mpc, fixture, name):
    case, ev, lines, want_sizes, want_clusters = _setup(mpc, fixture, name)
    sizes, clusters = ev.compress_lines(lines)
    vpc_ref.check_lines(name, sizes, clusters, want_sizes, want_clusters)
    _check_totals(ev, case, fixture)
    ev.close()


@pytest.mark.parametrize("name", NAMES)
def test_ragged_calls(mpc, fixture, name):
    case, ev, lines, want_sizes, want_clusters = _setup(mpc, fixture, name)
    cuts = np.cumsum(vpc_ref.RAGGED)
    assert cuts[-1] < len(lines)
    sizes, clusters = [], []
    for part in np.split(lines, cuts):
        s, c = ev.compress_lines(part)
        sizes.append(s)
        clusters.append(c)
    vpc_ref.check_lines(name, np.concatenate(sizes), np.concatenate(clusters), want_sizes, want_clusters)
    _check_totals(ev, case, fixture)
    ev.close()


@pytest.mark.parametrize("name", NAMES)
def test_device_path(mpc, fixture, name):
    import torch
    case, ev, lines, want_sizes, want_clusters = _setup(mpc, fixture, name)
    d_lines = torch.from_numpy(lines).to("cuda:0")
    d_sizes = torch.empty(len(lines), dtype=torch.int16, device="cuda:0")
    d_sel = torch.full((len(lines),), -2, dtype=torch.int8, device="cuda:0")
    ev.compress_device(d_lines.data_ptr(), len(lines), d_sizes.data_ptr(), d_sel.data_ptr(),
                       stream=torch.cuda.current_stream().cuda_stream)
    ev.sync()
    torch.cuda.synchronize()
    vpc_ref.check_lines(name, d_sizes.cpu().numpy().view(np.uint16), d_sel.cpu().numpy(), want_sizes, want_clusters)
    _check_totals(ev, case, fixture)
    ev.close()


@pytest.mark.parametrize("name", NAMES)
def test_two_handles_merged(mpc, fixture, name):
    case, a, lines, _, _ = _setup(mpc, fixture, name)
    b = mpc.VPC(vpc_ref.case_config(case))
    h = len(lines) // 3
    a.compress_lines(lines[:h], want_sizes=False, want_selected=False)
    b.compress_lines(lines[h:], want_sizes=False, want_selected=False)
    a.stats_merge(b.stats_vector())
    _check_totals(a, case, fixture)
    a.close()
    b.close()


@pytest.mark.parametrize("name", AT_CREATION)
def test_compiled_at_creation_cases_without_the_run_time_compiler(mpc, fixture, name, monkeypatch):
    monkeypatch.setenv("MPC_JIT", "0")
    case, ev, lines, want_sizes, want_clusters = _setup(mpc, fixture, name, forms=("run-time loop", "generic"))
    sizes, clusters = ev.compress_lines(lines)
    vpc_ref.check_lines(name, sizes, clusters, want_sizes, want_clusters)
    _check_totals(ev, case, fixture)
    ev.close()


def test_cli_csv_is_the_reference_text(fixture, traces, tmp_path):
    """`compressor -a VPC -c <name>.json -i <dir>/<name>.npy`: the *_results.csv and *_results_detail.csv the command line
    writes are the text the reference's VPCResult::Print / PrintDetail wrote for the same lines (all rows but the last),
    byte for byte; for line sizes that are not powers of two only *_results.csv."""
    pkg("build").build_all()
    cli = os.path.join(ROOT, "bin", "compressor")
    meta = fixture[0]
    assert len(meta["print"]) >= 6
    for rec in meta["print"]:
        case = vpc_ref.fixture_case(fixture, rec["case"])
        out = tmp_path / rec["case"]
        npy = out / rec["npy"]
        npy.parent.mkdir(parents=True)
        traces.save_npy(str(npy), vpc_ref.case_input(case))
        cfg = pkg("configs").write_config(vpc_ref.case_config(case), str(out / (rec["case"] + ".json")))
        r = subprocess.run([cli, "-a", "VPC", "-c", cfg, "-i", str(npy), "-o", str(out)], cwd=os.path.join(ROOT, "bin"),
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        assert (out / f"{rec['case']}_results.csv").read_text() == rec["results"], rec["case"]
        if case["L"] & (case["L"] - 1) == 0:
            assert (out / f"{rec['case']}_results_detail.csv").read_text() == rec["detail"], rec["case"]


def test_long_cases_under_a_capped_grid(fixture):
    """Tens of thousands of alternating mixed lines at 64 and 32 bytes with the grid capped to one workgroup (test
    library, a fresh process): waves set lines aside and drain them inside the loop and switch to paired groups.  Per-line
    digests and statistics against the reference; the route counters say that those routes ran."""
    import test_gpu_parity
    code = r"""
sys.path.insert(0, "tests")
import vpc_ref
meta, arrays = vpc_ref.load_fixture("tests/golden/ref_vpc_vectors.npz")
res = {}
for case in meta["long"]:
    lines = vpc_ref.case_input(case)
    ev = mpc.VPC(vpc_ref.case_config(case))
    assert vpc_ref.form_of(ev.kernel_form) == case["form"], ev.kernel_form
    s, k = ev.compress_lines(lines)
    assert (vpc_ref.digest(s), vpc_ref.digest(k)) == (case["sizes_sha256"], case["clusters_sha256"]), case["name"]
    assert (ev.stats_vector() == vpc_ref.stats_vector(case, arrays, ev.hist_bins)).all(), case["name"]
    res[case["name"]] = routes(ev)
    ev.close()
print("ROUTES " + json.dumps(res))
"""
    res = test_gpu_parity._run_with_test_library(code, grid_cap=1, timeout=600)
    assert sorted(res) == sorted(c["name"] for c in fixture[0]["long"])
    for name, r in res.items():
        assert r["vpc_paired_blocks"] > 0 and r["vpc_deferred"] > 0 and r["vpc_drains"] > 0, (name, r)
