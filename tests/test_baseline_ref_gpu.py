"""BDI, FPC and BPC kernels against the reference's own compressors (tests/golden/ref_baseline_vectors.npz), not
against the oracle: every fixture case, i.e. the unrolled kernels at 32 / 64 / 128 bytes and the loop kernel
(baseline_generic_kernel) at every other line size, through the host stager in one call and in ragged calls, through
the device path, and the command line's CSV text byte for byte."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, pkg

import baseline_ref

pytestmark = pytest.mark.gpu

NAMES = [c["name"] for c in baseline_ref.CASES]
RAGGED = (1, 63, 64, 65, 511, 512, 513)          # then the rest: the in-place path (<= 512 lines) and the staged one


@pytest.fixture(scope="module")
def mpc():
    m = pkg()
    m.lib()
    return m


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return baseline_ref.load_fixture(os.path.join(golden_dir, "ref_baseline_vectors.npz"))


def _setup(mpc, fixture, name):
    meta, arrays = fixture
    case = next(c for c in meta["cases"] if c["name"] == name)
    ev = getattr(mpc, case["comp"])(case["L"])
    assert ev.kernel_path == {"BDI": mpc.MPC_PATH_BDI, "FPC": mpc.MPC_PATH_FPC, "BPC": mpc.MPC_PATH_BPC}[case["comp"]]
    want_sel = arrays[name + ".states"] if case["comp"] == "BDI" else np.zeros(case["n"], np.int8)
    return case, ev, baseline_ref.case_input(case), arrays[name + ".sizes"], want_sel


def _check_totals(ev, case, fixture):
    arrays = fixture[1]
    name, comp = case["name"], case["comp"]
    stats = arrays[name + ".stats"]
    assert (ev.stats_vector() == baseline_ref.stats_vector(comp, case["n"], stats)).all(), name
    res = ev.result()
    assert res["comp_ratio"] == float(arrays[name + ".ratio"][0]), name            # the same double
    if comp != "BDI":
        assert res["total_words"] == int(stats[2]), name


def _check_lines(name, sizes, sel, want_sizes, want_sel):
    bad = np.nonzero((sizes != want_sizes) | (sel != want_sel))[0]
    assert bad.size == 0, (f"{name}: {bad.size} lines differ, first {bad[:5]}: sizes {sizes[bad[:5]]} vs "
                           f"{want_sizes[bad[:5]]}, selected {sel[bad[:5]]} vs {want_sel[bad[:5]]}")


@pytest.mark.parametrize("name", NAMES)
def test_one_call(mpc, fixture, name):
    case, ev, lines, want_sizes, want_sel = _setup(mpc, fixture, name)
    sizes, sel = ev.compress_lines(lines)
    _check_lines(name, sizes, sel, want_sizes, want_sel)
    _check_totals(ev, case, fixture)
    ev.close()


@pytest.mark.parametrize("name", NAMES)
def test_ragged_calls(mpc, fixture, name):
    case, ev, lines, want_sizes, want_sel = _setup(mpc, fixture, name)
    cuts = np.cumsum(RAGGED)
    assert cuts[-1] < len(lines)
    sizes, sel = [], []
    for part in np.split(lines, cuts):
        s, c = ev.compress_lines(part)
        sizes.append(s)
        sel.append(c)
    _check_lines(name, np.concatenate(sizes), np.concatenate(sel), want_sizes, want_sel)
    _check_totals(ev, case, fixture)
    ev.close()


@pytest.mark.parametrize("name", NAMES)
def test_device_path(mpc, fixture, name):
    import torch
    case, ev, lines, want_sizes, want_sel = _setup(mpc, fixture, name)
    d_lines = torch.from_numpy(lines).to("cuda:0")
    d_sizes = torch.empty(len(lines), dtype=torch.int16, device="cuda:0")
    d_sel = torch.full((len(lines),), -1, dtype=torch.int8, device="cuda:0")
    ev.compress_device(d_lines.data_ptr(), len(lines), d_sizes.data_ptr(), d_sel.data_ptr(),
                       stream=torch.cuda.current_stream().cuda_stream)
    ev.sync()
    torch.cuda.synchronize()
    _check_lines(name, d_sizes.cpu().numpy().view(np.uint16), d_sel.cpu().numpy(), want_sizes, want_sel)
    _check_totals(ev, case, fixture)
    ev.close()


def test_cli_csv_is_the_reference_text(fixture, traces, tmp_path):
    """`compressor -a BDI|FPC|BPC -i <dir>/<name>.npy`: the *_results.csv the command line writes is the text the
    reference's Result::Print wrote for the same lines (all rows but the last), byte for byte."""
    pkg("build").build_all()
    cli = os.path.join(ROOT, "bin", "compressor")
    meta = fixture[0]
    assert len(meta["print"]) == 6
    for rec in meta["print"]:
        case = next(c for c in meta["cases"] if c["name"] == rec["case"])
        out = tmp_path / rec["case"]
        npy = out / rec["npy"]
        npy.parent.mkdir(parents=True)
        traces.save_npy(str(npy), baseline_ref.case_input(case))
        r = subprocess.run([cli, "-a", rec["comp"], "-i", str(npy), "-o", str(out)], cwd=os.path.join(ROOT, "bin"),
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        assert (out / f"{rec['comp']}_results.csv").read_text() == rec["text"], rec["case"]
