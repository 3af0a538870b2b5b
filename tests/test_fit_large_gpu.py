"""The two Fit analyses on one device batch of more than 2^32 bytes and more than 2^27 lines, in the product library.

One buffer of 2^32 bytes plus 12 345 lines of 32 bytes (n = 2^27 + 12 345 lines), filled on the device by synth_fill kind
"mixed".  One handle takes it in one call; two more take the two parts of a cut at line 2^26 + 37, and their vectors,
merged, must equal the first handle's: an index or byte offset that wrapped at 2^31 or 2^32 on either side of the cut
would count other lines in one of the three.  Every pair's bins sum to the line count, the diagonal is all zero
residues, and the first 4096 lines fed alone equal tests/fit_ref.py on the same lines from traces.mixed, which pins the
kernels at this size to the definition.  All comparisons are exact.  A case that cannot allocate its buffer fails; none
skips."""
import numpy as np
import pytest

from conftest import pkg

import fit_ref

pytestmark = pytest.mark.gpu

L = 32
N = (1 << 32) // L + 12345
CUT = (1 << 26) + 37


@pytest.fixture(scope="module")
def mpc():
    return pkg()


@pytest.fixture(scope="module")
def buffer(mpc):
    import torch
    assert N * L > 1 << 32 and N > 1 << 27 and CUT * L > 1 << 31 and (CUT * L) % 16 == 0
    try:
        buf = torch.empty(N * L, dtype=torch.uint8, device="cuda:0")
    except RuntimeError as e:
        free, total = torch.cuda.mem_get_info(0)
        pytest.fail(f"cannot allocate the {N * L} byte buffer: {free} of {total} bytes free on the device ({e})")
    mpc.synth_fill(buf.data_ptr(), N, L, "mixed")
    torch.cuda.synchronize()
    yield buf
    del buf
    torch.cuda.empty_cache()


def _same(tag, got, want):
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{tag}: {bad.size} of {got.size} differ, first at {bad[:6].tolist()}: {got[bad[:6]].tolist()} vs {want[bad[:6]].tolist()}"


def _whole_and_parts(make, buffer):
    """-> the whole batch's vector; asserts that the two parts' vectors, merged, equal it."""
    import time
    import torch
    whole, head, tail = make(), make(), make()
    p = buffer.data_ptr()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    whole.compress_device(p, N)
    whole.sync()
    print(f"{type(whole).__name__}: {N} lines of {L} bytes in {1e3 * (time.perf_counter() - t0):.1f} ms")
    head.compress_device(p, CUT)
    tail.compress_device(p + CUT * L, N - CUT)
    v = whole.stats_vector()
    vh, vt = head.stats_vector(), tail.stats_vector()
    assert int(v[0]) == N and int(vh[0]) == CUT and int(vt[0]) == N - CUT and int(v[1]) == 0 and int(v[2]) == 0
    head.stats_merge(vt)
    _same("the parts, merged", head.stats_vector(), v)
    prefix = make()
    prefix.compress_device(p, 4096)
    vp = prefix.stats_vector()
    for e in (whole, head, tail, prefix):
        e.close()
    return v, vp


def test_pairs_past_2_to_32_bytes(mpc, traces, buffer):
    v, vp = _whole_and_parts(lambda: mpc.FitPairs(L), buffer)
    P = v[3:].reshape(L, L, 9)
    assert (P.sum(axis=2) == N).all()
    assert (P[np.arange(L), np.arange(L), 0] == N).all()
    _same("the first 4096 lines", vp, fit_ref.pairs_vector(traces.mixed(4096, L)))


def test_residues_past_2_to_32_bytes(mpc, traces, buffer):
    base = [max(i - 4, 0) for i in range(L)]
    v, vp = _whole_and_parts(lambda: mpc.FitResidues(L, base), buffer)
    V = v[3:].reshape(L, 256)
    assert (V.sum(axis=1) == N).all()
    assert int(V[0, 0]) == N      # byte 0 is its own base
    _same("the first 4096 lines", vp, fit_ref.residues_vector(traces.mixed(4096, L), base))
