"""SC2 on the MI355X on chosen words (tests/sc2_keys.py): probe chains that wrap in the LDS and in the global counting
table, a radix select whose cut falls in every digit, bucket layouts that overflow and retry, word 0 as a miss.  Every
case goes to `mpc.SC2(L, S)` and to sc2_ref.SC2Ref; all sizes, `selected`, the statistics vector and `table()` are compared
for integer equality.  tests/test_sc2_keys_cpu.py shows which path each case reaches and which mistakes it rejects."""
import functools
import math
import time

import numpy as np
import pytest

from conftest import pkg

import sc2_keys
import sc2_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mpc():
    return pkg()


@functools.lru_cache(maxsize=None)
def _expected(name):
    """(sizes, selected, statistics, symbols, lengths) of SC2Ref on a case, computed once."""
    lines, L, S, _ = sc2_keys.build(name)
    ref = sc2_ref.SC2Ref(L, S)
    sizes, sel = ref.feed(lines)
    return sizes, sel, ref.stats_vector().tolist(), ref.table_syms.tolist(), ref.table_lens.tolist()


def _check(name, ev, sizes, sel, want):
    want_sizes, want_sel, stats, syms, lens = want
    bad = np.nonzero(sizes != want_sizes)[0]
    assert len(bad) == 0, (name, bad[:10], sizes[bad[:10]], want_sizes[bad[:10]])
    assert (sel == want_sel).all(), name
    sym, ln = ev.table()
    assert sym.tolist() == syms, (name, len(sym), len(syms), sorted(set(sym.tolist()) ^ set(syms))[:10])
    assert ln.tolist() == lens, name
    assert ev.stats_vector().tolist() == stats, name


SMALL = [n for n in sc2_keys.names() if n not in sc2_keys.LARGE]


@pytest.mark.parametrize("name", SMALL)
def test_compress_lines(mpc, name):
    lines, L, S, _ = sc2_keys.build(name)
    ev = mpc.SC2(L, S, device=0)
    sizes, sel = ev.compress_lines(lines)
    _check(name, ev, sizes, sel, _expected(name))
    ev.close()


@pytest.mark.parametrize("name", sc2_keys.names("a", "b", "d"))
def test_compress_device_in_two_calls_split_inside_the_warm_up(mpc, name):
    import torch
    lines, L, S, _ = sc2_keys.build(name)
    align = 16 // math.gcd(L, 16)                            # a device call starts on a 16-byte boundary
    n, cut = len(lines), max(align, S // 2 // align * align)    # (4-byte lines, S = 1 and 2: line 4, past the warm-up)
    ev = mpc.SC2(L, S, device=0)
    d = torch.from_numpy(np.array(lines)).to("cuda:0")
    ds = torch.zeros(n, dtype=torch.int16, device="cuda:0")
    dk = torch.full((n,), -1, dtype=torch.int8, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    for a, b in ((0, cut), (cut, n)):
        ev.compress_device(d[a:].data_ptr(), b - a, ds[a:].data_ptr(), dk[a:].data_ptr(), stream=stream)
    ev.sync()
    torch.cuda.synchronize()
    _check(name, ev, ds.cpu().numpy().view(np.uint16), dk.cpu().numpy(), _expected(name))
    ev.close()


@pytest.mark.parametrize("name", ["global_chain_knife_edge", "retry_twice"])
def test_member_of_a_set_next_to_bdi(mpc, name):
    lines, L, S, _ = sc2_keys.build(name)
    members = [mpc.BDI(L, device=0), mpc.SC2(L, S, device=0)]
    group = mpc.EvaluatorSet(members)
    outs = group.compress_lines(lines)
    _check(name, members[1], outs[1][0], outs[1][1], _expected(name))
    solo = mpc.BDI(L, device=0)
    s, k = solo.compress_lines(lines)
    assert (outs[0][0] == s).all() and (outs[0][1] == k).all()
    assert (members[0].stats_vector() == solo.stats_vector()).all()
    group.close()
    for e in members + [solo]:
        e.close()


def test_counts_of_2_24_and_2_24_minus_1(mpc):
    """The one large case (about 128 MiB of warm-up lines, a counting table of 2^27 slots): two words whose counts have
    a nonzero top digit (count >> 24) in the first pass of the select.  Runs are cheap everywhere (numpy sorts them
    quickly, a workgroup sends one atomic per run): on an MI355X the test takes 0.1 s, 0.02 s of it in compress_lines."""
    lines, L, S, _ = sc2_keys.build("count_2_24")
    ref = sc2_ref.SC2Ref(L, S)
    want_sizes, want_sel = ref.feed(lines)
    assert int(max(ref.counts.values())) == 1 << 24 and sorted(ref.counts.values())[-2] == (1 << 24) - 1
    ev = mpc.SC2(L, S, device=0)
    t0 = time.perf_counter()
    sizes, sel = ev.compress_lines(lines)
    print(f"count_2_24: {len(lines)} lines of {L} B, compress_lines {time.perf_counter() - t0:.2f} s")
    _check("count_2_24", ev, sizes, sel,
           (want_sizes, want_sel, ref.stats_vector().tolist(), ref.table_syms.tolist(), ref.table_lens.tolist()))
    ev.close()
