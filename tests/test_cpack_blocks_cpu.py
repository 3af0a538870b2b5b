"""C-Pack with a dictionary shared by blocks of N lines, without a device: the block restatement
(tests/cpack_blocks_ref.py) against the reference's own numbers -- the new fixture (a fresh reference comp::CPACK every N
lines) and both ends in tests/golden/ref_cpack_vectors.npz (N = 1: a fresh object per line; N beyond the trace: one object
over all of it) --, that the natural-order inputs tell the three behaviours apart, the new symbols and their refusals
before a device is touched, the kernel in the gfx950 code object, shard_range's alignment and comp::CPACK's new
constructor (a native probe with its own main, built with the address and undefined-behaviour sanitizers)."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, pkg

import cpack_blocks_ref as B
import cpack_ref
from test_group_cpu import _gfx950_code_objects

HOST = os.path.join(ROOT, "cal_22-mpc_amd", "host")
NAMES = [c["name"] for c in B.CASES]
ORDERED = [c["name"] for c in B.ORDERED]
SHUFFLED = [c["name"] for c in B.SHUFFLED]


@pytest.fixture(scope="module")
def mpc():
    m = pkg()
    m.lib()
    return m


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return B.load_fixture(os.path.join(golden_dir, "ref_cpack_block_vectors.npz"))


@pytest.fixture(scope="module")
def ends(golden_dir):
    return cpack_ref.load_fixture(os.path.join(golden_dir, "ref_cpack_vectors.npz"))


@pytest.fixture(scope="module")
def inputs(fixture):
    return {c["name"]: B.case_input(c) for c in fixture[0]["cases"]}


def _case(fixture, name):
    return next(c for c in fixture[0]["cases"] if c["name"] == name)


def test_fixture_covers_the_issue_cases(fixture):
    meta, z = fixture
    assert [{k: c[k] for k in ("name", "L", "seed")} for c in meta["cases"]] == B.CASES
    assert sorted({c["L"] for c in meta["cases"]}) == [4, 32, 36, 64, 128, 256] and len(meta["cases"]) == 12
    assert meta["blocks"] == [2, 3, 4, 16, 64, 1000] == B.BLOCKS
    for c in meta["cases"]:
        for N in B.BLOCKS:
            sizes, st, ratio = (z[f"{c['name']}.N{N}.{k}"] for k in ("sizes", "stats", "ratio"))
            assert sizes.dtype == np.uint16 and sizes.shape == (c["n"],) and c["n"] >= B.MIN_LINES
            assert st.dtype == np.uint64 and st.shape == (9,) and ratio.dtype == np.float64
            assert int(st[0]) == 8 * c["L"] * c["n"] and int(st[1]) == int(sizes.astype(np.uint64).sum())
            assert int(st[2]) == c["n"] * (c["L"] // 4) == int(st[3:].sum())
            assert int(st[1]) == int(st[3:].astype(np.int64) @ np.array(cpack_ref.BITS))
    golden = os.path.dirname(os.path.abspath(os.path.join(ROOT, "tests", "golden", "ref_cpack_block_vectors.npz")))
    mine = os.path.getsize(os.path.join(golden, "ref_cpack_block_vectors.npz"))
    assert mine <= max(os.path.getsize(os.path.join(golden, f)) for f in os.listdir(golden) if f != "ref_cpack_block_vectors.npz")
    # the issue's own example
    assert [int(z[f"cpack_L64.N{N}.stats"][1]) for N in (2, 4, 64, 1000)] == [704694, 703412, 702068, 701842]


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_the_reference_for_every_block_length(fixture, inputs, name):
    meta, z = fixture
    c, lines = _case(fixture, name), inputs[name]
    for N in B.BLOCKS:
        sizes, counts = B.compress_blocks(lines, N)
        assert (sizes == z[f"{name}.N{N}.sizes"]).all(), N
        v, st = cpack_ref.stats_vector(c["L"], sizes, counts), z[f"{name}.N{N}.stats"]
        assert int(v[0]) == c["n"] and (v[1:4] == st[:3]).all() and (v[4:] == st[3:]).all(), N
        assert cpack_ref.comp_ratio(c["L"], sizes) == float(z[f"{name}.N{N}.ratio"][0]), N           # the same double


@pytest.mark.parametrize("name", SHUFFLED)
def test_restatement_ends_are_the_per_line_and_the_carried_dictionary(ends, inputs, name):
    """N = 1 is the reference's fresh object per line, N = n and N = 2^32 - 1 its one object over the whole case; the
    numbers in between are neither."""
    meta, z = ends
    lines = inputs[name]
    L, n = lines.shape[1], len(lines)
    sizes, counts = B.compress_blocks(lines, 1)
    assert (sizes == z[name + ".sizes"]).all() and (counts == z[name + ".counts"]).all()
    for N in (n, 2 ** 32 - 1):
        sizes, counts = B.compress_blocks(lines, N)
        assert (sizes == z[name + ".carried"]).all(), N
        v, st = cpack_ref.stats_vector(L, sizes, counts), z[name + ".carried_stats"]
        assert (v[1:4] == st[:3]).all() and (v[4:] == st[3:]).all(), N


@pytest.mark.parametrize("name", SHUFFLED)
def test_block_lengths_in_between_differ_from_both_ends(fixture, ends, name):
    """(Not N = 1000: after the first 1000 of some 1800 shuffled lines the fresh dictionary may cost no line a bit.)"""
    for N in B.BLOCKS[:-1]:
        s = fixture[1][f"{name}.N{N}.sizes"]
        assert (s != ends[1][name + ".sizes"]).any() and (s != ends[1][name + ".carried"]).any(), N


@pytest.mark.parametrize("name", ORDERED)
def test_natural_order_inputs_separate_the_three_behaviours(fixture, inputs, name):
    """A property of the inputs: at N = 4 and N = 64 the sizes differ from the per-line and from the carried sizes."""
    lines = inputs[name]
    per, car = cpack_ref.compress(lines, "line")[0], cpack_ref.compress(lines, "carried")[0]
    for N in (4, 64):
        s = fixture[1][f"{name}.N{N}.sizes"]
        assert (s != per).any() and (s != car).any(), N
        assert (s != fixture[1][f"{name}.N{2 if N == 4 else 16}.sizes"]).any(), N


@pytest.mark.parametrize("name", ORDERED)
def test_hand_built_runs_cross_line_boundaries_with_the_outcomes_the_issue_names(inputs, name):
    """Each run alone, from a fresh dictionary, with the whole run in one block: the outcomes per word."""
    L = inputs[name].shape[1]
    W = L // 4
    outcome = lambda run: B.compress_blocks(B._lay(run, W).astype("<u4").view(np.uint8).reshape(-1, L), 10 ** 6)[1].astype(int).sum(axis=0).tolist()[2:]      # noqa: E731
    for rep in range(4):
        runs = B.hand_runs(L, rep)
        assert all(len(B._lay(r, W)) >= 2 for r in runs)                   # pushed in one line, met again in a later one
        assert outcome(runs[0]) == [1, 1, 1, 1]                            # MMMM, MMMX, MMXX against the entry of the line before
        assert outcome(runs[1]) == [1, 0, 0, 16]                           # 15 other misses between: a hit
        assert outcome(runs[2]) == [0, 0, 0, 18]                           # 16: evicted
        assert outcome(runs[3]) == [1, 0, 0, 18]                           # a hit does not refresh
        assert outcome(runs[4]) == [1, 1, 0, 18]                           # pushed again: the later entry decides (MMMM, then MMMX against it)
        k0 = B.key0_run(rep)
        seq = np.array(k0 + [0] * (-len(k0) % W), dtype="<u4").view(np.uint8).reshape(-1, L)
        assert B.compress_blocks(seq, 10 ** 6)[1].astype(int).sum(axis=0).tolist()[2:] == [1, 1, 2, 17]
    starts = B.key0_run_starts(next(c for c in B.ORDERED if c["name"] == name))
    assert len(starts) == 4 and all(s % 64 == 0 for s in starts)          # the 16th miss OF THE BLOCK for N = 2, 4, 16, 64


def test_restatement_continues_an_open_block():
    lines = B.case_lines(B.ORDERED[1])[:700]
    for N in (3, 64, 1000):
        whole = B.compress_blocks(lines, N)
        fifo, at, parts = [0] * 16, 0, []
        for n in (1, 63, 64, 65, 300, 207):
            parts.append(B.compress_blocks(lines[at:at + n], N, first_line=at, fifo=fifo))
            at += n
        assert at == 700 and (np.concatenate([p[0] for p in parts]) == whole[0]).all() and (np.concatenate([p[1] for p in parts]) == whole[1]).all()


def test_the_generator_reproduces_the_fixture_where_the_reference_is():
    ref = os.environ.get("REF", "/root/reference")             # (as oracle/Makefile)
    if not os.path.isfile(os.path.join(ref, "src", "compressor", "CPACK.cpp")):
        pytest.skip("the reference sources are not here")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "make_ref_cpack_block_vectors.py"), "--check"],
                       capture_output=True, text=True, timeout=600, env=dict(os.environ, REF=ref))
    assert r.returncode == 0 and "no difference" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


# ---- the interface ---------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_bound(mpc):
    with open(os.path.join(ROOT, "include", "mpc_hip.h")) as f:
        hdr = f.read()
    assert re.search(r"\bint mpc_create_cpack_blocks\s*\(unsigned line_size, uint64_t block_lines, int device, mpc_handle \*\*out\);", hdr)
    assert re.search(r"\bint mpc_cpack_blocks_restart\s*\(mpc_handle \*h\);", hdr)
    assert re.search(r"\bint mpc_cpack_block_lines\s*\(const mpc_handle \*h, uint64_t \*n\);", hdr)
    raw = C.CDLL(mpc.LIB_PATH)
    for name in ("mpc_create_cpack_blocks", "mpc_cpack_blocks_restart", "mpc_cpack_block_lines"):
        assert name in mpc.EXPORTED_SYMBOLS and hasattr(raw, name) and getattr(mpc.lib(), name).argtypes is not None, name
    assert re.search(r"#define MPC_PATH_CPACK_BLOCKS\s+10\b", hdr) and mpc.MPC_PATH_CPACK_BLOCKS == 10
    assert re.search(r"#define MPC_ABI_VERSION\s+1\b", hdr)
    with open(os.path.join(ROOT, "cal_22-mpc_amd", "csrc", "mpc_device.h")) as f:
        assert re.search(r"#define MPC_CPACK_RAW_LEN\s+7\b", f.read())
    # what the header has to say about the blocks
    text = " ".join(hdr.split())
    for words in ("depends on where blocks begin", "must start at multiples of N", "one lane's sequential work", "`-a CPACK` run", "exact and slow"):
        assert words in text, words
    with open(os.path.join(ROOT, "cal_22-mpc_amd", "csrc", "mpc_launch.h")) as f:
        assert "mpc_launch_cpack_blocks" in f.read()
    units = [os.path.basename(u[0]) for u in pkg("build").lib_units()]
    assert "mpc_cpack_blocks.hip" in units and "mpc_cpack.hip" in units


@pytest.mark.parametrize("L,N,words", [(64, 0, ("block_lines 0", "4294967295")), (64, 2 ** 32, ("block_lines 4294967296", "4294967295")),
                                       (0, 4, ("multiple of 4",)), (6, 4, ("multiple of 4",)), (260, 4, ("multiple of 4", "256")),
                                       (6, 0, ("multiple of 4",))])
def test_create_refuses_before_touching_a_device(mpc, L, N, words):
    h = C.c_void_p()
    env_before = dict(os.environ)
    rc = mpc.lib().mpc_create_cpack_blocks(L, N, 10 ** 6, C.byref(h))      # (a device ordinal no machine has: it is never looked at)
    assert rc == -22 and not h
    msg = mpc.lib().mpc_last_error(None).decode()
    assert msg.startswith("C-Pack") and all(w in msg for w in words), msg
    assert dict(os.environ) == env_before


def test_python_binding_refusals_need_no_device(mpc):
    with pytest.raises(ValueError, match="block_lines"):
        mpc.CPACK(64, dictionary="block", device=10 ** 6)
    with pytest.raises(ValueError, match="block_lines"):
        mpc.CPACK(64, dictionary="line", device=10 ** 6, block_lines=4)
    with pytest.raises(ValueError, match="block_lines"):
        mpc.CPACK(64, device=10 ** 6, block_lines=4)
    with pytest.raises(TypeError):
        mpc.CPACK(64, "block", 10 ** 6, 4)                                 # block_lines is keyword-only
    for N, L in ((0, 64), (2 ** 32, 64), (4, 6), (4, 0), (4, 260)):
        with pytest.raises(mpc.MpcError) as e:
            mpc.CPACK(L, dictionary="block", block_lines=N, device=10 ** 6)
        assert e.value.code == -22 and "C-Pack" in str(e.value)
    # the per-line refusals are what they were
    for d in ("carried", "global", "", 0, 2):
        with pytest.raises(mpc.MpcError) as e:
            mpc.CPACK(64, dictionary=d)
        assert e.value.code == -22 and "C-Pack" in str(e.value)
    assert isinstance(mpc.CPACK.block_lines, property) and callable(mpc.CPACK.restart)


def test_restart_and_block_lines_refuse_other_handles(mpc):
    n = C.c_uint64(7)
    assert mpc.lib().mpc_cpack_blocks_restart(None) == -22 and mpc.lib().mpc_cpack_block_lines(None, C.byref(n)) == -22 and n.value == 7


def test_kernel_in_the_code_object(tmp_path):
    """cpack_block_kernel is in the library's gfx950 code object, beside the four per-line kernels; no scratch, no spills,
    64 lanes a workgroup and the 16-word rings of its 64 lanes in LDS."""
    build = pkg("build")
    lib_path = build.build_lib()
    readelf = shutil.which("llvm-readelf") or os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(build.HIPCC))), "llvm", "bin", "llvm-readelf")
    if not os.path.exists(readelf):
        readelf = "/opt/rocm/llvm/bin/llvm-readelf"
    assert os.path.exists(readelf), "llvm-readelf (ROCm's LLVM tools) not found"
    found, per_line = [], 0
    for i, obj in enumerate(_gfx950_code_objects(lib_path)):
        path = tmp_path / f"co{i}.elf"
        path.write_bytes(obj)
        notes = subprocess.run([readelf, "--notes", str(path)], capture_output=True, text=True, check=True).stdout
        for block in notes.split("- .agpr_count:")[1:]:
            name = re.search(r"\.name:\s+(\S+)", block).group(1)
            per_line += bool(re.match(r"_Z12cpack_kernelILi(\d+)E", name) or name.startswith("_Z16cpack_any_kernel"))
            if name.startswith("_Z18cpack_block_kernel"):
                found.append({k: int(re.search(rf"\.{k}:\s+(\d+)", block).group(1))
                              for k in ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count", "max_flat_workgroup_size",
                                        "group_segment_fixed_size", "vgpr_count")})
    assert len(found) == 1 and per_line == 4, (found, per_line)
    k = found[0]
    assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k
    assert k["max_flat_workgroup_size"] == 64 and 16 * 64 * 4 <= k["group_segment_fixed_size"] <= 16 * 64 * 4 + 64, k
    assert k["vgpr_count"] <= 128, k          # 8 waves per SIMD stay possible


@pytest.mark.parametrize("n,world,align", [(0, 4, 4), (1, 4, 4), (1000, 8, 64), (1001, 8, 64), (123457, 8, 1000), (64, 8, 64), (63, 3, 64),
                                           (10 ** 6, 7, 96), (1000, 1, 3)])
def test_shard_range_with_align(n, world, align):
    sharded = pkg("sharded")
    cuts = [sharded.shard_range(n, r, world, align=align) for r in range(world)]
    assert cuts[0][0] == 0 and cuts[-1][1] == n
    assert all(cuts[r][1] == cuts[r + 1][0] for r in range(world - 1))                     # every line exactly once
    assert all(b % align == 0 and b <= e for b, e in cuts)
    assert all(abs(b - (r * n) // world) < align for r, (b, e) in enumerate(cuts))         # rounded down to a multiple, no further
    # the default is what it was
    assert [sharded.shard_range(n, r, world) for r in range(world)] == [((r * n) // world, ((r + 1) * n) // world) for r in range(world)]
    assert [sharded.shard_range(n, r, world, 1) for r in range(world)] == [sharded.shard_range(n, r, world) for r in range(world)]


def test_shard_range_refuses_a_zero_alignment():
    with pytest.raises(ValueError):
        pkg("sharded").shard_range(10, 0, 2, align=0)


# ---- the host class (a stand-alone program under the sanitizers) -----------------------------------------------------------
@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    build = pkg("build")
    build.build_lib()
    out = str(tmp_path_factory.mktemp("cpack_blocks_probe") / "cpack_blocks_probe")
    srcs = [os.path.join(ROOT, "tests", "native", "cpack_blocks_probe.cpp")] + [os.path.join(HOST, f) for f in sorted(os.listdir(HOST)) if f.endswith(".cpp") and f != "main.cpp"]
    pkg_dir = os.path.dirname(build.LIB)
    # host code only: the host compiler, as the other native probes of the suite are built
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "include"), "-I", HOST, *srcs, "-L", pkg_dir, "-lmpc_hip",
                    f"-Wl,-rpath,{pkg_dir}", "-o", out], check=True, capture_output=True, text=True)
    return out


def _run_probe(probe, *args, ok=0):
    # (the library's HIP runtime is loaded, never initialised: what it allocates while loading is not this program's leak)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    r = subprocess.run([probe, *[str(a) for a in args]], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == ok and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stdout + r.stderr
    return r.stdout


def test_host_class_refusals(probe):
    """comp::CPACK(lineSize, scope, blockLines): only PerBlock, and the library's limits; a message and exit(1), no device."""
    out = _run_probe(probe, "refuse", 2, 64, 0, ok=1)
    assert out.startswith("CPACK: cannot create the evaluator (-22): C-Pack: block_lines 0") and "4294967295" in out
    out = _run_probe(probe, "refuse", 2, 64, 2 ** 32, ok=1)
    assert out.startswith("CPACK: cannot create the evaluator (-22): C-Pack: block_lines 4294967296")
    out = _run_probe(probe, "refuse", 2, 6, 4, ok=1)
    assert out.startswith("CPACK: cannot create the evaluator (-22): C-Pack") and "multiple of 4" in out
    for scope in (0, 1):
        out = _run_probe(probe, "refuse", scope, 64, 4, ok=1)
        assert out.startswith("CPACK: cannot create the evaluator (-22): C-Pack:") and "PerBlock" in out
    with open(os.path.join(HOST, "CPACK.h")) as f:
        h = f.read()
    assert re.search(r"CPACK\(unsigned lineSize, CPACKDictionary scope\);", h)                   # the declaration that was there
    assert re.search(r"CPACK\(unsigned lineSize, CPACKDictionary scope, uint64_t blockLines\);", h) and "void Restart();" in h
    assert re.search(r"PerLine = 1, PerBlock = 2", h)


def test_cpack_result_prints_a_block_run_like_any_other(probe, fixture, tmp_path):
    """CPACKResult and its Print are unchanged: the reference's header and a row of the block totals."""
    meta, z = fixture
    st = z["cpack_order_L64.N4.stats"]
    n = _case(fixture, "cpack_order_L64")["n"]
    v = [n] + [int(x) for x in st]
    csv = tmp_path / "blocks.csv"
    out = _run_probe(probe, "print", 64, "blocks_N4", csv, *v)
    ratio = float.fromhex(out.split()[3])
    assert out.split()[:3] == ["result", str(v[1]), str(v[2])] and ratio == float(z["cpack_order_L64.N4.ratio"][0]) and out.split()[4] == str(v[3])
    text = csv.read_text().split("\n")
    assert text[0] + "\n" == cpack_ref.HEADER and text[1].startswith(f"blocks_N4,{v[1]},{v[2]},") and text[1].endswith("," + "".join(f"{x}," for x in v[3:]))
