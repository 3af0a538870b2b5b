"""Groups of evaluators (mpc_group, `compressor -a A,B,...`): what can be checked without a device -- the command
line's handling of a list of algorithms, the exported entry points, and the shared BDI/FPC/BPC kernels in the gfx950
code object of the built library (present for 32-, 64- and 128-byte lines, no scratch memory)."""
import ctypes as C
import os
import re
import shutil
import struct
import subprocess

import pytest

from conftest import ROOT, pkg

BIN = os.path.join(ROOT, "bin")


@pytest.fixture(scope="module")
def cli():
    pkg("build").build_all()
    return os.path.join(BIN, "compressor")


@pytest.fixture()
def trace(traces, tmp_path):
    d = tmp_path / "ds"
    d.mkdir()
    return traces.save_npy(str(d / "t.npy"), traces.zeros(8, 64))


def run(cmd):
    return subprocess.run(cmd, cwd=BIN, capture_output=True, text=True, timeout=600)


def test_list_of_algorithms_is_accepted(cli, trace, tmp_path):
    """`-a BDI,FPC` is a list, not an invalid name: without a device the run is refused the way a single name is
    (exit status 1, "no CPU fallback"); with one it evaluates both and prints one ratio line per name."""
    import torch
    out = tmp_path / "out"
    out.mkdir()
    r = run([cli, "-a", "BDI,FPC", "-i", trace, "-o", str(out)])
    assert "Invalid name of algorithm" not in r.stderr
    if not torch.cuda.is_available():
        assert r.returncode == 1 and "no CPU fallback" in r.stdout, r.stdout + r.stderr
        assert os.listdir(out) == []
    else:
        assert r.returncode == 0, r.stdout + r.stderr
        assert [ln.split(":")[0] for ln in r.stdout.strip().split("\n")] == ["BDI comp.ratio", "FPC comp.ratio"]


@pytest.mark.parametrize("args,text", [
    (["-a", "BDI,CPACK"], "Algorithm CPACK is not part of this build"),
    (["-a", "SC2,BDI"], "Algorithm SC2 is not part of this build"),
    (["-a", "BDI,LZ4"], 'Invalid name of algorithm in the list "BDI,LZ4": "LZ4"'),
    (["-a", "BDI,FPC,BDI"], "Algorithm BDI is named twice"),
    (["-a", "BDI,,FPC"], 'Invalid name of algorithm in the list "BDI,,FPC": ""'),
    (["-a", "BDI,"], 'Invalid name of algorithm in the list "BDI,": ""'),
    (["-a", "BDI,FPC", "--per-line"], "--per-line / --line-buffer evaluate one algorithm"),
    (["-a", "BDI,FPC", "--line-buffer", "64"], "--per-line / --line-buffer evaluate one algorithm"),
])
def test_refused_lists_write_nothing(cli, trace, tmp_path, args, text):
    out = tmp_path / "out"
    out.mkdir()
    r = run([cli, *args, "-i", trace, "-o", str(out)])
    assert r.returncode == 1 and text in r.stdout, r.stdout + r.stderr
    assert os.listdir(out) == []


def test_single_names_keep_their_text(cli, trace, tmp_path):
    """A single name goes the way it always went: the refusal of the four algorithms outside this build, and the abort on
    an unknown name."""
    r = run([cli, "-a", "CPACK", "-i", trace, "-o", str(tmp_path)])
    assert r.returncode == 1 and r.stdout.startswith("Algorithm CPACK is not part of this build: VPC, BDI, FPC and BPC are")
    assert "A list (VPC,BDI,FPC,BPC) is evaluated in one pass." in run([cli, "-h"]).stdout


GROUP_SYMBOLS = ["mpc_group_create", "mpc_group_destroy", "mpc_group_last_error", "mpc_group_form", "mpc_group_compress_batch",
                 "mpc_group_compress_batch_device", "mpc_group_compress_npy", "mpc_group_compress_gpgpusim_log", "mpc_group_sync"]


def test_group_entry_points_declared_exported_and_bound():
    mpc = pkg()
    pkg("build").build_lib()
    with open(os.path.join(ROOT, "include", "mpc_hip.h")) as f:
        hdr = f.read()
    declared = set(re.findall(r"\b(mpc_group_[a-z_]+)\s*\(", hdr))
    assert declared == set(GROUP_SYMBOLS)
    lib = C.CDLL(mpc.LIB_PATH)
    for name in GROUP_SYMBOLS:
        assert hasattr(lib, name) and name in mpc.EXPORTED_SYMBOLS, name
    assert hasattr(mpc, "EvaluatorSet")


def test_group_create_rejects_bad_sets_without_a_device():
    """The argument checks come before any HIP call."""
    mpc = pkg()
    pkg("build").build_lib()
    L = mpc.lib()
    g = C.c_void_p()
    assert L.mpc_group_create(None, 0, C.byref(g)) == -22 and not g
    assert b"at least one member" in L.mpc_group_last_error(None)
    arr = (C.c_void_p * 2)(None, None)
    assert L.mpc_group_create(arr, 2, C.byref(g)) == -22 and not g
    assert b"member 0 is NULL" in L.mpc_group_last_error(None)
    with pytest.raises(mpc.MpcError) as e:
        mpc.EvaluatorSet([])
    assert e.value.code == -22


def test_a_set_is_destroyed_before_its_members_whoever_goes_first(monkeypatch):
    """mpc_group_destroy reads the group's members, so the binding destroys a set before any of its members: when the
    members are closed while a set that was never closed is still alive (held by the traceback of an exception one of
    its methods raised, say), and when the garbage collector finalizes a forgotten set and its members in an order of
    its own.  The library is a stand-in that records the order of the destroy calls."""
    import gc
    mpc = pkg()
    alive, groups, order, wrong = set(), {}, [], []

    class Lib:
        def mpc_group_create(self, arr, n, out):
            out._obj.value = 1000 + len(order) + len(groups)
            groups[out._obj.value] = [arr[i] for i in range(n)]
            return 0

        def mpc_group_destroy(self, g):
            wrong.extend(h for h in groups.pop(g.value) if h not in alive)
            order.append("set")

        def mpc_destroy(self, h):
            alive.discard(h.value)
            order.append("member")

    monkeypatch.setattr(mpc, "lib", lambda: Lib())

    def members():
        out = []
        for k in (len(alive) + 1, len(alive) + 2):
            e = object.__new__(mpc.BDI)
            e._h, e.line_size = C.c_void_p(k), 64
            alive.add(k)
            out.append(e)
        return out

    # closed in the right order: nothing is left behind
    m = members()
    s = mpc.EvaluatorSet(m)
    s.close()
    assert all(e._sets == [] for e in m)
    for e in m:
        e.close()
    assert order == ["set", "member", "member"] and not wrong and not alive and not groups
    # a set that is never closed and stays alive in a cycle, the members closed by hand
    del order[:]
    m = members()
    s = mpc.EvaluatorSet(m)
    s.cycle = s
    del s
    m[1].close()
    assert order == ["set", "member"] and not m[0]._sets
    m[0].close()
    gc.collect()
    assert order == ["set", "member", "member"] and not wrong and not alive and not groups
    # two sets over the same members, everything forgotten: the collector's order
    del order[:]
    m = members()
    s, t = mpc.EvaluatorSet(m), mpc.EvaluatorSet(m[:1])
    s.cycle = s
    del s, t, m, e
    gc.collect()
    assert sorted(order) == ["member", "member", "set", "set"] and not wrong and not alive and not groups


def _gfx950_code_objects(lib_path):
    """The gfx950 entries of the clang offload bundles in the library's .hip_fatbin section."""
    with open(lib_path, "rb") as f:
        blob = f.read()
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    pos = 0
    while True:
        at = blob.find(magic, pos)
        if at < 0:
            return
        n, = struct.unpack_from("<Q", blob, at + len(magic))
        p = at + len(magic) + 8
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", blob, p)
            p += 24
            triple = blob[p:p + tlen].decode()
            p += tlen
            if "gfx950" in triple and size:
                yield blob[at + off:at + off + size]
        pos = at + len(magic)


def test_shared_baseline_kernels_in_the_code_object(tmp_path):
    """baselines_kernel<NW, MASK> for NW = 8, 16, 32 in the library's gfx950 code object, each with 0 bytes of scratch and
    no spilled VGPR at 256 threads per workgroup.  Not asserted, because it does not hold: the instantiations with BDI
    as a member spill SGPRs to VGPR lanes (no memory involved), 2 ... 54 of them (<16, 7>: 54, <32, 7>: 44), as
    bdi_kernel itself does (8 at 64 bytes, 39 at 128); the listing is profiles/group_kernel_resource_usage.txt."""
    build = pkg("build")
    lib_path = build.build_lib()
    readelf = shutil.which("llvm-readelf") or os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(build.HIPCC))), "llvm", "bin", "llvm-readelf")
    if not os.path.exists(readelf):
        readelf = "/opt/rocm/llvm/bin/llvm-readelf"
    assert os.path.exists(readelf), "llvm-readelf (ROCm's LLVM tools) not found"
    kernels = {}
    for i, obj in enumerate(_gfx950_code_objects(lib_path)):
        path = tmp_path / f"co{i}.elf"
        path.write_bytes(obj)
        notes = subprocess.run([readelf, "--notes", str(path)], capture_output=True, text=True, check=True).stdout
        # one metadata map per kernel: .name ... .private_segment_fixed_size ... .sgpr_spill_count ... .vgpr_spill_count
        for block in notes.split("- .agpr_count:")[1:]:
            name = re.search(r"\.name:\s+(\S+)", block).group(1)
            m = re.match(r"_Z16baselines_kernelILi(\d+)ELi(\d+)E", name)
            if m:
                kernels[(int(m.group(1)), int(m.group(2)))] = {
                    k: int(re.search(rf"\.{k}:\s+(\d+)", block).group(1))
                    for k in ("private_segment_fixed_size", "vgpr_spill_count", "max_flat_workgroup_size", "group_segment_fixed_size")}
    # words per line 8, 16, 32 x members (bit 0 BDI, bit 1 FPC, bit 2 BPC; at least two)
    assert sorted(kernels) == [(nw, mask) for nw in (8, 16, 32) for mask in (3, 5, 6, 7)], sorted(kernels)
    for key, k in kernels.items():
        assert k["private_segment_fixed_size"] == 0, (key, k)      # no scratch
        assert k["vgpr_spill_count"] == 0, (key, k)
        assert k["max_flat_workgroup_size"] == 256, (key, k)
        assert k["group_segment_fixed_size"] <= 64 * 1024, (key, k)
