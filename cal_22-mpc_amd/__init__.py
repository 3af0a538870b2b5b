"""MI355X-native per-cache-line multi-prediction compression evaluator.

Python is only a thin ctypes binding over the C ABI of ``include/mpc_hip.h``
(``libmpc_hip.so``: hand-written gfx950 kernels + the pinned double-buffered
stager).  There is no Python or CPU evaluation path here: if the native library
is missing or no HIP device is present, construction raises.

The classes mirror the reference's operator interface for this path
(``comp::VPC`` / ``comp::BDI`` behind ``comp::Compressor``; reference
``src/compressor/Compressor.h:18-33``, ``VPC.h:241-283``, ``BDI.h:90-107``):
``compress_lines`` is the batch form of ``CompressLine`` and ``result()`` the
``GetResult()`` statistics.
"""
from __future__ import annotations

import ctypes as C
import json
import os
from typing import Dict, Optional, Tuple

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MPC_HIP_LIB") or os.path.join(HERE, "libmpc_hip.so")   # override: development builds only

MPC_SIZE_BINS = 4096          # bins of a size histogram (include/mpc_hip_sizes.h)
MPC_CLASS_COUNT, MPC_CLASS_ROW = 256, 10      # a class table is uint64[256][10] (include/mpc_hip_classes.h)
MPC_CLASS_TABLE_LEN = MPC_CLASS_COUNT * MPC_CLASS_ROW
MPC_CLASS_BEST = -1           # mpc_group_class_stats_get: the best-of's table
MPC_PACK_MAX_SECTORS = 1024   # a pack table is uint64[8 + 1024] (include/mpc_hip_pack.h)
MPC_PACK_TABLE_LEN = 8 + MPC_PACK_MAX_SECTORS
MPC_PACK_BEST = -1            # mpc_group_pack_stats_get: the table of the per-line minimum
MPC_IMAGE_MAX_SECTORS = 1024  # an image table is uint64[16 + 1024] (include/mpc_hip_image.h)
MPC_IMAGE_TABLE_LEN = 16 + MPC_IMAGE_MAX_SECTORS
MPC_IMAGE_MAX_CAPACITY = 1 << 28
MPC_REWRITE_MAX_CLASSES = 32  # a rewrite table is uint64[144 + 32 * 32] (include/mpc_hip_rewrite.h)
MPC_REWRITE_TABLE_LEN = 144 + MPC_REWRITE_MAX_CLASSES * MPC_REWRITE_MAX_CLASSES
MPC_REWRITE_MAX_CAPACITY = 1 << 28
MPC_SNAPSHOT_MAX_CAPACITY = 1 << 28   # include/mpc_hip_snapshot.h
MPC_SNAPSHOT_TABLE_LEN = 8            # a snapshot's stats and plan vectors
SNAPSHOT_PARTIAL = {"skip": 0, "zero": 1}      # MPC_SNAPSHOT_PARTIAL_*
CLASS_LOG_FIELDS = {None: 0, "kernel": 1, "rw": 2, "mftype": 3}      # MPC_CLASS_LOG_*
MPC_PATH_VPC_FAST, MPC_PATH_VPC_GENERIC, MPC_PATH_BDI, MPC_PATH_FPC, MPC_PATH_BPC, MPC_PATH_SC2, MPC_PATH_PATTERN = 1, 2, 3, 4, 5, 6, 7
MPC_PATH_PATTERN_EVICTING = 9
MPC_PATH_CPACK = 8
MPC_PATH_CPACK_BLOCKS = 10
MPC_PATH_FIT_PAIRS, MPC_PATH_FIT_RESIDUES = 11, 12
MPC_CPACK_DICT_CARRIED, MPC_CPACK_DICT_PER_LINE = 0, 1     # mpc_create_cpack's dictionary_scope
SYNTH_KINDS = {"zeros": 0, "random_u32": 1, "sine_f32": 2, "mixed": 3, "pointers_u64": 4}


class MpcError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"mpc error {code}: {msg}")
        self.code = code


class Info(C.Structure):
    _fields_ = [("abi_version", C.c_int32), ("algorithm", C.c_int32), ("line_size", C.c_int32),
                ("num_modules", C.c_int32), ("num_clusters", C.c_int32), ("hist_bins", C.c_int32),
                ("kernel_path", C.c_int32), ("device", C.c_int32), ("stats_len", C.c_uint64)]


_lib = None


def _share_host_hip_runtime() -> None:
    """One HIP runtime per process.  The PyTorch wheel bundles its own
    libamdhip64.so / libhsa-runtime64.so next to libtorch_hip.so; if libmpc_hip.so
    brought up the system copy (/opt/rocm) as well, the process would hold two HSA
    runtimes, PyTorch could no longer see the GPU, and streams / device pointers
    could not be shared.  Promoting PyTorch's copy to the global symbol scope
    BEFORE libmpc_hip.so is bound (RTLD_NOW) makes every hip* reference of
    libmpc_hip.so resolve to that one runtime.  Without PyTorch (the C++ CLI)
    libmpc_hip.so simply uses the system runtime it is linked against."""
    try:
        import torch  # noqa: F401
        cand = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
        if os.path.exists(cand):
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
    except Exception:
        pass


def lib() -> C.CDLL:
    """Load libmpc_hip.so (in-tree).  Raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is missing: run `python {HERE}/build.py` "
                              "(there is no fallback implementation)")
        _share_host_hip_runtime()
        L = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL | os.RTLD_NOW)
        H = C.c_void_p
        sigs = {
            "mpc_create_vpc": ([C.c_char_p, C.c_int, C.POINTER(H)], C.c_int),
            "mpc_create_vpc_from_string": ([C.c_char_p, C.c_int, C.POINTER(H)], C.c_int),
            "mpc_create_bdi": ([C.c_uint, C.c_int, C.POINTER(H)], C.c_int),
            "mpc_create_fpc": ([C.c_uint, C.c_int, C.POINTER(H)], C.c_int),
            "mpc_create_bpc": ([C.c_uint, C.c_int, C.POINTER(H)], C.c_int),
            "mpc_create_sc2": ([C.c_uint, C.c_uint64, C.c_int, C.POINTER(H)], C.c_int),
            "mpc_sc2_sampling_lines": ([C.c_uint64], C.c_uint64),
            "mpc_sc2_code_lengths": ([C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p], C.c_int),
            "mpc_sc2_table": ([H, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)], C.c_int),
            "mpc_create_pattern": ([C.c_uint, C.c_int, C.POINTER(H)], C.c_int),
            "mpc_create_pattern_evicting": ([C.c_uint, C.c_uint64, C.c_int, C.POINTER(H)], C.c_int),
            "mpc_pattern_distinct_lines": ([H, C.POINTER(C.c_uint64)], C.c_int),
            "mpc_create_cpack": ([C.c_uint, C.c_int, C.c_int, C.POINTER(H)], C.c_int),
            "mpc_create_cpack_blocks": ([C.c_uint, C.c_uint64, C.c_int, C.POINTER(H)], C.c_int),
            "mpc_cpack_blocks_restart": ([H], C.c_int),
            "mpc_cpack_block_lines": ([H, C.POINTER(C.c_uint64)], C.c_int),
            "mpc_create_fit_pairs": ([C.c_uint, C.c_int, C.POINTER(H)], C.c_int),
            "mpc_create_fit_residues": ([C.c_uint, C.c_void_p, C.c_int, C.POINTER(H)], C.c_int),
            "mpc_fit_base_table": ([H, C.c_void_p, C.c_size_t], C.c_int),
            "mpc_destroy": ([H], None),
            "mpc_get_info": ([H, C.POINTER(Info)], C.c_int),
            "mpc_last_error": ([H], C.c_char_p),
            "mpc_path_reason": ([H], C.c_char_p),
            "mpc_kernel_form": ([H], C.c_char_p),
            "mpc_jit_compile_check": ([C.c_char_p, C.c_char_p, C.c_size_t], C.c_longlong),
            "mpc_compress_batch": ([H, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p], C.c_int),
            "mpc_compress_batch_device": ([H, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p], C.c_int),
            "mpc_sync": ([H], C.c_int),
            "mpc_stats_len": ([H, C.POINTER(C.c_uint64)], C.c_int),
            "mpc_stats_get": ([H, C.c_void_p, C.c_size_t], C.c_int),
            "mpc_stats_merge": ([H, C.c_void_p, C.c_size_t], C.c_int),
            "mpc_stats_set": ([H, C.c_void_p, C.c_size_t], C.c_int),
            "mpc_stats_reset": ([H], C.c_int),
            "mpc_stats_raw_len": ([H, C.POINTER(C.c_uint64)], C.c_int),
            "mpc_stats_copy_raw_device": ([H, C.c_void_p, C.c_void_p], C.c_int),
            "mpc_stats_from_raw": ([H, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t], C.c_int),
            "mpc_config_describe": ([C.c_char_p, C.c_char_p, C.c_size_t], C.c_int),
            "mpc_compress_npy": ([H, C.c_char_p, C.c_uint64, C.c_uint64, C.c_int, C.POINTER(C.c_uint64)], C.c_int),
            "mpc_npy_shape": ([C.c_char_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)], C.c_int),
            "mpc_compress_gpgpusim_log": ([H, C.c_char_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)], C.c_int),
            "mpc_gpgpusim_log_line_size": ([C.c_char_p, C.POINTER(C.c_uint32)], C.c_int),
            "mpc_group_create": ([C.POINTER(H), C.c_size_t, C.POINTER(H)], C.c_int),
            "mpc_group_destroy": ([H], None),
            "mpc_group_last_error": ([H], C.c_char_p),
            "mpc_group_form": ([H], C.c_char_p),
            "mpc_group_compress_batch": ([H, C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)], C.c_int),
            "mpc_group_compress_batch_device": ([H, C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_void_p], C.c_int),
            "mpc_group_compress_npy": ([H, C.c_char_p, C.c_uint64, C.c_uint64, C.c_int, C.POINTER(C.c_uint64)], C.c_int),
            "mpc_group_compress_gpgpusim_log": ([H, C.c_char_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)], C.c_int),
            "mpc_group_sync": ([H], C.c_int),
            "mpc_synth_fill": ([C.c_void_p, C.c_uint64, C.c_uint, C.c_int, C.c_uint64, C.c_uint64, C.c_void_p], C.c_int),
            "mpc_read_bandwidth_probe": ([C.c_void_p, C.c_uint64, C.c_void_p], C.c_int),
            "mpc_size_hist_enable": ([H], C.c_int),
            "mpc_size_hist_get": ([H, C.c_void_p, C.c_size_t], C.c_int),
            "mpc_group_best_enable": ([H], C.c_int),
            "mpc_group_best_get": ([H, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)], C.c_int),
            "mpc_group_best_reset": ([H], C.c_int),
            "mpc_size_sectors": ([C.c_void_p, C.c_size_t, C.c_uint, C.c_uint, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint64),
                                  C.POINTER(C.c_double)], C.c_int),
            "mpc_class_stats_enable": ([H, C.c_uint], C.c_int),
            "mpc_class_stats_get": ([H, C.c_void_p, C.c_size_t], C.c_int),
            "mpc_class_stats_merge": ([H, C.c_void_p, C.c_size_t], C.c_int),
            "mpc_class_sector_bytes": ([H, C.POINTER(C.c_uint)], C.c_int),
            "mpc_compress_batch_classed": ([H, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p], C.c_int),
            "mpc_compress_batch_device_classed": ([H, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p], C.c_int),
            "mpc_class_log_field": ([H, C.c_int], C.c_int),
            "mpc_group_class_stats_enable": ([H, C.c_uint], C.c_int),
            "mpc_group_class_stats_get": ([H, C.c_int, C.c_void_p, C.c_size_t], C.c_int),
            "mpc_group_compress_batch_classed": ([H, C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)], C.c_int),
            "mpc_group_compress_batch_device_classed": ([H, C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                                         C.c_void_p], C.c_int),
            "mpc_group_class_log_field": ([H, C.c_int], C.c_int),
            "mpc_group_class_from_member": ([H, C.c_int], C.c_int),
            "mpc_pack_stats_enable": ([H, C.c_uint64, C.c_uint, C.c_uint], C.c_int),
            "mpc_pack_check_values": ([C.c_uint, C.c_uint64, C.c_uint, C.c_uint], C.c_int),
            "mpc_pack_stats_get": ([H, C.c_void_p, C.c_size_t], C.c_int),
            "mpc_pack_stats_merge": ([H, C.c_void_p, C.c_size_t], C.c_int),
            "mpc_pack_sectors_of_tail": ([C.c_void_p, C.c_size_t, C.c_uint, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)], C.c_int),
            "mpc_group_pack_stats_enable": ([H, C.c_uint64, C.c_uint, C.c_uint], C.c_int),
            "mpc_group_pack_stats_get": ([H, C.c_int, C.c_void_p, C.c_size_t], C.c_int),
            "mpc_image_stats_enable": ([H, C.c_uint64, C.c_uint64, C.c_uint, C.c_uint], C.c_int),
            "mpc_image_check_values": ([C.c_uint, C.c_uint64, C.c_uint64, C.c_uint, C.c_uint], C.c_int),
            "mpc_image_stats_get": ([H, C.c_void_p, C.c_size_t], C.c_int),
            "mpc_compress_batch_addressed": ([H, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p], C.c_int),
            "mpc_compress_batch_device_addressed": ([H, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p], C.c_int),
            "mpc_image_hash": ([C.c_uint64], C.c_uint64),
            "mpc_group_image_stats_enable": ([H, C.c_uint64, C.c_uint64, C.c_uint, C.c_uint], C.c_int),
            "mpc_group_image_stats_get": ([H, C.c_int, C.c_void_p, C.c_size_t], C.c_int),
            "mpc_group_compress_batch_addressed": ([H, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p], C.c_int),
            "mpc_group_compress_batch_device_addressed": ([H, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p], C.c_int),
            "mpc_rewrite_stats_enable": ([H, C.c_uint64, C.c_uint], C.c_int),
            "mpc_rewrite_check_values": ([C.c_uint, C.c_uint64, C.c_uint], C.c_int),
            "mpc_rewrite_stats_get": ([H, C.c_void_p, C.c_size_t], C.c_int),
            "mpc_group_rewrite_stats_enable": ([H, C.c_uint64, C.c_uint], C.c_int),
            "mpc_group_rewrite_stats_get": ([H, C.c_int, C.c_void_p, C.c_size_t], C.c_int),
            "mpc_snapshot_check_values": ([C.c_uint, C.c_uint64, C.c_uint], C.c_int),
            "mpc_snapshot_create": ([C.c_uint, C.c_uint64, C.c_int, C.POINTER(H)], C.c_int),
            "mpc_snapshot_destroy": ([H], None),
            "mpc_snapshot_reset": ([H], C.c_int),
            "mpc_snapshot_last_error": ([H], C.c_char_p),
            "mpc_snapshot_add": ([H, C.c_void_p, C.c_uint64, C.c_void_p], C.c_int),
            "mpc_snapshot_add_device": ([H, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p], C.c_int),
            "mpc_snapshot_add_gpgpusim_log": ([H, C.c_char_p, C.POINTER(C.c_uint64)], C.c_int),
            "mpc_snapshot_stats": ([H, C.c_void_p], C.c_int),
            "mpc_snapshot_plan": ([H, C.c_uint, C.c_int, C.c_void_p], C.c_int),
            "mpc_snapshot_write_lines": ([H, C.c_uint, C.c_int, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p], C.c_int),
            "mpc_snapshot_read_lines": ([H, C.c_uint, C.c_int, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p], C.c_int),
            "mpc_snapshot_evaluate": ([H, H, C.c_uint, C.c_int, C.c_int], C.c_int),
            "mpc_snapshot_evaluate_group": ([H, H, C.c_uint, C.c_int, C.c_int], C.c_int),
        }
        for name, (args, res) in sigs.items():
            fn = getattr(L, name)
            fn.argtypes = args
            fn.restype = res
        _lib = L
    return _lib


EXPORTED_SYMBOLS = [
    "mpc_create_vpc", "mpc_create_vpc_from_string", "mpc_create_bdi", "mpc_create_fpc", "mpc_create_bpc", "mpc_destroy", "mpc_get_info",
    "mpc_last_error", "mpc_path_reason", "mpc_kernel_form", "mpc_jit_compile_check", "mpc_compress_batch", "mpc_compress_batch_device", "mpc_sync", "mpc_stats_len",
    "mpc_stats_get", "mpc_stats_merge", "mpc_stats_set", "mpc_stats_reset", "mpc_stats_raw_len",
    "mpc_stats_copy_raw_device", "mpc_stats_from_raw", "mpc_config_describe",
    "mpc_compress_npy", "mpc_npy_shape", "mpc_compress_gpgpusim_log", "mpc_gpgpusim_log_line_size",
    "mpc_synth_fill", "mpc_read_bandwidth_probe",
    "mpc_group_create", "mpc_group_destroy", "mpc_group_last_error", "mpc_group_form", "mpc_group_compress_batch",
    "mpc_group_compress_batch_device", "mpc_group_compress_npy", "mpc_group_compress_gpgpusim_log", "mpc_group_sync",
    "mpc_create_pattern", "mpc_pattern_distinct_lines", "mpc_create_cpack", "mpc_create_pattern_evicting",
    "mpc_create_cpack_blocks", "mpc_cpack_blocks_restart", "mpc_cpack_block_lines",
    "mpc_create_fit_pairs", "mpc_create_fit_residues", "mpc_fit_base_table",
]
# The SC2 entry points of include/mpc_hip.h.  Kept apart from EXPORTED_SYMBOLS, which lists the names of the
# header's lowercase-letter form (mpc_[a-z_]+) only; every one of both lists is exported by libmpc_hip.so.
EXPORTED_SC2_SYMBOLS = ["mpc_create_sc2", "mpc_sc2_sampling_lines", "mpc_sc2_code_lengths", "mpc_sc2_table"]
# The size accounting entry points, declared in include/mpc_hip_sizes.h (which mpc_hip.h includes).
EXPORTED_SIZE_SYMBOLS = ["mpc_size_hist_enable", "mpc_size_hist_get", "mpc_group_best_enable", "mpc_group_best_get",
                         "mpc_group_best_reset", "mpc_size_sectors"]
# The per-class accounting entry points, declared in include/mpc_hip_classes.h (which mpc_hip.h includes).
EXPORTED_CLASS_SYMBOLS = ["mpc_class_stats_enable", "mpc_class_stats_get", "mpc_class_stats_merge", "mpc_class_sector_bytes",
                          "mpc_compress_batch_classed", "mpc_compress_batch_device_classed", "mpc_class_log_field",
                          "mpc_group_class_stats_enable", "mpc_group_class_stats_get", "mpc_group_compress_batch_classed",
                          "mpc_group_compress_batch_device_classed", "mpc_group_class_log_field", "mpc_group_class_from_member"]
# The pack accounting entry points, declared in include/mpc_hip_pack.h (which mpc_hip.h includes).
EXPORTED_PACK_SYMBOLS = ["mpc_pack_stats_enable", "mpc_pack_check_values", "mpc_pack_stats_get", "mpc_pack_stats_merge", "mpc_pack_sectors_of_tail",
                         "mpc_group_pack_stats_enable", "mpc_group_pack_stats_get"]
# The image accounting entry points, declared in include/mpc_hip_image.h (which mpc_hip.h includes).
EXPORTED_IMAGE_SYMBOLS = ["mpc_image_stats_enable", "mpc_image_check_values", "mpc_image_stats_get", "mpc_compress_batch_addressed",
                          "mpc_compress_batch_device_addressed", "mpc_image_hash", "mpc_group_image_stats_enable", "mpc_group_image_stats_get",
                          "mpc_group_compress_batch_addressed", "mpc_group_compress_batch_device_addressed"]
# The rewrite accounting entry points, declared in include/mpc_hip_rewrite.h (which mpc_hip.h includes).
EXPORTED_REWRITE_SYMBOLS = ["mpc_rewrite_stats_enable", "mpc_rewrite_check_values", "mpc_rewrite_stats_get", "mpc_group_rewrite_stats_enable",
                            "mpc_group_rewrite_stats_get"]
# The snapshot entry points, declared in include/mpc_hip_snapshot.h (which mpc_hip.h includes).
EXPORTED_SNAPSHOT_SYMBOLS = ["mpc_snapshot_check_values", "mpc_snapshot_create", "mpc_snapshot_destroy", "mpc_snapshot_reset", "mpc_snapshot_last_error",
                             "mpc_snapshot_add", "mpc_snapshot_add_device", "mpc_snapshot_add_gpgpusim_log", "mpc_snapshot_stats", "mpc_snapshot_plan",
                             "mpc_snapshot_write_lines", "mpc_snapshot_read_lines", "mpc_snapshot_evaluate", "mpc_snapshot_evaluate_group"]


def gpgpusim_log_line_size(path: str) -> int:
    """Line size of a GPGPU-Sim ``.log`` trace: req_size of its first request (no device needed)."""
    sz = C.c_uint32()
    rc = lib().mpc_gpgpusim_log_line_size(path.encode(), C.byref(sz))
    if rc != 0:
        raise MpcError(rc, (lib().mpc_last_error(None) or b"").decode())
    return int(sz.value)


def describe_config(cfg) -> Dict:
    """Parse/validate a VPC configuration with the native parser (no device needed)."""
    text = cfg if isinstance(cfg, str) else json.dumps(cfg)
    buf = C.create_string_buffer(1 << 20)
    rc = lib().mpc_config_describe(text.encode(), buf, len(buf))
    out = json.loads(buf.value.decode())
    out["rc"] = rc
    return out


def jit_compile_check(cfg) -> int:
    """Build check of the run-time compilation (no device needed): when the configuration's module sequence would be compiled
    with hiprtc at handle creation, compile it now for gfx950 and return the code object's size; 0 when nothing would be
    compiled.  Raises MpcError with the compiler's log on failure."""
    text = cfg if isinstance(cfg, str) else json.dumps(cfg)
    log = C.create_string_buffer(1 << 16)
    n = lib().mpc_jit_compile_check(text.encode(), log, len(log))
    if n < 0:
        raise MpcError(int(n), log.value.decode(errors="replace"))
    return int(n)


def _as_lines(lines, line_size: int) -> np.ndarray:
    """The ``[n, L] uint8`` argument of ``compress_lines``, C-contiguous."""
    lines = np.ascontiguousarray(lines, dtype=np.uint8)
    if lines.ndim != 2 or lines.shape[1] != line_size:
        raise ValueError(f"expected [n, {line_size}] uint8")
    return lines


def _as_classes(classes, n: int) -> np.ndarray:
    """The ``classes=`` argument of ``compress_lines``: one uint8 per line, C-contiguous."""
    arr = np.asarray(classes)
    if arr.shape != (n,) or not (np.issubdtype(arr.dtype, np.integer) or arr.dtype == np.bool_):
        raise ValueError(f"classes: {n} integers from 0 to 255, one per line")
    if arr.size and (int(arr.min()) < 0 or int(arr.max()) > 255):
        raise ValueError("classes: a class is an integer from 0 to 255")
    return np.ascontiguousarray(arr, dtype=np.uint8)


def _as_addresses(addresses, n: int) -> np.ndarray:
    """The ``addresses=`` argument of ``compress_lines``: one uint64 per line, C-contiguous."""
    arr = np.asarray(addresses)
    if arr.shape != (n,) or not np.issubdtype(arr.dtype, np.integer):
        raise ValueError(f"addresses: {n} unsigned 64-bit integers, one per line")
    if arr.dtype != np.uint64 and arr.size and int(arr.min()) < 0:
        raise ValueError("addresses: an address is an unsigned 64-bit integer")
    return np.ascontiguousarray(arr, dtype=np.uint64)


def _class_log_field(field) -> int:
    if field not in CLASS_LOG_FIELDS:
        raise ValueError(f"class_log_field: one of 'kernel', 'rw', 'mftype' or None, not {field!r}")
    return CLASS_LOG_FIELDS[field]


def class_table_view(table: np.ndarray, line_size: int, sector_bytes: int) -> Dict:
    """A class table ``uint64[256 * MPC_CLASS_ROW]`` as a dict of arrays over the 256 classes: ``lines``, ``bits`` (the
    sum of the compressed sizes) and ``sectors[256, S]`` (column k - 1: lines that occupy k sectors), S =
    ceil(line_size / sector_bytes)."""
    t = np.asarray(table, dtype=np.uint64).reshape(MPC_CLASS_COUNT, MPC_CLASS_ROW)
    S = -(-int(line_size) // int(sector_bytes))
    return {"lines": t[:, 0].copy(), "bits": t[:, 1].copy(), "sectors": t[:, 2:2 + S].copy()}


def _pack_values(fn: str, block_lines, sector_bytes, header_bits):
    """The three values of ``enable_pack_stats`` as the C ABI takes them (unsigned)."""
    block_lines, sector_bytes, header_bits = int(block_lines), int(sector_bytes), int(header_bits)
    if not (0 <= block_lines < 1 << 64 and 0 <= sector_bytes < 1 << 32 and 0 <= header_bits < 1 << 32):
        raise MpcError(-22, f"{fn}: block_lines, sector_bytes and header_bits are unsigned")
    return block_lines, sector_bytes, header_bits


def pack_check_values(line_size: int, block_lines: int, sector_bytes: int = 32, header_bits: int = 0) -> None:
    """Raises ``MpcError`` with the message ``enable_pack_stats`` would give for these values (``mpc_pack_check_values``;
    no device)."""
    rc = lib().mpc_pack_check_values(int(line_size), *_pack_values("mpc_pack_check_values", block_lines, sector_bytes, header_bits))
    if rc != 0:
        raise MpcError(rc, (lib().mpc_last_error(None) or b"").decode())


def pack_sectors_of_tail(table, line_size: int):
    """``(tail_sectors, tail_cap)`` of a pack table's open block, closed as a short block (``mpc_pack_sectors_of_tail``;
    no device); ``(0, 0)`` without open lines."""
    t = np.ascontiguousarray(table, dtype=np.uint64).reshape(-1)
    sectors, cap = C.c_uint64(), C.c_uint64()
    rc = lib().mpc_pack_sectors_of_tail(t.ctypes.data, t.size, int(line_size), C.byref(sectors), C.byref(cap))
    if rc != 0:
        raise MpcError(rc, "mpc_pack_sectors_of_tail: not a pack table (MPC_PACK_TABLE_LEN entries, open lines below block_lines)")
    return int(sectors.value), int(cap.value)


def pack_table_view(table: np.ndarray, line_size: int, close_tail: bool = True) -> Dict:
    """A pack table ``uint64[MPC_PACK_TABLE_LEN]`` as a dict: ``block_lines``, ``sector_bytes``, ``header_bits``,
    ``block_sectors`` (S_B), ``blocks``, ``payload_bits``, ``sectors``, ``histogram[S_B]`` (entry k - 1: closed blocks
    that occupy k sectors), ``open_lines``, ``open_bits``, ``tail_sectors`` and ``tail_cap`` (the open block closed as a
    short one; both 0 with ``close_tail=False``), ``sector_ratio`` = (blocks x S_B + tail_cap) / (sectors +
    tail_sectors) and ``sector_ratio_closed``, the same without the tail (0.0 without sectors)."""
    t = np.asarray(table, dtype=np.uint64).reshape(MPC_PACK_TABLE_LEN)
    N, sb, hb = int(t[5]), int(t[6]), int(t[7])
    S = -(-N * int(line_size) // sb)
    blocks, sectors = int(t[0]), int(t[2])
    tail_sectors, tail_cap = pack_sectors_of_tail(t, line_size) if close_tail else (0, 0)
    total = sectors + tail_sectors
    return {"block_lines": N, "sector_bytes": sb, "header_bits": hb, "block_sectors": S, "blocks": blocks, "payload_bits": int(t[1]),
            "sectors": sectors, "histogram": t[8:8 + S].copy(), "open_lines": int(t[3]), "open_bits": int(t[4]),
            "tail_sectors": tail_sectors, "tail_cap": tail_cap,
            "sector_ratio": (blocks * S + tail_cap) / total if total else 0.0,
            "sector_ratio_closed": blocks * S / sectors if sectors else 0.0}


def _image_values(fn: str, capacity, block_lines, sector_bytes, header_bits):
    """The four values of ``enable_image_stats`` as the C ABI takes them (unsigned), capacity first."""
    capacity = int(capacity)
    if not 0 <= capacity < 1 << 64:
        raise MpcError(-22, f"{fn}: capacity is unsigned")
    return (capacity,) + _pack_values(fn, block_lines, sector_bytes, header_bits)


def image_check_values(line_size: int, block_lines: int, sector_bytes: int = 32, header_bits: int = 0, capacity: int = 1 << 24) -> None:
    """Raises ``MpcError`` with the message ``enable_image_stats`` would give for these values
    (``mpc_image_check_values``; no device)."""
    rc = lib().mpc_image_check_values(int(line_size), *_image_values("mpc_image_check_values", capacity, block_lines, sector_bytes, header_bits))
    if rc != 0:
        raise MpcError(rc, (lib().mpc_last_error(None) or b"").decode())


def image_hash(key: int) -> int:
    """``mpc_image_hash``: a key's first slot is ``image_hash(key) & (slots - 1)``, ``slots`` the smallest power of two
    >= 2 x capacity and at least 2 (no device)."""
    return int(lib().mpc_image_hash(int(key) & ((1 << 64) - 1)))


def image_table_view(table: np.ndarray, line_size: int) -> Dict:
    """An image table ``uint64[MPC_IMAGE_TABLE_LEN]`` as a dict of its named entries, ``block_sectors`` (S_B),
    ``histogram[S_B]`` (entry k - 1: touched blocks that occupy k sectors) and the three ratios ``traffic_ratio`` =
    lines x 8 L / bits, ``image_ratio`` = distinct_lines x 8 L / image_bits and ``image_sector_ratio`` = caps / sectors
    (each 0.0 where its divisor is 0)."""
    t = np.asarray(table, dtype=np.uint64).reshape(MPC_IMAGE_TABLE_LEN)
    v = [int(x) for x in t[:12]]
    L = int(line_size)
    S = -(-v[8] * L // v[9])
    return {"lines": v[0], "bits": v[1], "distinct_lines": v[2], "image_bits": v[3], "blocks": v[4], "sectors": v[5], "caps": v[6],
            "misaligned": v[7], "block_lines": v[8], "sector_bytes": v[9], "header_bits": v[10], "capacity": v[11], "block_sectors": S,
            "histogram": t[16:16 + S].copy(),
            "traffic_ratio": v[0] * 8 * L / v[1] if v[1] else 0.0,
            "image_ratio": v[2] * 8 * L / v[3] if v[3] else 0.0,
            "image_sector_ratio": v[6] / v[5] if v[5] else 0.0}


def _rewrite_values(fn: str, capacity, granule_bytes):
    """The two values of ``enable_rewrite_stats`` as the C ABI takes them (unsigned), capacity first."""
    capacity, granule_bytes = int(capacity), int(granule_bytes)
    if not 0 <= capacity < 1 << 64:
        raise MpcError(-22, f"{fn}: capacity is unsigned")
    if not 0 <= granule_bytes < 1 << 32:
        raise MpcError(-22, f"{fn}: granule_bytes is an unsigned 32-bit value")
    return capacity, granule_bytes


def rewrite_check_values(line_size: int, granule_bytes: int = 32, capacity: int = 1 << 24) -> None:
    """Raises ``MpcError`` with the message ``enable_rewrite_stats`` would give for these values
    (``mpc_rewrite_check_values``; no device)."""
    rc = lib().mpc_rewrite_check_values(int(line_size), *_rewrite_values("mpc_rewrite_check_values", capacity, granule_bytes))
    if rc != 0:
        raise MpcError(rc, (lib().mpc_last_error(None) or b"").decode())


def rewrite_table_view(table: np.ndarray, line_size: int) -> Dict:
    """A rewrite table ``uint64[MPC_REWRITE_TABLE_LEN]`` as a dict of its named sums, the four histograms ``first``,
    ``latest_classes``, ``peak_classes`` (entry c - 1: class c) and ``count_log2`` (entry b: keys with floor(log2(count))
    == b), ``trans`` as a ``[G + 1, G]`` array whose row 0 is the first touches and whose row c_old, column c_new - 1 is a
    transition, and the ratios ``overflow_rate`` = grows / rewrites, ``image_granule_ratio`` = D G / latest_granules,
    ``peak_granule_ratio`` = D G / peak_granules and ``traffic_ratio`` = lines x 8 L / bits (each 0.0 where its divisor is 0)."""
    t = np.asarray(table, dtype=np.uint64).reshape(MPC_REWRITE_TABLE_LEN)
    v = [int(x) for x in t[:16]]
    L, G, M = int(line_size), int(t[14]), MPC_REWRITE_MAX_CLASSES
    trans = np.zeros((G + 1, G), dtype=np.uint64)
    trans[0] = t[16:16 + G]
    trans[1:] = t[144:144 + M * M].reshape(M, M)[:G, :G]
    return {"lines": v[0], "bits": v[1], "distinct_lines": v[2], "misaligned": v[3], "rewrites": v[4], "grows": v[5], "shrinks": v[6],
            "equal_bits": v[7], "latest_granules": v[8], "peak_granules": v[9], "latest_bits": v[10], "peak_bits": v[11],
            "granule_bytes": v[12], "capacity": v[13], "classes": G,
            "first": t[16:16 + G].copy(), "latest_classes": t[48:48 + G].copy(), "peak_classes": t[80:80 + G].copy(),
            "count_log2": t[112:144].copy(), "trans": trans,
            "overflow_rate": v[5] / v[4] if v[4] else 0.0,
            "image_granule_ratio": v[2] * G / v[8] if v[8] else 0.0,
            "peak_granule_ratio": v[2] * G / v[9] if v[9] else 0.0,
            "traffic_ratio": v[0] * 8 * L / v[1] if v[1] else 0.0}


def _ratio(original, compressed, lines) -> float:
    """VPC (``VPC.h:49-60``): inf once lines of 0 bits are all there are, 0 before the first line."""
    if not lines:
        return 0.0
    return float(original) / float(compressed) if compressed else float("inf")


def _ratio_or_zero(original, compressed, lines) -> float:
    """BDI, FPC, BPC and SC2: 0 while there are no compressed bits."""
    return float(original) / float(compressed) if compressed else 0.0


def _totals(v, ratio=_ratio_or_zero) -> Dict:
    """What every ``result()`` starts with, from the head of the statistics vector."""
    return {"lines": int(v[0]), "original_bits": int(v[1]), "compressed_bits": int(v[2]), "comp_ratio": ratio(v[1], v[2], v[0])}


class _Evaluator:
    """Common part of the seven evaluators and the two Fit analyses: creates and owns one ``mpc_handle``."""

    def __init__(self, create: str, *args):
        """``create``: name of the library's create function; ``args``: its arguments in front of the handle."""
        self._h = C.c_void_p()
        self.info = Info()
        rc = getattr(lib(), create)(*args, C.byref(self._h))
        if rc != 0:
            raise MpcError(rc, (lib().mpc_last_error(None) or b"").decode())
        self._finish()
        self.kernel_path = self.info.kernel_path

    def _check(self, rc: int) -> None:
        if rc != 0:
            msg = lib().mpc_last_error(self._h if self._h else None)
            raise MpcError(rc, msg.decode() if msg else "")

    def _finish(self) -> None:
        self._check(lib().mpc_get_info(self._h, C.byref(self.info)))
        self.line_size = self.info.line_size
        self.stats_len = int(self.info.stats_len)

    _sets = ()          # the open EvaluatorSets this evaluator is a member of

    def close(self) -> None:
        if self._h:
            for s in list(self._sets):      # a group is destroyed before its members (mpc_group_destroy reads them)
                s.close()
            lib().mpc_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- hot path -----------------------------------------------------------
    def compress_lines(self, lines: np.ndarray, want_sizes: bool = True,
                       want_selected: bool = True, *, classes=None, addresses=None) -> Tuple[Optional[np.ndarray], Optional[np.ndarray]]:
        """Host buffer [n, L] uint8 -> (size_bits uint16[n], selected int8[n]); staged
        through the pinned double buffers.  Statistics accumulate in the handle.
        ``classes``: one class (0..255) per line for ``class_stats()``; needs ``enable_class_stats()``.
        ``addresses``: one uint64 line address per line for ``image_stats()``; needs ``enable_image_stats()`` (and is
        needed once that is on); not together with ``classes``: addressed lines count in class 0."""
        lines = _as_lines(lines, self.line_size)
        n = lines.shape[0]
        sizes = np.empty(n, dtype=np.uint16) if want_sizes else None
        sel = np.empty(n, dtype=np.int8) if want_selected else None
        if addresses is not None:
            if classes is not None:
                raise ValueError("compress_lines: classes= and addresses= cannot be given together")
            adr = _as_addresses(addresses, n)
            self._check(lib().mpc_compress_batch_addressed(self._h, lines.ctypes.data, n, adr.ctypes.data,
                                                           sizes.ctypes.data if want_sizes else None,
                                                           sel.ctypes.data if want_selected else None))
            return sizes, sel
        if classes is not None:
            cls = _as_classes(classes, n)
            self._check(lib().mpc_compress_batch_classed(self._h, lines.ctypes.data, n, cls.ctypes.data,
                                                         sizes.ctypes.data if want_sizes else None,
                                                         sel.ctypes.data if want_selected else None))
            return sizes, sel
        self._check(lib().mpc_compress_batch(self._h, lines.ctypes.data, n,
                                             sizes.ctypes.data if want_sizes else None,
                                             sel.ctypes.data if want_selected else None))
        return sizes, sel

    def compress_device(self, d_lines: int, n_lines: int, d_sizes: int = 0, d_selected: int = 0,
                        stream: int = 0, *, classes: int = 0, addresses: int = 0) -> None:
        """Device-resident lines (raw pointers, e.g. ``tensor.data_ptr()``); asynchronous.
        ``classes``: raw device pointer to ``n_lines`` uint8 classes; needs ``enable_class_stats()``.
        ``addresses``: raw device pointer to ``n_lines`` uint64 line addresses; needs ``enable_image_stats()``."""
        if addresses:
            if classes:
                raise ValueError("compress_device: classes= and addresses= cannot be given together")
            self._check(lib().mpc_compress_batch_device_addressed(self._h, d_lines, n_lines, addresses, d_sizes or None,
                                                                  d_selected or None, stream or None))
            return
        if classes:
            self._check(lib().mpc_compress_batch_device_classed(self._h, d_lines, n_lines, classes, d_sizes or None,
                                                                d_selected or None, stream or None))
            return
        self._check(lib().mpc_compress_batch_device(self._h, d_lines, n_lines, d_sizes or None,
                                                    d_selected or None, stream or None))

    def compress_npy(self, path: str, first_row: int = 0, n_rows: int = (1 << 62),
                     skip_last_row: bool = True) -> int:
        done = C.c_uint64()
        self._check(lib().mpc_compress_npy(self._h, path.encode(), first_row, n_rows,
                                           1 if skip_last_row else 0, C.byref(done)))
        return int(done.value)

    def compress_gpgpusim_log(self, path: str):
        """Stream a GPGPU-Sim ``.log`` trace (reference ``LoaderGPGPU.cpp`` + the driver's
        GLOBAL_ACC_R / GLOBAL_ACC_W filter, ``main.cpp:222-224``); returns
        (requests read, lines evaluated)."""
        req, done = C.c_uint64(), C.c_uint64()
        self._check(lib().mpc_compress_gpgpusim_log(self._h, path.encode(), C.byref(req), C.byref(done)))
        return int(req.value), int(done.value)

    def sync(self) -> None:
        self._check(lib().mpc_sync(self._h))

    # -- statistics -----------------------------------------------------------
    def stats_vector(self) -> np.ndarray:
        v = np.zeros(self.stats_len, dtype=np.uint64)
        self._check(lib().mpc_stats_get(self._h, v.ctypes.data, self.stats_len))
        return v

    def stats_raw_len(self) -> int:
        n = C.c_uint64()
        self._check(lib().mpc_stats_raw_len(self._h, C.byref(n)))
        return int(n.value)

    def stats_copy_raw_device(self, d_dst: int, stream: int = 0) -> None:
        """Asynchronous device-to-device copy of the raw uint64 accumulators into ``d_dst``
        (``stats_raw_len()`` words) on ``stream``: the operand of a device-side all-reduce."""
        self._check(lib().mpc_stats_copy_raw_device(self._h, d_dst, stream or None))

    def stats_from_raw(self, raw: np.ndarray) -> np.ndarray:
        """Statistics vector (ABI layout) of a raw accumulator array, e.g. an all-reduced one."""
        raw = np.ascontiguousarray(raw, dtype=np.uint64)
        v = np.zeros(self.stats_len, dtype=np.uint64)
        self._check(lib().mpc_stats_from_raw(self._h, raw.ctypes.data, raw.size, v.ctypes.data, v.size))
        return v

    def stats_merge(self, vec: np.ndarray) -> None:
        vec = np.ascontiguousarray(vec, dtype=np.uint64)
        self._check(lib().mpc_stats_merge(self._h, vec.ctypes.data, len(vec)))

    def stats_set(self, vec: np.ndarray) -> None:
        vec = np.ascontiguousarray(vec, dtype=np.uint64)
        self._check(lib().mpc_stats_set(self._h, vec.ctypes.data, len(vec)))

    def reset(self) -> None:
        self._check(lib().mpc_stats_reset(self._h))

    # -- size accounting ------------------------------------------------------
    def enable_size_histogram(self) -> None:
        """Count, from now on, how many lines compress to how many bits (``mpc_size_hist_enable``); idempotent."""
        self._check(lib().mpc_size_hist_enable(self._h))

    def size_histogram(self) -> np.ndarray:
        """``uint64[MPC_SIZE_BINS]``: bin s = lines of s bits since accounting was switched on or the last ``reset()``
        (the last bin also takes larger sizes).  Raises ``MpcError`` (MPC_E_INVAL) when accounting is off."""
        bins = np.zeros(MPC_SIZE_BINS, dtype=np.uint64)
        self._check(lib().mpc_size_hist_get(self._h, bins.ctypes.data, MPC_SIZE_BINS))
        return bins

    # -- per-class accounting -------------------------------------------------
    def enable_class_stats(self, sector_bytes: int = 32) -> None:
        """Sum, from now on, lines, compressed bits and sector counts per class of a line (``mpc_class_stats_enable``);
        idempotent for the same ``sector_bytes``.  Lines of calls without ``classes=`` count in class 0."""
        sector_bytes = int(sector_bytes)
        if not 0 <= sector_bytes < 1 << 32:
            raise MpcError(-22, "mpc_class_stats_enable: sector_bytes is unsigned")
        self._check(lib().mpc_class_stats_enable(self._h, sector_bytes))

    def class_sector_bytes(self) -> int:
        b = C.c_uint()
        self._check(lib().mpc_class_sector_bytes(self._h, C.byref(b)))
        return int(b.value)

    def class_table(self) -> np.ndarray:
        """The raw table ``uint64[256, MPC_CLASS_ROW]`` (``mpc_class_stats_get``): what ``class_stats_merge`` takes."""
        t = np.zeros(MPC_CLASS_TABLE_LEN, dtype=np.uint64)
        self._check(lib().mpc_class_stats_get(self._h, t.ctypes.data, t.size))
        return t.reshape(MPC_CLASS_COUNT, MPC_CLASS_ROW)

    def class_stats(self) -> Dict:
        """Arrays over the 256 classes since accounting was switched on or the last ``reset()``: ``lines``, ``bits``,
        ``sectors[256, S]``.  Raises ``MpcError`` (MPC_E_INVAL) when accounting is off."""
        return class_table_view(self.class_table(), self.line_size, self.class_sector_bytes())

    def class_stats_merge(self, table: np.ndarray) -> None:
        """Add another evaluator's ``class_table()`` (a shard's)."""
        table = np.ascontiguousarray(table, dtype=np.uint64)
        self._check(lib().mpc_class_stats_merge(self._h, table.ctypes.data, table.size))

    def class_log_field(self, field) -> None:
        """Which field of a ``.log`` record is the class of its line in ``compress_gpgpusim_log``: ``"kernel"`` (the
        kernel id), ``"rw"`` (0 = read, 1 = write), ``"mftype"`` or ``None`` (class 0)."""
        self._check(lib().mpc_class_log_field(self._h, _class_log_field(field)))


    # -- pack accounting --------------------------------------------------------
    def enable_pack_stats(self, block_lines: int, sector_bytes: int = 32, header_bits: int = 0) -> None:
        """Count, from now on, the sectors of ``sector_bytes`` bytes that blocks of ``block_lines`` consecutive lines
        occupy when their compressed lines are packed and rounded up once, ``header_bits`` added per block
        (``mpc_pack_stats_enable``); idempotent for the same values.  Lines are numbered from 0 in the order of the
        calls, from now or the last ``reset()``."""
        self._check(lib().mpc_pack_stats_enable(self._h, *_pack_values("mpc_pack_stats_enable", block_lines, sector_bytes, header_bits)))

    def pack_table(self) -> np.ndarray:
        """The raw table ``uint64[MPC_PACK_TABLE_LEN]`` (``mpc_pack_stats_get``): what ``pack_stats_merge`` takes."""
        t = np.zeros(MPC_PACK_TABLE_LEN, dtype=np.uint64)
        self._check(lib().mpc_pack_stats_get(self._h, t.ctypes.data, t.size))
        return t

    def pack_stats(self, close_tail: bool = True) -> Dict:
        """``pack_table_view`` of the table since accounting was switched on or the last ``reset()``."""
        return pack_table_view(self.pack_table(), self.line_size, close_tail)

    def pack_stats_merge(self, table: np.ndarray) -> None:
        """Add another evaluator's ``pack_table()`` (a shard's, cut at a multiple of ``block_lines``) and take over its
        open block."""
        table = np.ascontiguousarray(table, dtype=np.uint64).reshape(-1)
        self._check(lib().mpc_pack_stats_merge(self._h, table.ctypes.data, table.size))


    # -- image accounting -------------------------------------------------------
    def enable_image_stats(self, block_lines: int, sector_bytes: int = 32, header_bits: int = 0, capacity: int = 1 << 24) -> None:
        """Keep, from now on, the size of the latest line per line address (``addresses=``, or a ``.log``'s
        ``mem_addr``), for up to ``capacity`` distinct lines (32 bytes of device memory each), and report what
        address-aligned blocks of ``block_lines`` lines of that image occupy in sectors of ``sector_bytes`` bytes,
        ``header_bits`` added per block (``mpc_image_stats_enable``); idempotent for the same values."""
        self._check(lib().mpc_image_stats_enable(self._h, *_image_values("mpc_image_stats_enable", capacity, block_lines, sector_bytes, header_bits)))

    def image_table(self) -> np.ndarray:
        """The raw table ``uint64[MPC_IMAGE_TABLE_LEN]`` (``mpc_image_stats_get``); not destructive."""
        t = np.zeros(MPC_IMAGE_TABLE_LEN, dtype=np.uint64)
        self._check(lib().mpc_image_stats_get(self._h, t.ctypes.data, t.size))
        return t

    def image_stats(self) -> Dict:
        """``image_table_view`` of the image since accounting was switched on or the last ``reset()``."""
        return image_table_view(self.image_table(), self.line_size)

    # -- rewrite accounting -----------------------------------------------------
    def enable_rewrite_stats(self, granule_bytes: int = 32, capacity: int = 1 << 24) -> None:
        """Follow, from now on, the sequence of sizes per line address (``addresses=``, or a ``.log``'s ``mem_addr``),
        for up to ``capacity`` distinct lines (32 bytes of device memory each, and the scratch of a sub-batch), in
        size classes of ``granule_bytes`` bytes (``mpc_rewrite_stats_enable``); idempotent for the same values."""
        self._check(lib().mpc_rewrite_stats_enable(self._h, *_rewrite_values("mpc_rewrite_stats_enable", capacity, granule_bytes)))

    def rewrite_table(self) -> np.ndarray:
        """The raw table ``uint64[MPC_REWRITE_TABLE_LEN]`` (``mpc_rewrite_stats_get``); not destructive."""
        t = np.zeros(MPC_REWRITE_TABLE_LEN, dtype=np.uint64)
        self._check(lib().mpc_rewrite_stats_get(self._h, t.ctypes.data, t.size))
        return t

    def rewrite_stats(self) -> Dict:
        """``rewrite_table_view`` of the lines since accounting was switched on or the last ``reset()``."""
        return rewrite_table_view(self.rewrite_table(), self.line_size)


class VPC(_Evaluator):
    """``comp::VPC(configPath)`` (reference ``VPC.h:244-249``)."""

    def __init__(self, config, device: int = -1):
        if isinstance(config, dict):
            super().__init__("mpc_create_vpc_from_string", json.dumps(config).encode(), device)
        else:
            super().__init__("mpc_create_vpc", str(config).encode(), device)
        self.num_modules = self.info.num_modules
        self.hist_bins = self.info.hist_bins
        self.path_reason = (lib().mpc_path_reason(self._h) or b"").decode()   # why the generic kernel, if it is
        # "unrolled" | "unrolled, general layout" | "unrolled, compiled at creation[ (from the cache)]" | "run-time loop" | "generic"
        self.kernel_form = (lib().mpc_kernel_form(self._h) or b"").decode()

    def result(self) -> Dict:
        """``VPCResult`` (reference ``VPC.h:36-76``) derived from the integer vector."""
        return vpc_result_from_vector(self.stats_vector(), self.num_modules, self.hist_bins, self.line_size)


class BDI(_Evaluator):
    """``comp::BDI(lineSize)`` (reference ``BDI.h:90-107``)."""

    def __init__(self, line_size: int, device: int = -1):
        super().__init__("mpc_create_bdi", line_size, device)

    def result(self) -> Dict:
        v = self.stats_vector()
        return {**_totals(v), "counts": [int(x) for x in v[3:12]]}


class FPC(_Evaluator):
    """``comp::FPC(lineSize)`` (reference ``FPC.h:91-103``); per-line ``selected`` is always 0."""

    def __init__(self, line_size: int, device: int = -1):
        super().__init__("mpc_create_fpc", line_size, device)

    def result(self) -> Dict:
        v = self.stats_vector()
        return {**_totals(v), "total_words": int(v[3:11].sum()), "counts": [int(x) for x in v[3:11]]}


class BPC(_Evaluator):
    """``comp::BPC(lineSize)`` (reference ``BPC.h:90-107``); per-line ``selected`` is always 0."""

    def __init__(self, line_size: int, device: int = -1):
        super().__init__("mpc_create_bpc", line_size, device)

    def result(self) -> Dict:
        v = self.stats_vector()
        return {**_totals(v), "total_words": int(v[3]), "counts": [int(x) for x in v[4:11]]}


class SC2(_Evaluator):
    """``comp::SC2(lineSize, warmupCnt)`` (reference ``SC2.h:100-107``): lines 0 .. sampling_lines-1 of the trace, counted
    across every call on this object, are the warm-up sample; the code table is built when the next line arrives.
    Per-line ``selected``: 0 for a warm-up line, 1 for a line sized against the table."""

    def __init__(self, line_size: int, sampling_lines: int, device: int = -1):
        super().__init__("mpc_create_sc2", line_size, sampling_lines, device)
        self.sampling_lines = int(sampling_lines)

    @property
    def kernel_form(self) -> str:
        """"warm-up counting" before line S, "table sizing" after."""
        return (lib().mpc_kernel_form(self._h) or b"").decode()

    def result(self) -> Dict:
        """``CompResult`` (OriginalSize, CompressedSize, CompRatio; name "SC2-Huffman") plus the SC2 counters."""
        v = self.stats_vector()
        return {"name": "SC2-Huffman", **_totals(v), "warmup_lines": int(v[3]), "table_symbols": int(v[4]), "words_in_table": int(v[5])}

    def table(self) -> Tuple[np.ndarray, np.ndarray]:
        """(symbols uint32, code lengths uint16) in ascending symbol order; empty before line S."""
        sym = np.zeros(1024, dtype=np.uint32)
        lens = np.zeros(1024, dtype=np.uint16)
        n = C.c_size_t()
        self._check(lib().mpc_sc2_table(self._h, sym.ctypes.data, lens.ctypes.data, 1024, C.byref(n)))
        return sym[:n.value].copy(), lens[:n.value].copy()


def pattern_entropy(counts) -> float:
    """``PatternResult::ComputeEntropy`` (reference ``Pattern.h:124-154``): the map holds the symbols that occurred,
    ``entropy += -p * log2(p)`` in ascending symbol order."""
    import math
    counts = [int(c) for c in counts]
    total = sum(counts)
    entropy = 0.0
    for c in counts:
        if c:
            p = float(c) / float(total)
            entropy += -p * math.log2(p)
    return entropy


def pattern_result_from_vector(v: np.ndarray) -> Dict:
    """``PatternResult`` (reference ``Pattern.h:30-226``) from the statistics vector."""
    sym = [int(x) for x in v[22:278]]
    exc = [int(x) for x in v[278:534]]
    return {"name": "Pattern Checker", "lines": int(v[0]), "original_bits": 0, "compressed_bits": 0, "comp_ratio": 0.0,
            "size_bits": int(v[3]), "Z": int(v[4]), "R": int(v[5]), "T": int(v[6]), "U": int(v[7]), "Total": int(v[8]),
            "implicit_counts": [int(x) for x in v[9:15]], "explicit_counts": [int(x) for x in v[15:21]],
            "joined_lines": int(v[21]), "symbol_counts": sym, "symbol_counts_except": exc,
            "entropy": pattern_entropy(sym), "entropy_except": pattern_entropy(exc)}


class Pattern(_Evaluator):
    """``comp::Pattern(lineSize)`` (reference ``Pattern.h:228-252``): zero / repeated / already-seen / base-delta bytes and
    the byte entropy of a trace.  Per-line ``selected`` is the ``PatternState`` (0..5, 9 = NotDefined).  The set of
    lines seen lives on the device.  One object per trace and per GPU.

    ``on_full="refuse"`` (the default): the set holds up to 2**24 - 1 distinct lines; the reference evicts beyond that,
    this raises ``MpcError`` instead.  ``on_full="evict"``: the reference's eviction (a FIFO over insertions, see
    ``mpc_create_pattern_evicting`` in ``include/mpc_hip.h``) with ``capacity`` lines, ``None`` for the reference's
    2**24 - 1; it takes any trace, and beyond the capacity its numbers depend on the order of the lines.  Below the
    capacity both give the same numbers."""

    def __init__(self, line_size: int, device: int = 0, on_full: str = "refuse", capacity: Optional[int] = None):
        if on_full not in ("refuse", "evict"):
            raise ValueError(f"on_full is 'refuse' or 'evict', not {on_full!r}")
        if on_full == "refuse" and capacity is not None:
            raise ValueError("capacity is the evicting set's: on_full='evict'")
        self.on_full = on_full
        if on_full == "evict":
            if capacity is not None and (int(capacity) != capacity or capacity < 1):
                raise ValueError("capacity is None or an integer from 1 to 2**24 - 1")
            super().__init__("mpc_create_pattern_evicting", line_size, 0 if capacity is None else int(capacity), device)
        else:
            super().__init__("mpc_create_pattern", line_size, device)

    def result(self) -> Dict:
        """The counts of ``PatternResult`` and both entropies (the reference computes them in ``Print``)."""
        return pattern_result_from_vector(self.stats_vector())

    def distinct_lines(self) -> int:
        """Lines that joined the set since creation: the distinct lines, or with ``on_full="evict"`` the insertions
        (``reset()`` keeps the set)."""
        n = C.c_uint64()
        self._check(lib().mpc_pattern_distinct_lines(self._h, C.byref(n)))
        return int(n.value)


CPACK_DICTIONARY = {"carried": MPC_CPACK_DICT_CARRIED, "line": MPC_CPACK_DICT_PER_LINE}


class CPACK(_Evaluator):
    """C-Pack (reference ``CPACK.cpp``) with a PER-LINE dictionary: the numbers of a fresh ``comp::CPACK(lineSize)`` per
    line, NOT those of the reference's ``-a CPACK`` run, whose one object carries its dictionary from line to line.
    ``dictionary="line"`` is the only scope the library evaluates; ``"carried"`` (and anything else) raises ``MpcError``
    with the library's message.  Per-line ``selected`` is always 0; a size may exceed 8 x line_size.

    ``dictionary="block", block_lines=N`` (``mpc_create_cpack_blocks``): one dictionary per block of N lines, what a fresh
    ``comp::CPACK(lineSize)`` every N lines reports.  The object numbers its lines from 0 in the order of its calls (all
    ingestion paths, until ``restart()``), block b is lines [b N, (b + 1) N).  The result depends on where blocks begin
    (shards start at multiples of N: ``sharded.shard_range(..., align=N)``), a block is one lane's sequential work, and N
    beyond the trace is the reference's ``-a CPACK`` run on a single lane: exact and slow."""

    PATTERNS = ("ZZZZ", "ZZZX", "MMMM", "MMMX", "MMXX", "XXXX")      # CPACKPattern order; 2, 12, 6, 16, 24, 34 bits

    def __init__(self, line_size: int, dictionary: str = "line", device: int = -1, *, block_lines: Optional[int] = None):
        if dictionary == "block":
            if block_lines is None:
                raise ValueError("C-Pack: dictionary='block' needs block_lines (1 .. 2**32 - 1)")
            if int(block_lines) != block_lines or not 0 <= block_lines < 1 << 64:
                raise ValueError("C-Pack: block_lines is an integer from 1 to 2**32 - 1")
            super().__init__("mpc_create_cpack_blocks", line_size, int(block_lines), device)
            self.dictionary = "block"
            n = C.c_uint64()
            self._check(lib().mpc_cpack_block_lines(self._h, C.byref(n)))
            self._block_lines = int(n.value)
            return
        if block_lines is not None:
            raise ValueError("C-Pack: block_lines belongs to dictionary='block'")
        scope = CPACK_DICTIONARY.get(dictionary, -1) if isinstance(dictionary, str) else int(dictionary)
        super().__init__("mpc_create_cpack", line_size, scope, device)
        self.dictionary = "line"
        self._block_lines = None

    @property
    def block_lines(self) -> Optional[int]:
        """Lines per dictionary block; ``None`` for the per-line dictionary."""
        return self._block_lines

    @property
    def kernel_form(self) -> str:
        return (lib().mpc_kernel_form(self._h) or b"").decode()

    def restart(self) -> None:
        """The next line starts a block (``mpc_cpack_blocks_restart``): before a second trace.  The statistics stay."""
        self._check(lib().mpc_cpack_blocks_restart(self._h))

    def result(self) -> Dict:
        """``CPACKResult`` (reference ``CPACK.h:28-96``): the totals, ``total_words`` and the six pattern counts."""
        v = self.stats_vector()
        return {"name": "C-Pack", **_totals(v), "total_words": int(v[3]), "counts": [int(x) for x in v[4:10]]}


class _Fit(_Evaluator):
    """Common part of the two Fit analyses: no per-line result."""

    def compress_lines(self, lines: np.ndarray, want_sizes: bool = False, want_selected: bool = False):
        """Host buffer [n, L] uint8; the counts accumulate in the handle.  Returns ``(None, None)``: an analysis has no
        per-line result (asking for one raises ``MpcError``, the library's refusal)."""
        return super().compress_lines(lines, want_sizes, want_selected)

    @property
    def kernel_form(self) -> str:
        return (lib().mpc_kernel_form(self._h) or b"").decode()

    def lines(self) -> int:
        return int(self.stats_vector()[0])


class FitPairs(_Fit):
    """``mpc_create_fit_pairs``: for every byte pair (i, j) of the lines fed, how many lines have a residue
    ``(line[i] - line[j]) & 255`` of bit length k (0 for a zero residue, else 1..8).  ``fit.fit_base_table`` picks the
    BaseIndexTable of a DiffBase module from it.  line_size: 32, 64 or 128."""

    def __init__(self, line_size: int, device: int = -1):
        super().__init__("mpc_create_fit_pairs", line_size, device)

    def table(self) -> np.ndarray:
        """``uint64[L, L, 9]``: P[i][j][k]."""
        L = self.line_size
        return self.stats_vector()[3:].reshape(L, L, 9).copy()


class FitResidues(_Fit):
    """``mpc_create_fit_residues``: for every byte i how many lines have the residue ``(line[i] - line[base_table[i]]) &
    255 == v``.  ``fit.fit_diff_table`` picks the DiffTable from it.  ``base_table``: L entries below L, any table."""

    def __init__(self, line_size: int, base_table, device: int = -1):
        base = np.ascontiguousarray(base_table)
        if base.ndim != 1 or base.shape[0] != line_size or not np.issubdtype(base.dtype, np.integer) or \
                (base.size and (base.min() < 0 or base.max() > 255)):
            raise ValueError(f"base_table: {line_size} integers from 0 to 255")
        base = base.astype(np.uint8)
        super().__init__("mpc_create_fit_residues", line_size, base.ctypes.data, device)
        out = np.zeros(self.line_size, dtype=np.uint8)
        self._check(lib().mpc_fit_base_table(self._h, out.ctypes.data, out.size))
        self.base_table = [int(b) for b in out]

    def table(self) -> np.ndarray:
        """``uint64[L, 256]``: V[i][v]."""
        return self.stats_vector()[3:].reshape(self.line_size, 256).copy()


class EvaluatorSet:
    """A group of evaluators of one line size on one device that are fed together (``mpc_group``): the trace is
    staged once per chunk and every member sees every line as if it had been called alone.  The members keep their
    own statistics: read them with each member's ``result()`` / ``stats_vector()`` as usual.  The set borrows its
    members and has to go before them: it keeps them alive until it is closed, and closing (or collecting) a member
    closes every open set it belongs to first, in whatever order the garbage collector finalizes a forgotten set and
    its members."""

    def __init__(self, evaluators):
        self.members = list(evaluators)
        self._g = C.c_void_p()
        if any(not isinstance(e, _Evaluator) or not e._h for e in self.members):
            raise ValueError("EvaluatorSet takes open VPC / BDI / FPC / BPC / SC2 / Pattern / CPACK evaluators")
        arr = (C.c_void_p * max(1, len(self.members)))(*[e._h.value for e in self.members])
        rc = lib().mpc_group_create(arr, len(self.members), C.byref(self._g))
        if rc != 0:
            raise MpcError(rc, (lib().mpc_group_last_error(None) or b"").decode())
        for e in self.members:
            e._sets = list(e._sets) + [self]
        self.line_size = self.members[0].line_size

    def _check(self, rc: int) -> None:
        if rc != 0:
            raise MpcError(rc, (lib().mpc_group_last_error(self._g) or b"").decode())

    @property
    def form(self) -> str:
        """Which members share a kernel launch and which run their own, e.g.
        ``"VPC: unrolled; BDI+FPC+BPC: one kernel; SC2: own kernel"``."""
        return (lib().mpc_group_form(self._g) or b"").decode()

    def close(self) -> None:
        if self._g:
            lib().mpc_group_destroy(self._g)
            self._g = C.c_void_p()
            for e in self.members:
                e._sets = [s for s in e._sets if s is not self]

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _pointers(self, values):
        return (C.c_void_p * len(self.members))(*values)

    def compress_lines(self, lines: np.ndarray, want_sizes: bool = True, want_selected: bool = True, *, classes=None, addresses=None):
        """Host buffer [n, L] uint8 -> one ``(size_bits, selected)`` pair per member, in member order.
        ``classes``: one class (0..255) per line for ``class_stats()``; needs ``enable_class_stats()``.
        ``addresses``: one uint64 line address per line for ``image_stats()``; needs ``enable_image_stats()``."""
        lines = _as_lines(lines, self.line_size)
        n = lines.shape[0]
        sizes = [np.empty(n, dtype=np.uint16) if want_sizes else None for _ in self.members]
        sel = [np.empty(n, dtype=np.int8) if want_selected else None for _ in self.members]
        p_sizes = self._pointers([a.ctypes.data for a in sizes]) if want_sizes else None
        p_sel = self._pointers([a.ctypes.data for a in sel]) if want_selected else None
        if addresses is not None:
            if classes is not None:
                raise ValueError("compress_lines: classes= and addresses= cannot be given together")
            adr = _as_addresses(addresses, n)
            self._check(lib().mpc_group_compress_batch_addressed(self._g, lines.ctypes.data, n, adr.ctypes.data, p_sizes, p_sel))
        elif classes is not None:
            cls = _as_classes(classes, n)
            self._check(lib().mpc_group_compress_batch_classed(self._g, lines.ctypes.data, n, cls.ctypes.data, p_sizes, p_sel))
        else:
            self._check(lib().mpc_group_compress_batch(self._g, lines.ctypes.data, n, p_sizes, p_sel))
        return list(zip(sizes, sel))

    def compress_device(self, d_lines: int, n_lines: int, d_sizes=None, d_selected=None, stream: int = 0, *, classes: int = 0,
                        addresses: int = 0) -> None:
        """Device-resident lines; ``d_sizes`` / ``d_selected``: one raw device pointer (or 0 / None) per member.
        ``classes``: raw device pointer to ``n_lines`` uint8 classes; needs ``enable_class_stats()``.
        ``addresses``: raw device pointer to ``n_lines`` uint64 line addresses; needs ``enable_image_stats()``."""
        p_sizes = self._pointers([p or None for p in d_sizes]) if d_sizes is not None else None
        p_sel = self._pointers([p or None for p in d_selected]) if d_selected is not None else None
        if addresses:
            if classes:
                raise ValueError("compress_device: classes= and addresses= cannot be given together")
            self._check(lib().mpc_group_compress_batch_device_addressed(self._g, d_lines, n_lines, addresses, p_sizes, p_sel, stream or None))
        elif classes:
            self._check(lib().mpc_group_compress_batch_device_classed(self._g, d_lines, n_lines, classes, p_sizes, p_sel, stream or None))
        else:
            self._check(lib().mpc_group_compress_batch_device(self._g, d_lines, n_lines, p_sizes, p_sel, stream or None))

    def compress_npy(self, path: str, first_row: int = 0, n_rows: int = (1 << 62), skip_last_row: bool = True) -> int:
        done = C.c_uint64()
        self._check(lib().mpc_group_compress_npy(self._g, path.encode(), first_row, n_rows,
                                                 1 if skip_last_row else 0, C.byref(done)))
        return int(done.value)

    def compress_gpgpusim_log(self, path: str):
        req, done = C.c_uint64(), C.c_uint64()
        self._check(lib().mpc_group_compress_gpgpusim_log(self._g, path.encode(), C.byref(req), C.byref(done)))
        return int(req.value), int(done.value)

    def sync(self) -> None:
        self._check(lib().mpc_group_sync(self._g))

    # -- best-of ---------------------------------------------------------------
    def enable_best(self) -> None:
        """Account, from now on, the per-line smallest size over the members (all but ``Pattern`` ones); idempotent."""
        self._check(lib().mpc_group_best_enable(self._g))

    def best(self) -> Dict:
        """``bins``: histogram of the best size without tag bits; ``wins``: lines won per member (ties go to the first
        minimal member; 0 for a member outside the set); ``best_bits``: sum of the best sizes; ``lines``; ``tag_bits``:
        ceil(log2(members taking part)), what a hybrid stores per line to name the winner."""
        bins = np.zeros(MPC_SIZE_BINS, dtype=np.uint64)
        wins = np.zeros(len(self.members), dtype=np.uint64)
        bits, lines = C.c_uint64(), C.c_uint64()
        self._check(lib().mpc_group_best_get(self._g, bins.ctypes.data, MPC_SIZE_BINS, wins.ctypes.data, len(self.members),
                                             C.byref(bits), C.byref(lines)))
        taking_part = sum(1 for e in self.members if not isinstance(e, Pattern))
        return {"bins": bins, "wins": wins, "best_bits": int(bits.value), "lines": int(lines.value),
                "tag_bits": (taking_part - 1).bit_length()}

    def reset_best(self) -> None:
        self._check(lib().mpc_group_best_reset(self._g))

    # -- per-class accounting ----------------------------------------------------
    def enable_class_stats(self, sector_bytes: int = 32) -> None:
        """``enable_class_stats`` for every member; with ``enable_best()`` (before or after) also a table of the
        per-line smallest size.  Idempotent for the same ``sector_bytes``."""
        sector_bytes = int(sector_bytes)
        if not 0 <= sector_bytes < 1 << 32:
            raise MpcError(-22, "mpc_group_class_stats_enable: sector_bytes is unsigned")
        self._check(lib().mpc_group_class_stats_enable(self._g, sector_bytes))
        self._class_sector_bytes = sector_bytes

    def class_table(self, member: int) -> np.ndarray:
        """The raw table ``uint64[256, MPC_CLASS_ROW]`` of member ``member`` or, with ``MPC_CLASS_BEST``, of the best-of."""
        t = np.zeros(MPC_CLASS_TABLE_LEN, dtype=np.uint64)
        self._check(lib().mpc_group_class_stats_get(self._g, int(member), t.ctypes.data, t.size))
        return t.reshape(MPC_CLASS_COUNT, MPC_CLASS_ROW)

    def class_stats(self) -> Dict:
        """``{0: ..., 1: ..., "best": ...}``: one entry per member, in member order, and -- while the best-of is on --
        ``"best"``; each as ``_Evaluator.class_stats()`` returns it."""
        sb = getattr(self, "_class_sector_bytes", None)
        if sb is None:
            self._check(lib().mpc_group_class_stats_get(self._g, 0, None, 0))      # (raises: accounting is off)
        out = {i: class_table_view(self.class_table(i), self.line_size, sb) for i in range(len(self.members))}
        t = np.zeros(MPC_CLASS_TABLE_LEN, dtype=np.uint64)
        if lib().mpc_group_class_stats_get(self._g, MPC_CLASS_BEST, t.ctypes.data, t.size) == 0:
            out["best"] = class_table_view(t, self.line_size, sb)
        return out

    # -- pack accounting -----------------------------------------------------------
    def enable_pack_stats(self, block_lines: int, sector_bytes: int = 32, header_bits: int = 0) -> None:
        """``enable_pack_stats`` for every member with the same values; with ``enable_best()`` BEFORE it also a table of
        the per-line smallest size, counted with ``header_bits + block_lines x tag_bits``."""
        self._check(lib().mpc_group_pack_stats_enable(self._g, *_pack_values("mpc_group_pack_stats_enable", block_lines, sector_bytes,
                                                                              header_bits)))

    def pack_table(self, member: int) -> np.ndarray:
        """The raw table of member ``member`` or, with ``MPC_PACK_BEST``, of the per-line minimum."""
        t = np.zeros(MPC_PACK_TABLE_LEN, dtype=np.uint64)
        self._check(lib().mpc_group_pack_stats_get(self._g, int(member), t.ctypes.data, t.size))
        return t

    def pack_stats(self, close_tail: bool = True) -> Dict:
        """``{0: ..., 1: ..., "best": ...}``: one entry per member, in member order, and ``"best"`` if the best-of was
        on when pack accounting was switched on; each as ``_Evaluator.pack_stats()`` returns it."""
        out = {i: pack_table_view(self.pack_table(i), self.line_size, close_tail) for i in range(len(self.members))}
        t = np.zeros(MPC_PACK_TABLE_LEN, dtype=np.uint64)
        if lib().mpc_group_pack_stats_get(self._g, MPC_PACK_BEST, t.ctypes.data, t.size) == 0:
            out["best"] = pack_table_view(t, self.line_size, close_tail)
        return out

    # -- image accounting ----------------------------------------------------------
    def enable_image_stats(self, block_lines: int, sector_bytes: int = 32, header_bits: int = 0, capacity: int = 1 << 24) -> None:
        """``enable_image_stats`` for every member with the same values; a member's image is its own."""
        self._check(lib().mpc_group_image_stats_enable(self._g, *_image_values("mpc_group_image_stats_enable", capacity, block_lines, sector_bytes,
                                                                                header_bits)))

    def image_table(self, member: int) -> np.ndarray:
        """The raw table of member ``member``."""
        t = np.zeros(MPC_IMAGE_TABLE_LEN, dtype=np.uint64)
        self._check(lib().mpc_group_image_stats_get(self._g, int(member), t.ctypes.data, t.size))
        return t

    def image_stats(self) -> Dict:
        """``{0: ..., 1: ...}``: one entry per member, in member order, each as ``_Evaluator.image_stats()`` returns it."""
        return {i: image_table_view(self.image_table(i), self.line_size) for i in range(len(self.members))}

    # -- rewrite accounting --------------------------------------------------------
    def enable_rewrite_stats(self, granule_bytes: int = 32, capacity: int = 1 << 24) -> None:
        """``enable_rewrite_stats`` for every member with the same values; a member's map is its own."""
        self._check(lib().mpc_group_rewrite_stats_enable(self._g, *_rewrite_values("mpc_group_rewrite_stats_enable", capacity, granule_bytes)))

    def rewrite_table(self, member: int) -> np.ndarray:
        """The raw table of member ``member``."""
        t = np.zeros(MPC_REWRITE_TABLE_LEN, dtype=np.uint64)
        self._check(lib().mpc_group_rewrite_stats_get(self._g, int(member), t.ctypes.data, t.size))
        return t

    def rewrite_stats(self) -> Dict:
        """``{0: ..., 1: ...}``: one entry per member, in member order, each as ``_Evaluator.rewrite_stats()`` returns it."""
        return {i: rewrite_table_view(self.rewrite_table(i), self.line_size) for i in range(len(self.members))}

    def class_log_field(self, field) -> None:
        """``_Evaluator.class_log_field`` for ``compress_gpgpusim_log`` of the set."""
        self._check(lib().mpc_group_class_log_field(self._g, _class_log_field(field)))

    def class_from_member(self, member: Optional[int]) -> None:
        """The class of a line is member ``member``'s ``selected`` + 1 (``mpc_group_class_from_member``): for a VPC
        member 0 = uncompressed, k + 1 = module k's cluster; for a BDI member the state + 1.  ``None`` switches it off."""
        self._check(lib().mpc_group_class_from_member(self._g, -1 if member is None else int(member)))


def _snapshot_partial(partial) -> int:
    if partial not in SNAPSHOT_PARTIAL:
        raise ValueError(f"partial: 'skip' or 'zero', not {partial!r}")
    return SNAPSHOT_PARTIAL[partial]


def _snapshot_values(fn: str, unit_bytes, capacity, line_size):
    """The three values of a snapshot as the C ABI takes them (unsigned)."""
    unit_bytes, capacity, line_size = int(unit_bytes), int(capacity), int(line_size)
    if not (0 <= unit_bytes < 1 << 32 and 0 <= capacity < 1 << 64 and 0 <= line_size < 1 << 32):
        raise MpcError(-22, f"{fn}: unit_bytes, capacity and line_size are unsigned")
    return unit_bytes, capacity, line_size


def snapshot_check_values(unit_bytes: int = 32, capacity: int = 1 << 24, line_size: int = 0) -> None:
    """Raises ``MpcError`` with the message a ``Snapshot`` of these values, or its ``plan`` at ``line_size`` (0: none),
    would give (``mpc_snapshot_check_values``; no device)."""
    rc = lib().mpc_snapshot_check_values(*_snapshot_values("mpc_snapshot_check_values", unit_bytes, capacity, line_size))
    if rc != 0:
        raise MpcError(rc, (lib().mpc_snapshot_last_error(None) or b"").decode())


class Snapshot:
    """The memory image of a trace as data (``mpc_snapshot``, ``include/mpc_hip_snapshot.h``): per distinct unit
    address (``unit_bytes`` of 32, 64 or 128) the bytes of the latest unit added there, written out as address-aligned
    lines of ``line_size`` = 1, 2, 4 or 8 units in ascending address order and evaluated by any evaluator or set.
    ``partial="skip"`` emits the complete lines only, ``"zero"`` every touched line with its missing units as zeros.
    Device memory: 2 x (16 + ``unit_bytes``) bytes per unit of ``capacity`` rounded up to a power of two."""

    def __init__(self, unit_bytes: int = 32, capacity: int = 1 << 24, device: int = -1):
        self._s = C.c_void_p()
        u, cap, _ = _snapshot_values("mpc_snapshot_create", unit_bytes, capacity, 0)
        rc = lib().mpc_snapshot_create(u, cap, int(device), C.byref(self._s))
        if rc != 0:
            raise MpcError(rc, (lib().mpc_snapshot_last_error(None) or b"").decode())
        self.unit_bytes, self.capacity = u, cap

    def _check(self, rc: int) -> None:
        if rc != 0:
            raise MpcError(rc, (lib().mpc_snapshot_last_error(self._s if self._s else None) or b"").decode())

    def close(self) -> None:
        if self._s:
            lib().mpc_snapshot_destroy(self._s)
            self._s = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self) -> None:
        """Empties the snapshot; one that ran into its capacity takes units again."""
        self._check(lib().mpc_snapshot_reset(self._s))

    def add(self, units, addresses) -> None:
        """Host buffer [n, unit_bytes] uint8 with one uint64 address per unit; returns when the units are in."""
        units = _as_lines(units, self.unit_bytes)
        adr = _as_addresses(addresses, units.shape[0])
        self._check(lib().mpc_snapshot_add(self._s, units.ctypes.data, units.shape[0], adr.ctypes.data))

    def add_device(self, d_units: int, n: int, d_addresses: int, stream: int = 0) -> None:
        """Device-resident units and addresses (raw pointers); asynchronous on ``stream``."""
        self._check(lib().mpc_snapshot_add_device(self._s, d_units or None, int(n), d_addresses or None, stream or None))

    def add_gpgpusim_log(self, path: str) -> int:
        """Every evaluated record of a GPGPU-Sim ``.log`` at its ``mem_addr``, in file order; returns the units added."""
        done = C.c_uint64()
        self._check(lib().mpc_snapshot_add_gpgpusim_log(self._s, path.encode(), C.byref(done)))
        return int(done.value)

    def stats(self) -> Dict:
        t = np.zeros(MPC_SNAPSHOT_TABLE_LEN, dtype=np.uint64)
        self._check(lib().mpc_snapshot_stats(self._s, t.ctypes.data))
        v = [int(x) for x in t]
        return {"units": v[0], "distinct_units": v[1], "misaligned": v[2], "capacity": v[3], "unit_bytes": v[4]}

    def plan(self, line_size: int, partial: str = "skip") -> Dict:
        """What the snapshot holds at ``line_size``: ``touched``, ``complete`` and ``partial`` lines, the
        ``partial_units`` present in partial lines, the ``missing_units`` and ``n_out``, the lines that are emitted."""
        p = np.zeros(MPC_SNAPSHOT_TABLE_LEN, dtype=np.uint64)
        self._check(lib().mpc_snapshot_plan(self._s, int(line_size), _snapshot_partial(partial), p.ctypes.data))
        v = [int(x) for x in p]
        return {"touched": v[0], "complete": v[1], "partial": v[2], "partial_units": v[3], "missing_units": v[4], "n_out": v[5]}

    def write_lines(self, line_size: int, partial: str, first: int, n: int, d_lines: int, d_addresses: int = 0, d_presence: int = 0,
                    stream: int = 0) -> None:
        """Emitted lines [first, first + n) into caller-owned device memory (raw pointers, like ``compress_device``)."""
        self._check(lib().mpc_snapshot_write_lines(self._s, int(line_size), _snapshot_partial(partial), int(first), int(n), d_lines or None,
                                                   d_addresses or None, d_presence or None, stream or None))

    def read_lines(self, line_size: int, partial: str = "skip"):
        """``(lines uint8[n_out, line_size], addresses uint64[n_out], presence uint8[n_out])`` of all emitted lines."""
        n = self.plan(line_size, partial)["n_out"]
        lines = np.zeros((n, int(line_size)), dtype=np.uint8)
        adr = np.zeros(n, dtype=np.uint64)
        pres = np.zeros(n, dtype=np.uint8)
        self._check(lib().mpc_snapshot_read_lines(self._s, int(line_size), _snapshot_partial(partial), 0, n, lines.ctypes.data, adr.ctypes.data,
                                                  pres.ctypes.data))
        return lines, adr, pres

    def evaluate(self, evaluator_or_set, line_size: int, partial: str = "skip", by_presence: bool = False) -> int:
        """Feeds the emitted lines to an evaluator or an ``EvaluatorSet`` of ``line_size``-byte lines: with their addresses
        when image accounting is on there, with their presence masks as classes when ``by_presence`` is set and class
        accounting is on; waits.  Returns the number of lines fed."""
        e = evaluator_or_set
        if isinstance(e, EvaluatorSet):
            rc = lib().mpc_snapshot_evaluate_group(self._s, e._g, int(line_size), _snapshot_partial(partial), 1 if by_presence else 0)
        elif isinstance(e, _Evaluator):
            rc = lib().mpc_snapshot_evaluate(self._s, e._h, int(line_size), _snapshot_partial(partial), 1 if by_presence else 0)
        else:
            raise ValueError("evaluate takes an evaluator or an EvaluatorSet")
        self._check(rc)
        return self.plan(line_size, partial)["n_out"]


def size_sectors(bins, line_size: int, sector_bytes: int = 32) -> Dict:
    """The sectors of ``sector_bytes`` bytes that lines of ``line_size`` bytes with the size histogram ``bins`` occupy
    (``mpc_size_sectors``; no device): a line of s bits takes ``min(max(1, ceil(s / (8 * sector_bytes))),
    ceil(line_size / sector_bytes))``.  ``classes[c - 1]``: lines that occupy c sectors; ``total_sectors``; ``ratio`` =
    lines x classes / total sectors (0.0 without lines)."""
    bins = np.ascontiguousarray(bins, dtype=np.uint64)
    if bins.shape != (MPC_SIZE_BINS,):
        raise ValueError(f"a size histogram has {MPC_SIZE_BINS} bins")
    line_size, sector_bytes = int(line_size), int(sector_bytes)
    if line_size < 0 or sector_bytes < 0 or line_size >= 1 << 32 or sector_bytes >= 1 << 32:
        raise MpcError(-22, "mpc_size_sectors: line_size and sector_bytes are unsigned")
    n_classes = -(-line_size // sector_bytes) if sector_bytes > 0 else 0
    classes = np.zeros(max(n_classes, 1), dtype=np.uint64)
    total, ratio = C.c_uint64(), C.c_double()
    rc = lib().mpc_size_sectors(bins.ctypes.data, MPC_SIZE_BINS, line_size, sector_bytes, classes.ctypes.data, n_classes,
                                C.byref(total), C.byref(ratio))
    if rc != 0:
        raise MpcError(rc, "mpc_size_sectors: sector_bytes must be 1 .. line_size")
    return {"classes": classes[:n_classes].copy(), "total_sectors": int(total.value), "ratio": float(ratio.value)}


def sc2_sampling_lines(num_lines: int) -> int:
    """The reference driver's SC2 warm-up length for a trace of ``num_lines`` lines (``main.cpp:110-113``)."""
    return int(lib().mpc_sc2_sampling_lines(num_lines))


def sc2_code_lengths(symbols, freqs) -> np.ndarray:
    """The library's SC2 table builder (no device): code lengths of distinct ``symbols`` with warm-up ``freqs``, in
    input order; 0xFFFF for symbols outside the 1024 kept ones."""
    sym = np.ascontiguousarray(symbols, dtype=np.uint32)
    fr = np.ascontiguousarray(freqs, dtype=np.uint64)
    if sym.shape != fr.shape or sym.ndim != 1:
        raise ValueError("symbols and freqs must be 1-D arrays of one length")
    out = np.zeros(len(sym), dtype=np.uint16)
    rc = lib().mpc_sc2_code_lengths(sym.ctypes.data, fr.ctypes.data, len(sym), out.ctypes.data)
    if rc != 0:
        raise MpcError(rc, "mpc_sc2_code_lengths: empty input or repeated symbol")
    return out


def vpc_result_from_vector(v: np.ndarray, M: int, bins: int, L: int) -> Dict:
    K = M + 1
    # VPC.h:49-60: (double)original / (double)compressed after every line -- inf once lines of 0 bits are all there are
    # (a cluster whose id bits are 0: all-zero lines), 0 before the first line
    out = {**_totals(v, _ratio), "clusters": {}}
    for k in range(K):
        cnt, ob, cb, rl, sr, sr2 = (int(x) for x in v[3 + 6 * k: 3 + 6 * k + 6])
        out["clusters"][k - 1] = {
            "count": cnt, "original_bits": ob, "compressed_bits": cb,
            "comp_ratio": _ratio(ob, cb, cnt),
            "residue_lines": rl, "sum_r": sr, "sum_r2": sr2,
            # VPC.h:62-76: mean over lines of (sum over bytes / L)
            "mae": (float(sr) / float(L)) / float(rl) if rl else 0.0,
            "mse": (float(sr2) / float(L)) / float(rl) if rl else 0.0,
            "hist": v[3 + 6 * K + k * bins: 3 + 6 * K + (k + 1) * bins].copy(),
        }
    return out


def synth_fill(d_ptr: int, n_lines: int, line_size: int, kind: str, first_line: int = 0,
               seed: int = 12345, stream: int = 0) -> None:
    rc = lib().mpc_synth_fill(d_ptr, n_lines, line_size, SYNTH_KINDS[kind], first_line, seed, stream or None)
    if rc != 0:
        raise MpcError(rc, "mpc_synth_fill failed")


def read_bandwidth_probe(d_ptr: int, nbytes: int, stream: int = 0) -> None:
    rc = lib().mpc_read_bandwidth_probe(d_ptr, nbytes, stream or None)
    if rc != 0:
        raise MpcError(rc, "mpc_read_bandwidth_probe failed")
