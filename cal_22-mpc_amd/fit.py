"""Fit a DiffBase module's tables to a trace.

The reference's ``BaseIndexTable`` and ``DiffTable`` are arbitrary per-byte tables and it ships none; everything in
``configs.py`` is a hand-made guess.  This module picks both tables from two statistics that the library counts on the
GPU (``FitPairs`` and ``FitResidues`` of the package, ``mpc_create_fit_pairs`` / ``mpc_create_fit_residues`` in
``include/mpc_hip.h``):

``P[i][j][k]``  lines whose residue ``(line[i] - line[j]) & 255`` has bit length k (0 for 0, else 1..8)
``V[i][v]``     lines whose residue ``(line[i] - line[base[i]]) & 255`` is v

The fitting functions are pure functions on numpy tables and need neither the library nor a device; ``fit_config`` runs
the two passes over a trace and evaluates the result.

    python cal_22-mpc_amd/fit.py --trace t.npy [--lines N] [--with mpc] [--windowed] [--max-distance D] -o cfg.json
"""
from __future__ import annotations

import importlib
import json
import os
import sys
from typing import Dict, List, Optional

import numpy as np

if __package__:
    from . import configs
else:      # run as a script: the directory's name is not an identifier
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    configs = importlib.import_module(os.path.basename(os.path.dirname(os.path.abspath(__file__))) + ".configs")

BITLEN8 = np.array([int(v).bit_length() for v in range(256)], dtype=np.int64)      # bitlen8(v), v = 0..255


def _package():
    return importlib.import_module(__package__ or os.path.basename(os.path.dirname(os.path.abspath(__file__))))


def fit_base_table(P, windowed: bool = False, max_distance: Optional[int] = None) -> List[int]:
    """``BaseIndexTable`` from the pair table ``P`` (``[L, L, 9]``).  ``base[0] = 0``.  Byte i >= 1 is predicted from an
    earlier byte j < i (the table must be decodable from root 0: no byte predicts itself or a later byte), with
    ``j >= i - max_distance`` when that is given and ``j >= 4 (i // 4) - 4`` when ``windowed`` (the own or the previous
    32-bit word: the module then runs the unrolled kernel forms without the gather).  The candidate with the smallest
    ``sum_k k P[i][j][k]`` wins; ties go to the largest j."""
    P = np.asarray(P)
    L = P.shape[0]
    if P.shape != (L, L, 9):
        raise ValueError("P is [L, L, 9]")
    if max_distance is not None and max_distance < 1:
        raise ValueError("max_distance is at least 1")
    cost = [[sum(k * int(P[i, j, k]) for k in range(9)) for j in range(L)] for i in range(L)]      # Python integers: no overflow
    base = [0] * L
    for i in range(1, L):
        lo = 0
        if max_distance is not None:
            lo = max(lo, i - int(max_distance))
        if windowed:
            lo = max(lo, 4 * (i // 4) - 4)
        best = lo
        for j in range(lo, i):
            if cost[i][j] <= cost[i][best]:
                best = j
        base[i] = best
    return base


def fit_diff_table(V) -> List[int]:
    """``DiffTable`` from the residue histogram ``V`` (``[L, 256]``) of the chosen base table.  ``diff[0] = 0``.  For
    byte i >= 1 the constant c in 0..255 with the smallest ``sum_v V[i][v] bitlen8((v - c) & 255)``; 0 when it is among
    the minima, else the smallest such c."""
    V = np.asarray(V)
    L = V.shape[0]
    if V.shape != (L, 256):
        raise ValueError("V is [L, 256]")
    u = np.arange(256)
    bits = BITLEN8[(u[None, :] - u[:, None]) & 255]      # [c][v] = bitlen8((v - c) & 255)
    diff = [0] * L
    for i in range(1, L):
        row = [int(x) for x in V[i]]
        # (int64 holds 8 x the line count of any trace that fits a disk; Python integers beyond that)
        costs = (bits @ np.array(row, dtype=np.int64 if sum(row) < 1 << 59 else object)).tolist()
        least = min(costs)
        diff[i] = 0 if costs[0] == least else costs.index(least)
    return diff


def fit_module(L: int, base, diff, consecutive_xor: bool = True) -> Dict:
    """The fitted DiffBase module (root 0, identity plane-major scan)."""
    return configs.diff_base(L, list(base), list(diff), 0, consecutive_xor)


MODEL_SETS = ("none", "mpc", "probe")


def model_set(L: int, with_models: str = "none") -> List[Dict]:
    """The modules a fitted one is appended to: AllZero and AllWordSame alone, or those of ``mpc_config`` / ``probe_config``."""
    if with_models == "none":
        return [{"name": "AllZero"}, {"name": "AllWordSame"}]
    if with_models not in MODEL_SETS:
        raise ValueError(f"with_models is one of {MODEL_SETS}")
    cfg = configs.mpc_config(L) if with_models == "mpc" else configs.probe_config(L)
    return [cfg["modules"][str(i)] for i in range(cfg["overview"]["num_modules"])]


def _ratio(ev) -> float:
    v = ev.stats_vector()
    return float(v[1]) / float(v[2]) if v[2] else (float("inf") if v[0] else 0.0)


def fit_config(source, line_size: Optional[int] = None, lines: Optional[int] = None, with_models: str = "none",
               windowed: bool = False, max_distance: Optional[int] = None, device: int = -1) -> Dict:
    """Fit one DiffBase module to a trace and evaluate it.  ``source``: a ``[n, L]`` uint8 array, a ``.npy`` path or a
    GPGPU-Sim ``.log`` path (the line size comes from the file); ``lines``: only the first so many lines (arrays and
    ``.npy`` files).  One pass with ``FitPairs``, ``fit_base_table``, one pass with ``FitResidues``, ``fit_diff_table``;
    the module is appended to the model set ``with_models``; the result and the model set without it are evaluated on
    the same lines.  Returns ``config``, ``base``, ``diff``, ``lines``, ``ratio_fitted``, ``ratio_without`` and, from
    ``describe_config`` and the fitted handle, ``kernel_form`` and ``path_reason``."""
    mpc = _package()
    if isinstance(source, (str, os.PathLike)):
        path = os.fspath(source)
        if path.endswith(".log"):
            L = mpc.gpgpusim_log_line_size(path)

            def feed(ev):
                ev.compress_gpgpusim_log(path)
        else:
            rows, cols = mpc.C.c_uint64(), mpc.C.c_uint64()
            rc = mpc.lib().mpc_npy_shape(path.encode(), mpc.C.byref(rows), mpc.C.byref(cols))
            if rc != 0:
                raise mpc.MpcError(rc, (mpc.lib().mpc_last_error(None) or b"").decode())
            L = int(cols.value)

            def feed(ev):
                ev.compress_npy(path, 0, (1 << 62) if lines is None else int(lines), skip_last_row=False)
        if line_size is not None and int(line_size) != L:
            raise ValueError(f"{path} has {L}-byte lines, not {line_size}")
    else:
        arr = np.ascontiguousarray(source, dtype=np.uint8)
        if arr.ndim != 2:
            raise ValueError("source is a [n, L] uint8 array or a path")
        if lines is not None:
            arr = arr[:int(lines)]
        L = arr.shape[1]
        if line_size is not None and int(line_size) != L:
            raise ValueError(f"the array has {L}-byte lines, not {line_size}")

        def feed(ev):
            ev.compress_lines(arr, False, False)

    pairs = mpc.FitPairs(L, device)
    feed(pairs)
    n = pairs.lines()
    base = fit_base_table(pairs.table(), windowed, max_distance)
    pairs.close()
    res = mpc.FitResidues(L, base, device)
    feed(res)
    diff = fit_diff_table(res.table())
    res.close()

    others = model_set(L, with_models)
    cfg = configs.make_config(L, others + [fit_module(L, base, diff)])
    fitted, without = mpc.VPC(cfg, device), mpc.VPC(configs.make_config(L, others), device)
    feed(fitted)
    feed(without)
    described = mpc.describe_config(cfg)
    out = {"config": cfg, "base": base, "diff": diff, "lines": n, "ratio_fitted": _ratio(fitted), "ratio_without": _ratio(without),
           "kernel_form": fitted.kernel_form, "path_reason": fitted.path_reason or described.get("why_generic", "")}
    fitted.close()
    without.close()
    return out


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser(description="fit a DiffBase module to a trace and write the VPC configuration")
    ap.add_argument("--trace", required=True, help="a [n, L] uint8 .npy file or a GPGPU-Sim .log trace")
    ap.add_argument("--lines", type=int, default=None, help="only the first N lines (.npy)")
    ap.add_argument("--with", dest="with_models", default="none", choices=MODEL_SETS, help="the model set the fitted module is appended to")
    ap.add_argument("--windowed", action="store_true", help="base bytes from the own or the previous 32-bit word only")
    ap.add_argument("--max-distance", type=int, default=None, help="base bytes at most D bytes back")
    ap.add_argument("--device", type=int, default=-1)
    ap.add_argument("-o", "--output", required=True)
    a = ap.parse_args()
    r = fit_config(a.trace, lines=a.lines, with_models=a.with_models, windowed=a.windowed, max_distance=a.max_distance, device=a.device)
    configs.write_config(r.pop("config"), a.output)
    print(json.dumps(r))
