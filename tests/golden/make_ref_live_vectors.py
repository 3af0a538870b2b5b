#!/usr/bin/env python3
"""Generate tests/golden/ref_live_vectors.npz: the outputs of the REFERENCE's own stage classes
(oracle/_ref/libmpc_refstages.so, compiled unmodified by oracle/Makefile) for the seeded inputs of
test_oracle.py's two "live reference" tests -- scanned bit-plane arrays and common-encoder sizes of
the probe configuration's prediction modules, and predictions and scanned arrays of WeightBase
tables with odd and extreme weights.  With them stored, those tests need no reference build.

Run where the reference tree is mounted:
    make -C oracle _ref && python tests/golden/make_ref_live_vectors.py

The output holds the reference's outputs and a checksum of the (regenerable, seeded) inputs only.
Importing this file only defines the case generators; main() is what needs the reference build.
"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
FIXTURE = os.path.join(ROOT, "tests", "golden", "ref_live_vectors.npz")


class Case:
    """One stage input: an oracle OModule, the same tables as the arrays ref_stage_harness.cpp takes, one line."""

    def __init__(self, L, m, base, weight, diff, rows, cols, line):
        self.L, self.m, self.line = L, m, np.ascontiguousarray(line, dtype=np.uint8)
        self.base, self.weight, self.diff, self.rows, self.cols = base, weight, diff, rows, cols

    def ref_args(self):
        return (self.m.pred_kind, self.m.root, self.L, self.base.ctypes.data, self.weight.ctypes.data, self.diff.ctypes.data)

    def digest_into(self, h):
        m = self.m
        h.update(np.array([self.L, m.pred_kind, m.root, m.consecutive_xor, m.table_size], dtype="<i4").tobytes())
        for a in (self.base, self.weight, self.diff, self.rows, self.cols, self.line):
            h.update(a.tobytes())


def _tables(m, L, n):
    return (np.array(list(m.base)[:L], dtype=np.int32), np.array(list(m.weight)[:L], dtype=np.float32),
            np.array(list(m.diff)[:L], dtype=np.int32), np.array(list(m.rows)[:n], dtype=np.int32),
            np.array(list(m.cols)[:n], dtype=np.int32))


def stage_cases(oracle, configs):
    """Prediction modules 2..5 of the probe configuration at 32 / 64 / 128 B, 300 lines each: random, sparse,
    integer ramps and fp32 sine."""
    rng = np.random.default_rng(99)
    out = []
    for L in (32, 64, 128):
        oc = oracle.config_from_json(configs.probe_config(L))
        for mi in range(2, 6):
            m = oc.modules[mi]
            base, weight, diff, rows, cols = _tables(m, L, m.table_size)
            if m.pred_kind != 0:
                weight[:] = 1.0
            for trial in range(300):
                kind = trial % 4
                if kind == 0:
                    line = rng.integers(0, 256, L, dtype=np.uint8)
                elif kind == 1:
                    line = np.zeros(L, np.uint8)
                    line[rng.integers(0, L, 3)] = rng.integers(0, 256, 3)
                elif kind == 2:
                    w = (rng.integers(0, 1000) + np.arange(L // 4) * rng.integers(0, 5)).astype("<u4")
                    line = w.view(np.uint8).copy()
                else:
                    t = rng.integers(0, 1 << 20) + np.arange(L // 4)
                    line = np.sin(2 * np.pi * t / 1024).astype("<f4").view(np.uint8).copy()
                out.append(Case(L, m, base, weight, diff, rows, cols, line))
    return out


def odd_weight_cases(oracle):
    """WeightBase tables with weights that are not powers of two and extreme weights, 40 tables per line size
    (random or i-4 bases, zero or random roots, with and without the consecutive XOR), 25 lines each."""
    rng = np.random.default_rng(4321)
    weights = [0.3, 0.7, 3.0, 5.5, 300.0, 0.001, 1.0, 0.5, 1.5, 0.99, 1.99, 2.0, 4.01, 0.26, 0.24, 127.9,
               128.0, 0.0079, 0.0078125, 255.0, 0.126, 1e-6, 1e6]
    out = []
    for L in (32, 64, 128):
        for trial in range(40):
            m = oracle.OModule()
            m.kind, m.pred_kind = oracle.KIND_PREDCOMP, 0
            m.root = int(rng.integers(0, L)) if trial % 2 else 0
            m.consecutive_xor = trial % 3 != 0
            for j in range(L):
                m.base[j] = int(rng.integers(0, L)) if trial % 4 else max(j - 4, 0)
                m.weight[j] = weights[int(rng.integers(0, len(weights)))]
            m.table_size = 8 * L
            for j in range(8 * L):
                m.rows[j], m.cols[j] = j // L, j % L
            base, weight, _, rows, cols = _tables(m, L, 8 * L)
            diff = np.zeros(L, dtype=np.int32)
            for k in range(25):
                line = rng.integers(0, 256, L, dtype=np.uint8) if k % 2 else \
                    (rng.integers(0, 256) + np.arange(L) * rng.integers(0, 3)).astype(np.uint8)
                out.append(Case(L, m, base, weight, diff, rows, cols, line))
    return out


def digest(cases):
    h = hashlib.sha256()
    for c in cases:
        c.digest_into(h)
    return h.hexdigest()


def ref_scanned(R, c):
    sc = np.zeros(8 * c.L // 16, np.uint16)
    R.ref_scanned(*c.ref_args(), c.m.consecutive_xor, c.m.table_size, c.rows.ctypes.data, c.cols.ctypes.data,
                  c.line.ctypes.data, sc.ctypes.data)
    return sc


def ref_predict(R, c):
    p = np.zeros(c.L, np.uint8)
    R.ref_predict(*c.ref_args(), c.line.ctypes.data, p.ctypes.data)
    return p


def split(flat, cases, per_line):
    """The per-case slices of a concatenated fixture array (per_line(L) entries per case)."""
    out, o = [], 0
    for c in cases:
        out.append(flat[o:o + per_line(c.L)])
        o += per_line(c.L)
    assert o == len(flat)
    return out


def main():
    sys.path.insert(0, ROOT)
    import importlib
    from oracle import oracle as O
    configs = importlib.import_module("cal_22-mpc_amd.configs")
    R = O.ref_lib()
    if R is None:
        raise SystemExit("oracle/_ref is not built (make -C oracle _ref)")
    st, odd = stage_cases(O, configs), odd_weight_cases(O)
    st_sc = [ref_scanned(R, c) for c in st]
    np.savez_compressed(
        FIXTURE,
        provenance=np.array("outputs of the reference's own PredictorModule/ResidueModule/XORModule/ScanModule/FPCModule "
                            "classes (compiled unmodified, g++ -O3) driven by oracle/ref_stage_harness.cpp; generated by "
                            "tests/golden/make_ref_live_vectors.py"),
        stage_inputs_sha256=np.array(digest(st)),
        stage_scanned=np.concatenate(st_sc),
        stage_fpc=np.array([R.ref_fpc_size(sc.ctypes.data, len(sc)) for sc in st_sc], dtype=np.int32),
        odd_inputs_sha256=np.array(digest(odd)),
        odd_pred=np.concatenate([ref_predict(R, c) for c in odd]),
        odd_scanned=np.concatenate([ref_scanned(R, c) for c in odd]))
    print(FIXTURE, len(st), "stage cases,", len(odd), "odd-weight cases,", os.path.getsize(FIXTURE), "bytes")


if __name__ == "__main__":
    main()
