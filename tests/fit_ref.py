"""The reference of the two Fit analyses (include/mpc_hip.h: mpc_create_fit_pairs, mpc_create_fit_residues), straight
from their definitions in numpy, and the two traces the fit is judged on.  No test_ prefix: shared by
tests/test_fit_cpu.py, tests/test_fit_gpu.py and tests/test_fit_large_gpu.py."""
import numpy as np

BITLEN8 = np.array([int(v).bit_length() for v in range(256)], dtype=np.int64)      # 0 for 0, else 1..8


def pair_table(lines):
    """uint64[L, L, 9]: P[i][j][k] = lines with bitlen8((line[i] - line[j]) & 255) == k."""
    lines = np.ascontiguousarray(lines, dtype=np.uint8)
    n, L = lines.shape
    P = np.zeros((L, L, 9), dtype=np.uint64)
    for i in range(L):
        k = BITLEN8[(lines[:, i:i + 1] - lines) & 255]      # uint8 arithmetic wraps mod 256; [n, L]
        for j in range(L):
            P[i, j] = np.bincount(k[:, j], minlength=9)
    return P


def residue_table(lines, base):
    """uint64[L, 256]: V[i][v] = lines with (line[i] - line[base[i]]) & 255 == v."""
    lines = np.ascontiguousarray(lines, dtype=np.uint8)
    n, L = lines.shape
    assert len(base) == L and all(0 <= int(b) < L for b in base)
    r = (lines - lines[:, [int(b) for b in base]]) & 255
    V = np.zeros((L, 256), dtype=np.uint64)
    for i in range(L):
        V[i] = np.bincount(r[:, i], minlength=256)
    return V


def pairs_vector(lines):
    """The statistics vector of a FitPairs handle that was fed `lines`."""
    return np.concatenate([np.array([len(lines), 0, 0], dtype=np.uint64), pair_table(lines).reshape(-1)])


def residues_vector(lines, base):
    return np.concatenate([np.array([len(lines), 0, 0], dtype=np.uint64), residue_table(lines, base).reshape(-1)])


# ---- traces ------------------------------------------------------------------------------------------------------------
def records16(n, L, seed):
    """Lines of L / 16 records of 16 bytes {u32 counter, f32, u64 pointer}: record r of a line holds
    a0 + 3 r + {0, 1}, float32(100 g0 + 0.01 g_r) and 0x7f3a5c000000 + 8 u0 + 48 r; a0 (a random u32), g0 (normal) and
    u0 < 2^20 are drawn per line, the {0, 1} and g_r (normal) per record."""
    rng = np.random.default_rng(seed)
    R = L // 16
    r = np.arange(R, dtype=np.uint64)[None, :]
    a0 = rng.integers(0, 1 << 32, size=(n, 1), dtype=np.uint64)
    counter = ((a0 + 3 * r + rng.integers(0, 2, size=(n, R), dtype=np.uint64)) & 0xffffffff).astype("<u4")
    value = (100.0 * rng.standard_normal((n, 1)) + 0.01 * rng.standard_normal((n, R))).astype("<f4")
    u0 = rng.integers(0, 1 << 20, size=(n, 1), dtype=np.uint64)
    pointer = (np.uint64(0x7f3a5c000000) + 8 * u0 + 48 * r).astype("<u8")
    rec = np.zeros((n, R, 16), dtype=np.uint8)
    rec[:, :, 0:4] = counter[:, :, None].view(np.uint8).reshape(n, R, 4)
    rec[:, :, 4:8] = value[:, :, None].view(np.uint8).reshape(n, R, 4)
    rec[:, :, 8:16] = pointer[:, :, None].view(np.uint8).reshape(n, R, 8)
    return np.ascontiguousarray(rec.reshape(n, L))


def stride_u32(n, L, seed):
    """Lines of L / 4 little-endian u32: word w is s + 5 w, s < 2^30 drawn per line."""
    rng = np.random.default_rng(seed)
    s = rng.integers(0, 1 << 30, size=(n, 1), dtype=np.uint64)
    words = (s + 5 * np.arange(L // 4, dtype=np.uint64)[None, :]).astype("<u4")
    return np.ascontiguousarray(words.view(np.uint8).reshape(n, L))


TRACES = {"records16": records16, "stride_u32": stride_u32}
