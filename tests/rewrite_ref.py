"""The rewrite table of include/mpc_hip_rewrite.h, restated twice from its definitions: a line at position p with
address a and size s has key a // L; with granule_bytes g and G = ceil(L / g) the class of a size is
c(s) = min(max(1, ceil(s / (8 g))), G); the observations at a key, in ascending p, have sizes s_1 .. s_m; then
first[c(s_1)] += 1, for j >= 2 trans[c(s_{j-1})][c(s_j)] += 1 and equal_bits += (s_j == s_{j-1}), and the key's state is
latest = s_m, peak = max s_j, count = m.  `rewrite_table_loop` walks a dict line by line; `rewrite_table` is numpy
over a stable argsort and neighbour compares.  Everything is integers; the tests compare for equality."""
import numpy as np

MAX_CLASSES = 32
TABLE_LEN = 144 + MAX_CLASSES * MAX_CLASSES
FIRST, LATEST, PEAK, COUNT, TRANS = 16, 48, 80, 112, 144


def ceil_div(a, b):
    return -(-a // b)


def slots_of(capacity):
    """The smallest power of two >= 2 x capacity and at least 2."""
    slots = 2
    while slots < 2 * int(capacity):
        slots *= 2
    return slots


def classes_of(L, g):
    return ceil_div(int(L), int(g))


def class_of(s, L, g):
    """c(s), 1 .. G, of one size."""
    return min(max(1, ceil_div(int(s), 8 * int(g))), classes_of(L, g))


def class_of_array(s, L, g):
    s = np.asarray(s).astype(np.int64)
    return np.minimum(np.maximum(1, -(-s // (8 * int(g)))), classes_of(L, g))


def rewrite_table_loop(addresses, sizes, L, g, capacity=0):
    """uint64[TABLE_LEN] of these lines, in trace order: a dict of key -> [latest, peak, count]."""
    L, g = int(L), int(g)
    G = classes_of(L, g)
    assert 1 <= G <= MAX_CLASSES
    t = [0] * TABLE_LEN
    state = {}
    for a, s in zip([int(x) for x in np.asarray(addresses, dtype=np.uint64).reshape(-1)], [int(x) for x in np.asarray(sizes).reshape(-1)]):
        t[0] += 1
        t[1] += s
        t[3] += 1 if a % L else 0
        k = a // L
        if k not in state:
            t[FIRST + class_of(s, L, g) - 1] += 1
            state[k] = [s, s, 1]
            continue
        old = state[k]
        c_old, c_new = class_of(old[0], L, g), class_of(s, L, g)
        t[TRANS + (c_old - 1) * MAX_CLASSES + (c_new - 1)] += 1
        t[4] += 1
        t[5] += 1 if c_new > c_old else 0
        t[6] += 1 if c_new < c_old else 0
        t[7] += 1 if s == old[0] else 0
        state[k] = [s, max(old[1], s), min(old[2] + 1, (1 << 32) - 1)]
    t[2] = len(state)
    for latest, peak, count in state.values():
        cl, cp = class_of(latest, L, g), class_of(peak, L, g)
        t[8] += cl
        t[9] += cp
        t[10] += latest
        t[11] += peak
        t[LATEST + cl - 1] += 1
        t[PEAK + cp - 1] += 1
        t[COUNT + count.bit_length() - 1] += 1
    t[12], t[13], t[14] = g, int(capacity), G
    return np.array(t, dtype=np.uint64)


def rewrite_table(addresses, sizes, L, g, capacity=0):
    """The same, vectorised: a stable argsort of the keys keeps each key's observations in trace order."""
    L, g = int(L), int(g)
    G = classes_of(L, g)
    assert 1 <= G <= MAX_CLASSES
    addresses = np.asarray(addresses, dtype=np.uint64).reshape(-1)
    sizes = np.asarray(sizes).astype(np.int64).reshape(-1)
    assert addresses.shape == sizes.shape
    t = np.zeros(TABLE_LEN, np.uint64)
    t[12], t[13], t[14] = g, int(capacity), G
    n = addresses.size
    if n == 0:
        return t
    keys = addresses // np.uint64(L)
    order = np.argsort(keys, kind="stable")
    k, s = keys[order], sizes[order]
    c = class_of_array(s, L, g)
    head = np.ones(n, bool)
    head[1:] = k[1:] != k[:-1]
    tail = np.ones(n, bool)
    tail[:-1] = head[1:]
    inner = ~head                                                  # elements whose left neighbour has their key
    starts = np.nonzero(head)[0]
    t[0] = n
    t[1] = int(sizes.sum())
    t[2] = starts.size
    t[3] = int((addresses % np.uint64(L) != 0).sum())
    old, new = c[:-1][inner[1:]], c[1:][inner[1:]]
    trans = np.zeros((MAX_CLASSES, MAX_CLASSES), np.int64)
    np.add.at(trans, (old - 1, new - 1), 1)
    t[TRANS:] = trans.reshape(-1).astype(np.uint64)
    t[4] = int(inner.sum())
    t[5] = int((new > old).sum())
    t[6] = int((new < old).sum())
    t[7] = int((s[1:][inner[1:]] == s[:-1][inner[1:]]).sum())
    latest = s[tail]
    peak = np.maximum.reduceat(s, starts)
    count = np.diff(np.append(starts, n))
    cl, cp = class_of_array(latest, L, g), class_of_array(peak, L, g)
    t[8], t[9], t[10], t[11] = int(cl.sum()), int(cp.sum()), int(latest.sum()), int(peak.sum())
    t[FIRST:FIRST + MAX_CLASSES] = np.bincount(c[head] - 1, minlength=MAX_CLASSES).astype(np.uint64)
    t[LATEST:LATEST + MAX_CLASSES] = np.bincount(cl - 1, minlength=MAX_CLASSES).astype(np.uint64)
    t[PEAK:PEAK + MAX_CLASSES] = np.bincount(cp - 1, minlength=MAX_CLASSES).astype(np.uint64)
    log2 = np.frexp(count.astype(np.float64))[1].astype(np.int64) - 1      # the exponent: exact, counts are far below 2^53
    t[COUNT:COUNT + 32] = np.bincount(log2, minlength=32).astype(np.uint64)
    return t


def ratios(table, L):
    """(overflow_rate, image_granule_ratio, peak_granule_ratio, traffic_ratio), 0.0 where the divisor is 0."""
    t = [int(x) for x in np.asarray(table).reshape(-1)[:16]]
    G = t[14]
    return (t[5] / t[4] if t[4] else 0.0, t[2] * G / t[8] if t[8] else 0.0, t[2] * G / t[9] if t[9] else 0.0, t[0] * 8 * L / t[1] if t[1] else 0.0)


# ---- the text of comp::RewriteReport (host/RewriteReport.cpp): what <stem>_results_rewrites.csv holds ----
CSV_HEADER = ("Workload,Line Size,Granule Bytes,Lines,Distinct Lines,Rewrites,Grows,Shrinks,Equal Bits,Latest Granules,Peak Granules,"
              "Image Granule Ratio,Peak Granule Ratio,Transitions,\n")


def fmt_double(x: float) -> str:
    """The host code's text of a double (mpctext::num): shortest round-trip, no trailing ".0"."""
    r = repr(float(x))
    return r[:-2] if r.endswith(".0") else r


def csv_row(workload, t, L):
    G = int(t[14])
    parts = [f"0>{c}:{int(t[FIRST + c - 1])}" for c in range(1, G + 1) if int(t[FIRST + c - 1])]
    parts += [f"{o}>{c}:{int(t[TRANS + (o - 1) * MAX_CLASSES + c - 1])}" for o in range(1, G + 1) for c in range(1, G + 1)
              if int(t[TRANS + (o - 1) * MAX_CLASSES + c - 1])]
    _, image, peak, _ = ratios(t, L)
    return (f"{workload},{L},{int(t[12])},{int(t[0])},{int(t[2])},{int(t[4])},{int(t[5])},{int(t[6])},{int(t[7])},{int(t[8])},{int(t[9])},"
            f"{fmt_double(image)},{fmt_double(peak)},{';'.join(parts)},\n")


def same_table(tag, got, want):
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    assert got.dtype == np.uint64 and want.dtype == np.uint64 and got.shape == want.shape == (TABLE_LEN,), (tag, got.dtype, got.shape)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{tag}: {bad.size} entries differ, first {[(int(i), int(got[i]), int(want[i])) for i in bad[:6]]}"
