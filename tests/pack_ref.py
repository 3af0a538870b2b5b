"""The pack table of include/mpc_hip_pack.h in numpy, straight from its definition: block b is lines [b N, (b + 1) N) of
the per-line sizes in trace order; a closed block of `payload` bits occupies min(max(1, ceil((payload + header_bits) /
(8 sector_bytes))), S_B) sectors, S_B = ceil(N L / sector_bytes); the lines behind the last closed block are the open
block.  Everything is integers; the tests compare for equality."""
import numpy as np

MAX_SECTORS = 1024
TABLE_LEN = 8 + MAX_SECTORS


def ceil_div(a, b):
    return -(-a // b)


def block_sectors(N, L, sector_bytes):
    """S_B: the sectors an uncompressed block occupies."""
    return ceil_div(int(N) * int(L), int(sector_bytes))


def payloads(sizes, N):
    """The payload bits of the closed blocks, and (open lines, open bits)."""
    sizes = np.asarray(sizes).astype(np.int64).reshape(-1)
    N = int(N)
    nb = sizes.size // N
    closed = sizes[:nb * N].reshape(nb, N).sum(axis=1) if nb else np.zeros(0, np.int64)
    return closed, (sizes.size - nb * N, int(sizes[nb * N:].sum()))


def sectors_of(bits, sector_bytes, cap):
    """min(max(1, ceil(bits / (8 sector_bytes))), cap), elementwise."""
    bits = np.asarray(bits, dtype=np.int64)
    return np.minimum(np.maximum(1, -(-bits // (8 * int(sector_bytes)))), int(cap))


def pack_table(sizes, N, L, sector_bytes, header_bits=0):
    """uint64[TABLE_LEN] of these sizes, counted from line 0."""
    S = block_sectors(N, L, sector_bytes)
    assert 1 <= S <= MAX_SECTORS
    closed, (open_lines, open_bits) = payloads(sizes, N)
    sec = sectors_of(closed + int(header_bits), sector_bytes, S)
    t = np.zeros(TABLE_LEN, np.uint64)
    t[0] = closed.size
    t[1] = int(closed.sum())
    t[2] = int(sec.sum())
    t[3] = open_lines
    t[4] = open_bits
    t[5], t[6], t[7] = int(N), int(sector_bytes), int(header_bits)
    t[8:8 + S] = np.bincount(sec, minlength=S + 1)[1:].astype(np.uint64)
    return t


def pack_table_loop(sizes, N, L, sector_bytes, header_bits=0):
    """The same by a Python loop over the lines, one block at a time (the cross-check of pack_table)."""
    S = ceil_div(N * L, sector_bytes)
    t = [0] * TABLE_LEN
    lines, bits = 0, 0
    for s in [int(x) for x in np.asarray(sizes).reshape(-1)]:
        lines += 1
        bits += s
        if lines == N:
            k = min(max(1, ceil_div(bits + header_bits, 8 * sector_bytes)), S)
            t[0] += 1
            t[1] += bits
            t[2] += k
            t[8 + k - 1] += 1
            lines, bits = 0, 0
    t[3], t[4], t[5], t[6], t[7] = lines, bits, N, sector_bytes, header_bits
    return np.array(t, dtype=np.uint64)


def tail(table, L):
    """(tail_sectors, tail_cap): the open block of k lines closed as a short block; (0, 0) for k == 0."""
    k, bits, sb, hb = int(table[3]), int(table[4]), int(table[6]), int(table[7])
    if k == 0:
        return 0, 0
    cap = ceil_div(k * int(L), sb)
    return int(sectors_of(bits + hb, sb, cap)), cap


def merge(a, b):
    """Table a += shard b, b's open block taken over.  ValueError for other values or two open blocks."""
    a, b = np.asarray(a, np.uint64), np.asarray(b, np.uint64)
    if a[5:8].tolist() != b[5:8].tolist():
        raise ValueError("the tables count with different values")
    if int(a[3]) and int(b[3]):
        raise ValueError("both sides have an open block")
    out = a.copy()
    out[0:3] += b[0:3]
    out[8:] += b[8:]
    if int(b[3]):
        out[3:5] = b[3:5]
    return out


def sector_ratio(table, L, close_tail=True):
    S = block_sectors(table[5], L, table[6])
    ts, tc = tail(table, L) if close_tail else (0, 0)
    total = int(table[2]) + ts
    return (int(table[0]) * S + tc) / total if total else 0.0


def boundary_headers(sizes, N, L, sector_bytes):
    """Two header_bits values chosen from the reference sizes: with the first some closed block has exactly
    8 sector_bytes k bits (0 < k < S_B, so that neither the floor of 1 nor the cap hides it), with the second -- one
    more -- the same block has that value + 1.  None when no closed block lies in that range."""
    S = block_sectors(N, L, sector_bytes)
    sbits = 8 * int(sector_bytes)
    closed, _ = payloads(sizes, N)
    for p in closed.tolist():
        hb = (-p) % sbits
        k = (p + hb) // sbits
        if 0 < k < S and hb + 1 <= 65535:
            return hb, hb + 1
    return None


def coverage(sizes, N, L, sector_bytes, header_bits):
    """What the closed blocks of these sizes cover: the distinct sector counts, whether a block reaches the cap with an
    uncapped count above it, and whether a block has exactly 8 sector_bytes k bits or that + 1 (k >= 1)."""
    S = block_sectors(N, L, sector_bytes)
    sbits = 8 * int(sector_bytes)
    closed, _ = payloads(sizes, N)
    bits = closed + int(header_bits)
    sec = sectors_of(bits, sector_bytes, S)
    uncapped = np.maximum(1, -(-bits // sbits))
    return {"counts": set(sec.tolist()), "capped_above": bool((uncapped > S).any()),
            "exact": bool(((bits % sbits == 0) & (bits >= sbits)).any()), "plus_one": bool(((bits % sbits == 1) & (bits > sbits)).any())}


def same_table(tag, got, want):
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    assert got.dtype == np.uint64 and want.dtype == np.uint64 and got.shape == want.shape == (TABLE_LEN,), (tag, got.dtype, got.shape)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{tag}: {bad.size} entries differ, first {[(int(i), int(got[i]), int(want[i])) for i in bad[:6]]}"
