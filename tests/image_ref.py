"""The image table of include/mpc_hip_image.h in numpy, straight from its definitions: a line at position p with address
a and size s has key a // L; the image maps each key to the size of the line with the largest p among the lines of
that key; block b holds the keys [b N, (b + 1) N); a touched block with T keys in the image and `payload` = the sum of
their latest sizes occupies min(max(1, ceil((payload + header_bits) / (8 sector_bytes))), ceil(T L / sector_bytes))
sectors.  Everything is integers; the tests compare for equality."""
import numpy as np

MAX_SECTORS = 1024
TABLE_LEN = 16 + MAX_SECTORS


def ceil_div(a, b):
    return -(-a // b)


def slots_of(capacity):
    """The smallest power of two >= 2 x capacity and at least 2."""
    slots = 2
    while slots < 2 * int(capacity):
        slots *= 2
    return slots


def latest(addresses, sizes, L):
    """(keys ascending, the latest size of each): np.unique on the reversed keys finds the last occurrence per key."""
    keys = np.asarray(addresses, dtype=np.uint64).reshape(-1) // np.uint64(L)
    sizes = np.asarray(sizes).astype(np.int64).reshape(-1)
    assert keys.shape == sizes.shape
    uniq, first_in_reversed = np.unique(keys[::-1], return_index=True)
    return uniq, sizes[::-1][first_in_reversed]


def blocks_of(addresses, sizes, N, L):
    """(block numbers ascending, T of each, payload of each) of the image of these lines."""
    keys, last = latest(addresses, sizes, L)
    blocks, inverse, T = np.unique(keys // np.uint64(N), return_inverse=True, return_counts=True)
    payload = np.zeros(blocks.size, np.int64)
    np.add.at(payload, inverse.reshape(-1), last)
    return blocks, T.astype(np.int64), payload


def sectors_of(T, payload, L, sector_bytes, header_bits):
    """(sectors, caps) of touched blocks, elementwise."""
    caps = -(-(np.asarray(T, np.int64) * int(L)) // int(sector_bytes))
    sec = np.minimum(np.maximum(1, -(-(np.asarray(payload, np.int64) + int(header_bits)) // (8 * int(sector_bytes)))), caps)
    return sec, caps


def image_table(addresses, sizes, N, L, sector_bytes, header_bits=0, capacity=0):
    """uint64[TABLE_LEN] of these lines, in trace order."""
    S = ceil_div(int(N) * int(L), int(sector_bytes))
    assert 1 <= S <= MAX_SECTORS
    addresses = np.asarray(addresses, dtype=np.uint64).reshape(-1)
    sizes = np.asarray(sizes).astype(np.int64).reshape(-1)
    t = np.zeros(TABLE_LEN, np.uint64)
    t[8], t[9], t[10], t[11] = int(N), int(sector_bytes), int(header_bits), int(capacity)
    if addresses.size == 0:
        return t
    keys, last = latest(addresses, sizes, L)
    _, T, payload = blocks_of(addresses, sizes, N, L)
    sec, caps = sectors_of(T, payload, L, sector_bytes, header_bits)
    t[0] = addresses.size
    t[1] = int(sizes.sum())
    t[2] = keys.size
    t[3] = int(last.sum())
    t[4] = T.size
    t[5] = int(sec.sum())
    t[6] = int(caps.sum())
    t[7] = int((addresses % np.uint64(L) != 0).sum())
    t[16:16 + S] = np.bincount(sec, minlength=S + 1)[1:].astype(np.uint64)
    return t


def image_table_loop(addresses, sizes, N, L, sector_bytes, header_bits=0, capacity=0):
    """The same by a Python dict walked line by line (the cross-check of image_table)."""
    t = [0] * TABLE_LEN
    image = {}
    for a, s in zip([int(x) for x in np.asarray(addresses, dtype=np.uint64).reshape(-1)], [int(x) for x in np.asarray(sizes).reshape(-1)]):
        t[0] += 1
        t[1] += s
        t[7] += 1 if a % L else 0
        image[a // L] = s
    blocks = {}
    for k, s in image.items():
        T, payload = blocks.get(k // N, (0, 0))
        blocks[k // N] = (T + 1, payload + s)
    t[2] = len(image)
    t[3] = sum(image.values())
    t[4] = len(blocks)
    for T, payload in blocks.values():
        cap = ceil_div(T * L, sector_bytes)
        k = min(max(1, ceil_div(payload + header_bits, 8 * sector_bytes)), cap)
        t[5] += k
        t[6] += cap
        t[16 + k - 1] += 1
    t[8], t[9], t[10], t[11] = N, sector_bytes, header_bits, capacity
    return np.array(t, dtype=np.uint64)


def ratios(table, L):
    """(traffic_ratio, image_ratio, image_sector_ratio), 0.0 where the divisor is 0."""
    t = [int(x) for x in np.asarray(table).reshape(-1)[:8]]
    return (t[0] * 8 * L / t[1] if t[1] else 0.0, t[2] * 8 * L / t[3] if t[3] else 0.0, t[6] / t[5] if t[5] else 0.0)


def boundary_headers(addresses, sizes, N, L, sector_bytes):
    """Two header_bits values chosen from the reference sizes: with the first some touched block has exactly
    8 sector_bytes k bits (0 < k < its cap, so that neither the floor of 1 nor the cap hides it), with the second --
    one more -- the same block has that value + 1.  None when no touched block lies in that range."""
    sbits = 8 * int(sector_bytes)
    _, T, payload = blocks_of(addresses, sizes, N, L)
    for t_, p in zip(T.tolist(), payload.tolist()):
        hb = (-p) % sbits
        k = (p + hb) // sbits
        if 0 < k < ceil_div(t_ * L, sector_bytes) and hb + 1 <= 65535:
            return hb, hb + 1
    return None


# ---- the text of comp::ImageReport (host/ImageReport.cpp): what <stem>_results_image.csv holds ----
CSV_HEADER = "Workload,Line Size,Block Lines,Sector Bytes,Header Bits,Lines,Distinct Lines,Blocks,Traffic Ratio,Image Ratio,Image Sector Ratio,Histogram,\n"


def fmt_double(x: float) -> str:
    """The host code's text of a double (mpctext::num): shortest round-trip, no trailing ".0"."""
    r = repr(float(x))
    return r[:-2] if r.endswith(".0") else r


def csv_row(workload, t, L):
    S = ceil_div(int(t[8]) * L, int(t[9]))
    hist = ";".join(f"{k}:{int(t[16 + k - 1])}" for k in range(1, S + 1) if int(t[16 + k - 1]))
    traffic, image, sector = ratios(t, L)
    return (f"{workload},{L},{int(t[8])},{int(t[9])},{int(t[10])},{int(t[0])},{int(t[2])},{int(t[4])},{fmt_double(traffic)},{fmt_double(image)},"
            f"{fmt_double(sector)},{hist},\n")


def same_table(tag, got, want):
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    assert got.dtype == np.uint64 and want.dtype == np.uint64 and got.shape == want.shape == (TABLE_LEN,), (tag, got.dtype, got.shape)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{tag}: {bad.size} entries differ, first {[(int(i), int(got[i]), int(want[i])) for i in bad[:6]]}"
