"""The per-class table of include/mpc_hip_classes.h in numpy, straight from its definition: row c of uint64[256][10]
holds, for the lines of class c, [0] the lines, [1] the sum of their sizes in bits, [1 + k] the lines that occupy k
sectors (k = 1 .. S = ceil(line_size / sector_bytes)), the rest 0; a line of `bits` bits occupies
min(max(1, ceil(bits / (8 * sector_bytes))), S) sectors.  Shared by tests/test_classes_cpu.py and
tests/test_classes_gpu.py (no test_ prefix: not collected)."""
import numpy as np

CLASSES = 256
ROW = 10
TABLE_LEN = CLASSES * ROW


def sectors_of(sizes, line_size, sector_bytes):
    """Sectors per line, int64."""
    sizes = np.asarray(sizes).astype(np.int64)
    most = -(-int(line_size) // int(sector_bytes))
    sector_bits = 8 * int(sector_bytes)
    return np.minimum(np.maximum(1, -(-sizes // sector_bits)), most)


def class_table(classes, sizes, line_size, sector_bytes):
    """uint64[256, 10] of `sizes` (one per line) grouped by `classes` (one uint8 per line)."""
    classes = np.asarray(classes).astype(np.int64)
    sizes = np.asarray(sizes).astype(np.int64)
    assert classes.shape == sizes.shape and classes.ndim == 1
    assert classes.size == 0 or (0 <= classes.min() and classes.max() < CLASSES)
    most = -(-int(line_size) // int(sector_bytes))
    assert 1 <= most <= ROW - 2
    table = np.zeros((CLASSES, ROW), dtype=np.uint64)
    table[:, 0] = np.bincount(classes, minlength=CLASSES)
    # (float64 weights: exact while a class's bits stay below 2^53)
    table[:, 1] = np.rint(np.bincount(classes, weights=sizes.astype(np.float64), minlength=CLASSES)).astype(np.uint64)
    sec = sectors_of(sizes, line_size, sector_bytes)
    for k in range(1, most + 1):
        table[:, 1 + k] = np.bincount(classes[sec == k], minlength=CLASSES)
    return table


def classes_of_selected(selected):
    """mpc_group_class_from_member: the class of a line is the member's int8 `selected` + 1."""
    return (np.asarray(selected).astype(np.int64) + 1).astype(np.uint8)


# ---- class arrays ---------------------------------------------------------------------------------------------------
def class_patterns(n, seed=1):
    """name -> uint8[n]: one value, every value, noise, runs that fill and that straddle a wave's lines, two values."""
    i = np.arange(n)
    rng = np.random.default_rng(seed + n)
    return {
        "all 0": np.zeros(n, np.uint8),
        "all 255": np.full(n, 255, np.uint8),
        "i % 256": (i % 256).astype(np.uint8),
        "random": rng.integers(0, 256, n, dtype=np.uint8),
        "runs of 64": ((i // 64) % 256).astype(np.uint8),
        "runs of 65": ((i // 65) * 7 % 256).astype(np.uint8),
        "runs of 512": ((i // 512) * 3 % 256).astype(np.uint8),
        "runs of 513": ((i // 513) * 5 % 256).astype(np.uint8),
        "two alternating": np.where(i % 2 == 0, 3, 200).astype(np.uint8),
    }


def same_table(tag, got, want):
    got = np.asarray(got)
    assert got.dtype == np.uint64 and got.shape == (CLASSES, ROW), (tag, got.dtype, got.shape)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (f"{tag}: {len(bad)} entries differ, first (class, column) {bad[:6].tolist()}: "
                           f"{[int(got[c, k]) for c, k in bad[:6]]} vs {[int(want[c, k]) for c, k in bad[:6]]}")


# ---- a .log file read back (the layout traces.write_gpgpusim_log writes) ----------------------------------------------
LOG_FILE_HEADER = 1 + 7 * 17
LOG_RECORD_HEADER = 62


def log_fields(path, line_size):
    """-> (kernel id u8[n], mf_type u8[n], req_type u32[n], lines u8[n, L]) of every record of the file."""
    raw = np.fromfile(path, dtype=np.uint8)[LOG_FILE_HEADER:]
    rec = LOG_RECORD_HEADER + line_size
    assert raw.size % rec == 0
    raw = raw.reshape(-1, rec)
    req_type = np.ascontiguousarray(raw[:, 38:42]).view("<u4").reshape(-1)
    return raw[:, 0].copy(), raw[:, 1].copy(), req_type.copy(), np.ascontiguousarray(raw[:, LOG_RECORD_HEADER:])
