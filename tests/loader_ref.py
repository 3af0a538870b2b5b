"""The seeded trace files behind tests/golden/ref_loader_vectors.json: what the reference's own loaders (LoaderGPGPU.cpp with
its gpgpusim and apsim namespaces, LoaderNPY.cpp, compiled unmodified by tests/golden/make_ref_loader_vectors.py) deliver
for them is recorded there; this module only says how each input file is written, so that the generator and the tests
build the same bytes.  A case is a plain dict (it is copied into the fixture):

  .log   "parts": runs of records written by traces.write_gpgpusim_log (lines generator, line size -- 0 gives records
         without payload --, request types, writer seed) whose bodies are concatenated behind one file header; "tail":
         none | short1 (a record whose last payload byte is missing) | hdr17 (a record header cut after 17 bytes) |
         hdr62 (a complete record header without payload)
  .npy   one lines generator, written by traces.save_npy
  .txt   either "writer": arguments of traces.write_apsim_txt (plus "crlf"), or "header" + "rows": the literal text;
         "line_sizes": the line sizes the loader is asked for (32 = single beats, 64 = two beats of one channel)
"""
import hashlib
import os

import numpy as np

from conftest import pkg

LOG_FILE_HEADER = 1 + 7 * 17


# ---- lines -------------------------------------------------------------------------------------------------------
def gen_lines(spec) -> np.ndarray:
    T = pkg("traces")
    n, L, seed = spec["n"], spec["L"], spec.get("seed", 1)
    if L == 0:
        return np.zeros((n, 0), dtype=np.uint8)
    kind = spec["gen"]
    if kind == "structured":
        return T.structured(n, L, seed=seed)
    if kind == "random":
        return T.random_u32(n, L, seed=seed)
    if kind == "mixed":
        return T.mixed(n, L)
    if kind == "zeros":
        return T.zeros(n, L)
    if kind == "blend":      # compressible, incompressible and repeated lines in a seeded order (SC2 and Pattern see all kinds)
        a = np.concatenate([T.structured(n - n // 4 - n // 8, L, seed=seed), T.random_u32(n // 8, L, seed=seed), T.mixed(n // 4, L)])
        return a[np.random.default_rng(seed).permutation(n)]
    raise ValueError(kind)


def gen_types(spec, n) -> np.ndarray:
    kind = spec["kind"]
    if kind == "const":
        t = np.full(n, spec["value"], dtype=np.uint32)
    elif kind == "uniform9":            # every request type 0..8
        t = np.random.default_rng(spec["seed"]).integers(0, 9, n).astype(np.uint32)
    elif kind == "mostly_global":       # 19 of 20 requests a global read or write, the rest any other type
        rng = np.random.default_rng(spec["seed"])
        other = rng.choice([1, 2, 3, 5, 6, 7, 8], n)
        t = np.where(rng.integers(0, 20, n) == 0, other, rng.choice([0, 4], n)).astype(np.uint32)
    else:
        raise ValueError(kind)
    if "first" in spec and n:
        t[0] = spec["first"]
    return t


# ---- files -------------------------------------------------------------------------------------------------------
def _log_bytes(part, tmp_dir) -> bytes:
    T = pkg("traces")
    lines = gen_lines(part)
    p = T.write_gpgpusim_log(os.path.join(tmp_dir, "_part.log"), lines, gen_types(part["types"], len(lines)), seed=part.get("wseed", 3))
    with open(p, "rb") as f:
        data = f.read()
    os.unlink(p)
    return data


def build_input(case, dst_dir, name=None) -> str:
    """Writes the case's trace file into dst_dir and returns its path."""
    T = pkg("traces")
    path = os.path.join(dst_dir, (name or case["name"]) + "." + case["fmt"])
    if case["fmt"] == "npy":
        T.save_npy(path, gen_lines(case))
    elif case["fmt"] == "log":
        blobs = [_log_bytes(part, dst_dir) for part in case["parts"]]
        one = _log_bytes(dict(case["parts"][0], n=1), dst_dir)[LOG_FILE_HEADER:]
        tail = {"none": b"", "short1": one[:-1], "hdr17": one[:17], "hdr62": one[:62]}[case["tail"]]
        with open(path, "wb") as f:
            f.write(blobs[0] + b"".join(b[LOG_FILE_HEADER:] for b in blobs[1:]) + tail)
    elif case["fmt"] == "txt":
        if "writer" in case:
            w = case["writer"]
            T.write_apsim_txt(path, gen_lines(w["beats"]), write_trace=w["write_trace"], seed=w["seed"], final_newline=w["final_newline"],
                              idle_rows=w["idle_rows"])
            if w.get("crlf"):
                with open(path, "rb") as f:
                    text = f.read()
                with open(path, "wb") as f:
                    f.write(text.replace(b"\n", b"\r\n"))
        else:
            with open(path, "w", newline="") as f:
                f.write("\n".join([case["header"]] + case["rows"]) + ("\n" if case.get("final_newline", True) else ""))
    else:
        raise ValueError(case["fmt"])
    return path


def file_digest(path) -> str:
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def bytes_digest(data: bytes) -> str:
    return hashlib.sha256(data).hexdigest()


# ---- the cases ---------------------------------------------------------------------------------------------------
def _log(name, parts, tail="none", **kw):
    return dict(name=name, fmt="log", parts=parts, tail=tail, **kw)


def _part(n, L, types, gen="structured", seed=1, wseed=3):
    return dict(gen=gen, n=n, L=L, seed=seed, types=types, wseed=wseed)


U9 = lambda s: dict(kind="uniform9", seed=s)            # noqa: E731
CONST = lambda v: dict(kind="const", value=v)           # noqa: E731


def _hex(seed, nbytes=32) -> str:
    return np.random.default_rng(seed).integers(0, 256, nbytes, dtype=np.uint8).tobytes().hex()


def _row(cycle, clock, valid, ready, tail, data_seed, data=None, extra=()):
    d = data or [_hex(1000 * data_seed + k) for k in range(4)]
    return ",".join([str(cycle), str(clock)] + [str(v) for v in valid] + list(d) + [str(r) for r in ready] + [str(t) for t in tail] + list(extra))


def _header(tails):
    return ",".join(["Time", "clk"] + [f"valid_{i}" for i in range(4)] + [f"data_{i}" for i in range(4)] + [f"ready_{i}" for i in range(4)] + list(tails))


RD_HEADER = _header([f"last_{i}" for i in range(4)])


def _odd_rows():
    """Rows whose fields are not what a simulator writes: the reference narrows valid / ready / clock to uint8_t after
    std::stoi (257 and -255 are 1, 256 is 0), compares valid with 1 (2 is no handshake but keeps the row from being idle),
    accepts upper-case hex, reads the first 64 hex digits of a longer data field, skips leading spaces of a number and
    ignores fields behind the 18th."""
    upper = [_hex(40 + k).upper() for k in range(4)]
    long_ = [_hex(900 + k, 40) for k in range(4)]
    return [
        _row(10, 1, [1, 0, 0, 0], [1, 0, 0, 0], [0, 0, 0, 0], 1),                 # plain beat on channel 0
        _row(11, 1, [2, 1, 0, 0], [1, 1, 0, 0], [0, 0, 0, 0], 2),                 # valid 2: channel 1 only
        _row(12, 1, [2, 0, 0, 0], [1, 0, 0, 0], [0, 0, 0, 0], 3),                 # valid 2 alone: nothing
        _row(13, 1, [257, 0, 0, 0], [1, 0, 0, 0], [0, 0, 0, 0], 4),               # 257 -> 1
        _row(14, 1, [0, 0, -255, 0], [0, 0, 1, 0], [0, 0, 0, 0], 5),              # -255 -> 1
        _row(15, 1, [0, 0, 0, 1], [0, 0, 0, 257], [0, 0, 0, 0], 6),               # ready 257 -> 1
        _row(16, 2, [0, 1, 0, 0], [0, 1, 0, 0], [0, 0, 0, 0], 7),                 # clock 2: counts
        _row(17, 256, [1, 1, 1, 1], [1, 1, 1, 1], [0, 0, 0, 0], 8),               # clock 256 -> 0: skipped
        _row(18, 1, [1, 0, 0, 1], [1, 0, 0, 1], [1, 0, 0, 1], 9, data=upper),    # upper-case hex
        _row(19, 1, [0, 1, 1, 0], [0, 1, 1, 0], [0, 0, 0, 0], 10, data=long_),    # 80 hex digits: the first 64
        _row(" 20", " 1", [" 1", 0, 0, " 1"], [" 1", 0, 0, " 1"], [0, 0, 0, 0], 11),   # leading spaces
        _row(21, 1, [1, 1, 1, 1], [1, 1, 1, 1], [0, 1, 0, 1], 12, extra=["7", "zz", ""]),  # fields behind the 18th
        _row(22, 1, [0, 0, 1, 0], [0, 0, 1, 0], [0, 0, 0, 0], 13) + "\r",         # one CRLF row
        _row(23, 1, [1, 0, 0, 0], [1, 0, 0, 0], [0, 0, 0, 0], 14),
    ]


def _txt_writer(name, n, write_trace=False, seed=5, final_newline=True, idle_rows=True, crlf=False, gen="structured", line_sizes=(32, 64)):
    return dict(name=name, fmt="txt", line_sizes=list(line_sizes),
                writer=dict(beats=dict(gen=gen, n=n, L=32, seed=8), write_trace=write_trace, seed=seed, final_newline=final_newline,
                            idle_rows=idle_rows, crlf=crlf))


CASES = [
    # ---- GPGPU-Sim .log ----
    _log("log_all_types_32", [_part(300, 32, U9(1))]),
    _log("log_all_types_64", [_part(300, 64, U9(2))]),
    _log("log_all_types_128", [_part(300, 128, U9(3))]),
    _log("log_single_record", [_part(1, 64, CONST(0))]),
    _log("log_single_write_128", [_part(1, 128, CONST(4))]),
    _log("log_first_not_evaluated", [_part(50, 64, dict(kind="uniform9", seed=4, first=2))]),
    _log("log_none_evaluated", [_part(50, 32, CONST(2))]),
    _log("log_tail_short1_64", [_part(300, 64, U9(5))], tail="short1"),
    _log("log_tail_hdr17_64", [_part(300, 64, U9(6))], tail="hdr17"),
    _log("log_tail_hdr62_64", [_part(300, 64, U9(7))], tail="hdr62"),
    _log("log_tail_short1_32", [_part(77, 32, U9(8))], tail="short1"),
    _log("log_tail_hdr62_128", [_part(77, 128, U9(9))], tail="hdr62"),
    _log("log_other_sizes_between", [_part(40, 64, dict(kind="mostly_global", seed=10, first=0)), _part(5, 32, CONST(1), gen="random"),
                                     _part(3, 0, CONST(8)), _part(40, 64, U9(11), seed=2), _part(2, 128, CONST(6), gen="random"),
                                     _part(20, 64, CONST(4), seed=3)]),
    _log("log_other_sizes_then_tail", [_part(30, 32, dict(kind="mostly_global", seed=12, first=4)), _part(4, 64, CONST(3), gen="random"),
                                       _part(1, 0, CONST(5))], tail="hdr17"),
    _log("log_zero_size_evaluated", [_part(10, 64, CONST(0)), _part(1, 0, CONST(0)), _part(10, 64, CONST(4), seed=2)], deviation="zero_size"),
    _log("log_two_sizes_evaluated", [_part(10, 64, CONST(0)), _part(4, 32, CONST(4), seed=2)], deviation="two_sizes"),
    _log("log_big_64", [_part(12000, 64, dict(kind="mostly_global", seed=13), gen="blend", seed=21)], tail="short1"),
    # ---- .npy ----
    *[dict(name=f"npy_{n}x{L}", fmt="npy", gen="structured", n=n, L=L, seed=n + L) for L in (32, 64, 128) for n in (1, 2, 777)],
    dict(name="npy_big_64", fmt="npy", gen="blend", n=12001, L=64, seed=22),
    # ---- APSim .txt ----
    _txt_writer("txt_read", 501),
    _txt_writer("txt_write", 501, write_trace=True, seed=6),
    _txt_writer("txt_read_no_final_newline", 300, final_newline=False, seed=7),
    _txt_writer("txt_write_no_final_newline", 300, write_trace=True, final_newline=False, seed=8),
    _txt_writer("txt_read_crlf", 200, crlf=True, seed=9),
    _txt_writer("txt_write_crlf", 200, write_trace=True, crlf=True, seed=10),
    _txt_writer("txt_unpaired_beats_at_end", 9, idle_rows=False, seed=11, gen="random"),
    _txt_writer("txt_unpaired_beats_at_end_write", 23, write_trace=True, idle_rows=False, seed=12, gen="random"),
    dict(name="txt_odd_rows", fmt="txt", line_sizes=[32, 64], header=RD_HEADER, rows=_odd_rows()),
    dict(name="txt_odd_rows_no_final_newline", fmt="txt", line_sizes=[32, 64], header=RD_HEADER, rows=_odd_rows(), final_newline=False),
    dict(name="txt_header_last_then_strb", fmt="txt", line_sizes=[32, 64],
         header=_header(["last_0", "strb_1", "last_2", "strb_3"]),
         rows=[_row(5 + k, 1, [1, k % 2, 0, 1], [1, 1, 0, k % 2], [1, 0, 1, 0], 100 + k) for k in range(6)]),
    dict(name="txt_header_strb_then_last", fmt="txt", line_sizes=[32, 64],
         header=_header(["strb_0", "last_1", "strb_2", "last_3"]),
         rows=[_row(5 + k, 1, [1, k % 2, 0, 1], [1, 1, 0, k % 2], ["ff00ff00", "0", "deadbeef", "1"], 200 + k) for k in range(6)]),
]
