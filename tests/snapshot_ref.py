"""Reference of the snapshot (include/mpc_hip_snapshot.h), twice: a plain dict loop and a vectorised numpy version of
add, plan and read, compared with each other by tests/test_snapshot_cpu.py and with the library by
tests/test_snapshot_gpu.py.  Everything is integers and bytes; every comparison is equality."""
import numpy as np

UNITS = (32, 64, 128)
KS = (1, 2, 4, 8)
MAX_LINE = 256
PLAN_KEYS = ("touched", "complete", "partial", "partial_units", "missing_units", "n_out")
CSV_HEADER = ("Workload,Unit Bytes,Line Size,Partial,Units,Distinct Units,Misaligned,Touched Lines,Complete Lines,Partial Lines,"
              "Missing Units,Evaluated Lines,\n")


class Overflow(Exception):
    """more distinct units than the capacity: the snapshot is finished"""


def check_values(U, capacity, L=0):
    """the refusals of mpc_snapshot_check_values: None, or a word of the message"""
    if U not in UNITS:
        return "unit_bytes"
    if capacity < 1 or capacity > 1 << 28:
        return "capacity_units"
    if L == 0:
        return None
    if L > MAX_LINE:
        return "above 256"
    if L % U or L // U not in KS:
        return "is not 1, 2, 4 or 8 units"
    return None


def slots_of(capacity):
    s = 2
    while s < 2 * capacity:
        s *= 2
    return s


# ---- the dict loop ---------------------------------------------------------------------------------------------------
class LoopSnapshot:
    def __init__(self, U=32, capacity=1 << 24):
        assert check_values(U, capacity) is None
        self.U, self.capacity = U, capacity
        self.reset()

    def reset(self):
        self.mem, self.units, self.misaligned = {}, 0, 0

    def add(self, units, addrs):
        units = np.asarray(units, dtype=np.uint8).reshape(-1, self.U)
        assert len(units) == len(addrs)
        for data, a in zip(units, addrs):
            a = int(a)
            key = a // self.U
            if key not in self.mem and len(self.mem) == self.capacity:
                raise Overflow(self.capacity)
            self.mem[key] = data.tobytes()           # a later unit of the same key replaces the earlier one
            self.misaligned += a % self.U != 0
            self.units += 1

    def stats(self):
        return {"units": self.units, "distinct_units": len(self.mem), "misaligned": self.misaligned, "capacity": self.capacity,
                "unit_bytes": self.U}

    def _lines(self, L):
        assert check_values(self.U, self.capacity, L) is None
        k = L // self.U
        out = {}
        for key in self.mem:
            out.setdefault(key // k, []).append(key % k)
        return k, out

    def plan(self, L, partial="skip"):
        k, lines = self._lines(L)
        touched = len(lines)
        complete = sum(1 for js in lines.values() if len(js) == k)
        punits = sum(len(js) for js in lines.values() if len(js) < k)
        n_out = {"skip": complete, "zero": touched}[partial]
        return dict(zip(PLAN_KEYS, (touched, complete, touched - complete, punits, k * (touched - complete) - punits, n_out)))

    def read(self, L, partial="skip"):
        k, lines = self._lines(L)
        U = self.U
        rows, addrs, pres = [], [], []
        for lk in sorted(lines):
            js = lines[lk]
            if partial == "skip" and len(js) < k:
                continue
            row = bytearray(L)
            for j in js:
                row[j * U:(j + 1) * U] = self.mem[lk * k + j]
            rows.append(bytes(row))
            addrs.append(lk * L)
            pres.append(sum(1 << j for j in js))
        lines_out = np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(len(rows), L).copy() if rows else np.zeros((0, L), np.uint8)
        return lines_out, np.array(addrs, dtype=np.uint64), np.array(pres, dtype=np.uint8)


# ---- numpy, over everything that was added ---------------------------------------------------------------------------
def latest(units, addrs, U, capacity=1 << 24):
    """(keys ascending uint64, their latest units uint8[D, U], misaligned) of all units added, in order"""
    units = np.asarray(units, dtype=np.uint8).reshape(-1, U)
    addrs = np.asarray(addrs, dtype=np.uint64)
    assert len(units) == len(addrs)
    keys = addrs // np.uint64(U)
    mis = int((addrs % np.uint64(U) != 0).sum())
    order = np.argsort(keys, kind="stable")                     # equal keys stay in the order they were added
    sk = keys[order]
    last = np.ones(len(sk), dtype=bool)
    last[:-1] = sk[1:] != sk[:-1]
    if int(last.sum()) > capacity:
        raise Overflow(capacity)
    return sk[last], units[order[last]], mis


def stats(units, addrs, U, capacity=1 << 24):
    keys, _, mis = latest(units, addrs, U, capacity)
    return {"units": len(addrs), "distinct_units": len(keys), "misaligned": mis, "capacity": capacity, "unit_bytes": U}


def _group(keys, k):
    lk = keys // np.uint64(k)
    head = np.ones(len(keys), dtype=bool)
    head[1:] = lk[1:] != lk[:-1]
    line_of = np.cumsum(head) - 1                                # index of each unit's line among the touched lines
    count = np.bincount(line_of, minlength=int(head.sum())) if len(keys) else np.zeros(0, dtype=np.int64)
    return lk, head, line_of, count


def plan(units, addrs, U, L, partial="skip", capacity=1 << 24):
    assert check_values(U, capacity, L) is None
    k = L // U
    keys, _, _ = latest(units, addrs, U, capacity)
    _, _, _, count = _group(keys, k)
    touched, complete = len(count), int((count == k).sum())
    punits = int(count[count < k].sum())
    n_out = {"skip": complete, "zero": touched}[partial]
    return dict(zip(PLAN_KEYS, (touched, complete, touched - complete, punits, k * (touched - complete) - punits, n_out)))


def read(units, addrs, U, L, partial="skip", capacity=1 << 24):
    assert check_values(U, capacity, L) is None
    k = L // U
    keys, data, _ = latest(units, addrs, U, capacity)
    lk, head, line_of, count = _group(keys, k)
    T = len(count)
    lines = np.zeros((T, k, U), dtype=np.uint8)
    j = (keys % np.uint64(k)).astype(np.int64)
    lines[line_of, j] = data
    pres = np.zeros(T, dtype=np.int64)
    np.add.at(pres, line_of, 1 << j)
    line_addrs = lk[head] * np.uint64(L)
    keep = count == k if partial == "skip" else np.ones(T, dtype=bool)
    return np.ascontiguousarray(lines.reshape(T, L)[keep]), line_addrs[keep].astype(np.uint64), pres[keep].astype(np.uint8)


def plan_identities(p, k, D, partial):
    """the identities include/mpc_hip_snapshot.h states for a plan"""
    assert k * p["complete"] + p["partial_units"] == D, (p, k, D)
    assert p["partial_units"] + p["missing_units"] == k * p["partial"], (p, k)
    assert p["touched"] == p["complete"] + p["partial"], p
    assert p["n_out"] == (p["complete"] if partial == "skip" else p["touched"]), (p, partial)


def csv_row(workload, U, L, partial, st, p):
    """a row of <stem>_results_snapshot.csv (host/SnapshotReport.cpp)"""
    return (f"{workload},{U},{L},{partial},{st['units']},{st['distinct_units']},{st['misaligned']},{p['touched']},{p['complete']},"
            f"{p['partial']},{p['missing_units']},{p['n_out']},\n")
