"""The footprint of a device-path call (mpc_compress_batch_device / mpc_group_compress_batch_device): what a call writes
and reads OUTSIDE the range it was asked for.  Shared by tests/test_device_footprint_gpu.py and the child processes it
starts (no test_ prefix: a fresh interpreter imports this module on its own).

One call, `check_call`, surrounds everything the kernels touch with memory the test owns and looks at afterwards:

  lines    one uint8 tensor of 64 KiB + off + n L + 64 KiB; the lines start at base + 64 KiB + off (off % 16 == 0: the
           16-byte alignment the C ABI asks for and not a byte more).  The bytes around the lines are poison: all zero
           in one run (a line read past the end would look like an AllZero line), seeded random bytes in the other (it
           would look incompressible).
  sizes    one int16 tensor of 4096 + 1 + n + 4096 elements per member, filled with 0xA5A5; the array handed to the
           library starts at element 4097: 2-byte aligned, not 4-byte aligned.  No evaluator produces 0xA5A5
           (csrc/mpc_sizes.h bounds every size at 2240 for lines of up to 256 bytes).
  selected one int8 tensor of the same shape, filled with 0x5A (90, above every VPC module index, BDI state, Pattern
           state and SC2 flag); the array starts at the odd element 4097.

After the call and a sync: elements [0, n) of every array that was asked for equal the CPU reference's, EVERY other
element of both tensors still holds its canary (the whole array of an output that was not asked for included), the
input tensor is byte for byte what was uploaded, and the statistics vector is the reference's for exactly these
lines -- its line count is where a line past the end shows up.  All comparisons are exact.

The margins are there so that a wrong kernel still reads and writes inside the test's own allocations: these tests
observe corruption, they never touch the end of an allocation.

Evaluators and references are fed cumulatively: a handle (and its reference) takes every call of a sweep, as a trace
evaluator does, and the statistics are compared after every call."""
import numpy as np

IN_MARGIN = 64 << 10
OUT_MARGIN = 4096
OUT_START = OUT_MARGIN + 1
SIZES_CANARY = 0xA5A5
SEL_CANARY = 0x5A
MODES = {"both": (True, True), "sizes only": (True, False), "sel only": (False, True), "none": (False, False)}
# wave (64 lanes), 64-line group, 128-line block and 256-thread workgroup edges
LINE_COUNTS = (1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 1023, 1025)
MODE_COUNTS = (65, 129, 257)          # every output mode at these; mode "both" at the others
POISON_SEEDS = (0, 0xF007)            # 0: all-zero poison; otherwise the seed of random poison


def offsets_for(L):
    return (0, 16) + ((L // 2 + 16,) if L >= 64 else ())


# ---- references: feed(lines) -> (sizes uint16[n], selected int8[n]), stats_vector(); cumulative like the handles ------
class OracleRef:
    """oracle.VpcOracle / BdiOracle / FpcOracle / BpcOracle (FPC and BPC: `selected` is written as 0).  These evaluators
    are stateless per line and their statistics are plain integer sums (include/mpc_hip.h: mpc_stats_merge is +=), so
    the oracle runs once per distinct batch of lines -- a sweep feeds the same lines at several offsets, modes and
    poisons -- and the running statistics are the sum of the batches' own."""

    def __init__(self, o):
        self.o, self.seen, self.total = o, {}, None

    def feed(self, lines):
        key = (lines.shape, lines.tobytes())
        if key not in self.seen:
            self.o.reset()
            r = self.o.compress(lines)
            self.seen[key] = (r if isinstance(r, tuple) else (r, np.zeros(len(lines), np.int8))) + (self.o.stats_vector(),)
        sizes, sel, v = self.seen[key]
        self.total = v.copy() if self.total is None else self.total + v
        return sizes, sel

    def stats_vector(self):
        return self.total


class PatternRef:
    """pattern_ref.analyse over the calls of one handle.  Everything but T ([6]) and the lines that joined the set
    ([21]) is a sum over lines, taken from analyse() of the call's lines; those two follow from the number of distinct
    lines fed so far (T = L x (lines - distinct)), kept in a Python set of the lines' bytes.  `whole()` is analyse() of
    everything fed so far in one piece, for a cross-check at the end of a sweep."""

    def __init__(self, L):
        self.L, self.set, self.fed, self.v = L, set(), [], None

    def feed(self, lines):
        import pattern_ref
        sizes, sel, v = pattern_ref.analyse(lines, with_set=False)
        self.v = v if self.v is None else self.v + v
        self.fed.append(np.array(lines))
        self.set.update(bytes(row) for row in lines)
        return sizes, sel

    def stats_vector(self):
        v = self.v.copy()
        v[21] = len(self.set)
        v[6] = self.L * (int(v[0]) - len(self.set))
        return v

    def whole(self):
        import pattern_ref
        return pattern_ref.analyse(np.concatenate(self.fed))[2]


# ---- lines -----------------------------------------------------------------------------------------------------------
def _gen(gen, n, L, **kw):
    """Lines of L bytes from a trace generator: its own at 32 / 64 / 128 bytes, the head of its 128-byte lines elsewhere."""
    return gen(n, L, **kw) if L in (32, 64, 128) else np.ascontiguousarray(gen(n, 128, **kw)[:, :L])


def line_pool(traces, L, n=1260):
    """A fixed, permuted pool of structured, interleaved, random, zero and word-same lines (the mix of
    test_block_and_group_boundaries); a case takes its first lines."""
    k = -(-n // 1260)
    pool = np.concatenate([_gen(traces.structured, 700 * k, L, seed=5), _gen(traces.mixed, 300 * k, L), _gen(traces.random_u32, 200 * k, L),
                           _gen(traces.zeros, 30 * k, L), _gen(traces.word_same, 30 * k, L)])
    return np.ascontiguousarray(pool[np.random.default_rng(L).permutation(len(pool))][:n])


def pattern_pool(traces, L, n=1260, period=40):
    """The pool with repeats: every third line is one of the first `period` lines again."""
    pool = line_pool(traces, L, n).copy()
    idx = np.arange(2, n, 3)
    pool[idx] = pool[idx % period]
    return pool


def zipf_lines(n, L, seed):
    """Words drawn from a pool of 4000 with a Zipf-like law, one word in ten replaced by noise (the generator of
    tests/test_sc2_gpu.py): an SC2 table that hits often and misses often."""
    rng = np.random.default_rng(seed)
    pool = rng.integers(0, 1 << 32, size=4000, dtype=np.uint64).astype(np.uint32)
    p = 1.0 / np.arange(1, len(pool) + 1) ** 1.05
    p /= p.sum()
    words = pool[rng.choice(len(pool), size=n * (L // 4), p=p)]
    noise = rng.random(words.size) < 0.1
    words = np.where(noise, rng.integers(0, 1 << 32, size=words.size, dtype=np.uint64).astype(np.uint32), words)
    return words.astype("<u4").view(np.uint8).reshape(n, L)


def capped_pool(traces, L, n):
    """Mostly incompressible lines with compressible ones scattered among them: few lines of a group pass a module's
    prefilter, which is when the VPC and BDI kernels set lines aside into their queues."""
    k = -(-n // 20)
    pool = np.concatenate([traces.random_u32(11 * k, L), traces.mixed(4 * k, L), traces.structured(3 * k, L, seed=3),
                           traces.bdi_screen_stress(2 * k, L)])
    return np.ascontiguousarray(pool[np.random.default_rng(7 + L).permutation(len(pool))][:n])


# ---- VPC configurations of the forms the sweep covers (as tests/test_gpu_parity.py builds them) ----------------------
AZ, AWS = {"name": "AllZero"}, {"name": "AllWordSame"}


def plane_major(L, ts):
    return None if ts is None else {"TableSize": ts, "Rows": [i // L for i in range(ts)], "Cols": [i % L for i in range(ts)]}


def byte_major(L, ts=None):
    ts = 8 * L if ts is None else ts
    return {"TableSize": ts, "Rows": [i % 8 for i in range(ts)], "Cols": [i // 8 for i in range(ts)]}


def probe_layout_config(configs, L, roots=(0, 0, 0), scan=None):
    """The probe configuration's four predictors with RootIndex `roots` and the scan table `scan`."""
    prev4 = [max(i - 4, 0) for i in range(L)]
    w2 = [[1.0, 0.5][i % 2] for i in range(L)]
    d1 = [1 if i % 4 == 0 else 0 for i in range(L)]
    return configs.make_config(L, [AZ, AWS, configs.one_base(L, roots[0], True, scan), configs.consecutive_base(L, 0, True, scan),
                                   configs.diff_base(L, prev4, d1, roots[1], False, scan), configs.weight_base(L, prev4, w2, roots[2], True, scan)])


def new_sequence_config(configs, L):
    """OneBase DiffBase WeightBase OneBase: a module sequence without a built-in unrolled instantiation."""
    prev1 = [max(i - 1, 0) for i in range(L)]
    prev4 = [max(i - 4, 0) for i in range(L)]
    diff = [(-2 + (i % 5)) for i in range(L)]
    w2 = [[1.0, 0.5][i % 2] for i in range(L)]
    return configs.make_config(L, [AZ, AWS, configs.one_base(L, 0, True), configs.diff_base(L, prev1, diff, 0, False),
                                   configs.weight_base(L, prev4, w2, 0, True), configs.one_base(L, 0, False)])


def mixed_scan_orders_config(configs, L):
    """One module scans byte-major, the other plane-major: no fast form."""
    return configs.make_config(L, [AZ, configs.one_base(L, 0, True, byte_major(L)), configs.one_base(L, 0, False)])


def permuted_scan_config(configs, L):
    """Random tables, roots and a permuted, truncated scan table (test_vpc_generic_path)."""
    rng = np.random.default_rng(L)
    n = 8 * L
    perm = rng.permutation(n)
    scan = {"TableSize": n - 16, "Rows": [int(p) // L for p in perm[: n - 16]], "Cols": [int(p) % L for p in perm[: n - 16]]}
    rb = [int(x) for x in rng.integers(0, L, L)]
    rd = [int(x) for x in rng.integers(-300, 300, L)]
    rw = [float(2.0 ** int(x)) for x in rng.integers(-9, 10, L)]
    return configs.make_config(L, [AZ, AWS, configs.one_base(L, root=5, consecutive_xor=True), configs.consecutive_base(L, 0, False, scan=scan),
                                   configs.diff_base(L, rb, rd, root=3, consecutive_xor=True),
                                   configs.weight_base(L, rb, rw, root=L - 1, consecutive_xor=False, scan=scan)])


# ---- one call --------------------------------------------------------------------------------------------------------
def _poison(nbytes, seed):
    if seed == 0:
        return np.zeros(nbytes, np.uint8)
    return np.random.default_rng(seed).integers(0, 256, nbytes, dtype=np.uint8)


def _check_array(tag, got, n, want, canary):
    """`got`: the whole tensor; elements [OUT_START, OUT_START + n) are the array the library was (or was not) given."""
    outside = np.ones(len(got), bool)
    if want is not None:
        outside[OUT_START:OUT_START + n] = False
    stray = np.nonzero(outside & (got != canary))[0]
    assert stray.size == 0, (f"{tag}: canary overwritten at {stray.size} elements outside the {n if want is not None else 0} that were asked for; "
                             f"first at array index {(stray[:6] - OUT_START).tolist()}, values {got[stray[:6]].tolist()}")
    if want is not None:
        body = got[OUT_START:OUT_START + n]
        bad = np.nonzero(body != want)[0]
        assert bad.size == 0, f"{tag}: {bad.size} of {n} differ from the reference, first at {bad[:6].tolist()}: {body[bad[:6]].tolist()} vs {want[bad[:6]].tolist()}"


def check_call(target, refs, lines, off=0, mode="both", poison=0, ask=None, stream=0, tag=""):
    """One device-path call of `target` (an evaluator, or an EvaluatorSet) on `lines` [n, L], and every check of the
    module docstring.  refs: one reference per member, fed the same lines.  mode: which arrays are handed over.  ask:
    the members of a set that get arrays at all (default: all); the others get null pointers, and their own canaried
    arrays must stay untouched."""
    import torch
    members = target.members if hasattr(target, "members") else [target]
    assert len(refs) == len(members)
    lines = np.ascontiguousarray(lines, dtype=np.uint8)
    n, L = lines.shape
    assert off % 16 == 0 and L == target.line_size
    want_sizes, want_sel = MODES[mode]
    ask = set(range(len(members))) if ask is None else set(ask)
    tag = f"{tag} L={L} n={n} off={off} mode={mode} poison={'zero' if poison == 0 else 'random'}"

    host = _poison(IN_MARGIN + off + n * L + IN_MARGIN, poison)
    host[IN_MARGIN + off:IN_MARGIN + off + n * L] = lines.reshape(-1)
    d_in = torch.from_numpy(host).to("cuda:0")
    total = OUT_MARGIN + 1 + n + OUT_MARGIN
    d_sizes = [torch.full((total,), SIZES_CANARY - 0x10000, dtype=torch.int16, device="cuda:0") for _ in members]
    d_sel = [torch.full((total,), SEL_CANARY, dtype=torch.int8, device="cuda:0") for _ in members]
    p_lines = d_in.data_ptr() + IN_MARGIN + off
    p_sizes = [t.data_ptr() + 2 * OUT_START if want_sizes and i in ask else 0 for i, t in enumerate(d_sizes)]
    p_sel = [t.data_ptr() + OUT_START if want_sel and i in ask else 0 for i, t in enumerate(d_sel)]
    assert p_lines % 16 == 0 and d_in.data_ptr() % 256 == 0
    assert all(t.data_ptr() % 4 == 0 for t in d_sizes) and all(t.data_ptr() % 2 == 0 for t in d_sel)      # so the arrays are 2 mod 4 / odd
    torch.cuda.synchronize()

    if hasattr(target, "members"):
        target.compress_device(p_lines, n, p_sizes if any(p_sizes) else None, p_sel if any(p_sel) else None, stream=stream)
    else:
        target.compress_device(p_lines, n, p_sizes[0], p_sel[0], stream=stream)
    target.sync()
    torch.cuda.synchronize()

    for i, (ev, ref) in enumerate(zip(members, refs)):
        s_ref, k_ref = ref.feed(lines)
        who = f"{tag} member {i} ({type(ev).__name__})"
        _check_array(who + " sizes", d_sizes[i].cpu().numpy().view(np.uint16), n, s_ref if p_sizes[i] else None, SIZES_CANARY)
        _check_array(who + " selected", d_sel[i].cpu().numpy(), n, k_ref if p_sel[i] else None, SEL_CANARY)
        got, want = ev.stats_vector(), ref.stats_vector()
        assert got.shape == want.shape, who
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, f"{who}: statistics differ at {bad[:8].tolist()}: {got[bad[:8]].tolist()} vs {want[bad[:8]].tolist()}"
    back = d_in.cpu().numpy()
    changed = np.nonzero(back != host)[0]
    assert changed.size == 0, f"{tag}: the input tensor changed at {changed.size} bytes, first at {(changed[:6] - IN_MARGIN - off).tolist()} relative to the lines"


def sweep(target, refs, pool, counts=LINE_COUNTS, offsets=None, modes_at=MODE_COUNTS, ask=None, streams=(0,), tag=""):
    """check_call over the line counts, the offsets, the output modes (all of them at `modes_at`, "both" elsewhere) and
    both kinds of poison; consecutive calls take `streams` in turn.  Returns the number of calls."""
    offsets = offsets_for(pool.shape[1]) if offsets is None else offsets
    calls = 0
    for n in counts:
        for off in offsets:
            for mode in (MODES if n in modes_at else ("both",)):
                for poison in POISON_SEEDS:
                    check_call(target, refs, pool[:n], off, mode, poison, ask, streams[calls % len(streams)], tag)
                    calls += 1
    return calls


# ---- the rows that run under a capped grid (a child process bound to the test library) --------------------------------
CAPPED_COUNTS = (20001, 16384 + 65)


def capped_grid_rows(mpc, configs, traces, oracle, routes):
    """With one workgroup (MPC_TEST_GRID=1) every wave reuses its ring stages and fills and drains its deferred-line
    queue inside the loop: the late stores of queued lines are the ones most likely to carry a stale index.  Returns
    the route counters per row."""
    res = {}
    rows = [("vpc 64", 64, lambda: mpc.VPC(configs.probe_config(64)), lambda: oracle.VpcOracle(configs.probe_config(64)), "unrolled"),
            ("vpc 32", 32, lambda: mpc.VPC(configs.probe_config(32)), lambda: oracle.VpcOracle(configs.probe_config(32)), "unrolled"),
            ("twin 64", 64, lambda: mpc.VPC(probe_layout_config(configs, 64, (5, 3, 2))),
             lambda: oracle.VpcOracle(probe_layout_config(configs, 64, (5, 3, 2))), "unrolled, general layout"),
            ("bdi 64", 64, lambda: mpc.BDI(64), lambda: oracle.BdiOracle(64), "unrolled")]
    pools = {L: capped_pool(traces, L, max(CAPPED_COUNTS)) for L in (64, 32)}
    for name, L, make_ev, make_o, form in rows:
        ev, ref = make_ev(), OracleRef(make_o())
        assert (mpc.lib().mpc_kernel_form(ev._h) or b"").decode() == form, name
        sweep(ev, [ref], pools[L], counts=CAPPED_COUNTS, offsets=(16,), modes_at=(), tag=name)
        for n in CAPPED_COUNTS:
            for poison in POISON_SEEDS:
                check_call(ev, [ref], pools[L][:n], 16, "sizes only", poison, tag=name)
        res[name] = routes(ev)
        ev.close()
    members = [mpc.BDI(32), mpc.FPC(32), mpc.BPC(32)]
    group = mpc.EvaluatorSet(members)
    assert group.form == "BDI+FPC+BPC: one kernel", group.form
    refs = [OracleRef(oracle.BdiOracle(32)), OracleRef(oracle.FpcOracle(32)), OracleRef(oracle.BpcOracle(32))]
    sweep(group, refs, pools[32], counts=CAPPED_COUNTS, offsets=(16,), modes_at=(), tag="group 32")
    for n in CAPPED_COUNTS:
        for poison in POISON_SEEDS:
            check_call(group, refs, pools[32][:n], 16, "sizes only", poison, tag="group 32")
    res["group 32"] = routes(members[0])
    group.close()
    for ev in members:
        ev.close()
    return res
