"""CPU oracle pinned against (a) the known answers SURVEY.md 8c / BASELINE.md 2
captured from the reference's object code, (b) vectors produced by the
reference's own stage classes (tests/golden/ref_stage_vectors.json), and
(c) the outputs of that same reference build for further seeded inputs
(tests/golden/ref_live_vectors.npz), checked live as well where oracle/_ref is built."""
import ctypes as C
import json
import os

import numpy as np
import pytest


# ---------------------------------------------------------------- known answers
def test_kat_vpc_zero_wordsame_random(oracle, configs, traces):
    v = oracle.VpcOracle(configs.probe_config(64))
    s, sel = v.compress(traces.zeros(1000))
    assert (s == 3).all() and (sel == 0).all()
    assert repr(v.st.comp_ratio) == "170.66666666666666"
    v.reset()
    s, sel = v.compress(traces.word_same(1000))
    assert (s == 35).all() and (sel == 1).all()
    v.reset()
    s, sel = v.compress(traces.random_u32(4096))
    assert (s == 515).all() and (sel == -1).all()
    assert repr(v.st.comp_ratio) == "0.9941747572815534"


def test_kat_vpc_sine(oracle, configs, traces):
    # 4096-line fp32 sine: 3456 lines at 515 (cluster -1), rest cluster 5,
    # total 2 105 344 bits
    v = oracle.VpcOracle(configs.probe_config(64))
    s, sel = v.compress(traces.sine_f32(4096))
    assert int((s == 515).sum()) == 3456
    assert int((sel == -1).sum()) == 3456 and int((sel == 5).sum()) == 640
    assert int(s.astype(np.int64).sum()) == 2105344
    assert v.st.compressed_bits == 2105344


def test_kat_vpc_128(oracle, configs, traces):
    v = oracle.VpcOracle(configs.probe_config(128))
    s, sel = v.compress(traces.random_u32(64, 128))
    assert (s == 1027).all() and (sel == -1).all()


def test_kat_bdi(oracle, traces):
    b = oracle.BdiOracle(64)
    assert (b.compress(traces.zeros(8))[0] == 12).all()
    rep = np.tile(np.arange(1, 9, dtype=np.uint8), (8, 8))
    s, sel = b.compress(rep)
    assert (s == 68).all() and (sel == 1).all()
    s, sel = b.compress(traces.random_u32(2000))
    assert (s == 516).all() and (sel == 8).all()
    b128 = oracle.BdiOracle(128)
    s, sel = b128.compress(traces.pointers_u64(4096))
    assert (s == 564).all() and (sel == 4).all()  # all B8D4


def test_bdi_reduce_sign_quirks(oracle):
    rs = oracle.lib().mpc_o_bdi_reduce_sign
    M = (1 << 64) - 1
    assert rs(5) == 5 and rs(255) == 255
    assert rs(M) == M                      # -1 is returned unchanged -> never fits
    assert rs(M - 1) == 2                  # -2 -> 0b10
    assert rs((-128) & M) == 0x80          # -128 -> 8 low bits
    assert rs((-129) & M) == 0x17F         # -129 -> 9 low bits
    assert rs(1 << 63) == (1 << 63)        # i = 62 -> keeps 64 bits


def test_bdi_all_immediate_wrap(oracle):
    # all values immediate: (maskSize - imm - 1) wraps in 32-bit unsigned (BDI.cpp:200)
    line = np.arange(64, dtype=np.uint8) % 7
    line[1::2] = 0
    L = 64
    got = oracle.lib().mpc_o_bdi_check(line.ctypes.data, L, 2, 1)
    n = L // 2
    assert got == (n + 8 * (n * 1 + 2 - 1)) % (1 << 32)


# ------------------------------------------------------- golden reference vectors
def _module(oracle, v):
    m = oracle.OModule()
    L = v["L"]
    m.kind = oracle.KIND_PREDCOMP
    m.pred_kind = v["kind"]
    m.root = v["root"]
    m.consecutive_xor = v["cx"]
    for j in range(L):
        m.base[j] = v["base"][j] if v["base"] else 0
        m.weight[j] = v["weight"][j] if v["weight"] else 1.0
        m.diff[j] = v["diff"][j] if v["diff"] else 0
    if v["scan"] is None:
        rows = [i // L for i in range(8 * L)]
        cols = [i % L for i in range(8 * L)]
    else:
        rows, cols = v["scan"]["rows"], v["scan"]["cols"]
    m.table_size = len(rows)
    for j in range(len(rows)):
        m.rows[j] = rows[j]
        m.cols[j] = cols[j]
    return m


def test_oracle_matches_golden_stage_vectors(oracle, golden_dir):
    with open(os.path.join(golden_dir, "ref_stage_vectors.json")) as f:
        g = json.load(f)
    lib = oracle.lib()
    assert len(g["stage_vectors"]) >= 100
    for v in g["stage_vectors"]:
        L = v["L"]
        m = _module(oracle, v)
        line = np.frombuffer(bytes.fromhex(v["line"]), dtype=np.uint8).copy()
        pred = np.zeros(L, np.uint8)
        res = np.zeros(L, np.uint8)
        sc = np.zeros(8 * L // 16, np.uint16)
        lib.mpc_o_predict(C.byref(m), L, line.ctypes.data, pred.ctypes.data)
        lib.mpc_o_residue(C.byref(m), L, line.ctypes.data, res.ctypes.data)
        lib.mpc_o_scanned(C.byref(m), L, line.ctypes.data, sc.ctypes.data)
        assert pred.tobytes().hex() == v["pred"]
        assert res.tobytes().hex() == v["residue"]
        assert [int(x) for x in sc] == v["scanned"]
        assert lib.mpc_o_fpc_size(sc.ctypes.data, len(sc)) == v["fpc"]
        # GetMAE/GetMSE: residues over all positions as unsigned bytes
        r = (line.astype(np.int64) - pred.astype(np.int64)) % 256
        assert float(r.sum()) / L == float.fromhex(v["mae"])
        assert float((r * r).sum()) / L == float.fromhex(v["mse"])
    for e in g["encoder_vectors"]:
        rows = np.array(e["rows"], dtype=np.uint16)
        assert lib.mpc_o_fpc_size(rows.ctypes.data, len(rows)) == e["size"]


# ------------------------------------------------------ live reference stage build
def _live_vectors():
    """The seeded case generators of tests/golden/make_ref_live_vectors.py and the reference outputs it stored."""
    import importlib.util
    here = os.path.dirname(os.path.abspath(__file__))
    spec = importlib.util.spec_from_file_location("make_ref_live_vectors",
                                                  os.path.join(here, "golden", "make_ref_live_vectors.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen, np.load(gen.FIXTURE)


def test_oracle_matches_live_reference_stages(oracle, configs):
    """The probe configuration's prediction modules on random, sparse, ramp and sine lines: scanned arrays and
    common-encoder sizes of the reference's compiled classes (stored in tests/golden/ref_live_vectors.npz; where
    oracle/_ref is built, the live build is checked against the stored outputs as well)."""
    gen, fx = _live_vectors()
    cases = gen.stage_cases(oracle, configs)
    assert gen.digest(cases) == str(fx["stage_inputs_sha256"]), "regenerated inputs differ from the fixture's"
    ref_scs = gen.split(fx["stage_scanned"], cases, lambda L: 8 * L // 16)
    R = oracle.ref_lib()
    lib = oracle.lib()
    for i, (c, ref_sc, ref_fpc) in enumerate(zip(cases, ref_scs, fx["stage_fpc"])):
        if R is not None:
            assert (gen.ref_scanned(R, c) == ref_sc).all(), i
            assert R.ref_fpc_size(ref_sc.ctypes.data, len(ref_sc)) == ref_fpc, i
        my_sc = np.zeros(8 * c.L // 16, np.uint16)
        lib.mpc_o_scanned(C.byref(c.m), c.L, c.line.ctypes.data, my_sc.ctypes.data)
        assert (ref_sc == my_sc).all(), i
        assert ref_fpc == lib.mpc_o_fpc_size(my_sc.ctypes.data, len(my_sc)), i


def test_oracle_matches_live_reference_odd_weights(oracle):
    """WeightBase tables with weights that are not powers of two and with extreme weights:
    (int)log2f(w) truncates toward zero (PredictorModule.cpp:30).  Against the outputs of the reference's
    compiled classes (stored in tests/golden/ref_live_vectors.npz; live as well where oracle/_ref is built);
    the same kind of tables are also in the committed stage vectors."""
    gen, fx = _live_vectors()
    cases = gen.odd_weight_cases(oracle)
    assert gen.digest(cases) == str(fx["odd_inputs_sha256"]), "regenerated inputs differ from the fixture's"
    ref_ps = gen.split(fx["odd_pred"], cases, lambda L: L)
    ref_scs = gen.split(fx["odd_scanned"], cases, lambda L: 8 * L // 16)
    R = oracle.ref_lib()
    lib = oracle.lib()
    for i, (c, ref_p, ref_sc) in enumerate(zip(cases, ref_ps, ref_scs)):
        if R is not None:
            assert (gen.ref_predict(R, c) == ref_p).all(), i
            assert (gen.ref_scanned(R, c) == ref_sc).all(), i
        my_p = np.zeros(c.L, np.uint8)
        lib.mpc_o_predict(C.byref(c.m), c.L, c.line.ctypes.data, my_p.ctypes.data)
        assert (ref_p == my_p).all(), i
        my_sc = np.zeros(8 * c.L // 16, np.uint16)
        lib.mpc_o_scanned(C.byref(c.m), c.L, c.line.ctypes.data, my_sc.ctypes.data)
        assert (ref_sc == my_sc).all(), i


# ------------------------------------------------- reference-derived whole-line vectors
def test_oracle_matches_reference_line_vectors(oracle):
    """Whole lines of the BASELINE workloads: per prediction module the oracle's scanned array has the
    leading-zero-row count and the common-encoder size the reference's compiled classes produced
    (tests/golden/ref_line_vectors.json), and the oracle's per-line (size, selected) is what the
    selector / decision rule of VPC.cpp:366-415 gives on those reference numbers."""
    import ref_lines
    lib = oracle.lib()
    cases = ref_lines.load_cases()
    assert len(cases) >= 10
    for name, cfg, lines, c in cases:
        oc = oracle.config_from_json(cfg)
        L = oc.line_size
        rows = 8 * L // 16
        z, enc = np.array(c["z"]), np.array(c["enc"])
        sc = np.zeros(rows, np.uint16)
        step = 1 if len(lines) <= 600 else 3          # the stage check on every third line of the long traces
        for n in range(0, len(lines), step):
            for q, mi in enumerate(c["module_index"]):
                lib.mpc_o_scanned(C.byref(oc.modules[mi]), L, lines[n].ctypes.data, sc.ctypes.data)
                nz = np.flatnonzero(sc)
                assert (int(nz[0]) if len(nz) else rows) == z[n, q], (name, n, q)
                assert lib.mpc_o_fpc_size(sc.ctypes.data, rows) == enc[n, q], (name, n, q)
        size, sel = ref_lines.expected_sizes(oracle, cfg, lines, c)
        s, k = oracle.VpcOracle(cfg).compress(lines)
        assert (s == size).all() and (k == sel).all(), name
        # the traces must keep exercising the selector: several modules win, and ties occur
        if name.startswith("structured/64"):
            assert len(set(sel.tolist())) >= 4
            assert (np.sort(z, axis=1)[:, -1] == np.sort(z, axis=1)[:, -2]).any()


# ------------------------------------------------------------ statistics plumbing
def test_stats_consistency(oracle, configs, traces):
    v = oracle.VpcOracle(configs.probe_config(64))
    lines = np.concatenate([traces.zeros(10), traces.word_same(7), traces.mixed(500),
                            traces.random_u32(100)])
    s, sel = v.compress(lines)
    st = v.st
    assert st.lines == len(lines)
    assert st.original_bits == 512 * len(lines)
    assert st.compressed_bits == int(s.astype(np.int64).sum())
    h = v.hist()
    for c in range(-1, 6):
        k = c + 1
        assert st.count[k] == int((sel == c).sum())
        assert int(h[k].sum()) == st.count[k]
        # MAE/MSE only for lines that reached checkOtherPatterns (VPC.cpp:412)
        expect = 0 if c in (0, 1) else st.count[k]
        assert st.residue_lines[k] == expect
        if expect:
            # integer sums reproduce the reference's running doubles (L power of 2)
            assert st.sum_mae[k] == st.sum_r[k] / 64.0
            assert st.sum_mse[k] == st.sum_r2[k] / 64.0
    vec = v.stats_vector()
    assert vec[0] == len(lines) and len(vec) == 3 + 7 * 6 + 7 * v.bins


def test_rejects_ub_configs(oracle, configs):
    cfg = configs.probe_config(64)
    cfg["modules"]["0"], cfg["modules"]["2"] = cfg["modules"]["2"], cfg["modules"]["0"]
    with pytest.raises(ValueError):
        oracle.VpcOracle(cfg)
    cfg = configs.make_config(64, [{"name": "AllZero"}, configs.consecutive_base(64, root=3)])
    with pytest.raises(ValueError):
        oracle.VpcOracle(cfg)


def test_only_allzero_config(oracle, configs, traces):
    # no prediction module: empty scanned array -> size 0 + id bits, cluster -1
    cfg = configs.make_config(64, [{"name": "AllZero"}])
    v = oracle.VpcOracle(cfg)
    s, sel = v.compress(traces.random_u32(4))
    assert (s == 1).all() and (sel == -1).all()


def test_bdi_screen_stress_trace_reaches_every_outcome(oracle, traces):
    """The trace that drives the BDI kernel's screening thresholds on the GPU must keep
    exercising every (base, delta) selection and the uncompressed outcome."""
    for L in (32, 64, 128):
        o = oracle.BdiOracle(L)
        _, sel = o.compress(traces.bdi_screen_stress(4800, L))
        assert set(np.unique(sel)) >= {2, 3, 4, 5, 6, 7, 8}, (L, np.unique(sel))


def test_kat_fpc_by_hand(oracle):
    """FPC sizes worked out by hand from FPC.cpp:16-84 (prefix 3 bits + payload; a zero run costs 6
    bits once).  The reference ships no fixture for FPC: these pin the restatement to the source
    reading only."""
    o = oracle.FpcOracle(64)

    def size(words):
        return int(o.compress(np.array(words, dtype="<u4").view(np.uint8).reshape(1, -1))[0])
    assert size([0] * 16) == 6
    assert size([5] * 16) == 16 * 7 and size([0xFFFFFFF9] * 16) == 16 * 7
    assert size([100] * 16) == 16 * 11 and size([0xFFFFFF80] * 16) == 16 * 11
    assert size([1000] * 16) == 16 * 19 and size([0x12340000] * 16) == 16 * 19
    assert size([0x007F0001] * 16) == 16 * 19 and size([0xFF80FF81] * 16) == 16 * 19
    assert size([0xABABABAB] * 16) == 16 * 11 and size([0x12345678] * 16) == 16 * 35
    assert size([0, 0, 5, 0, 0, 0, 7, 0] + [0x12345678] * 8) == 6 + 7 + 6 + 7 + 6 + 8 * 35
    assert size([1] + [0] * 15) == 7 + 6                 # a run that reaches the end of the line
    assert o.st.total_words == 13 * 16 and sum(o.st.counts) == 13 * 16


def test_kat_bpc_by_hand(oracle):
    """BPC sizes worked out by hand from BPC.cpp:20-185: first word always 3+4 bits; 33 delta bit
    planes, zero-DBX runs 3 / 7 bits, zero DBP or all-ones (31 deltas only) 5, one 1 or two adjacent
    1s 10, else 32.  No reference fixture exists for BPC: source reading only."""
    def size(L, words):
        o = oracle.BpcOracle(L)
        return int(o.compress(np.array(words, dtype="<u4").view(np.uint8).reshape(1, -1))[0]), o
    for L in (32, 64, 128):
        n = L // 4
        assert size(L, [0] * n)[0] == 7 + 7                       # one run of 33 zero planes
        assert size(L, [0xDEADBEEF] * n)[0] == 7 + 7              # all deltas zero
        s, o = size(L, list(range(n)))                            # delta +1: plane 0 all ones, planes 32..1 zero
        assert s == 7 + 7 + (5 if L == 128 else 32) and o.st.total_words == 33
        s, o = size(L, list(range(n, 0, -1)))                     # delta -1: every plane all ones, DBX only on plane 32
        assert s == 7 + (5 if L == 128 else 32) + 7
        s, o = size(L, [0] * (n - 1) + [1])                       # one delta of +1 in the last row: single one on plane 0
        assert s == 7 + 7 + 10 and list(o.st.counts) == [0, 1, 0, 1, 0, 0, 0]
        s, o = size(L, [0] * (n - 2) + [1, 2])                    # two adjacent ones on plane 0
        assert s == 7 + 7 + 10 and list(o.st.counts) == [0, 1, 0, 0, 1, 0, 0]
        s, o = size(L, [0, 2] + [2] * (n - 2))                    # a single +2: single one on plane 1, then plane 0: DBP 0 -> "Zero"
        assert s == 7 + 7 + 10 + 5 and list(o.st.counts) == [0, 1, 1, 1, 0, 0, 0]
    rnd = np.random.default_rng(1).integers(0, 256, (1, 64), dtype=np.uint8)
    assert int(oracle.BpcOracle(64).compress(rnd)[0]) == 7 + 33 * 32      # nothing compresses: larger than the line

