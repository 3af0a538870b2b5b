"""Every configuration of tests/vpc_plan_cases.py on the kernel its plan picks, against the CPU oracle.

tests/test_vpc_plan_cpu.py shows without a device that the plan is the table's and that the planned kernel's inputs
name the configured bytes; here the kernel runs.  One test per case, so that a case costs one compilation at most
(2.5-5 s; the code objects are cached for the module).  Lines, at most 4096 per case: the walking-one and
leading-zero-rows families of every prediction module (tests/vpc_synth.py: one bit in the scanned array under the TRUE
predictor -- a wrong base byte, shift or mask turns it into many; a seeded sample of them where a configuration has
more than fit), a seeded sample of the other families, 512 structured and 256 random lines, all-zero and word-same
lines; in a seeded order, in four calls of 128 k + r lines, r = 0, 1, 63, 65.  Per-line sizes and selectors and the
statistics vector must equal the oracle's; then the statistics-only instantiation; then the same configuration under
MPC_JIT=0, on the form of expected_plan's no-compiler column.

Against the planner before its fix the four back8_*_shift_classes cases failed here with per-line mismatches (wrong
sizes, no fault), e.g.
  back8_3_shift_classes_root_0_L128 (compiler): 1773 of 2433 lines differ from the oracle ... line 0 [family
  walking_one, module 2, scan position 981]: size 33 vs 23, selector 2 vs 2
(root 5, 32 bytes: 596 of 1409; four classes, 64 bytes: 1011 of 1793; four classes, root 5, 128 bytes: 1553 of 2305)."""
import numpy as np
import pytest

from conftest import pkg

import vpc_plan_cases as P
import vpc_ref
import vpc_synth as S

pytestmark = pytest.mark.gpu

MAX_LINES, STRUCTURED, RANDOM, OTHER = 4096, 512, 256, 200


@pytest.fixture(scope="module")
def mpc():
    m = pkg()
    m.lib()
    return m


@pytest.fixture(scope="module")
def jit_cache(tmp_path_factory):
    return str(tmp_path_factory.mktemp("jit"))


def case_lines(name, cfg, traces):
    """-> (calls: the lines of the four calls, label per line)."""
    L = int(cfg["overview"]["lineSize"])
    seed = sum(name.encode()) + L
    rng = np.random.default_rng(seed)
    must, other = [], []
    for b in S.build(cfg, seed=seed % 97):
        into = must if b["family"] in ("walking_one", "leading_zero_rows") else other
        into += [(line, f"family {b['family']}, module {b['module']}, {lb}") for line, lb in zip(b["lines"], b["labels"])]
    edge = [(np.zeros(L, np.uint8), "all-zero")] * 8 + [(line, "word-same") for line in traces.word_same(16, L, seed=seed)]
    fixed = STRUCTURED + RANDOM + len(edge) + 128 + 65            # (the last call is filled up from the first lines)
    other = [other[i] for i in np.sort(rng.choice(len(other), min(OTHER, len(other)), replace=False))]
    room = MAX_LINES - fixed - len(other)
    if len(must) > room:
        must = [must[i] for i in np.sort(rng.choice(len(must), room, replace=False))]
    wide = 128 if L <= 128 else 256
    pool = must + other + edge + [(line, "structured") for line in traces.structured(STRUCTURED, wide, seed=seed)[:, :L]] \
        + [(line, "random") for line in traces.random_u32(RANDOM, wide, seed=seed)[:, :L]]
    order = rng.permutation(len(pool))
    lines = np.ascontiguousarray(np.array([pool[i][0] for i in order], np.uint8).reshape(-1, L))
    labels = [pool[i][1] for i in order]
    n, at, calls, lab = len(lines), 0, [], []
    for j, r in enumerate(S.TAILS):
        want = n * (j + 1) // 4 - at
        size = 128 * max(((want - r + 127) if j == 3 else (want - r)) // 128, 1) + r
        idx = np.arange(at, at + size) % n
        calls.append(np.ascontiguousarray(lines[idx]))
        lab += [labels[i] for i in idx]
        at += size
    assert sum(len(c) for c in calls) <= MAX_LINES and [len(c) % 128 for c in calls] == list(S.TAILS), name
    return calls, lab


def _explain(name, what, lab, s, k, s_ref, k_ref):
    bad = np.nonzero((s != s_ref) | (k != k_ref))[0]
    if bad.size == 0:
        return None
    kinds = sorted({", ".join(lab[i].split(", ")[:2]) for i in bad})
    first = "; ".join(f"line {i} [{lab[i]}]: size {s[i]} vs {s_ref[i]}, selector {k[i]} vs {k_ref[i]}" for i in bad[:5])
    return f"{name} ({what}): {bad.size} of {len(s)} lines differ from the oracle, in {kinds[:8]}; {first}"


def _run(mpc, name, what, cfg, form, calls, lab, ref, per_line):
    s_ref, k_ref, v_ref = ref
    ev = mpc.VPC(cfg)
    try:
        assert vpc_ref.form_of(ev.kernel_form) == form, f"{name} ({what}): runs {ev.kernel_form!r} ({ev.path_reason}), planned {form!r}"
        if per_line:
            out = [ev.compress_lines(c) for c in calls]
            msg = _explain(name, what, lab, np.concatenate([o[0] for o in out]), np.concatenate([o[1] for o in out]), s_ref, k_ref)
            assert msg is None, msg
        else:
            for c in calls:
                ev.compress_lines(c, want_sizes=False, want_selected=False)
        v = ev.stats_vector()
        assert (v == v_ref).all(), f"{name} ({what}{'' if per_line else ', statistics only'}): statistics differ at {np.nonzero(v != v_ref)[0][:10]}"
    finally:
        ev.close()


@pytest.mark.parametrize("name", list(P.ALL))
def test_planned_kernel_against_oracle(mpc, oracle, traces, jit_cache, monkeypatch, name):
    monkeypatch.setenv("MPC_JIT_CACHE", jit_cache)
    monkeypatch.delenv("MPC_JIT", raising=False)
    monkeypatch.delenv("MPC_JIT_MAX_MODULES", raising=False)
    cfg = P.ALL[name]()
    calls, lab = case_lines(name, cfg, traces)
    o = oracle.VpcOracle(cfg)
    s_ref, k_ref = o.compress(np.concatenate(calls))
    ref = (s_ref, k_ref, o.stats_vector())
    # what the description says without a device is what the handle launches
    form = vpc_ref.described_form(mpc.describe_config(cfg))
    want = P.expected_plan(cfg, True)
    assert form.split(",")[0] == (want["sequence"] or "generic"), (name, form, want)
    _run(mpc, name, "compiler", cfg, form, calls, lab, ref, True)
    _run(mpc, name, "compiler", cfg, form, calls, lab, ref, False)
    monkeypatch.setenv("MPC_JIT", "0")
    form0 = vpc_ref.described_form(mpc.describe_config(cfg))
    want0 = P.expected_plan(cfg, False)
    assert form0.split(",")[0] == (want0["sequence"] or "generic") and "at creation" not in form0, (name, form0, want0)
    _run(mpc, name, "MPC_JIT=0", cfg, form0, calls, lab, ref, True)
