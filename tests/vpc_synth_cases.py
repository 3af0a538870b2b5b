"""The configurations that the synthesised-line tests run (tests/test_vpc_synth_cpu.py, tests/test_vpc_synth_gpu.py): the
cases of tests/vpc_ref.py that have a prediction module, their companions, the built families of each (once per
process) and the random lines that the arrangements of tests/vpc_synth.py put around them."""
import functools

import numpy as np

from conftest import pkg

import vpc_ref
import vpc_synth as S

FREE_KINDS = ("OneBasePredictor", "DiffBasePredictor", "WeightBasePredictor")


# ---- companions -----------------------------------------------------------------------------------------------------
# A configuration whose last prediction module is ConsecutiveBase or has a forced byte cannot show the row classes and
# the ladder (they are built for the last module, which takes the ties).  It gets a companion of the same kernel form
# whose last module is free: one model, or the same models reordered.
def _companions():
    C, R = pkg("configs"), vpc_ref
    az, aws = R.AZ, R.AWS

    def swapped_tail(cfg_fn):
        def make():
            cfg = cfg_fn()
            M = int(cfg["overview"]["num_modules"])
            cfg["modules"][str(M - 1)], cfg["modules"][str(M - 2)] = cfg["modules"][str(M - 2)], cfg["modules"][str(M - 1)]
            return cfg
        return make
    bm = R._byte(64)
    return {
        # name: (companion of, form, configuration)
        # (general layout: FULL tables, so that the ladder reaches 8 L and the certificate of the general-layout kernels,
        # behind the rotated root, can close a line; the probe sequence with OneBase's root alone moved, and one model)
        "probe_root100_L64": ("root1_L64", "unrolled, general layout", lambda: C.make_config(64, R._probe_seq(64, (1, 0, 0)))),
        "one_root11_L64": ("root1_L64", "unrolled, general layout", lambda: C.make_config(64, [az, aws, C.one_base(64, 11, True)])),
        "one_root11_L32": ("root7_L32", "unrolled, general layout", lambda: C.make_config(32, [az, aws, C.one_base(32, 11, True)])),
        "one_root11_L128": ("root15_L128", "unrolled, general layout", lambda: C.make_config(128, [az, aws, C.one_base(128, 11, True)])),
        "probe_root100_L128": ("root15_L128", "unrolled, general layout",
                               lambda: C.make_config(128, R._probe_seq(128, (1, 0, 0)))),
        "one_root40_L64": ("jit_root40_L64", "unrolled, compiled at creation",
                           lambda: C.make_config(64, [az, aws, C.consecutive_base(64, 0, True), C.one_base(64, 40, True)])),
        "weights_last_L64": ("jit_weights_L64", "unrolled, compiled at creation", swapped_tail(R._cfg_jit_weights64)),
        "perm_one_last_L64": ("perm_L64", "generic", swapped_tail(R._cfg_perm64)),
        "loop_bm_one_last_L64": ("loop_bm_root_L64", "run-time loop",
                                 lambda: C.make_config(64, [az, aws, C.diff_base(64, R._prev(64, 4), R._lsb(64, 4), 5, False, bm),
                                                            C.one_base(64, 3, True, bm)])),
        "loop_many_one_last_L32": ("loop_many_L32", "run-time loop", swapped_tail(R._cfg_loop_many32)),
    }


COMPANIONS = _companions()
NAMES = [c["name"] for c in vpc_ref.CASES if vpc_ref.n_pred(vpc_ref.case_config(c)) > 0]
ALL = NAMES + sorted(COMPANIONS)


def config_of(name: str) -> dict:
    return COMPANIONS[name][2]() if name in COMPANIONS else vpc_ref._CONFIGS[name]()


def form_of(name: str) -> str:
    return COMPANIONS[name][1] if name in COMPANIONS else vpc_ref._SPECS[name]["form"]


@functools.lru_cache(maxsize=None)
def _oracle_built():
    from oracle import oracle as O
    O.build(ref=True)
    return O


@functools.lru_cache(maxsize=None)
def built(name: str):
    """vpc_synth.build of a configuration: once per process."""
    _oracle_built()
    out = S.build(config_of(name))
    for b in out:
        b["rows"].setflags(write=False)
        b["lines"].setflags(write=False)
    return out


def needs_companion(cfg: dict) -> bool:
    cons = S.residue_constraints(cfg, S.pred_modules(cfg)[-1])
    return cons["kind"] not in FREE_KINDS or not S.is_free(cons)




def filler(n: int, L: int, seed: int) -> np.ndarray:
    """Random lines for the planted and cold arrangements (the package's traces.random_u32, cut to L)."""
    return np.ascontiguousarray(pkg("traces").random_u32(n, 128 if L <= 128 else 256, seed=seed)[:, :L])


def planted_per_family(L: int):
    """The planted arrangement runs every built line up to 64-byte lines (where the kernels set lines aside); beyond, a
    seeded sample of at most 16384 / L lines of every (family, module), so that a case stays at a few seconds."""
    return None if L <= 64 else 16384 // L
