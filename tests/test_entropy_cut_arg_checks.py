"""The entropy cuts' argument checks.  The launcher's status codes (asd_entropy_cut_rows rejects, or finds nothing to do, before
anything is launched, so the calls below need no GPU and dereference nothing), in the order the other launchers use: negative
sizes, the empty call, unsupported, NULL / strides, alignment.  Then the ValueErrors of serving/stage_args.py::check_entropy_cuts,
of kernels.check_entropy_cut_rows and of Stage.generate, which refuses before the prompts are encoded and before any ops call."""
import ctypes as C

import numpy as np
import pytest

import asd_amd
from asd_amd import _binding as B
from asd_amd import kernels as K
from asd_amd.serving.stage_args import CUT_EPSILON, CUT_ETA, CUT_OFF, CUT_TYPICAL, check_entropy_cuts
from asd_amd.serving.stages import StageConfig, StageManager
from tests.entropy_cut_ref import VOCAB, EntropyCutOracleOps
from tests.oracle_backend import OracleBackend
from tests.stage_scenario import NAMES, PROMPTS, stage_configs

OK, INVALID, UNSUPPORTED, ALIGNMENT = 0, -1, -2, -5
BF16, F32 = B.DTYPE_BF16, B.DTYPE_F32


@pytest.fixture(autouse=True)
def oracle_backend():
    asd_amd.set_backend(OracleBackend())
    yield
    asd_amd.set_backend(None)


def test_launcher_status_codes():
    lib = B.load_library()
    buf = (C.c_ubyte * 512)()
    p = (C.addressof(buf) + 255) & ~255                                      # stands for every device buffer: aligned, never read
    nb, K1, V = 4, 5, 1024

    def call(x=p, dt=BF16, b=nb, k1=K1, v=V, lds=K1 * V, ldr=V, table=p):
        return lib.asd_entropy_cut_rows(x, dt, b, k1, v, lds, ldr, table, None)
    assert call(b=-1) == INVALID and call(k1=-1) == INVALID and call(v=-1) == INVALID
    assert call(b=-1, k1=0) == INVALID                                       # ... before the empty call
    for zero in (dict(b=0), dict(k1=0), dict(v=0)):
        assert call(x=None, dt=99, table=None, lds=0, ldr=0, **zero) == OK   # nothing to do: nothing else is looked at
    assert call(dt=99) == UNSUPPORTED
    assert call(x=None, dt=99) == UNSUPPORTED                                # unsupported before NULL
    assert call(b=2 ** 31 - 1, k1=2, lds=2 * V) == UNSUPPORTED               # B * K1 > INT32_MAX
    assert call(dt=F32, v=2 ** 29, ldr=2 ** 29, lds=K1 * 2 ** 29) == UNSUPPORTED     # V * 4 > INT32_MAX
    assert call(dt=BF16, v=2 ** 30, ldr=2 ** 30, lds=K1 * 2 ** 30) == UNSUPPORTED    # V * 2 > INT32_MAX
    assert call(x=None, v=2 ** 30, ldr=0) == UNSUPPORTED                     # ... before NULL and before the strides
    assert call(x=None) == INVALID and call(table=None) == INVALID
    assert call(x=None, ldr=V - 1) == INVALID
    assert call(ldr=V - 1) == INVALID and call(lds=K1 * V - 1) == INVALID
    assert call(x=p + 1, ldr=V - 1) == INVALID                               # invalid before alignment
    assert call(x=p + 1) == ALIGNMENT and call(dt=F32, x=p + 2) == ALIGNMENT
    assert call(table=p + 2) == ALIGNMENT
    assert B.ENTROPY_CUT_REC_BYTES == 12


def test_check_entropy_cuts():
    f = lambda v: float(np.float32(v))                                       # noqa: E731
    assert check_entropy_cuts(1.0, 0.0, 0.0, 3) == [(CUT_OFF, 0.0)] * 3
    assert check_entropy_cuts(0, 0, 0, 2) == [(CUT_OFF, 0.0)] * 2
    assert check_entropy_cuts(0.9, 0.0, 0.0, 2) == [(CUT_TYPICAL, f(0.9))] * 2
    assert check_entropy_cuts(1.0, np.float32(3e-4), 0, 1) == [(CUT_EPSILON, f(3e-4))]
    assert check_entropy_cuts([0.2, 1.0, 0.0], [0.0, 0.01, 0.0], (0, 0, 0.5), 3) == \
        [(CUT_TYPICAL, f(0.2)), (CUT_EPSILON, f(0.01)), (CUT_ETA, f(0.5))]
    for bad in (True, float("nan"), -0.1, 1.5, "0.5", None, [0.5], [0.5, 0.5, 0.5], [0.5, None]):
        with pytest.raises(ValueError, match="typical_p"):
            check_entropy_cuts(bad, 0.0, 0.0, 2)
    for name, args in (("epsilon_cutoff", lambda v: (1.0, v, 0.0)), ("eta_cutoff", lambda v: (1.0, 0.0, v))):
        for bad in (False, float("nan"), -1e-3, 1.0, 2, "x", None, [0.1], [0.1, True]):
            with pytest.raises(ValueError, match=name):
                check_entropy_cuts(*args(bad), 2)
    for two in ((0.5, 0.1, 0.0), (0.5, 0.0, 0.1), (1.0, 0.1, 0.1), ([1.0, 0.5], [0.0, 0.1], 0.0)):
        with pytest.raises(ValueError, match="not built"):
            check_entropy_cuts(*two, 2)


def test_check_entropy_cut_rows():
    rec = K.check_entropy_cut_rows([1.0, 2.0], [0, 1], [0.0, 0.5])
    assert rec.dtype.itemsize == 12 and rec["mode"].tolist() == [0, 1] and rec["value"].tolist() == [0.0, 0.5]
    for bad in (([1.0], [1, 1], [0.5, 0.5]), ([1.0], [4], [0.5]), ([1.0], [True], [0.5]), ([0.0], [1], [0.5]),
                ([float("inf")], [1], [0.5]), ([float("nan")], [0], [0.0]), ([1.0], [1], [0.0]), ([1.0], [2], [1.0]),
                ([1.0], [3], [float("nan")])):
        with pytest.raises(ValueError):
            K.check_entropy_cut_rows(*bad)


@pytest.mark.parametrize("name", NAMES)
def test_generate_refuses_before_encoding(name):
    ops = EntropyCutOracleOps()
    stage = StageManager(stage_configs(vocab=VOCAB), ops=ops).get_stage(name)
    encoded = []
    stage._encode = lambda prompts, _orig=stage._encode: (encoded.append(1), _orig(prompts))[1]
    n = len(PROMPTS)
    for kw, match in ((dict(typical_p=True), "typical_p"), (dict(typical_p=1.5), "typical_p"), (dict(typical_p=[0.5] * (n - 1)), "typical_p"),
                      (dict(epsilon_cutoff=1.0), "epsilon_cutoff"), (dict(epsilon_cutoff=float("nan")), "epsilon_cutoff"),
                      (dict(eta_cutoff=-0.5), "eta_cutoff"), (dict(eta_cutoff="0.1"), "eta_cutoff"),
                      (dict(typical_p=0.5, eta_cutoff=0.1), "not built"),
                      (dict(typical_p=[0.5] + [1.0] * (n - 1), epsilon_cutoff=[0.1] + [0.0] * (n - 1)), "not built")):
        for temperature in (0.7, 0.0):                                       # greedy ignores the values, not their errors
            with pytest.raises(ValueError, match=match):
                stage.generate(prompts=PROMPTS, max_tokens=2, temperature=temperature, **kw)
    assert not encoded and not ops.trace
    stage.generate(prompts=PROMPTS, max_tokens=2, temperature=0.7, typical_p=0.5)
    assert encoded and "entropy_cut_rows" in [c for c, _ in ops.trace]


def test_configuration_values():
    """None takes the configuration's value; a stage refuses a bad configuration when it is built; a keyword beside a
    configured mode of another kind is two modes on one row."""
    with pytest.raises(ValueError, match="eta_cutoff"):
        StageManager(stage_configs(vocab=VOCAB, eta_cutoff=1.0), ops=EntropyCutOracleOps())
    with pytest.raises(ValueError, match="not built"):
        StageManager(stage_configs(vocab=VOCAB, target_typical_p=0.5, target_epsilon_cutoff=0.1), ops=EntropyCutOracleOps())
    cfg = StageConfig()
    assert (cfg.typical_p, cfg.epsilon_cutoff, cfg.eta_cutoff) == (1.0, 0.0, 0.0)
    assert (cfg.target_typical_p, cfg.target_epsilon_cutoff, cfg.target_eta_cutoff) == (1.0, 0.0, 0.0)
    ops = EntropyCutOracleOps()
    sm = StageManager(stage_configs(vocab=VOCAB, typical_p=0.5, target_typical_p=0.6), ops=ops)
    for name in NAMES:
        stage = sm.get_stage(name)
        del ops.trace[:]
        stage.generate(prompts=PROMPTS, max_tokens=2, temperature=0.7, typical_p=None)
        assert "entropy_cut_rows" in [c for c, _ in ops.trace]
        with pytest.raises(ValueError, match="not built"):
            stage.generate(prompts=PROMPTS, max_tokens=2, temperature=0.7, epsilon_cutoff=0.1)
        stage.generate(prompts=PROMPTS, max_tokens=2, temperature=0.7, typical_p=1.0, epsilon_cutoff=0.1)    # the keyword replaces it
