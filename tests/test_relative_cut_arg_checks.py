"""The relative cuts' argument checks, all without a GPU: both new launchers' status codes (they reject, or find nothing to do,
before anything is launched), check_relative_cuts, and Stage.generate, which refuses before the prompts are encoded and before
any ops call."""
import ctypes as C

import pytest

import asd_amd
from asd_amd import _binding as B
from asd_amd.serving.stage_args import check_relative_cuts
from asd_amd.serving.stages import StageManager
from tests.mirostat_ref import VOCAB, MirostatOracleOps
from tests.oracle_backend import OracleBackend
from tests.stage_scenario import NAMES, PROMPTS, stage_configs

OK, INVALID, UNSUPPORTED, ALIGNMENT = 0, -1, -2, -5
BUF = (C.c_ubyte * 512)()
P = (C.addressof(BUF) + 255) & ~255                                          # stands for every device buffer: aligned, never read


@pytest.fixture(autouse=True)
def oracle_backend():
    asd_amd.set_backend(OracleBackend())
    yield
    asd_amd.set_backend(None)


def test_launcher_status_codes():
    def cut(x=P, dt=B.DTYPE_BF16, b=4, k1=5, v=1024, lds=5 * 1024, ldr=1024, table=P, coins=P, ldc=5):
        return B.load_library().asd_relative_cut_rows(x, dt, b, k1, v, lds, ldr, table, coins, ldc, None)
    assert cut(b=-1) == cut(k1=-1) == cut(v=-1) == INVALID
    assert cut(x=None, dt=99, b=0) == cut(x=None, dt=99, v=0) == OK
    assert cut(dt=99) == cut(x=None, v=2 ** 30, ldr=0) == UNSUPPORTED
    assert cut(x=None) == cut(table=None) == cut(ldr=1023) == cut(lds=5 * 1024 - 1) == cut(ldc=4) == INVALID
    assert cut(x=P + 1) == cut(dt=B.DTYPE_F32, x=P + 2) == cut(table=P + 2) == cut(coins=P + 2) == ALIGNMENT
    assert B.RELATIVE_CUT_REC_BYTES == 16

    def uni(b=4, kd=3, ka=3, rd=P, u=P, rc=P, coin=P, kc=4, seeds=P):
        return B.load_library().asd_step_uniforms_ex(seeds, 0, 0, b, kd, ka, rd, u, rc, coin, kc, None)
    assert uni(b=0) == uni(kd=65) == uni(kc=66) == uni(kc=-1) == uni(seeds=None) == INVALID
    assert uni(coin=None) == uni(kc=0) == uni(rd=None, u=None, rc=None, coin=None, kc=0) == INVALID
    assert uni(coin=P + 2) == uni(seeds=P + 4) == ALIGNMENT


def test_check_relative_cuts():
    assert check_relative_cuts(0, 0, None, 0, 2) == [(0, 0.0, 0.0)] * 2
    assert check_relative_cuts([1.5, 0, 0], [0, 0.25, 0], 0.25, [0, 0, 0.5], 3) == [(1, 1.5, 0.0), (2, 0.25, 0.0), (3, 0.25, 0.5)]
    assert check_relative_cuts(0, 0, [0.125, 0.75], 0.5, 2, True) == [(3, 0.125, 0.5), (0, 0.0, 0.0)]     # off above 0.5
    for bad in (dict(top_n_sigma=1.0, top_a=0.5), dict(top_a=0.5, xtc_probability=0.5), dict(top_n_sigma=True),
                dict(top_a=float("nan")), dict(top_n_sigma=float("inf")), dict(top_a=1.5), dict(xtc_threshold=-0.1),
                dict(xtc_probability=[0.5]), dict(top_n_sigma="1"), dict(xtc_probability=0.5, xtc_threshold=0.6)):
        kw = dict(dict(top_n_sigma=0, top_a=0, xtc_threshold=None, xtc_probability=0), **bad)
        with pytest.raises(ValueError):
            check_relative_cuts(kw["top_n_sigma"], kw["top_a"], kw["xtc_threshold"], kw["xtc_probability"], 2, "xtc_probability" in bad)
    with pytest.raises(ValueError, match="top_a"):                                       # a bad configuration: when the stage is built
        StageManager(stage_configs(vocab=VOCAB, target_top_a=2.0), ops=MirostatOracleOps())


@pytest.mark.parametrize("name", NAMES)
def test_generate_refuses_before_encoding(name):
    ops = MirostatOracleOps()
    stage = StageManager(stage_configs(vocab=VOCAB, top_p=1.0), ops=ops).get_stage(name)
    encoded = []
    stage._encode = lambda prompts, _orig=stage._encode: (encoded.append(1), _orig(prompts))[1]
    n = len(PROMPTS)
    for kw, match in ((dict(top_n_sigma=1.0, top_a=0.5), "more than one"), (dict(top_a=0.5, xtc_probability=0.5), "more than one"),
                      (dict(top_n_sigma=1.0, typical_p=0.9), "not built"), (dict(xtc_probability=0.5, epsilon_cutoff=1e-3), "not built"),
                      (dict(top_a=0.5, mirostat_tau=5.0), "Mirostat"), (dict(xtc_probability=0.5, xtc_threshold=0.6), "usable"),
                      (dict(top_a=True), "top_a"), (dict(top_n_sigma=float("nan")), "top_n_sigma"),
                      (dict(xtc_probability=[0.5] * (n - 1)), "xtc_probability")):
        for temperature in (0.7, 0.0):                                       # greedy ignores the values, not their errors
            with pytest.raises(ValueError, match=match):
                stage.generate(prompts=PROMPTS, max_tokens=2, temperature=temperature, **kw)
    assert not encoded and not ops.trace
