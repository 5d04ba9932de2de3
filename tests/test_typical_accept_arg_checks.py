"""Typical acceptance's argument checks, all without a GPU: the entry points' status codes and sizes, check_typical_accept, the
configuration's hand-on, and Stage.generate, which refuses before the prompts are encoded and before any ops call and makes the
calls it made before when the feature is off."""
import ctypes as C

import pytest

import asd_amd
from asd_amd import _binding as B
from asd_amd.serving.pipeline import PipelineConfig
from asd_amd.serving.stage_args import check_typical_accept
from asd_amd.serving.stages import StageManager
from tests.mirostat_ref import VOCAB
from tests.oracle_backend import OracleBackend
from tests.stage_scenario import NAMES, PROMPTS, stage_configs
from tests.typical_accept_ref import TypicalAcceptOracleOps

OK, INVALID, UNSUPPORTED, ALIGNMENT = 0, -1, -2, -5
BUF = (C.c_ubyte * 512)()
P = (C.addressof(BUF) + 255) & ~255                                          # stands for every device buffer: aligned, never read
N = len(PROMPTS)


@pytest.fixture(autouse=True)
def oracle_backend():
    asd_amd.set_backend(OracleBackend())
    yield
    asd_amd.set_backend(None)


def test_launcher_status_codes_and_workspace_size():
    lib = B.load_library()
    size = lambda b=4, k=5, v=1024, s=0: int(lib.asd_typical_accept_workspace_bytes(b, k, v, s))   # noqa: E731

    def call(x=P, dt=B.DTYPE_BF16, b=4, k=5, v=1024, lds=5 * 1024, ldr=1024, tok=P, table=P, s=1, ws=P, lp=P, h=P, bits=P, n=P):
        return lib.asd_typical_accept(x, dt, b, k, v, lds, ldr, tok, table, s, ws, lp, h, bits, n, None)
    assert call(b=-1) == call(k=-1) == call(v=-1) == INVALID
    assert call(k=17, lds=17 * 1024) == call(s=-1) == call(s=17) == UNSUPPORTED
    assert call(x=None, dt=99, b=0) == OK
    assert call(k=0) == call(v=0) == INVALID
    assert call(dt=99) == call(x=None, v=2 ** 30, ldr=0) == UNSUPPORTED
    assert {call(**{k: None}) for k in ("x", "tok", "table", "ws", "lp", "h", "bits", "n")} == {INVALID}
    assert call(ldr=1023) == call(lds=5 * 1024 - 1) == INVALID
    assert {call(**kw) for kw in (dict(x=P + 1), dict(dt=B.DTYPE_F32, x=P + 2), dict(tok=P + 2), dict(table=P + 8), dict(ws=P + 8),
                                  dict(lp=P + 2), dict(h=P + 2), dict(bits=P + 4), dict(n=P + 2))} == {ALIGNMENT}
    assert (B.TYPICAL_ACCEPT_REC_BYTES, B.TYPICAL_ACCEPT_MAX_K, B.TYPICAL_ACCEPT_MAX_SPLITS) == (16, 16, 16)
    assert size(s=3) == 4 * 5 * 3 * 16 + 64 == 1024 and size() == 4 * 5 * 16 * 16 and size(32, 8, 152064, 1) == 32 * 8 * 16
    assert size(b=0) == size(k=0) == size(v=-1) == size(k=17) == size(s=17) == 256


def test_check_typical_accept():
    assert check_typical_accept(None, None, 2) is None and check_typical_accept([None, None], None, 2) is None
    assert check_typical_accept(0.2, None, 2) == [(0.2, 0.3)] * 2                # the other's Medusa default
    assert check_typical_accept(None, 0.5, 2) == [(0.09, 0.5)] * 2
    assert check_typical_accept([0.1, None], [None, 100], 2) == [(0.1, 0.3), (0.09, 100.0)]
    assert check_typical_accept(1, 1e-9, 1) == [(1.0, 1e-9)]
    for bad in (True, float("nan"), 0, -0.5, 1.5, float("inf"), "0.5", [0.5], [0.5, 2.0]):
        with pytest.raises(ValueError, match="typical_acceptance_threshold"):
            check_typical_accept(bad, None, 2)
    for bad in (False, float("nan"), 0.0, 100.5, "1", [0.5, 0.5, 0.5]):
        with pytest.raises(ValueError, match="typical_acceptance_alpha"):
            check_typical_accept(None, bad, 2)
    with pytest.raises(ValueError, match="not built"):                           # a list that mixes on and off rows
        check_typical_accept([0.09, None], None, 2)
    with pytest.raises(ValueError, match="typical_acceptance_alpha"):            # a bad configuration: when the stage is built
        StageManager(stage_configs(vocab=VOCAB, typical_acceptance_alpha=0.0), ops=TypicalAcceptOracleOps())


def test_pipeline_config_hands_a_set_value_on():
    from asd_amd.serving.pipeline import AdaptiveSpeculativePipeline
    from tests.stage_scenario import LogprobPredictor
    ops = TypicalAcceptOracleOps()
    sm = StageManager(stage_configs(vocab=VOCAB), ops=ops)
    keys = ("typical_acceptance_threshold", "typical_acceptance_alpha")
    for cfg_kw in ({}, dict(typical_acceptance_threshold=0.2), dict(typical_acceptance_alpha=0.5)):
        pipe = AdaptiveSpeculativePipeline(sm, LogprobPredictor(), object(),
                                           PipelineConfig(lambda_value=100.0, stop_rule="full", stage_names=NAMES, **cfg_kw))
        calls = []
        for name in sm.names:
            stage = sm.get_stage(name)
            stage.generate = lambda *a, _orig=stage.generate, **kw: (calls.append(kw), _orig(*a, **kw))[1]
        try:
            del ops.trace[:]
            pipe.batch_process(PROMPTS, max_tokens=4, temperature=0.7)
        finally:
            for name in sm.names:
                del sm.get_stage(name).generate
            pipe.shutdown()
        assert calls and all((k in kw) == (k in cfg_kw) and (k not in kw or kw[k] == cfg_kw[k]) for kw in calls for k in keys)
        assert ("typical_accept" in [n for n, _ in ops.trace]) == bool(cfg_kw)


@pytest.mark.parametrize("name", NAMES[1:])
def test_generate_refuses_before_encoding(name):
    ops = TypicalAcceptOracleOps()
    stage = StageManager(stage_configs(vocab=VOCAB), ops=ops).get_stage(name)
    encoded = []
    stage._encode = lambda prompts, _orig=stage._encode: (encoded.append(1), _orig(prompts))[1]
    on = dict(typical_acceptance_threshold=0.09)
    for kw, match in ((dict(typical_acceptance_threshold=True), "threshold"), (dict(typical_acceptance_threshold=1.5), "threshold"),
                      (dict(typical_acceptance_alpha=float("nan")), "alpha"), (dict(typical_acceptance_alpha=[0.3] * (N - 1)), "alpha"),
                      (dict(on, top_k=5), "not built"), (dict(on, top_p=0.9), "not built"), (dict(on, min_p=0.1), "not built"),
                      (dict(on, top_p=[1.0] * (N - 1) + [0.5]), "not built"), (dict(on, mirostat_tau=5.0), "Mirostat"),
                      (dict(typical_acceptance_alpha=[0.3] + [None] * (N - 1)), "not built")):
        with pytest.raises(ValueError, match=match):
            stage.generate(prompts=PROMPTS, max_tokens=2, temperature=0.7, **kw)
    assert not encoded and not ops.trace


@pytest.mark.parametrize("name", NAMES[1:])
def test_calls_with_the_feature_off_and_on(name):
    ops = TypicalAcceptOracleOps()
    stage = StageManager(stage_configs(vocab=VOCAB), ops=ops).get_stage(name)
    run = lambda **kw: (ops.trace.clear(), stage.generate(**dict(dict(prompts=PROMPTS, max_tokens=3, temperature=0.7), **kw)),   # noqa: E731
                        [t[0] for t in ops.trace])
    _, plain_out, plain = run()
    assert run(typical_acceptance_threshold=None, typical_acceptance_alpha=[None] * N)[2] == plain   # off: the calls it made before
    assert "typical_accepted" not in plain_out[2]
    _, out, on = run(typical_acceptance_alpha=0.3)
    assert on.count("pack_typical_accept") == 1 and on.count("typical_accept") == out[2]["steps"]
    assert not any(c.startswith(("verify_accept", "residual_sample")) for c in on)
    acc, prop = out[2]["typical_accepted"], out[2]["typical_proposed"]
    assert len(acc) == len(prop) == N and all(0 <= a <= p for a, p in zip(acc, prop)) and sum(prop) > 0
    greedy = run(typical_acceptance_alpha=0.3, temperature=0.0)                  # greedy ignores the arguments ...
    assert not any("typical" in c for c in greedy[2]) and "typical_accepted" not in greedy[1][2]
    stage0 = StageManager(stage_configs(vocab=VOCAB), ops=ops).get_stage(NAMES[0])   # ... and so does a stage that verifies nothing
    ops.trace.clear()
    assert "typical_accepted" not in stage0.generate(prompts=PROMPTS, max_tokens=3, temperature=0.7, typical_acceptance_threshold=0.09)[2]
    assert not any("typical" in t[0] for t in ops.trace)
