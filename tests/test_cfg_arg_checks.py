"""Classifier-free guidance on CPU: asd_cfg_rows' status codes (made-up addresses: rejected before any launch), the binding's
copies of the header's constants, generate's ValueErrors before any encoding or ops call, a guided call on the CPU twin."""
import os
import re

import pytest

from tests.cfg_ref import CfgOracleOps
from tests.stage_scenario import NAMES, PROMPTS, stage_configs

OK, INVALID, UNSUPPORTED, ALIGNMENT = 0, -1, -2, -5
A = [0x7F0000000000 + (i << 24) for i in range(3)]      # made-up, aligned "device" addresses
VALID = dict(cond=A[0], dtype=1, B=4, K1=3, V=64, ld_seq=192, ld_row=64, uncond=A[1], Bu=2, ld_useq=210, ld_urow=70, table=A[2], stream=None)
CASES = [(dict(B=-1), INVALID), (dict(Bu=-1), INVALID), (dict(V=-1), INVALID), (dict(V=0, cond=None), OK),
         (dict(dtype=7, cond=None), UNSUPPORTED),                                              # ranges before null pointers
         (dict(cond=None), INVALID), (dict(uncond=None), INVALID), (dict(table=None, cond=A[0] + 1), INVALID),
         (dict(ld_row=63), INVALID), (dict(ld_seq=191), INVALID), (dict(ld_urow=63), INVALID), (dict(ld_useq=209), INVALID),
         (dict(cond=A[0] + 1), ALIGNMENT), (dict(uncond=A[1] + 1), ALIGNMENT), (dict(table=A[2] + 2), ALIGNMENT)]


@pytest.mark.parametrize("change,want", CASES, ids=str)
def test_rejected_calls_return_their_code(change, want):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: these calls carry made-up device addresses")
    from asd_amd import _binding
    assert _binding.load_library().asd_cfg_rows(*dict(VALID, **change).values()) == want


def test_the_binding_holds_the_headers_constants():
    from asd_amd import _binding
    from asd_amd.serving import stage_args
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "asd_hip.h")) as f:
        header = dict(re.findall(r"#define ASD_(CFG_REC_BYTES|CFG_RESIDENT_VECTORS|MAX_GUIDANCE_SCALE) ([0-9.]+)", f.read()))
    assert {k: float(v) for k, v in header.items()} == {k: float(getattr(_binding, k)) for k in header} and len(header) == 3
    assert stage_args.MAX_GUIDANCE_SCALE == _binding.MAX_GUIDANCE_SCALE


N = len(PROMPTS)


@pytest.mark.parametrize("kw", [
    dict(guidance_scale=True), dict(guidance_scale=float("nan")), dict(guidance_scale=-0.5), dict(guidance_scale=100.5),
    dict(guidance_scale="2"), dict(guidance_scale=[2.0] * (N - 1)), dict(guidance_scale=[2.0] * (N - 1) + [float("inf")]),
    dict(guidance_scale=2.0, negative_prompt=7), dict(guidance_scale=2.0, negative_prompt=["no"] * (N + 1)),
    dict(negative_prompt="no"), dict(guidance_scale=[1.0] * N, negative_prompt=[None] * (N - 1) + ["no"]),
    dict(guidance_scale=2.0, prompt_logprobs=0)], ids=str)
def test_generate_refuses_before_encoding(kw):
    from asd_amd.serving.stages import StageManager
    ops = CfgOracleOps()
    for name in NAMES[:2]:
        stage = StageManager(stage_configs(vocab=64), ops=ops).get_stage(name)
        stage._encode = None                                                     # (reaching it would raise TypeError)
        with pytest.raises(ValueError, match="is not built" if "prompt_logprobs" in kw else "guidance_scale|negative_prompt"):
            stage.generate(prompts=PROMPTS, max_tokens=2, temperature=0.0, **kw)
    assert not ops.calls


def test_a_guided_draft_stage_and_a_bad_configuration_are_refused():
    from asd_amd.serving.stages import StageManager
    ops = CfgOracleOps()
    verifier = StageManager(stage_configs(vocab=64, guidance_scale=1.5), ops=ops).get_stage(NAMES[1])
    with pytest.raises(ValueError, match="a guided draft model .* is not built"):
        verifier.generate(prompts=PROMPTS, max_tokens=2)
    with pytest.raises(ValueError, match="guidance_scale"):                      # a bad configuration: when the stage is built
        StageManager(stage_configs(vocab=64, guidance_scale=-1.0), ops=ops)
    assert not ops.calls


@pytest.mark.parametrize("name", NAMES[:2])
def test_a_guided_call_completes_on_the_cpu_twin(name):
    from asd_amd.serving.stages import StageManager
    ops = CfgOracleOps()
    stage = StageManager(stage_configs(vocab=64), ops=ops).get_stage(name)
    plain = stage.generate(prompts=PROMPTS, max_tokens=6, temperature=0.0)[0]
    assert not ops.calls["cfg_rows"]
    texts, lps, stats = stage.generate(prompts=PROMPTS, max_tokens=6, temperature=0.0, guidance_scale=2.0,
                                       negative_prompt=[None, "something else entirely"] + [None] * (N - 2))
    assert ops.calls["cfg_rows"] >= stats["steps"] and [len(t.split()) for t in texts] == [6] * N
    assert texts != plain and all((lp <= 0.0).all() for lp in lps)
