"""Prompt lookup on CPU: the status codes of asd_lookup_propose for every bad argument (rejected before any launch: the pointers
are made-up addresses, so no GPU is allowed), and Stage.generate's ValueErrors before the prompts are encoded and before any ops
call."""
import pytest

from tests.stage_scenario import NAMES, PROMPTS, StageOracleOps, stage_configs

OK, INVALID, UNSUPPORTED, ALIGNMENT = 0, -1, -2, -5
A = [0x7F0000000000 + (i << 24) for i in range(8)]      # made-up, aligned "device" addresses
ORDER = ["tokens", "ld_tokens", "row_start", "seq_len", "B", "start", "max_len", "K", "max_ngram", "min_ngram", "tok", "ld_tok",
         "matched", "counter", "onehot", "dtype", "ld_seq", "ld_row", "V", "stream"]
VALID = dict(tokens=A[0], ld_tokens=128, row_start=A[1], seq_len=A[2], B=4, start=8, max_len=128, K=4, max_ngram=3, min_ngram=1,
             tok=A[3], ld_tok=4, matched=A[4], counter=A[5], onehot=A[6], dtype=1, ld_seq=4 * 64, ld_row=64, V=64, stream=None)
CASES = [
    (dict(B=-1), INVALID), (dict(start=-1), INVALID), (dict(max_len=-1), INVALID), (dict(V=-1), INVALID),
    (dict(K=0), INVALID), (dict(max_ngram=0), INVALID), (dict(min_ngram=0), INVALID), (dict(min_ngram=4), INVALID),
    (dict(K=0, B=0), INVALID),                                               # the sizes before the empty batch
    (dict(B=0, tokens=None, K=17), OK),                                      # the empty batch before everything else
    (dict(K=17), UNSUPPORTED), (dict(max_ngram=9), UNSUPPORTED), (dict(dtype=7), UNSUPPORTED),
    (dict(max_len=2 ** 31 - 1, ld_tokens=2 ** 31), UNSUPPORTED),
    (dict(K=17, tokens=None), UNSUPPORTED),                                  # ranges before null pointers
    (dict(tokens=None), INVALID), (dict(seq_len=None), INVALID), (dict(tok=None), INVALID), (dict(matched=None), INVALID),
    (dict(ld_tokens=127), INVALID), (dict(start=129), INVALID), (dict(ld_tok=3), INVALID),
    (dict(V=0), INVALID), (dict(ld_row=63), INVALID), (dict(ld_seq=255), INVALID),
    (dict(tokens=None, seq_len=A[2] + 2), INVALID),                          # null pointers before alignment
    (dict(tokens=A[0] + 2), ALIGNMENT), (dict(row_start=A[1] + 1), ALIGNMENT), (dict(seq_len=A[2] + 2), ALIGNMENT),
    (dict(tok=A[3] + 2), ALIGNMENT), (dict(matched=A[4] + 2), ALIGNMENT), (dict(counter=A[5] + 2), ALIGNMENT),
    (dict(onehot=A[6] + 1), ALIGNMENT), (dict(onehot=A[6] + 2, dtype=0), ALIGNMENT),
]


@pytest.mark.parametrize("change,want", CASES, ids=str)
def test_rejected_calls_return_their_code(change, want):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: these calls carry made-up device addresses")
    from asd_amd import _binding
    args = dict(VALID, **change)
    assert _binding.load_library().asd_lookup_propose(*[args[a] for a in ORDER]) == want


@pytest.mark.parametrize("kw", [
    dict(prompt_lookup_num_tokens=True), dict(prompt_lookup_num_tokens=2.0), dict(prompt_lookup_num_tokens=[2] * len(PROMPTS)),
    dict(prompt_lookup_num_tokens=-1), dict(prompt_lookup_num_tokens=17), dict(prompt_lookup_num_tokens=4, prompt_lookup_max_ngram=0),
    dict(prompt_lookup_num_tokens=4, prompt_lookup_max_ngram=9), dict(prompt_lookup_num_tokens=4, prompt_lookup_max_ngram=True),
    dict(prompt_lookup_num_tokens=4, prompt_lookup_min_ngram=0), dict(prompt_lookup_num_tokens=4, prompt_lookup_min_ngram=4),
    dict(prompt_lookup_num_tokens=4, prompt_lookup_max_ngram=2, prompt_lookup_min_ngram=3),
    dict(prompt_lookup_num_tokens=4, prompt_lookup_min_ngram=1.0), dict(prompt_lookup_max_ngram=3), dict(prompt_lookup_min_ngram=1),
    dict(prompt_lookup_num_tokens=0, prompt_lookup_max_ngram=3), dict(prompt_lookup_num_tokens=4, guided_choice=[[3, 4], [5]], stop_token_ids=[9])], ids=str)
def test_generate_refuses_before_encoding(kw):
    from asd_amd.serving.stages import StageManager
    ops = StageOracleOps()
    for name in NAMES[:2]:
        stage = StageManager(stage_configs(vocab=64), ops=ops).get_stage(name)
        stage._encode = None                                                     # (reaching it would raise TypeError)
        for temperature in (0.7, 0.0):
            with pytest.raises(ValueError, match="prompt_lookup"):
                stage.generate(prompts=PROMPTS, max_tokens=2, temperature=temperature, **kw)
    assert not ops.calls
    with pytest.raises(ValueError, match="prompt_lookup_min_ngram"):             # a bad configuration: when the stage is built
        StageManager(stage_configs(vocab=64, prompt_lookup_num_tokens=2, prompt_lookup_min_ngram=5), ops=ops)
