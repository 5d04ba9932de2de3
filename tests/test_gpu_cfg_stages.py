"""Classifier-free guidance in Stage.generate on the kernels (HipOps), f32 stages of the tiny scenario: (a) a negative prompt
equal to the prompt is the identity; (b) every returned log-prob of a mixed call against a dense f64 forward over prompt +
returned tokens and over negative prompt + returned tokens, combined in f64; (c) the draft model never sees the extra rows.

THE BOUND of (b), from the reference side alone: eps_x = 4 max |dense in the stage's dtype - dense f64| over both contexts
(tests/teacher_forced_ref.py's); a log-softmax value moves by at most 2 eps_x, a guided value by 2 eps_x (|s| + |1 - s|), a
returned log-prob by twice that times inv_t, plus lp_bar = 2e-5.  No truncation is used: no position is left out."""
import copy

import numpy as np
import pytest
import torch

from tests.cfg_ref import log_softmax
from tests.stage_scenario import NAMES, text_ids

pytestmark = pytest.mark.gpu

LP_BAR = 2e-5
PROMPTS = ["a somewhat longer prompt , with punctuation .", "two words"]
NEGATIVE = "dull , repetitive and short"
PLAIN = dict(top_p=1.0, top_k=0, min_p=0.0)


@pytest.fixture(scope="module")
def manager():
    from asd_amd.serving.stages import StageManager
    from tests.stage_scenario import stage_configs
    return StageManager(stage_configs(dtype=torch.float32))


def dense(stage, padded, gens):
    """padded: one list of P ids per row.  -> (f64 logits [B, N, V] for the generated positions, max |own dtype - f64|)."""
    P, N = len(padded[0]), max(len(g) for g in gens)
    full = torch.zeros((len(padded), P + N), dtype=torch.int64)
    for b, (p, g) in enumerate(zip(padded, gens)):
        full[b, :P], full[b, P:P + len(g)] = torch.tensor(p), torch.tensor(g, dtype=torch.int64)
    m = stage.model
    m.reset()
    own = m.forward(full.to(stage.device)).double().cpu()
    m.reset()
    m64 = copy.deepcopy(m).to("cpu").double()
    m64.reset()
    with torch.no_grad():
        x = m64.forward(full)
    return x[:, P - 1:P - 1 + N].numpy(), float((own - x).abs().max())


def test_a_negative_prompt_equal_to_the_prompt_is_the_identity(manager):
    stage = manager.get_stage(NAMES[0])
    kw = dict(prompts=PROMPTS, max_tokens=8, temperature=1.0, seed=3, **PLAIN)
    texts, lps, _ = stage.generate(**kw)
    g_texts, g_lps, _ = stage.generate(guidance_scale=3.0, negative_prompt=list(PROMPTS), **kw)
    assert g_texts == texts
    ids, _ = stage._encode(PROMPTS)
    _, err = dense(stage, ids.tolist(), [text_ids(t) for t in texts])
    bound = 2.0 * (2.0 * (2.0 * 4.0 * err * (3.0 + 2.0)) + LP_BAR)
    assert max(float(np.abs(a - b).max()) for a, b in zip(lps, g_lps)) <= bound


@pytest.mark.parametrize("name,negative,kw", [(NAMES[0], [NEGATIVE, None], {}), (NAMES[1], [None, NEGATIVE], {}),
                                              (NAMES[0], [NEGATIVE, None], dict(prompt_lookup_num_tokens=4))],
                         ids=["stage 0", "verifying stage, None on the guided row", "stage 0 with lookup"])
def test_b_returned_logprobs_against_the_f64_combine(manager, name, negative, kw):
    stage = manager.get_stage(name)
    scales, T = [1.5, 1.0], 0.8
    texts, lps, _ = stage.generate(prompts=PROMPTS, max_tokens=10, temperature=T, seed=1, guidance_scale=scales,
                                   negative_prompt=negative, **PLAIN, **kw)
    gens = [text_ids(t) for t in texts]
    assert [len(g) for g in gens] == [10, 10]
    ids, _ = stage._encode(PROMPTS)
    P, V = ids.shape[1], stage.shape.vocab
    neg = [i % V for i in stage.tokenizer.encode(NEGATIVE, return_tensors=None)][-P:] if negative[0] else [int(ids[0, -1])]
    xc, err_c = dense(stage, ids.tolist(), gens)         # (None: the prompt's last token alone behind the padding)
    xu, err_u = dense(stage, [[0] * (P - len(neg)) + neg, ids[1].tolist()], gens)
    eps_x, inv_t = 4.0 * max(err_c, err_u), float(np.float32(1.0 / T))
    for b, s in enumerate(scales):
        bound = 2.0 * (2.0 * eps_x * (abs(s) + abs(1.0 - s))) * inv_t + LP_BAR
        for i, tok in enumerate(gens[b]):
            c, u = log_softmax(xc[b, i]), log_softmax(xu[b, i])
            want = log_softmax((c if s == 1.0 else u + s * (c - u)) * inv_t)[tok]
            assert abs(float(lps[b][i]) - want) <= bound, f"row {b} position {i}: returned {lps[b][i]!r}, f64 {want!r}, bound {bound:.3e} (eps_x {eps_x:.3e})"


def test_c_the_draft_model_never_sees_the_extra_rows(manager):
    stage = manager.get_stage(NAMES[1])
    seen = {"draft": set(), "own": set()}
    for key, model in (("draft", stage.draft.model), ("own", stage.model)):
        model.forward_ragged = lambda ids, *a, _k=key, _real=model.forward_ragged, **kw: seen[_k].add(ids.shape[0]) or _real(ids, *a, **kw)
    try:
        stage.generate(prompts=PROMPTS, max_tokens=6, temperature=0.0, guidance_scale=[2.0, 1.0], negative_prompt=NEGATIVE)
    finally:
        del stage.draft.model.forward_ragged, stage.model.forward_ragged
    assert seen == {"draft": {2}, "own": {3}}
