"""Logit edits (serving/stages.py, LOGIT EDITS; include/asd_hip.h, asd_logit_edit_rows): the torch-on-CPU reference of the
kernel, written from the header's text, the oracle ops twin that edits through it, and the stage-level scenarios that
tests/test_logit_edit_stages.py (CPU twin) and tests/test_gpu_logit_edit_stages.py (HipOps) both run.

TEST INFRASTRUCTURE, like tests/per_request_ref.py: never importable from the package."""
from types import SimpleNamespace

import numpy as np
import torch

from tests.finish_scenario import FinishOracleOps
from tests.per_request_ref import RowsOracleOps, inv_t_of
from tests.stage_scenario import MAX_TOKENS, PROMPTS, TEMPERATURE, check_generation, text_ids
from tests.top_logprobs_ref import TopOracleOps

FOREVER = 2 ** 31 - 1
SEEDS = [11, 2 ** 64 - 1, 33, 0, 55]
MIN_TOKENS = [0, 3, 5, 1, 12]
FORCED = 777


def ref_logit_edit(x, rows, seq_len, start, offset=0):
    """asd_logit_edit_rows on a CPU tensor, IN PLACE (-> x): x [B, V] or [B, K1, V] (any strides), rows = one list of
    (id, bias, until) per sequence, or ONE such list shared by every row when its first element is a tuple.  With
    g = seq_len[b] - start + offset + j: element id of row (b, j) becomes -inf where g < until, else
    (x.float() + bias).to(dtype) where bias != 0, else it is left alone; an id outside [0, V) is skipped."""
    view = x[:, None] if x.dim() == 2 else x
    Bv, K1, V = view.shape
    if rows and isinstance(rows[0], tuple):
        rows = [rows] * Bv
    assert len(rows) == Bv
    for b in range(Bv):
        entries = [e for e in rows[b] if 0 <= e[0] < V]
        if not entries:
            continue
        ids = torch.tensor([e[0] for e in entries], dtype=torch.int64)
        bias = torch.tensor([e[1] for e in entries], dtype=torch.float32)
        until = torch.tensor([e[2] for e in entries], dtype=torch.int64)
        for j in range(K1):
            g = int(seq_len[b]) - int(start) + int(offset) + j
            row = view[b, j]                                                        # a view: assignments land in x
            ban = until > g
            add = ~ban & (bias != 0.0)
            row[ids[add]] = (row[ids[add]].float() + bias[add]).to(view.dtype)
            row[ids[ban]] = float("-inf")
    return x


class EditOracleOps(RowsOracleOps, TopOracleOps, FinishOracleOps):
    """RowsOracleOps (+ the greedy, stop and finish twins a min_tokens run needs) + pack_logit_edits and logit_edit_rows on
    the reference above: the three tiny stages run without a GPU."""

    def pack_logit_edits(self, rows, device):
        self._note("pack_logit_edits", ())
        rows = [[(int(t), float(b), int(u)) for t, b, u in r] for r in rows]
        assert all(len({e[0] for e in r}) == len(r) <= 1024 for r in rows)          # the packing contract
        return SimpleNamespace(rows=rows)

    def logit_edit_rows(self, logits, edits, seq_len, start, offset=0):
        self._note("logit_edit_rows", ())
        return ref_logit_edit(logits, edits.rows, seq_len.tolist(), start, offset)


# ------------------------------------------------------------------------------------------ stage-level scenarios
def run_kept(stage, **kw):
    stage.keep_inputs = True
    try:
        return stage.generate(**kw)
    finally:
        stage.keep_inputs = False


def _cpu(s):
    return {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in s.items()}


def scenario_ban(stage, atol):
    """A seeded baseline; every row bans what it generated; the rerun holds none of it, both sides were edited, and the run
    replays through check_generation unchanged (the kept logits are the edited ones)."""
    base, _, _ = stage.generate(prompts=PROMPTS, max_tokens=MAX_TOKENS, temperature=TEMPERATURE, seed=SEEDS)
    banned = [sorted(set(text_ids(t))) for t in base]
    texts, lps, _ = run_kept(stage, prompts=PROMPTS, max_tokens=MAX_TOKENS, temperature=TEMPERATURE, seed=SEEDS,
                             banned_token_ids=banned)
    for b, t in enumerate(texts):
        assert not set(text_ids(t)) & set(banned[b]), b
        assert np.isfinite(lps[b]).all()
    assert stage.step_inputs
    for s in map(_cpu, stage.step_inputs):
        for b, ids in enumerate(banned):
            assert torch.isneginf(s["logits"][b][..., ids]).all()                  # [V] at stage 0, [K, V] above it
            if "tok" in s:
                assert torch.isneginf(s["bonus"][b][ids]).all()
                assert not set(s["tok"][b].tolist()) & set(ids), (b, s["tok"][b].tolist())   # the DRAFT side was edited too
    worst = check_generation(stage, texts, lps, inv_t_of(TEMPERATURE), atol=atol)
    return worst


def scenario_force(stage):
    """logit_bias = {t: 100}: the other 999 tokens keep at most 999 exp(-(100 - spread) / T) of the mass, far below f32
    resolution at this scenario's logit scale (|x| of a few tens), so every committed token is t with log-prob 0."""
    texts, lps, _ = stage.generate(prompts=PROMPTS, max_tokens=MAX_TOKENS, temperature=TEMPERATURE, logit_bias={FORCED: 100})
    for t, lp in zip(texts, lps):
        assert text_ids(t) == [FORCED] * MAX_TOKENS
        assert np.isfinite(lp).all() and (lp > -1e-6).all(), lp


def check_min_tokens_rule(stats, texts, stops, min_tokens, limit=MAX_TOKENS):
    for b, (t, m) in enumerate(zip(texts, min_tokens)):
        toks, n, why = text_ids(t), stats["n_tokens"][b], stats["finish_reasons"][b]
        assert len(toks) == n and not set(toks[:m]) & set(stops), (b, toks)
        if why == "stop":
            assert n >= m + 1 and toks[-1] in stops and not set(toks[:-1]) & set(stops), (b, toks)
        else:
            assert why == "length" and n == limit and not set(toks) & set(stops), (b, toks)


def scenario_min_tokens(stage):
    """Greedy: the rows' first tokens as stop ids end every row at n = 1; with min_tokens = [0, 3, 5, 1, 12] row 0 still does,
    and row i has no stop id among its first min_tokens[i] tokens.  Then the same rule on a sampled, seeded run, and with the
    stop ids given as one-token stop sequences (the finish route)."""
    free, _, _ = stage.generate(prompts=PROMPTS, max_tokens=MAX_TOKENS, temperature=0.0)
    stops = sorted({text_ids(t)[0] for t in free})
    assert 1 <= len(stops) <= 8
    texts, _, stats = stage.generate(prompts=PROMPTS, max_tokens=MAX_TOKENS, temperature=0.0, stop_token_ids=stops)
    assert stats["n_tokens"] == [1] * len(PROMPTS) and stats["finish_reasons"] == ["stop"] * len(PROMPTS)
    texts, lps, stats = stage.generate(prompts=PROMPTS, max_tokens=MAX_TOKENS, temperature=0.0, stop_token_ids=stops,
                                       min_tokens=MIN_TOKENS)
    assert stats["n_tokens"][0] == 1 and text_ids(texts[0]) == text_ids(free[0])[:1]
    assert stats["finish_reasons"][4] == "length"                                  # min_tokens == max_tokens: no stop can land
    check_min_tokens_rule(stats, texts, stops, MIN_TOKENS)
    assert all(np.isfinite(lp).all() for lp in lps)
    for kw in (dict(stop_token_ids=stops), dict(stop_sequences=[(s,) for s in stops])):
        texts, lps, stats = stage.generate(prompts=PROMPTS, max_tokens=MAX_TOKENS, temperature=TEMPERATURE, seed=SEEDS,
                                           min_tokens=MIN_TOKENS, **kw)
        check_min_tokens_rule(stats, texts, stops, MIN_TOKENS)
        assert all(np.isfinite(lp).all() for lp in lps)
    return stops


def scenario_rows_independent(stage):
    """Seeded, one dict and one ban list per prompt: row b is bit-equal, in text and log-prob bytes, to row b of the call that
    gives EVERY row b's edit (the same batch, so the same tilings)."""
    V = stage.shape.vocab
    base, _, _ = stage.generate(prompts=PROMPTS, max_tokens=MAX_TOKENS, temperature=TEMPERATURE, seed=SEEDS)
    toks = [text_ids(t) for t in base]
    bans = [[t[0], t[3]] for t in toks]                                             # the first token: every row changes
    bias = [{t[1]: -8.0, (t[2] + 1) % V: 6.0, t[0]: 3.0} for t in toks]             # (t[0]: the ban wins over the bias)
    bias[2] = None
    bans[3] = []
    kw = dict(prompts=PROMPTS, max_tokens=MAX_TOKENS, temperature=TEMPERATURE, seed=SEEDS)
    mixed = stage.generate(logit_bias=bias, banned_token_ids=bans, **kw)
    for b in range(len(PROMPTS)):
        scal = stage.generate(logit_bias=bias[b], banned_token_ids=bans[b], **kw)
        assert scal[0][b] == mixed[0][b], b
        assert scal[1][b].tobytes() == mixed[1][b].tobytes(), b
        assert not set(text_ids(mixed[0][b])) & set(bans[b])
    assert sum(m != t for m, t in zip(mixed[0], base)) >= 4                        # the edits are live
    return mixed


__all__ = ["EditOracleOps", "FORCED", "MIN_TOKENS", "SEEDS", "check_min_tokens_rule", "ref_logit_edit", "run_kept", "scenario_ban",
           "scenario_force", "scenario_min_tokens", "scenario_rows_independent"]
