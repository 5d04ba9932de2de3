"""DRY (serving/stages.py, DRY; include/asd_hip.h, asd_dry_rows): the plain reference of the kernel, written from the header's
text, the oracle ops twin that penalises through it, and the four stage-level scenarios that tests/test_dry_stages.py (CPU twin)
and tests/test_gpu_dry_stages.py (HipOps) both run on stage_configs(vocab=64).

TEST INFRASTRUCTURE, like tests/ngram_ref.py: never importable from the package."""
from collections import Counter
from types import SimpleNamespace

import numpy as np
import torch

from tests.entropy_cut_ref import EntropyCutOracleOps
from tests.logit_edit_ref import SEEDS, run_kept
from tests.per_request_ref import inv_t_of
from tests.stage_scenario import PROMPTS, TEMPERATURE, check_generation, text_ids

CAP = 64                                         # ASD_DRY_MAX_MATCH
VOCAB = 64                                       # the stages of the scenarios
MAX_TOKENS = 24


def dry_pen(multiplier, base, allowed):
    """pen[0 .. CAP] as the host builds it: float32(multiplier * base ** (m - allowed)) from f64, 0 below `allowed`."""
    pen = np.zeros(CAP + 1, dtype=np.float64)
    for m in range(allowed, CAP + 1):
        try:
            pen[m] = multiplier * float(base) ** (m - allowed)
        except OverflowError:
            pen[m] = np.inf
    with np.errstate(over="ignore"):
        return pen.astype(np.float32)


def ref_dry(x, rows, breakers, tokens, seq_len, row_start, start, max_len, step_tok=None, n_prev=0):
    """asd_dry_rows on a CPU tensor, IN PLACE (-> x): x [B, V] or [B, K1, V] (any strides); rows: one (multiplier, base,
    allowed_length, range) per sequence; breakers: the call's ids; the other arguments as tests/ngram_ref.py's."""
    view = x[:, None] if x.dim() == 2 else x
    Bv, K1, V = view.shape
    brk, lowest = set(breakers), torch.finfo(x.dtype).min
    for b, (mul, base, allowed, rng) in enumerate(rows):
        if not mul > 0:
            continue
        pen = dry_pen(mul, base, allowed)
        L = min(max(int(seq_len[b]), start), max_len)
        first = start if row_start is None else min(max(int(row_start[b]), 0), start)
        committed = [int(t) for t in tokens[b][first:L]]
        for j in range(K1):
            H = committed + ([] if step_tok is None else [int(t) for t in step_tok[b][:n_prev + j]])
            H = H[-rng:] if rng > 0 else H
            n = len(H)
            if n < 2 or H[-1] in brk:
                continue
            best = {}
            for i in range(n - 1):
                t = H[i + 1]
                if H[i] != H[-1] or t in brk or not 0 <= t < V:
                    continue
                m = 0
                while m < min(i + 1, CAP) and H[i - m] == H[n - 1 - m] and H[n - 1 - m] not in brk:
                    m += 1
                best[t] = max(best.get(t, 0), m)
            for t, m in best.items():
                if m >= allowed and torch.isfinite(view[b, j, t]):
                    with np.errstate(over="ignore"):
                        y = np.float32(view[b, j, t].float().item()) - pen[m]          # one f32 subtraction
                    view[b, j, t] = max(torch.tensor(y).to(x.dtype).item(), lowest)  # to nearest even, then the clamp
    return x


class DryOracleOps(EntropyCutOracleOps):
    """EntropyCutOracleOps + pack_dry and dry_rows on the reference above: the tiny stages run without a GPU."""

    def pack_dry(self, multipliers, bases, allowed_lengths, ranges, breakers, prompt_lens, P, device):
        self._note("pack_dry", ())
        rows = list(zip(multipliers, bases, allowed_lengths, ranges))
        assert len(rows) == len(prompt_lens) and len(breakers) <= 32 and all(1 <= r[2] <= CAP for r in rows)
        return SimpleNamespace(rows=rows, breakers=tuple(breakers), row_start=[int(P) - int(m) for m in prompt_lens], P=int(P))

    def dry_rows(self, logits, dry, tokens, seq_len, max_len, step_tok=None, n_prev=0):
        self._note("dry_rows", ())
        return ref_dry(logits, dry.rows, dry.breakers, tokens.numpy(), seq_len.tolist(), dry.row_start, dry.P, max_len,
                       None if step_tok is None else step_tok.numpy(), n_prev)


# ------------------------------------------------------------------------------------------ stage-level scenarios
STRICT = dict(dry_multiplier=1.0e4, dry_base=1.0, dry_allowed_length=1)             # every follower of `last` falls below every other token


def scenario_strict_is_bigram_ban(stage):
    """(a) Greedy, allowed length 1, base 1 and a multiplier above the logit spread: DRY lowers exactly the tokens that
    no_repeat_ngram_size = 2 bans, below every other one, so the TEXTS are those of the ban -- history, padding, proposals and
    both sides end to end.  The spread is asserted from the plain run's kept logits."""
    kw = dict(prompts=PROMPTS, max_tokens=MAX_TOKENS, temperature=0.0)
    plain = run_kept(stage, **kw)[0]
    spread = 0.0
    for s in stage.step_inputs:
        for x in (s["logits"], s.get("bonus")):
            if x is not None:
                spread = max(spread, float((x.float().amax(-1) - x.float().amin(-1)).max()))
    assert 0.0 < spread < 0.5 * STRICT["dry_multiplier"], spread
    banned = stage.generate(no_repeat_ngram_size=2, **kw)[0]
    assert banned != plain                                                           # never vacuous: the ban changes these rows
    assert stage.generate(**STRICT, **kw)[0] == banned
    return banned


PER_PROMPT = dict(dry_multiplier=[0.8, 0.0, 3.0, 0.5, 1.5], dry_base=[1.75, 1.75, 2.0, 1.2, 1.0], dry_allowed_length=[1, 2, 2, 1, 3],
                  dry_range=[0, 0, 6, 0, 12])


def scenario_per_prompt(stage):
    """(b) Seeded, one value per prompt: row b bit-equals, in text and log-prob bytes, row b of the call that gives EVERY row
    b's values; row 1 is off and equals the call without the keywords."""
    kw = dict(prompts=PROMPTS, max_tokens=MAX_TOKENS, temperature=TEMPERATURE, seed=SEEDS)
    base = stage.generate(**kw)
    mixed = stage.generate(**PER_PROMPT, **kw)
    for b in range(len(PROMPTS)):
        alone = stage.generate(**{k: v[b] for k, v in PER_PROMPT.items()}, **kw) if b != 1 else base
        assert alone[0][b] == mixed[0][b] and alone[1][b].tobytes() == mixed[1][b].tobytes(), b
    assert sum(m[0] != p[0] for m, p in zip(zip(*mixed[:2]), zip(*base[:2]))) >= 2   # ... and the penalty is felt
    return mixed


def scenario_multiplier_zero(stage):
    """(c) dry_multiplier = 0, with every other keyword set, returns the bits of the call without them and reaches neither op."""
    def never(*a, **k):
        raise AssertionError("a DRY op was called with every row off")
    kw = dict(prompts=PROMPTS, max_tokens=8, temperature=TEMPERATURE, seed=SEEDS)
    base = stage.generate(**kw)
    stage.ops.pack_dry = stage.ops.dry_rows = never
    try:
        off = stage.generate(dry_multiplier=[0.0] * len(PROMPTS), dry_base=2.0, dry_allowed_length=1, dry_range=5,
                             dry_sequence_breakers=[3], **kw)
    finally:
        del stage.ops.pack_dry, stage.ops.dry_rows
    assert off[0] == base[0] and all(a.tobytes() == b.tobytes() for a, b in zip(off[1], base[1]))


def scenario_breaker(stage):
    """(d) Seeded and sampled under STRICT: a breaker equal to the most frequently generated token changes the text, and the run
    replays.  In every kept step the logits below -multiplier / 2 are exactly the followers of the history's last token --
    none behind the breaker, the breaker never one -- on the target's K + 1 rows; no proposal is such a follower, so the draft
    side was penalised too; and check_generation replays commits and log-probs from those penalised logits."""
    # (top_p = 1: at this vocabulary a nucleus can hold ONE token, whose log-prob the samplers return as 0 up to a rounding of
    # +1e-8, with or without DRY; check_generation asks for <= 0, and this scenario is not about the nucleus)
    kw = dict(prompts=PROMPTS, max_tokens=MAX_TOKENS, temperature=TEMPERATURE, seed=SEEDS, top_p=1.0, **STRICT)
    free = stage.generate(**kw)[0]
    often = Counter(t for text in free for t in text_ids(text)).most_common(1)[0][0]
    texts, lps, _ = run_kept(stage, dry_sequence_breakers=[often], **kw)
    assert texts != free
    ids, real = stage._encode(PROMPTS)
    P, gen, hits = ids.shape[1], [text_ids(t) for t in texts], 0
    for step, s in enumerate(stage.step_inputs):
        verify = "tok" in s
        rows = torch.cat([s["logits"], s["bonus"][:, None]], 1).cpu() if verify else s["logits"][:, None].cpu()
        seq, tok = (s["seq_len"].tolist(), s["tok"].tolist()) if verify else ([P + step] * len(gen), [[]] * len(gen))
        for b in range(len(gen)):
            for j in range(rows.shape[1]):
                H = real[b] + gen[b][:seq[b] - P] + tok[b][:j]
                want = set() if H[-1] == often else {t for a, t in zip(H, H[1:]) if a == H[-1]} - {often}
                assert set((rows[b, j].float() < -0.5 * STRICT["dry_multiplier"]).nonzero().flatten().tolist()) == want, (step, b, j)
                assert j >= len(tok[b]) or tok[b][j] not in want, (step, b, j)
                hits += len(want)
    assert hits > 0
    check_generation(stage, texts, lps, inv_t_of(TEMPERATURE), atol=1e-6 if isinstance(stage.ops, DryOracleOps) else 2e-5,
                     max_tokens=MAX_TOKENS)                      # the twin's f64 value rounded to f32; the kernels' bar against f64
    return texts
