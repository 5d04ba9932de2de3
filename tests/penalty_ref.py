"""Stateful penalties (serving/stages.py, PENALTIES; include/asd_hip.h, asd_penalty_rows / asd_penalty_commit): the numpy-float32
references of the two kernels, written from the header's text in its operation order, the oracle ops twin that penalises through
them, the recorder that stands between a stage and its ops, and the stage-level scenarios that tests/test_penalty_stages.py (CPU
twin) and tests/test_gpu_penalty_stages.py (HipOps) both run.

TEST INFRASTRUCTURE, like tests/token_mask_ref.py: never importable from the package."""
from types import SimpleNamespace

import numpy as np
import torch

from tests import greedy_ref
from tests.logit_edit_ref import SEEDS, ref_logit_edit, run_kept
from tests.per_request_ref import inv_t_of
from tests.stage_scenario import MAX_TOKENS, PROMPTS, TEMPERATURE, check_generation, text_ids
from tests.token_mask_ref import MaskOracleOps

MAX_COMMIT = 65                                  # ASD_MAX_DRAFT_LEN + 1
_LARGEST = {torch.bfloat16: torch.finfo(torch.bfloat16).max, torch.float16: torch.finfo(torch.float16).max,
            torch.float32: torch.finfo(torch.float32).max}


def ref_seen_bits(rows, V):
    """uint32 [len(rows), W]: bit v & 31 of word v >> 5 of row r set for every id v of rows[r] (the header's sentence)."""
    out = np.zeros((len(rows), (V + 31) // 32), dtype=np.uint32)
    for r, ids in enumerate(rows):
        for v in ids:
            out[r, int(v) >> 5] |= np.uint32(1 << (int(v) & 31))
    return out


def _bit_set(words, V):
    v = np.arange(V)
    return ((np.asarray(words).astype(np.int64)[v >> 5] >> (v & 31)) & 1).astype(bool)


def ref_penalty(x, seen, counts, params, step_tok=None, n_prev=0):
    """asd_penalty_rows on a CPU tensor, IN PLACE (-> x): x [B, V] or [B, K1, V] (any strides); seen uint32 [B, W]; counts int32
    [B, V]; params float32 [B, 3]; step_tok int [B, n_tok] or None.  Position j of row b sees step_tok[b, :n_prev + j].  numpy
    float32 throughout: every operator below rounds once, none is fused."""
    view = x[:, None] if x.dim() == 2 else x
    Bv, K1, V = view.shape
    seen, counts = np.asarray(seen), np.asarray(counts)
    params = np.asarray(params, dtype=np.float32)
    assert n_prev == 0 or step_tok is not None
    for b in range(Bv):
        rep, pres, freq = (np.float32(t) for t in params[b])
        if not rep > 0:                                                  # <= 0 or NaN reads as 1
            rep = np.float32(1.0)
        if rep == 1 and pres == 0 and freq == 0:
            continue
        bit = _bit_set(seen[b], V)
        assert not (counts[b] > 0)[~bit].any()                           # the state contract
        for j in range(K1):
            see = [] if step_tok is None else [int(t) for t in np.asarray(step_tok)[b, :n_prev + j] if 0 <= int(t) < V]
            assert step_tok is None or n_prev + j <= np.asarray(step_tok).shape[1]
            occ = np.bincount(np.asarray(see, dtype=np.int64), minlength=V)
            was_seen = bit | (occ > 0)
            c = np.where(was_seen, counts[b].astype(np.int64) + occ, 0)
            row = view[b, j]                                             # a view: the assignment lands in x
            xf = row.float().numpy().astype(np.float32)
            with np.errstate(all="ignore"):
                y = xf.copy()
                if rep != 1:
                    y = np.where(was_seen, np.where(xf > 0, xf / rep, xf * rep), y).astype(np.float32)
                t = (freq * c.astype(np.float32)).astype(np.float32)     # one rounding ...
                z = (y - t).astype(np.float32)                           # ... another ...
                z = (z - pres).astype(np.float32)                        # ... and the third
                y = np.where(c > 0, z, y).astype(np.float32)
            store = torch.from_numpy(~(y == xf))                         # y == x: the bits stay (a NaN is stored)
            r = torch.from_numpy(y).to(view.dtype)                       # to nearest even
            r[torch.isposinf(r)] = _LARGEST[view.dtype]
            row[store] = r[store]
    return x


def ref_penalty_commit(tokens, seq_len, n_commit, V, max_len, seen, counts):
    """asd_penalty_commit on numpy arrays, IN PLACE on seen (uint32 [B, W]) and counts (int32 [B, V])."""
    tokens = np.asarray(tokens)
    for b in range(tokens.shape[0]):
        n = min(max(int(n_commit[b]), 0), MAX_COMMIT)
        for i in range(n):
            pos = min(max(int(seq_len[b]) - n + i, 0), max_len - 1)
            v = int(tokens[b, pos])
            if 0 <= v < V:
                counts[b, v] += 1
                seen[b, v >> 5] |= np.uint32(1 << (v & 31))
    return seen, counts


class PenaltyOracleOps(MaskOracleOps):
    """MaskOracleOps + pack_penalties, penalty_rows and penalty_commit on the references above: the tiny stages run without a
    GPU.  The state is numpy: seen uint32 [B, W], counts int32 [B, V], params float32 [B, 3]."""

    def pack_penalties(self, rep, pres, freq, prompt_ids, V, device):
        self._note("pack_penalties", ())
        assert len(rep) == len(pres) == len(freq) == len(prompt_ids)
        assert all(0 <= t < V for r in prompt_ids for t in r)                    # what the stage hands over
        return SimpleNamespace(seen=ref_seen_bits(prompt_ids, V), counts=np.zeros((len(rep), V), dtype=np.int32),
                               params=np.stack([np.asarray(v, dtype=np.float32) for v in (rep, pres, freq)], 1), V=V, B=len(rep))

    def penalty_rows(self, logits, pen, step_tok=None, n_prev=0):
        self._note("penalty_rows", ())
        return ref_penalty(logits, pen.seen, pen.counts, pen.params, None if step_tok is None else step_tok.numpy(), n_prev)

    def penalty_commit(self, tokens, seq_len, n_commit, pen, max_len):
        self._note("penalty_commit", ())
        ref_penalty_commit(tokens.numpy(), seq_len.tolist(), n_commit.tolist(), pen.V, max_len, pen.seen, pen.counts)


# ------------------------------------------------------------------------------------------ the recorder
def state_arrays(pen):
    """(seen uint32 [B, W], counts int32 [B, V], params float32 [B, 3]) as fresh numpy arrays, from the twin's state or HipOps'."""
    def host(a, dtype):
        a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
        return np.array(a.view(dtype) if a.dtype.itemsize == np.dtype(dtype).itemsize else a.astype(dtype), copy=True)
    return host(pen.seen, np.uint32), host(pen.counts, np.int32), host(pen.params, np.float32)


class PenaltyLog:
    """Stands between a stage and the three penalty ops of `ops` (instance attributes: the ops object stays what it is, so a
    StageManager still sees a HipOps).  events: ("pack", dict) | ("rows", dict) | ("commit", dict), in call order; a rows event
    holds clones of the logits before and after the call, of step_tok and of the state the call read; a commit event the state
    it left, with tokens / seq_len / n_commit."""

    def __init__(self, ops):
        self.ops, self.events = ops, []
        pack, rows, commit = ops.pack_penalties, ops.penalty_rows, ops.penalty_commit

        def pack_penalties(rep, pres, freq, prompt_ids, V, device):
            pen = pack(rep, pres, freq, prompt_ids, V, device)
            self.events.append(("pack", dict(rep=list(rep), pres=list(pres), freq=list(freq), prompt_ids=[list(r) for r in prompt_ids],
                                             V=int(V), state=state_arrays(pen))))
            return pen

        def penalty_rows(logits, pen, step_tok=None, n_prev=0):
            ev = dict(before=logits.detach().cpu().clone(), n_prev=n_prev, state=state_arrays(pen),
                      step_tok=None if step_tok is None else step_tok.detach().cpu().clone())
            out = rows(logits, pen, step_tok, n_prev)
            assert out is logits
            ev["after"] = logits.detach().cpu().clone()
            self.events.append(("rows", ev))
            return out

        def penalty_commit(tokens, seq_len, n_commit, pen, max_len):
            commit(tokens, seq_len, n_commit, pen, max_len)
            self.events.append(("commit", dict(state=state_arrays(pen), tokens=tokens.detach().cpu().clone(), max_len=int(max_len),
                                               seq_len=seq_len.cpu().tolist(), n_commit=n_commit.cpu().tolist())))
        ops.pack_penalties, ops.penalty_rows, ops.penalty_commit = pack_penalties, penalty_rows, penalty_commit

    def close(self):
        for name in ("pack_penalties", "penalty_rows", "penalty_commit"):
            delattr(self.ops, name)

    def steps(self):
        """-> (pack event, [(rows events of the step, its commit event)])."""
        kinds = [k for k, _ in self.events]
        assert kinds.count("pack") == 1 and kinds[0] == "pack" and kinds[-1] == "commit"
        out, cur = [], []
        for kind, ev in self.events[1:]:
            if kind == "rows":
                cur.append(ev)
            else:
                out.append((cur, ev))
                cur = []
        return self.events[0][1], out


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16).numpy().tobytes()


def check_recorded(stage, log, prompts, n_tokens=None):
    """Checks (a), (b), (c) of one recorded generate call that kept its step inputs.  -> elements the penalties changed."""
    pack, steps = log.steps()
    V, B = pack["V"], len(prompts)
    K = 0 if stage.draft is None else stage.config.draft_len
    ids = stage.encode_prompts(prompts).cpu()
    P = ids.shape[1]
    # the upload: the UNPADDED prompt (what the tokenizer gave, folded into the vocabulary, cut to its last P ids), counts 0
    want_prompt = [[i % V for i in stage.tokenizer.encode(p, return_tensors=None)][-P:] for p in prompts]
    assert pack["prompt_ids"] == want_prompt
    assert all(ids[b, P - len(r):].tolist() == r for b, r in enumerate(want_prompt))
    assert any(len(r) < P for r in want_prompt)                                  # some row IS padded, and the pad id is not history
    assert np.array_equal(pack["state"][0], ref_seen_bits(want_prompt, V)) and not pack["state"][1].any()
    assert np.array_equal(pack["state"][2], np.stack([np.asarray(pack[k], dtype=np.float32) for k in ("rep", "pres", "freq")], 1))
    assert len(steps) == len(stage.step_inputs) == stage.last_steps
    changed = 0
    for (rows, commit), kept in zip(steps, stage.step_inputs):
        # ---- (b) the arguments of every call of the step
        assert len(rows) == (K + 1 if K else 1)
        if K:
            tok = kept["tok"].cpu()
            for k, ev in enumerate(rows[:K]):
                assert ev["n_prev"] == k and tuple(ev["before"].shape) == (B, V)
                assert tuple(ev["step_tok"].shape) == (B, K) and torch.equal(ev["step_tok"][:, :k], tok[:, :k])
            assert rows[K]["n_prev"] == 0 and tuple(rows[K]["before"].shape) == (B, K + 1, V)
            assert torch.equal(rows[K]["step_tok"], tok)
        else:
            assert rows[0]["n_prev"] == 0 and rows[0]["step_tok"] is None and tuple(rows[0]["before"].shape) == (B, V)
        # ---- (a) the edit, bit for bit
        for ev in rows:
            seen, counts, params = ev["state"]
            want = ref_penalty(ev["before"].clone(), seen, counts, params,
                               None if ev["step_tok"] is None else ev["step_tok"].numpy(), ev["n_prev"])
            assert _bits(want) == _bits(ev["after"])
            changed += int((want.view(torch.int16 if want.element_size() == 2 else torch.int32)
                            != ev["before"].view(torch.int16 if want.element_size() == 2 else torch.int32)).sum())
        # ---- (c) the state behind the commit: a host recount of the committed tokens, plus the unpadded prompt
        seen, counts, _ = commit["state"]
        want_counts = np.zeros((B, V), dtype=np.int32)
        history = []
        for b in range(B):
            gen = commit["tokens"][b, P:commit["seq_len"][b]].tolist()
            np.add.at(want_counts[b], np.asarray(gen, dtype=np.int64), 1)
            history.append(want_prompt[b] + gen)
        assert np.array_equal(counts, want_counts)
        assert np.array_equal(seen, ref_seen_bits(history, V))
    if n_tokens is not None:                                                     # the final state holds exactly the returned tokens
        assert steps[-1][1]["state"][1].sum(axis=1).tolist() == list(n_tokens)
    return changed


# ------------------------------------------------------------------------------------------ stage-level scenarios
# Row 1 is neutral.  The replayed scenario (check_generation demands every log-prob <= 0, which an f32 sampler delivers only
# while no token holds all of a nucleus: tests/token_mask_ref.py, RESTRICT_TEMPERATURE) uses penalties that DISCOURAGE
# repetition, which flatten a row; the other signs -- rep < 1, negative presence and frequency -- run under checks (a)-(c).
DISCOURAGE = dict(repetition_penalty=[1.3, 1.0, 2.0, 1.0, 1.1], presence_penalty=[0.5, 0.0, 2.0, 0.0, 0.0],
                  frequency_penalty=[0.25, 0.0, 0.0, 1.5, 2.0])
ENCOURAGE = dict(repetition_penalty=[0.8, 1.0, 0.5, 1.0, 1.5], presence_penalty=[-1.0, 0.0, 0.0, -2.0, 0.5],
                 frequency_penalty=[-0.5, 0.0, 0.0, 0.25, -2.0])
RECUR = 777                                      # a bias on this token makes it recur, so that counts above 1 occur
RECUR_BIAS = {RECUR: 6.0}


def run_recorded(stage, **kw):
    log = PenaltyLog(stage.ops)
    try:
        out = run_kept(stage, **kw)
    finally:
        log.close()
    return out, log


def scenario_replay(stage, atol):
    """Sampled and seeded, discouraging penalties with a token that recurs: checks (a)-(c) on the record, and the kept
    (penalised) rows replay through check_generation at the caller's bar."""
    kw = dict(prompts=PROMPTS, max_tokens=MAX_TOKENS, temperature=TEMPERATURE, seed=SEEDS, logit_bias=RECUR_BIAS)
    base, _, _ = stage.generate(**kw)
    (texts, lps, stats), log = run_recorded(stage, **kw, **DISCOURAGE)
    assert check_recorded(stage, log, PROMPTS, stats["n_tokens"]) > 0
    worst = check_generation(stage, texts, lps, inv_t_of(TEMPERATURE), atol=atol)
    assert texts[1] == base[1] and texts != base                                 # the neutral row; the penalties are live
    assert any(len(set(text_ids(t))) < len(text_ids(t)) for t in texts)          # some token recurred
    return worst


def scenario_signs_and_stops(stage, prompts=PROMPTS, max_tokens=MAX_TOKENS, seeds=SEEDS, penalties=None):
    """rep < 1 and negative penalties, with a stop id that ends some rows early: checks (a)-(c); a finished row's state is
    frozen while the others go on (the recount of (c) is of its frozen length)."""
    penalties = ENCOURAGE if penalties is None else penalties
    kw = dict(prompts=prompts, max_tokens=max_tokens, temperature=TEMPERATURE, seed=seeds, logit_bias=RECUR_BIAS)
    free, _, _ = stage.generate(**kw, **penalties)
    stop = next(t for x in free for t in text_ids(x)[2:4] if t != RECUR)         # a token some row commits early, not at once
    (texts, lps, stats), log = run_recorded(stage, stop_token_ids=[stop], **kw, **penalties)
    assert check_recorded(stage, log, prompts, stats["n_tokens"]) > 0
    assert "stop" in stats["finish_reasons"] and "length" in stats["finish_reasons"]
    assert min(stats["n_tokens"]) < max_tokens
    _, steps = log.steps()
    early = int(np.argmin(stats["n_tokens"]))
    frozen = [c["state"][1][early].tobytes() for _, c in steps if c["seq_len"][early] == steps[-1][1]["seq_len"][early]]
    assert len(frozen) >= 2 and len(set(frozen)) == 1                            # steps ran on behind the row's end: nothing moved
    assert all(np.isfinite(lp).all() for lp in lps)
    return stats


def scenario_rows_independent(stage):
    """Seeded, one value per prompt: row b is bit-equal, in text and log-prob bytes, to row b of the call that gives EVERY row
    b's three values (the same batch, so the same tilings)."""
    kw = dict(prompts=PROMPTS, max_tokens=MAX_TOKENS, temperature=TEMPERATURE, seed=SEEDS, logit_bias=RECUR_BIAS)
    base = stage.generate(**kw)
    mixed = stage.generate(**kw, **DISCOURAGE)
    for b in range(len(PROMPTS)):
        scal = base if b == 1 else stage.generate(**kw, **{k: v[b] for k, v in DISCOURAGE.items()})
        assert scal[0][b] == mixed[0][b], b
        assert scal[1][b].tobytes() == mixed[1][b].tobytes(), b
    assert sum(m != t for m, t in zip(mixed[0], base[0])) >= 3                   # the penalties are live
    return mixed


# The teacher-forced scenario runs on FLOAT32 stages (stage_configs(dtype=torch.float32)): its dense forward and the loop's
# incremental passes may differ by a unit in the last place, which for bf16 logits between 8 and 16 is 0.0625, above
# greedy_ref.LOSSLESS_GAP -- a position that differs by one bf16 ulp would count as clear.  In f32 the two passes agree far
# inside the gap.  The bias lifts one token to the top, the penalties push it down again as it recurs: the scenario in which
# tokens recur AND the text differs from the unpenalised run, chosen on the CPU twin (shares 0.93, 0.93, 1.0 for the stages).
GREEDY = dict(repetition_penalty=1.2, presence_penalty=0.5, frequency_penalty=0.5)
GREEDY_BIAS = {RECUR: 6.0}


def scenario_greedy(stage):
    """temperature 0: checks (a)-(c), the kept rows replay through greedy_ref.check_replay (every committed token is the
    lowest-id arg-max of its penalised row), and the text is the TEACHER-FORCED penalised arg-max: a dense forward of the
    stage's model over prompt + text, the bias and then ref_penalty applied position by position with the prefix's history."""
    assert stage.config.dtype == torch.float32
    kw = dict(prompts=PROMPTS, max_tokens=MAX_TOKENS, temperature=0.0, logit_bias=GREEDY_BIAS)
    base, _, _ = stage.generate(**kw)
    (texts, lps, stats), log = run_recorded(stage, **kw, **GREEDY)
    assert check_recorded(stage, log, PROMPTS, stats["n_tokens"]) > 0
    greedy_ref.check_replay(stage, texts, lps)
    share = check_teacher_forced(stage, texts, GREEDY, GREEDY_BIAS)
    assert any(len(set(text_ids(t))) < len(text_ids(t)) for t in texts)          # some generated token recurred
    assert any(t != f for t, f in zip(texts, base))                              # and the penalties changed a text
    return share


def check_teacher_forced(stage, texts, penalties, bias, max_tokens=MAX_TOKENS):
    V = stage.shape.vocab
    ids = stage.encode_prompts(PROMPTS)
    P = ids.shape[1]
    prompt = [[i % V for i in stage.tokenizer.encode(p, return_tensors=None)][-P:] for p in PROMPTS]
    gen = [text_ids(t) for t in texts]
    m = stage.model
    m.reset()
    dense = m.forward(torch.cat([ids, torch.tensor(gen, dtype=torch.int64, device=ids.device)], 1)).cpu()[:, P - 1:P - 1 + max_tokens]
    m.reset()
    params = np.array([[penalties["repetition_penalty"], penalties["presence_penalty"], penalties["frequency_penalty"]]], np.float32)
    edits = [(t, float(v), 0) for t, v in sorted(bias.items())]
    clear = np.zeros((len(PROMPTS), max_tokens), dtype=bool)
    hit = np.zeros_like(clear)
    for b in range(len(PROMPTS)):
        for i in range(max_tokens):
            row = dense[b, i].clone()[None]                                      # [1, V], the model's dtype
            ref_logit_edit(row, [edits], [P + i], P)
            counts = np.bincount(np.asarray(gen[b][:i], dtype=np.int64), minlength=V).astype(np.int32)[None]
            ref_penalty(row, ref_seen_bits([prompt[b] + gen[b][:i]], V), counts, params)
            x = row[0].float().numpy()
            top2 = np.sort(x)[-2:]
            clear[b, i] = top2[1] - top2[0] > greedy_ref.LOSSLESS_GAP
            hit[b, i] = int(x.argmax()) == gen[b][i]
    assert clear.mean() >= greedy_ref.LOSSLESS_KEEP, clear.mean()
    assert hit[clear].all(), np.argwhere(clear & ~hit)
    return float(clear.mean())


__all__ = ["DISCOURAGE", "ENCOURAGE", "PenaltyLog", "PenaltyOracleOps", "check_recorded", "ref_penalty", "ref_penalty_commit",
           "ref_seen_bits", "run_recorded", "scenario_greedy", "scenario_replay", "scenario_rows_independent",
           "scenario_signs_and_stops", "state_arrays"]
