"""Allow-lists (serving/stages.py, ALLOW-LISTS; include/asd_hip.h, asd_logit_mask_rows): the torch-on-CPU reference of the
kernel, written from the header's text, the oracle ops twin that masks through it, and the stage-level scenarios that
tests/test_token_mask_stages.py (CPU twin) and tests/test_gpu_token_mask_stages.py (HipOps) both run.

TEST INFRASTRUCTURE, like tests/logit_edit_ref.py: never importable from the package."""
from types import SimpleNamespace

import numpy as np
import torch

from tests.logit_edit_ref import MIN_TOKENS, SEEDS, EditOracleOps, check_min_tokens_rule, run_kept
from tests.per_request_ref import inv_t_of
from tests.stage_scenario import MAX_TOKENS, PROMPTS, TEMPERATURE, check_generation, text_ids

FORCED = 777
# The replay of tests/stage_scenario.py (check_generation) demands every returned log-prob <= 0.  An f32 sampler delivers that
# only while the token's renormalised mass stays clear of 1: a list of 17 (or 5, or 4) ids at the scenario's temperature 0.7
# often leaves ONE token in the 0.9 nucleus, whose log-prob is 0 up to the last bit of the kernel's arithmetic, on either side
# (tests/logit_edit_ref.py::scenario_force sets its bar at > -1e-6 for the same reason).  So the runs that are replayed use a
# temperature at which no list of >= 4 ids can do that: with |x| <= RESTRICT_LOGIT_BOUND (asserted on the kept logits) two
# logits differ by at most 2 nats at T = 100, the top token of n ids holds at most e^2 / (e^2 + n - 1) -- 0.71 at n = 4 -- so
# the nucleus keeps at least two tokens and a renormalised mass is at most 0.71 / 0.9.  The peaked end is scenario_single's
# and scenario_greedy's.
RESTRICT_TEMPERATURE = 100.0
RESTRICT_LOGIT_BOUND = 100.0


def ref_pack_bits(lists, V):
    """One uint32 [W] word array per id list, from the header's sentence: bit v & 31 of word v >> 5 is set when v is kept."""
    W = (V + 31) // 32
    out = np.zeros((len(lists), W), dtype=np.uint32)
    for r, ids in enumerate(lists):
        for v in ids:
            out[r, v >> 5] |= np.uint32(1 << (v & 31))
    return out


def ref_logit_mask(x, bits, mask_row=None):
    """asd_logit_mask_rows on a CPU tensor, IN PLACE (-> x): x [B, V] or [B, K1, V] (any strides); bits [R, W] (numpy uint32 /
    int32, or an int32 tensor), W = (V + 31) // 32; mask_row: B ints or None (every sequence uses mask 0).  Element v < V of
    every position of sequence b becomes -inf when bit v & 31 of word v >> 5 of mask mask_row[b] is clear; a sequence whose
    index is outside [0, R) is not touched; bits at v >= V are never looked at."""
    view = x[:, None] if x.dim() == 2 else x
    Bv, K1, V = view.shape
    words = (bits.cpu().numpy() if isinstance(bits, torch.Tensor) else np.asarray(bits)).astype(np.int64) & 0xFFFFFFFF
    R = words.shape[0]
    v = np.arange(V)
    for b in range(Bv):
        r = 0 if mask_row is None else int(mask_row[b])
        if not 0 <= r < R:
            continue
        clear = torch.from_numpy(((words[r][v >> 5] >> (v & 31)) & 1) == 0)
        for j in range(K1):
            view[b, j][clear] = float("-inf")                                      # a view: the assignment lands in x
    return x


class MaskOracleOps(EditOracleOps):
    """EditOracleOps + pack_token_masks and logit_mask_rows on the reference above: the three tiny stages run without a GPU."""

    def pack_token_masks(self, rows, V, device):
        self._note("pack_token_masks", ())
        lists, mask_row = [], []
        for ids in rows:
            if ids is None:
                mask_row.append(-1)
                continue
            ids = tuple(int(t) for t in ids)
            assert ids and list(ids) == sorted(set(ids)) and 0 <= ids[0] and ids[-1] < V     # what the stage hands over
            if ids not in lists:
                lists.append(ids)
            mask_row.append(lists.index(ids))
        return SimpleNamespace(bits=ref_pack_bits(lists, V), mask_row=mask_row, R=len(lists))

    def logit_mask_rows(self, logits, masks):
        self._note("logit_mask_rows", ())
        return ref_logit_mask(logits, masks.bits, masks.mask_row)


# ------------------------------------------------------------------------------------------ stage-level scenarios
def allow_list(V, n, seed):
    """n distinct ids of [0, V), sorted; the ends of the vocabulary and the word boundary 31 | 32 come first."""
    ids = set([V - 1, 0, 32, 31][:n])
    for t in np.random.default_rng(seed).permutation(np.arange(1, V - 1)):
        if len(ids) >= n:
            break
        ids.add(int(t))
    return sorted(ids)


def per_prompt_lists(V):
    """One list per prompt, of different sizes, prompt 2 without one."""
    return [allow_list(V, 17, 1), allow_list(V, 5, 2), None, allow_list(V, 64, 3), allow_list(V, 17, 1)]


def _cpu(s):
    return {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in s.items()}


def _outside(V, ids):
    keep = torch.zeros(V, dtype=torch.bool)
    keep[list(ids)] = True
    return ~keep


def check_restricted(stage, texts, lps, lists):
    """Every committed, proposed and kept-bonus token is in its row's list; the kept draft and target logits are -inf outside
    it (and not all -inf inside); log-probs are finite."""
    V = stage.shape.vocab
    assert stage.step_inputs
    for b, ids in enumerate(lists):
        assert np.isfinite(lps[b]).all()
        if ids is None:
            continue
        assert set(text_ids(texts[b])) <= set(ids), (b, texts[b])
        out = _outside(V, ids)
        for s in map(_cpu, stage.step_inputs):
            assert torch.isneginf(s["logits"][b][..., out]).all()                  # [V] at stage 0, [K, V] above it
            assert torch.isfinite(s["logits"][b][..., ids]).all()
            assert float(s["logits"][b][..., ids].float().abs().max()) <= RESTRICT_LOGIT_BOUND
            assert int(s["drawn"][b]) in ids
            if "bonus" in s:
                assert torch.isneginf(s["bonus"][b][out]).all()
            if "tok" in s and s["tok"] is not None:
                assert set(s["tok"][b].tolist()) <= set(ids), (b, s["tok"][b].tolist())      # the DRAFT side was masked too


def scenario_restrict(stage, atol):
    """A 17-id list for the call, then one list per prompt with one prompt None; the runs replay through check_generation
    unchanged (the kept logits are the masked ones).  At RESTRICT_TEMPERATURE: see there."""
    V = stage.shape.vocab
    kw = dict(prompts=PROMPTS, max_tokens=MAX_TOKENS, temperature=RESTRICT_TEMPERATURE, seed=SEEDS)
    worst = 0.0
    for lists in (allow_list(V, 17, 1), per_prompt_lists(V)):
        texts, lps, _ = run_kept(stage, allowed_token_ids=lists, **kw)
        per_row = lists if lists[2] is None else [lists] * len(PROMPTS)
        check_restricted(stage, texts, lps, per_row)
        worst = max(worst, check_generation(stage, texts, lps, inv_t_of(RESTRICT_TEMPERATURE), atol=atol))
    return worst


def scenario_single(stage):
    """A one-id list: the only finite logit of every row, so every committed token is that id with log-prob 0 (scenario_force's
    bar: > -1e-6)."""
    texts, lps, _ = stage.generate(prompts=PROMPTS, max_tokens=MAX_TOKENS, temperature=TEMPERATURE, allowed_token_ids=[FORCED])
    for t, lp in zip(texts, lps):
        assert text_ids(t) == [FORCED] * MAX_TOKENS
        assert np.isfinite(lp).all() and (lp > -1e-6).all(), lp


def scenario_greedy(stage):
    """temperature 0: every committed token is the lowest-id arg-max of its kept row restricted to the row's list."""
    V = stage.shape.vocab
    lists = per_prompt_lists(V)
    free, _, _ = stage.generate(prompts=PROMPTS, max_tokens=MAX_TOKENS, temperature=0.0)
    texts, lps, _ = run_kept(stage, prompts=PROMPTS, max_tokens=MAX_TOKENS, temperature=0.0, allowed_token_ids=lists)
    assert texts[2] == free[2] and sum(t != f for t, f in zip(texts, free)) == 4   # the row without a list; the lists are live
    n_checked = 0
    for s in map(_cpu, stage.step_inputs):
        for b, ids in enumerate(lists):
            if ids is None:
                continue
            rows = s["logits"][b].float().reshape(-1, V)                           # [1, V] at stage 0, [K + 1, V] above it
            n_acc = int(s["n_acc"][b])
            committed = ([] if s["tok"] is None else s["tok"][b, :n_acc].tolist()) + [int(s["drawn"][b])]
            for i, t in enumerate(committed):
                vals = rows[i][ids]
                assert t == ids[int(torch.nonzero(vals == vals.max())[0])], (b, i, t)
                assert torch.isneginf(rows[i][_outside(V, ids)]).all()
                n_checked += 1
    assert n_checked >= 4 * MAX_TOKENS
    for b, ids in enumerate(lists):
        assert ids is None or set(text_ids(texts[b])) <= set(ids)
        assert np.isfinite(lps[b]).all()


def scenario_rows_independent(stage):
    """Seeded, one list (or None) per prompt: row b is bit-equal, in text and log-prob bytes, to row b of the call that gives
    EVERY row list b (the same batch, so the same tilings)."""
    lists = per_prompt_lists(stage.shape.vocab)
    kw = dict(prompts=PROMPTS, max_tokens=MAX_TOKENS, temperature=TEMPERATURE, seed=SEEDS)
    base = stage.generate(**kw)
    mixed = stage.generate(allowed_token_ids=lists, **kw)
    alone = {}
    for b, ids in enumerate(lists):
        key = None if ids is None else tuple(ids)
        if key not in alone:
            alone[key] = base if ids is None else stage.generate(allowed_token_ids=ids, **kw)
        scal = alone[key]
        assert scal[0][b] == mixed[0][b], b
        assert scal[1][b].tobytes() == mixed[1][b].tobytes(), b
    assert sum(m != t for m, t in zip(mixed[0], base[0])) == 4                     # the lists are live
    return mixed


def scenario_with_edits(stage):
    """Allow-list, bias, ban and min_tokens in one seeded call == the call whose allow-list is written as a ban of the
    complement (vocabulary 1000: the complement fits the sparse edit's 1024 entries), bit for bit in text and log-prob bytes.
    The stop ids are the rows' first tokens under the list, so min_tokens has something to hold back."""
    V = stage.shape.vocab
    assert V == 1000
    allowed = allow_list(V, 40, 4)
    kw = dict(prompts=PROMPTS, max_tokens=MAX_TOKENS, temperature=TEMPERATURE, seed=SEEDS)
    base, _, _ = stage.generate(allowed_token_ids=allowed, **kw)
    toks = [text_ids(t) for t in base]
    stops = sorted({t[0] for t in toks})
    bans = [[t[3]] for t in toks]
    complement = sorted(set(range(V)) - set(allowed))
    # (the last bias names a masked id: it stays -inf under the mask, and the ban wins over it in the other call)
    bias = [{t[1]: -8.0, allowed[(allowed.index(t[2]) + 1) % len(allowed)]: 6.0, complement[0]: 3.0} for t in toks]
    kw.update(stop_token_ids=stops, min_tokens=MIN_TOKENS, logit_bias=bias)
    a = stage.generate(allowed_token_ids=allowed, banned_token_ids=bans, **kw)
    b = stage.generate(banned_token_ids=[sorted(set(complement) | set(x)) for x in bans], **kw)
    assert a[0] == b[0]
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a[1], b[1]))
    assert a[2]["n_tokens"] == b[2]["n_tokens"] and a[2]["finish_reasons"] == b[2]["finish_reasons"]
    check_min_tokens_rule(a[2], a[0], stops, MIN_TOKENS)
    for r, t in enumerate(a[0]):
        assert set(text_ids(t)) <= set(allowed) - set(bans[r]) and np.isfinite(a[1][r]).all()
    assert a[0] != base


def scenario_top_n(stage):
    """A 3-id list with logprobs = 5: slots 0..2 of every committed token's table are the list, slots 3 and 4 hold -1 / -inf."""
    ids = allow_list(stage.shape.vocab, 3, 5)
    texts, lps, stats = stage.generate(prompts=PROMPTS, max_tokens=MAX_TOKENS, temperature=TEMPERATURE, seed=SEEDS, logprobs=5,
                                       allowed_token_ids=ids)
    for b in range(len(PROMPTS)):
        top_id, top_lp = stats["top_token_ids"][b], stats["top_logprobs"][b]
        assert top_id.shape == top_lp.shape == (MAX_TOKENS, 5)
        assert (top_id[:, 3:] == -1).all() and np.isneginf(top_lp[:, 3:]).all()
        assert all(sorted(row) == ids for row in top_id[:, :3].tolist())
        assert np.isfinite(top_lp[:, :3]).all() and (np.diff(top_lp[:, :3], axis=1) <= 0).all()
        assert set(text_ids(texts[b])) <= set(ids) and np.isfinite(lps[b]).all()


__all__ = ["FORCED", "MaskOracleOps", "RESTRICT_TEMPERATURE", "allow_list", "check_restricted", "per_prompt_lists", "ref_logit_mask", "ref_pack_bits",
           "scenario_greedy", "scenario_restrict", "scenario_rows_independent", "scenario_single", "scenario_top_n",
           "scenario_with_edits"]
