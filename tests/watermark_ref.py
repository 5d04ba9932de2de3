"""The green-list watermark (serving/stages.py, WATERMARK; include/asd_hip.h, asd_watermark_rows / asd_watermark_score): the
numpy statement of the predicate on tests/philox_ref.philox4x32_10, the plain references of the two kernels written from the
header's text, the oracle ops twin that serves them to the stage loops, and the stage scenario that
tests/test_watermark_arg_checks.py (CPU twin) and tests/test_gpu_watermark.py (HipOps) both run.

TEST INFRASTRUCTURE, like tests/dry_ref.py: never importable from the package."""
from types import SimpleNamespace

import numpy as np
import torch

from tests.dry_ref import DryOracleOps
from tests.logit_edit_ref import SEEDS, run_kept
from tests.philox_ref import philox4x32_10
from tests.stage_scenario import MAX_TOKENS, PROMPTS, TEMPERATURE, text_ids

NONE = 0xFFFFFFFF                                # the filler of a context narrower than 3
FMAX = np.finfo(np.float32).max


def threshold(gamma):
    return min(max(int(round(float(gamma) * 65536.0)), 1), 65535)


def green(key, h, thr, H, v):
    """bool like v: token v is green behind the history H (a list, len(H) >= h) under (key, h, thr): ONE Philox call per
    token, counter (v >> 3, H[-1], H[-2] | NONE, H[-3] | NONE), halfword v & 7."""
    v = np.asarray(v, dtype=np.int64).astype(np.uint64) & np.uint64(NONE)
    ctx = [(int(H[-1 - i]) & NONE) if i < h else NONE for i in range(3)]
    w = philox4x32_10((v >> np.uint64(3), *ctx), (int(key) & NONE, int(key) >> 32)).astype(np.uint64)
    word = np.take_along_axis(w, ((v >> np.uint64(1)) & np.uint64(3)).astype(np.int64)[..., None], -1)[..., 0]
    return ((word >> (np.uint64(16) * (v & np.uint64(1)))) & np.uint64(0xFFFF)) < np.uint64(thr)


def _live(rec):
    key, delta, thr, h = rec
    return key is not None and thr != 0 and 1 <= h <= 3 and 0.0 < float(np.float32(delta)) < np.inf


def ref_watermark_rows(x, recs, tokens, seq_len, row_start, start, max_len, step_tok=None, n_prev=0):
    """asd_watermark_rows on a CPU tensor, IN PLACE (-> x): x [B, V] or [B, K1, V] (any strides); recs: one (key or None,
    delta, thr, h) per sequence as the record holds them; the other arguments as tests/dry_ref.py's."""
    view = x[:, None] if x.dim() == 2 else x
    Bv, K1, V = view.shape
    top = torch.finfo(x.dtype).max
    for b, rec in enumerate(recs):
        if not _live(rec):
            continue
        key, delta, thr, h = rec
        L = min(max(int(seq_len[b]), start), max_len)
        first = start if row_start is None else min(max(int(row_start[b]), 0), start)
        committed = [int(t) for t in tokens[b][first:L]]
        for j in range(K1):
            H = committed + ([] if step_tok is None else [int(t) for t in step_tok[b][:n_prev + j]])
            if len(H) < h:
                continue
            xf = view[b, j].float().numpy()
            with np.errstate(over="ignore", invalid="ignore"):
                y = np.minimum(xf + np.float32(delta), FMAX)                         # one f32 add
            new = torch.from_numpy(y).to(x.dtype)                                    # to nearest even
            new = torch.where(torch.isinf(new), torch.full_like(new, top), new)      # ... then the clamp
            go = torch.from_numpy(green(key, h, thr, H, np.arange(V)) & np.isfinite(xf))
            view[b, j] = torch.where(go, new, view[b, j])
    return x


def ref_watermark_score(tokens, recs, row_start, row_from, seq_len, max_len):
    """asd_watermark_score -> int32 [B, 2]: {n_scored, n_green}."""
    out = np.zeros((len(recs), 2), dtype=np.int32)
    for b, (key, _, thr, h) in enumerate(recs):
        if key is None or thr == 0 or not 1 <= h <= 3:
            continue
        L = min(max(int(seq_len[b]), 0), max_len)
        first = 0 if row_start is None else min(max(int(row_start[b]), 0), L)
        lo = max(min(max(int(row_from[b]), first), L), first + h)
        for i in range(lo, L):
            out[b] += (1, int(green(key, h, thr, list(tokens[b][first:i]), tokens[b][i])))
    return out


class WatermarkOracleOps(DryOracleOps):
    """DryOracleOps + pack_watermark, watermark_rows and watermark_score on the references above: the tiny stages run without a GPU."""

    def pack_watermark(self, keys, deltas, gammas, contexts, prompt_lens, P, device):
        self._note("pack_watermark", ())
        thr = [0 if k is None else threshold(g) for k, g in zip(keys, gammas)]
        return SimpleNamespace(recs=list(zip(keys, deltas, thr, contexts)), thr=tuple(thr), P=int(P), B=len(thr),
                               row_start=[int(P) - int(m) for m in prompt_lens])

    def watermark_rows(self, logits, wm, tokens, seq_len, max_len, step_tok=None, n_prev=0):
        self._note("watermark_rows", ())
        return ref_watermark_rows(logits, wm.recs, tokens.numpy(), seq_len.tolist(), wm.row_start, wm.P, max_len,
                                  None if step_tok is None else step_tok.numpy(), n_prev)

    def watermark_score(self, tokens, wm, row_from, seq_len, max_len):
        self._note("watermark_score", ())
        return torch.from_numpy(ref_watermark_score(tokens.numpy(), wm.recs, wm.row_start, row_from.tolist(), seq_len.tolist(), max_len))


# ------------------------------------------------------------------------------------------ the stage-level scenario
KEY, GAMMA, DELTA, MARGIN = 0xC0FFEE0123456789, 0.5, 90.0, 40.0


def scenario_every_token_green(stage, greedy):
    """A seeded (or greedy) call with a key, gamma 0.5 and a delta above the spread of the stage's finite logits: on the kept
    rows, with the bias taken off again, max - min stays MARGIN under DELTA (at temperature 0.7 a token that is not green
    then has probability below 64 e^-57), so EVERY generated token is green under the reference predicate; stats and
    detect_watermark return those counts; a per-prompt list of None keys is the call without the keywords, bit for bit."""
    kw = dict(prompts=PROMPTS, max_tokens=MAX_TOKENS, temperature=0.0 if greedy else TEMPERATURE, seed=SEEDS)
    plain = stage.generate(**kw)
    on = dict(watermark_key=KEY, watermark_gamma=GAMMA, watermark_delta=DELTA)
    texts, _, stats = run_kept(stage, **on, **kw)
    ids, real = stage._encode(PROMPTS)
    P, gen, thr, V = ids.shape[1], [text_ids(t) for t in texts], threshold(GAMMA), stage.shape.vocab
    spread = 0.0
    for step, s in enumerate(stage.step_inputs):
        verify, x = s.get("tok") is not None, s["logits"].cpu()                    # (a greedy step keeps its K + 1 rows in one tensor)
        rows = torch.cat([x, s["bonus"].cpu()[:, None]], 1) if "bonus" in s else (x[:, None] if x.dim() == 2 else x)
        seq, tok = (s["seq_len"].tolist(), s["tok"].tolist()) if verify else ([P + step] * len(gen), [[]] * len(gen))
        for b in range(len(gen)):
            for j in range(rows.shape[1]):
                x = rows[b, j].double().numpy() - DELTA * green(KEY, 1, thr, real[b] + gen[b][:seq[b] - P] + tok[b][:j], np.arange(V))
                spread = max(spread, float(x[np.isfinite(x)].max() - x[np.isfinite(x)].min()))
    assert 0.0 < spread < DELTA - MARGIN, spread
    assert texts != plain[0]
    for b, g in enumerate(gen):
        n = sum(bool(green(KEY, 1, thr, real[b] + g[:i], g[i])) for i in range(len(g)))
        assert n == len(g) == MAX_TOKENS, (b, n)
        z = (n - thr / 65536.0 * n) / np.sqrt(n * thr / 65536.0 * (1.0 - thr / 65536.0))
        assert stats["watermark"][b] == {"n_scored": n, "n_green": n, "z": z}
    assert stage.detect_watermark(texts, KEY, gamma=GAMMA, prompts=PROMPTS) == stats["watermark"]
    assert stage.detect_watermark(gen, KEY, gamma=GAMMA)[0]["n_scored"] == MAX_TOKENS - 1      # no prompt: the first token is context
    off = stage.generate(watermark_key=[None] * len(PROMPTS), **kw)
    assert off[0] == plain[0] and all(a.tobytes() == b.tobytes() for a, b in zip(off[1], plain[1])) and "watermark" not in off[2]
