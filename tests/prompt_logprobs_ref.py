"""prompt_logprobs (serving/stages.py, PROMPT LOG-PROBS; include/asd_hip.h, asd_prompt_logprobs): the numpy f64 reference of the
kernel, written from the header's text, the oracle ops twin that scores through it, and the stage-level scenarios that
tests/test_prompt_logprobs_stages.py (CPU twin) and tests/test_gpu_prompt_logprobs_stages.py (HipOps) both run on
stage_configs(vocab=64).

TEST INFRASTRUCTURE, like tests/ngram_ref.py: never importable from the package."""
import numpy as np
import torch

from tests.logit_edit_ref import SEEDS, run_kept
from tests.ngram_ref import NgramOracleOps, real_ids
from tests.stage_scenario import NAMES, PROMPTS, TEMPERATURE, LogprobPredictor
from tests.top_logprobs_ref import LP_ATOL, ref_top_logprobs

VOCAB = 64                                       # the stages of the scenarios: stage_configs(vocab=VOCAB)
PL_MAX_TOKENS = 6
TABLE_KEYS = ("prompt_top_token_ids", "prompt_top_logprobs")
KEYS = ("prompt_token_ids", "prompt_logprobs", "prompt_ranks") + TABLE_KEYS


def ref_prompt_logprobs(x, target, first, n, inv_t=1.0):
    """asd_prompt_logprobs in numpy f64.  x: [B, T, V] f32 (the stored values, upcast: exact); target: int [B, T]; first: B ints
    or None -> (lp f64 [B,T], rank int32 [B,T], top_id int32 [B,T,n], top_lp f64 [B,T,n]).  Scored row (t >= first[b]), g =
    target[b,t]: lp = x[g]*a - lse(x*a); rank = 1 + #{v: x[v] > x[g], or x[v] == x[g] and v < g} (NaN elements never counted, -inf
    like any value); g outside [0, V) or a NaN x[g]: lp NaN, rank 0; the table is ref_top_logprobs'.  Skipped row: lp 0, rank 0,
    ids -1, table -inf."""
    x = np.asarray(x, dtype=np.float32)
    B, T, V = x.shape
    target = np.asarray(target).reshape(B, T)
    first = [0] * B if first is None else [int(f) for f in first]
    a = float(np.float32(inv_t))
    lp = np.zeros((B, T), np.float64)
    rank = np.zeros((B, T), np.int32)
    top_id, top_lp = ref_top_logprobs(x, n, inv_t) if n else (np.zeros((B, T, 0), np.int32), np.zeros((B, T, 0), np.float64))
    idx = np.arange(V)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for b in range(B):
            for t in range(T):
                if t < first[b]:
                    top_id[b, t], top_lp[b, t] = -1, -np.inf
                    continue
                row, g = x[b, t], int(target[b, t])
                if not 0 <= g < V or np.isnan(row[g]):
                    lp[b, t] = np.nan
                    continue
                z = row.astype(np.float64) * a
                if np.isnan(z).any():
                    lse = np.nan
                else:
                    m = z.max()
                    lse = m + np.log(np.exp(z - m).sum()) if np.isfinite(m) else m
                lp[b, t] = z[g] - lse
                rank[b, t] = 1 + int(np.count_nonzero((row > row[g]) | ((row == row[g]) & (idx < g))))
    return lp, rank, top_id, top_lp


class PromptOracleOps(NgramOracleOps):
    """NgramOracleOps + prompt_logprobs on the reference above: the tiny stages run without a GPU."""

    def prompt_logprobs(self, logits, target, first, n, inv_temperature=1.0, splits=0):
        self._note("prompt_logprobs", ())
        assert logits.dim() == 3 and tuple(target.shape) == tuple(logits.shape[:2]) and target.dtype == torch.int32
        assert first is None or (tuple(first.shape) == (logits.shape[0],) and first.dtype == torch.int32)
        lp, rank, top_id, top_lp = ref_prompt_logprobs(logits.float().numpy(), target.numpy(), None if first is None else first.tolist(),
                                                       n, inv_temperature)
        f32 = lambda v: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32))   # noqa: E731
        return f32(lp), torch.from_numpy(rank), (torch.from_numpy(top_id) if n else None), (f32(top_lp) if n else None)


class AllCalls:
    """Stands between a stage and EVERY public op of `ops` (instance attributes: the ops object stays what it is) and notes the
    order of their calls; works on the twin and on HipOps alike."""

    def __init__(self, ops):
        self.ops, self.names, self.wrapped = ops, [], []
        for name in dir(ops):
            orig = getattr(ops, name)
            if name.startswith("_") or not callable(orig) or isinstance(orig, type):
                continue

            def wrapped(*a, _orig=orig, _name=name, **kw):
                self.names.append(_name)
                return _orig(*a, **kw)
            setattr(ops, name, wrapped)
            self.wrapped.append(name)

    def close(self):
        for name in self.wrapped:
            delattr(self.ops, name)


# ------------------------------------------------------------------------------------------ stage-level scenarios
def _bits(arrays):
    return [np.asarray(a).tobytes() for a in arrays]


def check_stats(stage, stats, n, prompts=PROMPTS):
    """Scenario (a): keys, shapes and dtypes; m_i = (real prompt tokens of row i) - 1."""
    real, _ = real_ids(stage, prompts)
    for key in KEYS:
        assert (key in stats) == (n > 0 or key not in TABLE_KEYS), key
        if key in stats:
            assert len(stats[key]) == len(prompts)
    for i, r in enumerate(real):
        m = max(len(r) - 1, 0)
        assert stats["prompt_token_ids"][i].dtype == np.int32 and stats["prompt_token_ids"][i].tolist() == list(r)
        assert stats["prompt_logprobs"][i].shape == (m,) and stats["prompt_logprobs"][i].dtype == np.float32
        assert stats["prompt_ranks"][i].shape == (m,) and stats["prompt_ranks"][i].dtype == np.int32
        if n:
            assert stats["prompt_top_token_ids"][i].shape == (m, n) and stats["prompt_top_token_ids"][i].dtype == np.int32
            assert stats["prompt_top_logprobs"][i].shape == (m, n) and stats["prompt_top_logprobs"][i].dtype == np.float32
    return [max(len(r) - 1, 0) for r in real]


def check_values(stage, stats, n, prompts=PROMPTS):
    """Scenario (b): what the call kept (stage.prompt_inputs) is the prefill of the padded prompts, and the returned numbers are
    the f64 reference's on those logits: ids and ranks exact on every entry, log-probs within LP_ATOL.  -> max |lp - f64|."""
    kept = stage.prompt_inputs
    assert kept is not None
    ids, real = stage._encode(prompts)
    B, P = ids.shape
    x = kept["logits"].float().cpu().numpy()
    target, first = kept["target"].cpu().numpy(), kept["first"].cpu().tolist()
    assert x.shape[:2] == (B, P - 1) and np.array_equal(target, ids.cpu().numpy()[:, 1:]) and first == [P - len(r) for r in real]
    lp, rank, top_id, top_lp = ref_prompt_logprobs(x, target, first, n)
    worst = 0.0
    for i, r in enumerate(real):
        m = max(len(r) - 1, 0)
        got_lp, got_rank = stats["prompt_logprobs"][i], stats["prompt_ranks"][i]
        assert np.array_equal(got_rank, rank[i, P - 1 - m:]), i
        assert (got_rank >= 1).all() and np.isfinite(got_lp).all()
        diffs = [np.abs(got_lp.astype(np.float64) - lp[i, P - 1 - m:])]
        if n:
            assert np.array_equal(stats["prompt_top_token_ids"][i], top_id[i, P - 1 - m:]), i
            diffs.append(np.abs(stats["prompt_top_logprobs"][i].astype(np.float64) - top_lp[i, P - 1 - m:]).ravel())
            for j in range(m):                                           # a listed prompt token carries its table entry's bits
                if got_rank[j] <= n:
                    assert stats["prompt_top_token_ids"][i][j, got_rank[j] - 1] == r[j + 1]
                    assert stats["prompt_top_logprobs"][i][j, got_rank[j] - 1].tobytes() == got_lp[j].tobytes()
                else:
                    assert r[j + 1] not in stats["prompt_top_token_ids"][i][j].tolist()
        if m:
            worst = max(worst, max(float(d.max()) for d in diffs))
    assert worst <= LP_ATOL, worst
    return worst


def scenario_values(stage, n, temperature=TEMPERATURE):
    """Scenarios (a), (b) and (e) on PROMPTS: unequal lengths (so padding is present), rows with m_i = 0 ("hard") and 1."""
    texts, lps, stats = run_kept(stage, prompts=PROMPTS, max_tokens=PL_MAX_TOKENS, temperature=temperature, seed=SEEDS,
                                 prompt_logprobs=n)
    m = check_stats(stage, stats, n)
    assert 0 in m and 1 in m and max(m) > 2 and len(set(m)) > 2
    check_values(stage, stats, n)
    assert stage.generate(prompts=PROMPTS, max_tokens=2, temperature=0.0)[2].keys().isdisjoint(KEYS)       # off: no key
    assert stage.prompt_inputs is None
    return stats


def scenario_same_bits(stage, temperature=TEMPERATURE):
    """Scenario (c): the same seeded call with and without prompt_logprobs returns bit-equal texts, log-probs and top-N tables."""
    kw = dict(prompts=PROMPTS, max_tokens=PL_MAX_TOKENS, temperature=temperature, seed=SEEDS, logprobs=2)
    off = stage.generate(**kw)
    for n in (0, 3):
        on = stage.generate(prompt_logprobs=n, **kw)
        assert on[0] == off[0] and _bits(on[1]) == _bits(off[1])
        assert _bits(on[2]["top_token_ids"]) == _bits(off[2]["top_token_ids"])
        assert _bits(on[2]["top_logprobs"]) == _bits(off[2]["top_logprobs"])
        assert on[2]["n_tokens"] == off[2]["n_tokens"] and "prompt_ranks" in on[2] and "prompt_ranks" not in off[2]


def scenario_call_trace(stage):
    """Scenario (d): the ops calls of a call with the feature on are those of the call without it plus exactly one
    prompt_logprobs, made before the first step's ops; None and a configuration without a value make none."""
    kw = dict(prompts=PROMPTS, max_tokens=4, temperature=TEMPERATURE, seed=SEEDS, logprobs=2)
    log = AllCalls(stage.ops)
    try:
        stage.generate(**kw)
        off = list(log.names)
        del log.names[:]
        stage.generate(prompt_logprobs=None, **kw)
        none = list(log.names)
        del log.names[:]
        stage.generate(prompt_logprobs=2, **kw)
        on = list(log.names)
    finally:
        log.close()
    assert off and none == off and "prompt_logprobs" not in off
    assert on.count("prompt_logprobs") == 1
    at = on.index("prompt_logprobs")
    assert on[:at] + on[at + 1:] == off
    firsts = [i for i, name in enumerate(off) if name in ("step_uniforms", "draft_sample", "draft_sample_rows", "verify_greedy")]
    assert firsts and at <= firsts[0]                                    # ahead of everything a step draws with
    return on


def scenario_composition(stage):
    """Scenario (f): an allow-list, a bias and penalties change the generated text and leave the prompt's numbers alone -- the
    prompt is scored on the raw logits."""
    V = stage.shape.vocab
    kw = dict(prompts=PROMPTS, max_tokens=PL_MAX_TOKENS, temperature=0.0, prompt_logprobs=3)
    plain = stage.generate(**kw)
    allowed = [t for t in range(V) if t % 4 != 1]
    edited = stage.generate(allowed_token_ids=allowed, logit_bias={allowed[5]: 4.0}, repetition_penalty=1.3, frequency_penalty=0.5,
                            presence_penalty=0.2, no_repeat_ngram_size=2, **kw)
    assert edited[0] != plain[0]
    for key in KEYS:
        assert _bits(edited[2][key]) == _bits(plain[2][key]), key
    check_stats(stage, edited[2], 3)


def scenario_pipeline(manager):
    """Scenario (g): PipelineConfig.prompt_logprobs reaches every stage call, and every stage's entry carries the prompt's
    log-probs and ranks; without it the keyword is not passed and the entries hold neither."""
    from asd_amd.serving.pipeline import AdaptiveSpeculativePipeline, PipelineConfig
    found = {}
    for value in (None, 2):
        cfg = PipelineConfig(lambda_value=100.0, stop_rule="full", stage_names=NAMES, prompt_logprobs=value)
        pipe = AdaptiveSpeculativePipeline(manager, LogprobPredictor(), object(), cfg)
        entries, calls = [], []
        allocate = pipe.cache_manager.allocate
        pipe.cache_manager.allocate = lambda rid, i, entry: (entries.append((i, entry)), allocate(rid, i, entry))[1]
        restore = []
        for name in manager.names:
            stage = manager.get_stage(name)

            def wrapped(*a, _orig=stage.generate, **kw):
                calls.append(kw)
                return _orig(*a, **kw)
            stage.generate = wrapped
            restore.append(stage)
        try:
            res = pipe.batch_process(PROMPTS, max_tokens=PL_MAX_TOKENS, temperature=0.0)
        finally:
            for stage in restore:
                del stage.generate
            pipe.shutdown()
        assert calls and entries and max(r.stages_run for r in res) > 1
        assert all(("prompt_logprobs" in kw) == (value is not None) for kw in calls)
        assert all(kw.get("prompt_logprobs", 2) == 2 for kw in calls)
        for i, entry in entries:
            assert ("prompt_logprobs" in entry) == ("prompt_ranks" in entry) == (value is not None)
            if value is not None:
                assert entry["prompt_logprobs"].dtype == np.float32 and entry["prompt_ranks"].dtype == np.int32
                assert entry["prompt_logprobs"].shape == entry["prompt_ranks"].shape and (entry["prompt_ranks"] >= 1).all()
        found[value] = [r.output for r in res]
    assert found[None] == found[2]                                       # the outputs do not depend on it
    return found


__all__ = ["AllCalls", "KEYS", "PL_MAX_TOKENS", "PromptOracleOps", "TABLE_KEYS", "VOCAB", "check_stats", "check_values",
           "ref_prompt_logprobs", "scenario_call_trace", "scenario_composition", "scenario_pipeline", "scenario_same_bits",
           "scenario_values"]
