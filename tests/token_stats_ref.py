"""token_stats (serving/stages.py, TOKEN STATS; include/asd_hip.h, asd_token_stats): the numpy f64 reference of the kernel, written
from the header's text, the oracle ops twin that scores through it, and the stage-level scenarios that
tests/test_token_stats_stages.py (CPU twin) and tests/test_gpu_token_stats_stages.py (HipOps) both run on
stage_configs(vocab=64).

TEST INFRASTRUCTURE, like tests/prompt_logprobs_ref.py: never importable from the package."""
import numpy as np
import torch

from tests.logit_edit_ref import SEEDS, run_kept
from tests.per_request_ref import inv_t_of
from tests.prompt_logprobs_ref import AllCalls, PromptOracleOps
from tests.stage_scenario import MAX_TOKENS, NAMES, PROMPTS, TEMPERATURE, LogprobPredictor, text_ids
from tests.top_logprobs_ref import LP_ATOL, ref_top_logprobs, step_rows

VOCAB = 64                                       # the stages of the scenarios: stage_configs(vocab=VOCAB)
H_ATOL, H_RTOL = 1e-4, 1e-5                      # the entropy's bar: tests/test_gpu_verify.py holds the verify kernel's to it
KEYS = ("token_entropy", "token_max_logprobs", "token_argmax_ids", "token_ranks", "predictor_features")
ROW_TEMPERATURES = [0.7, 1.0, 0.5, 1.3, 0.7]


def ref_entropy(row, a):
    """H = -sum p ln p in nats of softmax(row * a), f64.  A -inf element carries no mass; no finite element, or a NaN: NaN."""
    z = np.asarray(row, dtype=np.float32).astype(np.float64) * a
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if np.isnan(z).any() or not np.isfinite(z.max()):
            return np.nan
        e = np.exp(z - z.max())
        p = e / e.sum()
        keep = p > 0
        return float(-(p[keep] * np.log(p[keep])).sum())


def ref_token_stats(x, tok, n_acc, drawn, n=0, inv_t=1.0):
    """asd_token_stats in numpy f64.  x: [B, K1, V] f32 (the stored values, upcast: exact); tok: int [B, K1 - 1] or None (K1 == 1);
    n_acc, drawn: B ints; inv_t: one number, or B of them (inv_t_rows) -> (stat_id int32 [B,K1,2] (rank, arg-max id), stat_val f64
    [B,K1,2] (entropy, max log-prob), top_id int32 [B,K1,n], top_lp f64 [B,K1,n]).  With a = clamp(n_acc[b], 0, K1 - 1) row j is
    live while j <= a and scores g = tok[b, j] (j < a) or drawn[b] (j == a): rank = 1 + #{v: x[v] > x[g], or x[v] == x[g] and
    v < g}, 0 for g outside [0, V) or a NaN x[g]; arg-max and table: ref_top_logprobs'; entropy: ref_entropy.  Other rows are
    neutral: rank 0, id -1, 0.0, 0.0, table (-1, -inf)."""
    x = np.asarray(x, dtype=np.float32)
    B, K1, V = x.shape
    inv = [float(inv_t)] * B if np.ndim(inv_t) == 0 else [float(v) for v in inv_t]
    stat_id = np.zeros((B, K1, 2), np.int32)
    stat_id[..., 1] = -1
    stat_val = np.zeros((B, K1, 2), np.float64)
    top_id = np.full((B, K1, n), -1, np.int32)
    top_lp = np.full((B, K1, n), -np.inf, np.float64)
    idx = np.arange(V)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for b in range(B):
            a = min(max(int(n_acc[b]), 0), K1 - 1)
            t_id, t_lp = ref_top_logprobs(x[b, :a + 1], max(n, 1), inv[b])
            for j in range(a + 1):
                row, g = x[b, j], int(tok[b][j]) if j < a else int(drawn[b])
                if 0 <= g < V and not np.isnan(row[g]):
                    stat_id[b, j, 0] = 1 + int(np.count_nonzero((row > row[g]) | ((row == row[g]) & (idx < g))))
                stat_id[b, j, 1], stat_val[b, j, 1] = t_id[j, 0], t_lp[j, 0]
                stat_val[b, j, 0] = ref_entropy(row, float(np.float32(inv[b])))
                top_id[b, j], top_lp[b, j] = t_id[j, :n], t_lp[j, :n]
    return stat_id, stat_val, top_id, top_lp


def same_values(got, want, atol, rtol, what):
    """NaN and infinite positions exactly; finite ones within atol + rtol |want| -> the largest finite error."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, got, want)
    fin = np.isfinite(want)
    assert np.array_equal(got[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)]), what
    err = np.abs(got[fin] - want[fin])
    assert (err <= atol + rtol * np.abs(want[fin])).all(), (what, float(err.max()))
    return float(err.max()) if fin.any() else 0.0


def check_kernel_outputs(got, want, V, what, live=None):
    """(stat_id, stat_val, top_id | None, top_lp | None) of a launch against ref_token_stats': ranks and ids exact on every row,
    log-probs within LP_ATOL, the entropy within H_ATOL + H_RTOL |H| and inside [-1e-5, ln V + 1e-4]."""
    stat_id, stat_val, top_id, top_lp = [None if t is None else np.asarray(t) for t in got]
    assert stat_id.dtype == np.int32 and stat_val.dtype == np.float32
    assert np.array_equal(stat_id, want[0]), (what, np.argwhere(stat_id != want[0])[:5])
    same_values(stat_val[..., 1], want[1][..., 1], LP_ATOL, 0.0, (what, "max lp"))
    same_values(stat_val[..., 0], want[1][..., 0], H_ATOL, H_RTOL, (what, "entropy"))
    h = stat_val[..., 0][~np.isnan(stat_val[..., 0])]
    assert (h >= -1e-5).all() and (h <= np.log(V) + 1e-4).all(), what
    if top_id is not None:
        n = top_id.shape[-1]
        assert top_id.dtype == np.int32 and top_lp.dtype == np.float32
        assert np.array_equal(top_id, want[2][..., :n]), what
        same_values(top_lp, want[3][..., :n], LP_ATOL, 0.0, (what, "table"))


class TokenStatsOracleOps(PromptOracleOps):
    """PromptOracleOps + token_stats on the reference above: the tiny stages run without a GPU."""

    def token_stats(self, logits, tok, n_acc, drawn, n=0, inv_temperature=1.0, rows=None, splits=0):
        self._note("token_stats", ())
        x = logits.float().numpy()
        x = x[:, None] if x.ndim == 2 else x
        assert (tok is None) == (x.shape[1] == 1) and n_acc.dtype == torch.int32 and drawn.dtype == torch.int32
        assert tok is None or (tok.dtype == torch.int32 and tuple(tok.shape) == (x.shape[0], x.shape[1] - 1))
        stat_id, stat_val, top_id, top_lp = ref_token_stats(x, None if tok is None else tok.numpy(), n_acc.tolist(), drawn.tolist(), n,
                                                            inv_temperature if rows is None else rows.inv_t)
        f32 = lambda v: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32))   # noqa: E731
        return torch.from_numpy(stat_id), f32(stat_val), (torch.from_numpy(top_id) if n else None), (f32(top_lp) if n else None)


# ------------------------------------------------------------------------------------------ stage-level scenarios
def _bits(arrays):
    return [np.asarray(a).tobytes() for a in arrays]


def _cpu(s):
    return {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in s.items()}


def check_stage_stats(stage, texts, stats, inv_t, n=0, prompts=PROMPTS):
    """From the kept steps: every step's figures are the reference's on the kept rows (ranks and ids exact on every row, the
    rest within the kernel tolerances), the entries appended per sequence are the step's first n_commit rows, bit for bit, n_i
    entries per row with the right dtypes, the arg-max pair is table slot 0 with its bits, rank <= n finds the token in slot
    rank - 1, and predictor_features is extract_device on the returned arrays."""
    from asd_amd.serving.components import FeatureExtractor
    B, V = len(texts), stage.shape.vocab
    assert stage.step_inputs and all(k in stats for k in KEYS)
    want = [[[], []] for _ in range(B)]
    for s in stage.step_inputs:
        c = _cpu(s)
        x = step_rows(c)
        tok = c["tok"].numpy() if c.get("tok") is not None else None
        ref = ref_token_stats(x, tok, c["n_acc"].tolist(), c["drawn"].tolist(), n, inv_t)
        got = (c["stat_id"].numpy(), c["stat_val"].numpy(), c["top_id"].numpy() if n else None, c["top_lp"].numpy() if n else None)
        assert got[0].shape == (B, x.shape[1], 2)
        check_kernel_outputs(got, ref, V, "step")
        if n:                                                            # slot 0 carries the arg-max pair's bits on live rows
            live = got[0][..., 1] >= 0
            assert np.array_equal(got[2][..., 0][live], got[0][..., 1][live])
            assert got[3][..., 0][live].tobytes() == got[1][..., 1][live].tobytes()
        nc = c["n_commit"].numpy()
        for b in range(B):
            assert 0 <= nc[b] <= min(max(int(c["n_acc"][b]), 0), x.shape[1] - 1) + 1
            for j in range(int(nc[b])):
                want[b][0].append(got[0][b, j])
                want[b][1].append(got[1][b, j])
    for b in range(B):
        toks = text_ids(texts[b])
        n_b = len(toks)
        assert stats["n_tokens"][b] == n_b
        ids = np.array(want[b][0], np.int32).reshape(-1, 2)
        vals = np.array(want[b][1], np.float32).reshape(-1, 2)
        for key, dtype, ref in (("token_entropy", np.float32, vals[:, 0]), ("token_max_logprobs", np.float32, vals[:, 1]),
                                ("token_argmax_ids", np.int32, ids[:, 1]), ("token_ranks", np.int32, ids[:, 0])):
            got = stats[key][b]
            assert got.shape == (n_b,) and got.dtype == dtype, (key, b)
            assert got.tobytes() == np.ascontiguousarray(ref).tobytes(), (key, b)
        assert (stats["token_ranks"][b] >= 1).all() and np.isfinite(stats["token_entropy"][b]).all()
        if n:
            for i, t in enumerate(toks):
                r = int(stats["token_ranks"][b][i])
                row = stats["top_token_ids"][b][i].tolist()
                assert (row[r - 1] == t) if r <= n else (t not in row), (b, i)
                assert row[0] == stats["token_argmax_ids"][b][i]
                assert stats["top_logprobs"][b][i][0].tobytes() == stats["token_max_logprobs"][b][i].tobytes()
    # the feature batch from the returned arrays
    T = max(max(stats["n_tokens"]), 1)
    pad = lambda key: torch.from_numpy(np.stack([np.pad(a, (0, T - len(a))) for a in stats[key]]))      # noqa: E731
    feats = FeatureExtractor.extract_device(pad("token_max_logprobs"), pad("token_entropy"), [len(p.split()) for p in prompts],
                                            [float(v) for v in stats["n_tokens"]], stage.index,
                                            n_valid=torch.tensor(stats["n_tokens"]))
    got = stats["predictor_features"]
    assert got.shape == (B, 256) and got.dtype == np.float32
    assert np.allclose(got, feats.numpy(), rtol=1e-6, atol=1e-6)
    assert (got[:, 5:] == 0).all() and (got[:, 0] > 0).any()


def scenario_values(stage, temperature=TEMPERATURE, n=0, **kw):
    """Scenario (a): values, shapes, dtypes and the feature batch on a seeded call; off: none of the keys."""
    texts, _, stats = run_kept(stage, prompts=PROMPTS, max_tokens=MAX_TOKENS, temperature=temperature, seed=SEEDS, token_stats=True,
                               logprobs=n, **kw)
    inv_t = 1.0 if np.ndim(temperature) == 0 and temperature == 0.0 else \
        [inv_t_of(t) for t in temperature] if np.ndim(temperature) else inv_t_of(temperature)
    check_stage_stats(stage, texts, stats, inv_t, n)
    assert stage.generate(prompts=PROMPTS, max_tokens=2, temperature=0.0)[2].keys().isdisjoint(KEYS)
    return texts, stats


def scenario_greedy(stage):
    """Greedy rows have rank 1 and are the arg-max."""
    texts, stats = scenario_values(stage, temperature=0.0, n=2)
    for b, text in enumerate(texts):
        assert (stats["token_ranks"][b] == 1).all() and stats["token_argmax_ids"][b].tolist() == text_ids(text)


def scenario_sampled_ranks(stage):
    """A sampled call at a high temperature commits tokens that are not the arg-max: ranks above 1 occur."""
    texts, _, stats = run_kept(stage, prompts=PROMPTS, max_tokens=MAX_TOKENS, temperature=1.5, seed=SEEDS, token_stats=True, logprobs=3)
    check_stage_stats(stage, texts, stats, inv_t_of(1.5), 3)
    assert max(int(r.max()) for r in stats["token_ranks"]) > 1


def scenario_same_bits(stage, temperature=TEMPERATURE):
    """The same seeded call with and without token_stats returns bit-equal texts, log-probs and top-N tables."""
    for n in (0, 2):
        kw = dict(prompts=PROMPTS, max_tokens=MAX_TOKENS, temperature=temperature, seed=SEEDS, logprobs=n)
        off = stage.generate(**kw)
        on = stage.generate(token_stats=True, **kw)
        assert on[0] == off[0] and _bits(on[1]) == _bits(off[1]) and on[2]["n_tokens"] == off[2]["n_tokens"]
        if n:
            assert _bits(on[2]["top_token_ids"]) == _bits(off[2]["top_token_ids"])
            assert _bits(on[2]["top_logprobs"]) == _bits(off[2]["top_logprobs"])
        assert all(k in on[2] for k in KEYS) and off[2].keys().isdisjoint(KEYS)


def scenario_call_trace(stage):
    """The ops calls with the feature on are those without it plus exactly one token_stats and one commit_top_logprobs per
    step; with logprobs = 3 token_stats stands where top_logprobs stood.  None and False make exactly the default call's."""
    found = {}
    for n in (0, 3):
        kw = dict(prompts=PROMPTS, max_tokens=4, temperature=TEMPERATURE, seed=SEEDS, logprobs=n)
        log = AllCalls(stage.ops)
        try:
            runs = []
            for extra in ({}, dict(token_stats=None), dict(token_stats=False), dict(token_stats=True)):
                del log.names[:]
                stage.generate(**extra, **kw)
                runs.append((list(log.names), stage.last_steps))
        finally:
            log.close()
        (off, steps), (none, _), (false, _), (on, steps_on) = runs
        assert off and none == off and false == off and "token_stats" not in off and steps_on == steps
        assert on.count("token_stats") == steps and "top_logprobs" not in on and "top_logprobs_rows" not in on
        assert on.count("commit_top_logprobs") == off.count("commit_top_logprobs") + steps
        assert off.count("top_logprobs") == (steps if n else 0)
        back = []
        for i, name in enumerate(on):                                    # undo the change: the default call's trace comes back
            if name == "token_stats":
                back += ["top_logprobs"] if n else []                    # (one for one where the table's call stood)
            elif name == "commit_top_logprobs" and (not n or on[i - 1] == "commit_top_logprobs"):
                pass                                                     # the added commit: directly behind the table's
            else:
                back.append(name)
        assert back == off, n
        found[n] = on
    return found


def scenario_rows_route(stage):
    """The rows route: every row's figures are those of a scalar call at that row's own temperature, bit for bit."""
    texts, stats = scenario_values(stage, temperature=ROW_TEMPERATURES, n=2)
    stage.keep_inputs = True
    try:
        stage.generate(prompts=PROMPTS, max_tokens=4, temperature=ROW_TEMPERATURES, seed=SEEDS, token_stats=True)
    finally:
        stage.keep_inputs = False
    steps = stage.step_inputs
    assert steps
    for s in steps[:2]:
        x = s["logits"] if "bonus" not in s else torch.cat([s["logits"], s["bonus"][:, None]], 1)
        for b, t in enumerate(ROW_TEMPERATURES):
            one = stage.ops.token_stats(x, s.get("tok"), s["n_acc"], s["drawn"], n=0, inv_temperature=inv_t_of(t))
            assert torch.equal(one[0][b], s["stat_id"][b])
            assert one[1][b].cpu().numpy().tobytes() == s["stat_val"][b].cpu().numpy().tobytes(), (b, t)


def scenario_stops(stage):
    """Stop ids and unequal max_tokens: rows end at different lengths and a finished row's entries stay as committed."""
    base = stage.generate(prompts=PROMPTS, max_tokens=MAX_TOKENS, temperature=0.0)
    limits = [MAX_TOKENS, 5, MAX_TOKENS, 7, 9]
    rows = [text_ids(t) for t in base[0]]

    def ends(stop):                                                      # greedy: the rerun commits the baseline's tokens
        return [min(lim, r.index(stop) + 1 if stop in r else lim) for r, lim in zip(rows, limits)]
    # a token of row 0 that ends rows at the most different lengths and leaves a row running to its limit
    stop = max(rows[0][1:6], key=lambda s: (any(s not in r[:lim] for r, lim in zip(rows, limits)), len(set(ends(s)))))
    want = ends(stop)
    assert len(set(want)) > 1 and any(stop not in r[:lim] for r, lim in zip(rows, limits))
    texts, _, stats = run_kept(stage, prompts=PROMPTS, max_tokens=limits, temperature=0.0, stop_token_ids=[stop], token_stats=True,
                               logprobs=1)
    assert stats["n_tokens"] == want and {"stop", "length"} <= set(stats["finish_reasons"])
    check_stage_stats(stage, texts, stats, 1.0, 1)


class FeaturePredictor(LogprobPredictor):
    """LogprobPredictor with the feature entry point: notes the rows it is handed."""

    def __init__(self):
        self.rows = []

    def predict_features(self, features):
        features = np.asarray(features)
        assert features.ndim == 2 and features.shape[1] == 256 and features.dtype == np.float32
        self.rows.extend(features)
        return np.clip(0.5 + 0.1 * features[:, 3], 0.01, 0.99)


def scenario_pipeline(manager):
    """PipelineConfig.token_stats reaches every stage call, every stage's entry carries the figures and the feature row, and a
    predictor with predict_features is fed that row; without it the keyword is not passed."""
    from asd_amd.serving.pipeline import AdaptiveSpeculativePipeline, PipelineConfig
    for value in (None, True):
        cfg = PipelineConfig(lambda_value=100.0, stop_rule="full", stage_names=NAMES, token_stats=value)
        predictor = FeaturePredictor()
        pipe = AdaptiveSpeculativePipeline(manager, predictor, object(), cfg)
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
            res = pipe.batch_process(PROMPTS, max_tokens=6, temperature=0.0)
        finally:
            for stage in restore:
                del stage.generate
            pipe.shutdown()
        assert calls and entries and len(res) == len(PROMPTS)
        assert all(("token_stats" in kw) == (value is not None) for kw in calls)
        assert bool(predictor.rows) == (value is not None)
        for i, entry in entries:
            for key in ("token_entropy", "token_max_logprobs", "token_ranks", "features"):
                assert (key in entry) == (value is not None), key
            if value is not None:
                n = len(entry["output"].split())
                assert entry["token_entropy"].shape == entry["token_max_logprobs"].shape == entry["token_ranks"].shape == (n,)
                assert entry["features"].shape == (256,) and entry["features"].dtype == np.float32
                assert entry["features"][4] == np.float32(i / 4.0)
        if value is not None:
            fed = {r.tobytes() for r in predictor.rows}
            assert {e["features"].tobytes() for i, e in entries if i < len(NAMES) - 1} <= fed


__all__ = ["FeaturePredictor", "H_ATOL", "H_RTOL", "KEYS", "ROW_TEMPERATURES", "TokenStatsOracleOps", "VOCAB", "check_kernel_outputs",
           "check_stage_stats", "ref_entropy", "ref_token_stats", "same_values", "scenario_call_trace", "scenario_greedy",
           "scenario_pipeline", "scenario_rows_route", "scenario_sampled_ranks", "scenario_same_bits", "scenario_stops",
           "scenario_values"]
