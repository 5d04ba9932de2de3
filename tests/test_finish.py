"""Per-request max_tokens and multi-token stop sequences in Stage.generate and the pipeline, on CPU tensors with the ops twin of
tests/finish_scenario.py: a run returns every row of the free run up to and including the first position at which one of the
row's own stop sequences is complete in the GENERATED tokens -- wherever the step boundaries fall -- or up to the row's own
limit, says why and by which sequence each row ended, and without the new arguments makes the calls it made before."""
import numpy as np
import pytest

import asd_amd
from asd_amd.serving.pipeline import AdaptiveSpeculativePipeline, PipelineConfig
from asd_amd.serving.stages import StageManager
from tests.finish_scenario import (KINDS, FinishOracleOps, assert_finish_prefix, check_combined, check_greedy,
                                   expected_with_sequences, match_kind, pick_stop_sequences, step_of)
from tests.oracle_backend import OracleBackend
from tests.philox_ref import PhiloxOracleOps
from tests.stage_scenario import MAX_TOKENS, NAMES, PROMPTS, TEMPERATURE, stage_configs
from tests.stop_scenario import free_run

B = len(PROMPTS)
LIMITS = [1, 12, 5, 12, 7]


class FullOracleOps(PhiloxOracleOps, FinishOracleOps):
    """Every op of the stage loops (stop / greedy / top-N / seeded) + commit_step_finish."""


@pytest.fixture(autouse=True)
def oracle_backend():
    asd_amd.set_backend(OracleBackend())
    yield
    asd_amd.set_backend(None)


def fresh_manager(ops=None, **kw):
    return StageManager(stage_configs(**kw), ops=FinishOracleOps() if ops is None else ops)


def run(stage, **kw):
    kw.setdefault("max_tokens", MAX_TOKENS)
    return stage.generate(prompts=PROMPTS, temperature=TEMPERATURE, **kw)


@pytest.fixture(scope="module")
def free():
    """The free run of every stage: each on its first generate call of one manager (the seeds of `stage_configs`)."""
    asd_amd.set_backend(OracleBackend())
    sm = fresh_manager()
    out = {n: free_run(sm.get_stage(n)) for n in NAMES}
    assert sm.ops.calls["commit_step_finish"] == 0 and sm.ops.calls["commit_step_stop"] == 0 and sm.ops.calls["commit_step_lp"] > 0
    return out


def bigram_positions(fr, want):
    """(row, i): the bigram ending at generated token i of row `row` is committed in the way `want`."""
    return [(r, i) for r, kinds in enumerate(fr["kinds"]) for i in range(1, len(kinds)) if match_kind(kinds, i, 2) == want]


# ------------------------------------------------------------------------------------------ the prefix property
def test_stop_sequences_return_the_free_runs_prefix(free):
    sm = fresh_manager()
    seen = set()
    for name in NAMES:
        seqs = pick_stop_sequences(free[name])
        assert 1 <= len(seqs) <= 8 and all(2 <= len(s) <= 3 for s in seqs)
        before = (sm.ops.calls["commit_step_lp"], sm.ops.calls["commit_step_stop"])
        texts, lps, stats = run(sm.get_stage(name), stop_sequences=[list(s) for s in seqs])
        want = assert_finish_prefix(free[name], [seqs] * B, texts, lps, stats)
        assert (sm.ops.calls["commit_step_lp"], sm.ops.calls["commit_step_stop"]) == before
        assert stats["steps"] <= free[name]["stats"]["steps"]
        seen |= {kind for _, _, _, kind in want}
    assert sm.ops.calls["commit_step_finish"] > 0
    # over the three stages: a match inside one step that ends on an accepted token, one that ends on the drawn token of a step
    # with n_acc >= 1, one that straddles two steps, and a row that runs to its limit
    assert seen >= set(KINDS) | {None}, seen


def test_the_scenario_offers_every_kind_of_match(free):
    assert all(bigram_positions(free["13b"], k) for k in KINDS)
    assert bigram_positions(free["8b"], "straddle") and not bigram_positions(free["8b"], "accepted")


def test_the_configs_stop_sequences_are_the_default_and_strings_are_encoded(free):
    seqs = pick_stop_sequences(free["13b"])
    sm = fresh_manager(stop_sequences=tuple(seqs))
    texts, lps, stats = run(sm.get_stage("13b"))
    assert_finish_prefix(free["13b"], [seqs] * B, texts, lps, stats)
    assert "stop" in stats["finish_reasons"]
    # the argument replaces the configuration's; an empty one turns it off
    texts, lps, stats = run(fresh_manager(stop_sequences=tuple(seqs)).get_stage("13b"), stop_sequences=[])
    assert_finish_prefix(free["13b"], [[]] * B, texts, lps, stats)
    # a string is encoded by the stage's tokenizer and folded into the vocabulary like a prompt
    stage = fresh_manager().get_stage("8b")
    ids = [int(i) for i in stage.encode_prompts(["hard one"])[0]]
    assert len(ids) == 2
    row = free["8b"]["tokens"][0]
    texts, lps, stats = run(stage, stop_sequences=["hard one", row[3:5]])
    want = assert_finish_prefix(free["8b"], [[tuple(ids), tuple(row[3:5])]] * B, texts, lps, stats)
    assert want[0][1] == "stop"


# ------------------------------------------------------------------------------------------ traps
def test_a_last_token_that_never_follows_the_first_does_not_stop(free):
    for name in NAMES:
        fr = free[name]
        rows = []
        for toks in fr["tokens"]:
            t = toks[5]
            x = next(x for x in toks if all(not (a == x and b == t) for a, b in zip(toks, toks[1:])))
            rows.append([(x, t), (x, x, t)])
        texts, lps, stats = run(fresh_manager().get_stage(name), stop_sequences_per_prompt=rows)
        assert_finish_prefix(fr, rows, texts, lps, stats)
        assert stats["finish_reasons"] == ["length"] * B and stats["stop_matches"] == [None] * B


def test_a_match_never_begins_in_the_prompt(free):
    for name in NAMES:
        sm = fresh_manager()
        stage = sm.get_stage(name)
        last = [int(i) for i in stage.encode_prompts(PROMPTS)[:, -1]]
        fr = free[name]
        rows = [[(last[b], fr["tokens"][b][0])] for b in range(B)]
        for b in range(B):                                    # (the bigram must not ALSO occur inside the generated tokens)
            assert rows[b][0] not in set(zip(fr["tokens"][b], fr["tokens"][b][1:]))
        texts, lps, stats = run(stage, stop_sequences_per_prompt=rows)
        assert_finish_prefix(fr, rows, texts, lps, stats)
        assert stats["finish_reasons"] == ["length"] * B and sm.ops.calls["commit_step_finish"] > 0


def test_a_match_whose_last_token_the_limit_cuts_off_ends_with_length(free):
    cut_inside_a_step = 0
    for name in NAMES:
        fr = free[name]
        rows, limits = [], []
        for toks, kinds in zip(fr["tokens"], fr["kinds"]):
            steps = step_of(kinds)
            # prefer a position whose predecessor was committed by the same step: the limit then cuts inside a step's append
            cands = [i for i in range(2, MAX_TOKENS) if tuple(toks[i - 1:i + 1]) not in set(zip(toks[:i], toks[1:i]))]
            inside = [i for i in cands if steps[i] == steps[i - 1]]
            i = (inside or cands)[0]
            cut_inside_a_step += bool(inside)
            rows.append([tuple(toks[i - 1:i + 1])])
            limits.append(i)                                  # token i, the match's last, is the first one cut off
        texts, lps, stats = run(fresh_manager().get_stage(name), max_tokens=limits, stop_sequences_per_prompt=rows)
        assert_finish_prefix(fr, rows, texts, lps, stats, limits)
        assert stats["finish_reasons"] == ["length"] * B and stats["n_tokens"] == limits
    assert cut_inside_a_step >= 1


# ------------------------------------------------------------------------------------------ per-row limits and lists
def test_every_row_keeps_its_own_max_tokens(free):
    for name in NAMES:
        sm = fresh_manager()
        texts, lps, stats = run(sm.get_stage(name), max_tokens=LIMITS)
        assert_finish_prefix(free[name], [[]] * B, texts, lps, stats, LIMITS)
        assert stats["n_tokens"] == LIMITS and stats["finish_reasons"] == ["length"] * B
        assert sm.ops.calls["commit_step_finish"] > 0 and sm.ops.calls["commit_step_lp"] == 0
        # a numpy array is a sequence too
        texts2, _, stats2 = run(fresh_manager().get_stage(name), max_tokens=np.array(LIMITS))
        assert stats2["n_tokens"] == LIMITS


def shared_sequence(fr):
    """(owner row, other row, sequence): the longest-first sequence of 2 or 1 tokens that occurs in two rows' outputs."""
    for m in (2, 1):
        for r, toks in enumerate(fr["tokens"]):
            for i in range(m - 1, len(toks)):
                s = tuple(toks[i - m + 1:i + 1])
                for o, other in enumerate(fr["tokens"]):
                    if o != r and any(tuple(other[k - m + 1:k + 1]) == s for k in range(m - 1, len(other))):
                        return r, o, s
    return None


def test_a_rows_own_list_stops_that_row_only(free):
    found = 0
    for name in NAMES:
        hit = shared_sequence(free[name])
        if hit is None:
            continue
        found += 1
        r, o, s = hit
        rows = [[s] if b == r else [] for b in range(B)]
        texts, lps, stats = run(fresh_manager().get_stage(name), stop_sequences_per_prompt=rows)
        want = assert_finish_prefix(free[name], rows, texts, lps, stats)
        assert want[r][1] == "stop" and stats["stop_matches"][r] == s
        assert all(w[1] == "length" for b, w in enumerate(want) if b != r)
        # owned by every row it stops the other row too
        assert expected_with_sequences(free[name], [[s]] * B)[o][1] == "stop"
    assert found >= 1, "no stage's free run repeats a token across rows"


def test_stop_ids_come_first_in_a_rows_list(free):
    """A row's list is its stop ids, then the common sequences, then its own: where a stop id and a sequence end on the same
    token, the stop id is the reported match."""
    fr = free["13b"]
    toks = fr["tokens"][1]
    i = next(i for i in range(1, MAX_TOKENS) if toks[i] not in toks[:i] and tuple(toks[i - 1:i + 1]) not in set(zip(toks, toks[1:i])))
    sid, seq = toks[i], tuple(toks[i - 1:i + 1])
    rows = [[seq] if b == 1 else [] for b in range(B)]
    texts, lps, stats = run(fresh_manager().get_stage("13b"), stop_token_ids=[sid], stop_sequences_per_prompt=rows)
    assert stats["n_tokens"][1] == i + 1 and stats["stop_matches"][1] == (sid,) and stats["finish_reasons"][1] == "stop"


# ------------------------------------------------------------------------------------------ combined with the other arguments
def test_with_top_logprobs_and_per_prompt_seeds_everything_is_ragged_alike():
    for name in NAMES[1:]:
        ops = FullOracleOps()
        check_combined(fresh_manager(ops).get_stage(name))
        names = ops.names()
        assert ops.calls["commit_step_finish"] > 0 and "step_uniforms" in names and "commit_top_logprobs" in names
        # the seeded free run inside made the parent's commits, the cut run none of them
        first_finish = next(i for i, e in enumerate(ops.log) if e["name"] == "commit_top_logprobs")
        assert ops.calls["commit_step_stop"] == 0 and "commit_step_lp" in names[:first_finish + 1]


def test_greedy_decoding_has_the_same_prefix_property():
    for name in NAMES:
        ops = FullOracleOps()
        check_greedy(fresh_manager(ops).get_stage(name), LIMITS[::-1])
        assert ops.calls["commit_step_finish"] > 0 and "verify_greedy" in ops.names()


# ------------------------------------------------------------------------------------------ the route
@pytest.mark.parametrize("how", ["nothing", "equal_limits", "empty_lists", "stop_ids_only"])
def test_with_nothing_new_asked_for_the_parents_calls_are_made(free, how):
    sm = fresh_manager()
    kw = {"nothing": {}, "equal_limits": dict(max_tokens=[MAX_TOKENS] * B),
          "empty_lists": dict(stop_sequences=[], stop_sequences_per_prompt=[[] for _ in range(B)]),
          "stop_ids_only": dict(stop_token_ids=[free["8b"]["tokens"][1][2]])}[how]
    for name in NAMES:
        texts, lps, stats = run(sm.get_stage(name), **kw)
        if how != "stop_ids_only":
            assert_finish_prefix(free[name], [[]] * B, texts, lps, stats)
            assert stats["steps"] == free[name]["stats"]["steps"]
        else:
            assert_finish_prefix(free[name], [[(kw["stop_token_ids"][0],)]] * B, texts, lps, stats)
    assert sm.ops.calls["commit_step_finish"] == 0
    if how == "stop_ids_only":
        assert sm.ops.calls["commit_step_stop"] > 0 and sm.ops.calls["commit_step_lp"] == 0
    else:
        assert sm.ops.calls["commit_step_lp"] > 0 and sm.ops.calls["commit_step_stop"] == 0


BAD = [dict(max_tokens=[1, 2]), dict(max_tokens=[1, 2, 3, 4, 0]), dict(max_tokens=[1, 2, 3, 4, -5]), dict(max_tokens=[1, 2, 3, 4, 2.0]),
       dict(max_tokens=[1, 2, 3, 4, True]), dict(max_tokens=4.0), dict(max_tokens="4"), dict(max_tokens=None), dict(max_tokens=True),
       dict(max_tokens=[[1, 2, 3, 4, 5]]),
       dict(stop_sequences=[[]]), dict(stop_sequences=[""]), dict(stop_sequences=[list(range(9))]), dict(stop_sequences=[[1000]]),
       dict(stop_sequences=[[-1, 2]]), dict(stop_sequences=[[1, 2], [1, 2]]), dict(stop_sequences=[[1.0, 2]]),
       dict(stop_sequences="ab"), dict(stop_sequences=[5]), dict(stop_sequences=["a b c d e f g h i"]),
       dict(stop_sequences=[[i, i + 1] for i in range(17)]),
       dict(stop_sequences=[[i, i + 1] for i in range(10)], stop_token_ids=list(range(7))),
       dict(stop_sequences=[[3]], stop_token_ids=[3]),
       dict(stop_sequences_per_prompt=[[[1, 2]]]), dict(stop_sequences_per_prompt=[[[1, 2]], [], [], [], [[]]]),
       dict(stop_sequences_per_prompt=[[], [], [], [], [[5, 6], [5, 6]]]),
       dict(stop_sequences=[[5, 6]], stop_sequences_per_prompt=[[], [], [[5, 6]], [], []]),
       dict(stop_sequences=[[i, i + 1] for i in range(16)], stop_sequences_per_prompt=[[], [], [], [[900]], []])]


@pytest.mark.parametrize("bad", BAD, ids=[str(i) for i in range(len(BAD))])
def test_bad_arguments_raise_before_any_ops_call(bad):
    sm = fresh_manager()
    for name in NAMES[:2]:
        kw = dict(dict(max_tokens=4), **bad)
        with pytest.raises(ValueError):
            sm.get_stage(name).generate(prompts=PROMPTS, temperature=TEMPERATURE, **kw)
        with pytest.raises(ValueError):
            sm.get_stage(name).generate(prompts=PROMPTS, temperature=0.0, **kw)
    assert not sm.ops.calls
    if set(bad) == {"stop_sequences"}:                        # ... and from the configuration
        with pytest.raises(ValueError):
            fresh_manager(stop_sequences=bad["stop_sequences"]).get_stage("8b").generate(prompts=PROMPTS, max_tokens=4)


def test_sixteen_entries_are_accepted(free):
    row = free["13b"]["tokens"][0]
    seqs = [tuple(row[6:8])] + [(990 - i, 991 - i) for i in range(8)]
    rows = [[(900 + b, 7 * i + 1, 3) for i in range(4)] for b in range(B)]
    texts, lps, stats = run(fresh_manager().get_stage("13b"), stop_token_ids=[997, 998, 999], stop_sequences=seqs,
                            stop_sequences_per_prompt=rows)
    full = [[(997,), (998,), (999,)] + seqs + r for r in rows]
    assert all(len(r) == 16 for r in full)
    want = assert_finish_prefix(free["13b"], full, texts, lps, stats)
    assert want[0][1] == "stop" and want[0][0] <= 8


# ------------------------------------------------------------------------------------------ the pipeline
class LimitRecordingStage:
    """The pipeline's stage duck type: logs every call and answers with max_tokens[i] tokens per row."""

    def __init__(self, name, cost):
        self.name, self.cost_per_token, self.calls = name, cost, []

    def generate(self, prompts, max_tokens, temperature, return_logprobs=True, **kw):
        self.calls.append(dict(prompts=list(prompts), max_tokens=max_tokens, kw=dict(kw)))
        limits = max_tokens if isinstance(max_tokens, list) else [max_tokens] * len(prompts)
        return ([" ".join(["t1"] * n) for n in limits], [np.full(n, -0.1, np.float32) for n in limits],
                {"generation_time_ms": 1.0})


class LimitRecordingManager:
    def __init__(self, names=("8b", "13b", "34b", "70b"), costs=(1.0, 1.6, 4.2, 8.8)):
        self.stages = {n: LimitRecordingStage(n, c) for n, c in zip(names, costs)}

    def get_stage(self, name):
        return self.stages[name]


class WordPredictor:
    def predict(self, prompt, draft_output, draft_logprobs, stage_id, feature_extractor):
        return min(0.99, {"easy": 0.97, "mid": 0.6, "hard": 0.05}.get(prompt.split()[0], 0.5) + 0.2 * stage_id)


@pytest.mark.parametrize("grouping", ["predicted_stage", "none"])
def test_pipeline_delivers_each_request_its_own_max_tokens(grouping):
    prompts = ["easy a", "hard a", "mid a", "hard b", "easy b", "mid b", "hard c"]
    limits = [3, 9, 1, 4, 7, 2, 5]
    sm = LimitRecordingManager()
    pipe = AdaptiveSpeculativePipeline(sm, WordPredictor(), object(),
                                       PipelineConfig(lambda_value=30.0, stop_rule="full", risk_adjustment=False,
                                                      batch_grouping=grouping))
    if grouping == "predicted_stage":
        assert len(set(pipe.predict_stop_stages(prompts).tolist())) >= 2        # the population really splits
    res = pipe.batch_process(prompts, max_tokens=limits)
    assert [len(r.output.split()) for r in res] == limits
    seen = 0
    for stage in sm.stages.values():
        for call in stage.calls:
            assert call["kw"] == {} and isinstance(call["max_tokens"], list) and len(call["max_tokens"]) == len(call["prompts"])
            for p, n in zip(call["prompts"], call["max_tokens"]):
                owner = [i for i, orig in enumerate(prompts) if p == orig or p.startswith(orig + " ")]
                assert len(owner) == 1 and n == limits[owner[0]], (p, n)
                seen += 1
    assert seen == sum(r.stages_run for r in res) > len(prompts)             # later stages saw subsets
    # an int reaches the stages as the int it was, with no new keyword
    for st in sm.stages.values():
        st.calls.clear()
    pipe.batch_process(prompts[:3], max_tokens=4)
    assert sm.stages["8b"].calls and all(c["max_tokens"] == 4 and c["kw"] == {} for st in sm.stages.values() for c in st.calls)
    n = len(sm.stages["8b"].calls)
    for bad in ([1, 2], [1, 0, 3], [1, 2.0, 3], 2.5, "3", [1, True, 3]):
        with pytest.raises(ValueError, match="max_tokens"):
            pipe.batch_process(prompts[:3], max_tokens=bad)
    assert len(sm.stages["8b"].calls) == n
    pipe.shutdown()


def test_pipeline_config_stop_sequences_reach_every_call_and_come_from_yaml(tmp_path):
    sm = LimitRecordingManager()
    seqs = ("the end", (5, 6, 7))
    pipe = AdaptiveSpeculativePipeline(sm, WordPredictor(), object(),
                                       PipelineConfig(lambda_value=30.0, risk_adjustment=False, stop_sequences=seqs))
    pipe.batch_process(["hard a", "easy a"], max_tokens=[2, 3])
    pipe.shutdown()
    calls = [c for st in sm.stages.values() for c in st.calls]
    assert len(calls) >= 2 and all(c["kw"] == {"stop_sequences": list(seqs)} for c in calls)
    assert PipelineConfig().stop_sequences is None
    path = tmp_path / "serving.yaml"
    path.write_text("pipeline:\n  lambda_value: 2.0\n  stop_sequences:\n    - \"the end\"\n    - [5, 6, 7]\n")
    assert PipelineConfig.from_yaml(str(path)).stop_sequences == seqs
    path.write_text("pipeline:\n  lambda_value: 2.0\n")
    assert PipelineConfig.from_yaml(str(path)).stop_sequences is None


def test_pipeline_on_real_stages_keeps_every_limit(free):
    ops = FinishOracleOps()
    sm = StageManager(stage_configs(), ops=ops)
    from tests.stage_scenario import LogprobPredictor
    pipe = AdaptiveSpeculativePipeline(sm, LogprobPredictor(), object(),
                                       PipelineConfig(lambda_value=30.0, stop_rule="full", stage_names=NAMES))
    res = pipe.batch_process(PROMPTS, max_tokens=LIMITS, temperature=TEMPERATURE)
    pipe.shutdown()
    assert [len(r.output.split()) for r in res] == LIMITS
    assert ops.calls["commit_step_finish"] > 0
