"""What Stage.generate RETURNS against the f64 teacher-forced reference of tests/teacher_forced_ref.py, on CPU: the three tiny
stages of tests/stage_scenario.py in float32 on the oracle twin of tests/prompt_logprobs_ref.py (every op a numpy reference), the
scenarios of tests/teacher_forced_scenarios.py that tests/test_gpu_teacher_forced_stages.py runs on the kernels, and the negative
controls: defects of the loop's plumbing that leave its own record self-consistent and that the check must see -- among them
the automaton's state columns, the n-gram rule's history and the prefill that prompt_logprobs scores.

The sharp check is the float32 one (eps_x about 4e-5, bounds about 1e-4: six orders below a plumbing defect); the bfloat16 stages
run the same formulas at eps_x about 0.5."""
import pytest
import torch

import asd_amd
from asd_amd.serving.stages import StageManager
from tests import teacher_forced_scenarios as S
from tests.logit_edit_ref import SEEDS, run_kept
from tests.oracle_backend import OracleBackend
from tests.penalty_ref import RECUR_BIAS
from tests.per_request_ref import MIXED, inv_t_of
from tests.prompt_logprobs_ref import PromptOracleOps
from tests.stage_scenario import MAX_TOKENS, NAMES, PROMPTS, TEMPERATURE, check_generation, stage_configs, text_ids
from tests.teacher_forced_ref import TeacherForcedError, check, run_checked

LP_BAR = 1e-6      # the twin's lp is the f64 value at its row rounded to f32 (tests/test_stages.py)
VERIFYING = NAMES[1:]


@pytest.fixture(autouse=True)
def oracle_backend():
    asd_amd.set_backend(OracleBackend())
    yield
    asd_amd.set_backend(None)


def _manager(dtype=torch.float32, draft_len=None, **kw):
    cfgs = stage_configs(dtype=dtype, **kw)
    for c in cfgs:
        c.draft_len = draft_len or c.draft_len
    return StageManager(cfgs, ops=PromptOracleOps())


@pytest.fixture(scope="module")
def manager():
    return _manager()


@pytest.fixture(scope="module")
def manager_bf16():
    return _manager(torch.bfloat16)


# ------------------------------------------------------------------------------------------ the scenarios
@pytest.mark.parametrize("seeded", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_defaults(manager, name, seeded):
    stage = manager.get_stage(name)
    rep = S.defaults(stage, LP_BAR, seeded)
    assert name == NAMES[0] or rep["ambiguous"] == 0                              # the untruncated target
    assert name != "13b" or stage.last_steps < MAX_TOKENS                         # its draft's weights are its own: blocks pass


@pytest.mark.parametrize("which", sorted(S.TARGET_TRUNCATION))
@pytest.mark.parametrize("name", VERIFYING)
def test_target_truncation(manager, name, which):
    S.target_truncation(manager.get_stage(name), LP_BAR, which)


@pytest.mark.parametrize("which", sorted(S.ROWS))
@pytest.mark.parametrize("name", NAMES)
def test_rows_route(manager, name, which):
    S.rows_route(manager.get_stage(name), LP_BAR, which)


@pytest.mark.parametrize("sync_every", [1, 4])
@pytest.mark.parametrize("name", NAMES)
def test_ragged_ends(manager, name, sync_every):
    S.ragged_ends(manager.get_stage(name), LP_BAR, sync_every)


@pytest.mark.parametrize("name", NAMES)
def test_everything_on(manager, name):
    S.everything(manager.get_stage(name), LP_BAR)


@pytest.mark.parametrize("name", NAMES)
def test_greedy_with_a_stop_id_and_penalties(manager, name):
    S.greedy(manager.get_stage(name), LP_BAR)


@pytest.mark.parametrize("name", NAMES)
def test_one_manager_calls_back_to_back(name):
    S.back_to_back(_manager().get_stage(name), LP_BAR)


# ---- the edges of the loop
@pytest.mark.parametrize("edge", sorted(S.EDGES))
def test_edges_of_the_loop(edge):
    S.edge(_manager, LP_BAR, edge)


@pytest.mark.parametrize("name", NAMES)
def test_bf16_defaults_and_everything_on(manager_bf16, name):
    """The production dtype under the same formulas: eps_x is near 0.5 and the bound correspondingly coarse; it shows that the
    casts of the bf16 path break nothing gross.  The sharp check is the float32 one above."""
    stage = manager_bf16.get_stage(name)
    S.bf16(stage, LP_BAR)


# ---- guided rows, n-gram bans, prompt log-probs
@pytest.fixture(scope="module")
def manager_v64():
    return _manager(vocab=S.NGRAM_VOCAB)


@pytest.mark.parametrize("name,how", S.guided_cases(NAMES))
def test_guided_rows(manager, name, how):
    S.guided(manager.get_stage(name), LP_BAR, how)


@pytest.mark.parametrize("greedy", [False, True], ids=["sampled", "greedy"])
def test_ngram_rows_with_live_bans(manager_v64, greedy):
    """All three stages in one test: the n = 3 row's live bans are counted over the scenario."""
    reps = [S.ngram(manager_v64.get_stage(name), LP_BAR, greedy) for name in NAMES]
    assert sum(rep["ngram_live"][2] for rep in reps) >= 1, [rep["ngram_live"] for rep in reps]


@pytest.mark.parametrize("name", NAMES)
def test_everything_now(manager, name):
    S.everything_now(manager.get_stage(name), LP_BAR)


@pytest.mark.parametrize("n,how", S.PROMPT_HOW)
@pytest.mark.parametrize("name", NAMES)
def test_prompt_logprobs(manager, name, n, how):
    S.prompt(manager.get_stage(name), LP_BAR, n, how)


@pytest.mark.parametrize("edge", sorted(S.EDGES))
def test_edges_of_the_loop_now(edge):
    S.edge_now(_manager, LP_BAR, edge)


@pytest.mark.parametrize("name", NAMES)
def test_one_manager_calls_back_to_back_now(name):
    S.back_to_back_now(_manager().get_stage(name), LP_BAR)


@pytest.mark.parametrize("name", NAMES)
def test_bf16_everything_now_and_prompt(manager_bf16, name):
    S.bf16_now(manager_bf16.get_stage(name), LP_BAR)


# ------------------------------------------------------------------------------------------ negative controls
# Each wraps the model or one op of the twin for ONE call of a scenario in which the defect is live.  The call itself must run
# (an exception in a wrapper is not a detection), the same call without the wrapper must pass, and the check must fail with
# its own error on a log-prob.
class patched:
    """Instance attributes over `obj`'s methods for the length of a with block: the object stays what it is."""

    def __init__(self, obj, **attrs):
        self.obj, self.attrs = obj, attrs

    def __enter__(self):
        for k, v in self.attrs.items():
            setattr(self.obj, k, v)

    def __exit__(self, *exc):
        for k in self.attrs:
            delattr(self.obj, k)


DIFF = r"\|diff\|"
DIFF_OR_REMOVED = r"\|diff\||is removed by the row's processors"      # a control whose defect may let a forbidden token through


def _control(stage, kw, patch, replay=None, match=DIFF, replay_stats=None, live=None):
    """The call passes unpatched and fails patched; replay(stage, texts, lps) / replay_stats(stage, stats): an existing check the
    patched run still passes; live(unpatched out, patched out): the defect demonstrably changed what was returned."""
    base, _ = run_checked(stage, LP_BAR, S.label(stage, "control, unpatched"), **kw)
    with patch:
        out = run_kept(stage, **kw)
    if replay is not None:
        replay(stage, out[0], out[1])
    if replay_stats is not None:
        replay_stats(stage, out[2])
    if live is not None:
        assert live(base, out)
    with pytest.raises(TeacherForcedError, match=match) as err:
        check(stage, kw, out, LP_BAR, S.label(stage, "control"))
    print(f"[control] {err.value}")
    return out


def _generated_differs(base, out):
    return base[0] != out[0] or any(a.tobytes() != b.tobytes() for a, b in zip(base[1], out[1]))


def _prompt_numbers_differ(base, out):
    return any(a.tobytes() != b.tobytes() for a, b in zip(base[2]["prompt_logprobs"], out[2]["prompt_logprobs"]))


def _seeded():
    return dict(S.KW, seed=SEEDS)


def _short_window(model, by=6):
    orig = model.forward_ragged
    return patched(model, forward_ragged=lambda ids, pos0, window, *a, **k: orig(ids, pos0, max(window - by, 1), *a, **k))


def _shifted_target_pass(stage):
    orig, T = stage.model.forward_ragged, stage.config.draft_len + 1
    return patched(stage.model, forward_ragged=lambda ids, pos0, *a, **k: orig(ids, pos0 + 1 if ids.shape[1] == T else pos0, *a, **k))


# "13b" shares its draft's weights, so its steps accept 0 .. 4 proposals and take bonus rows; "34b" and its draft are unrelated
# random models, whose steps accept next to nothing: a defect behind an ACCEPTED proposal is live on "13b" only.
@pytest.mark.parametrize("name", VERIFYING)
def test_control_target_window_six_short_passes_the_replay_and_fails_here(manager, name):
    stage = manager.get_stage(name)
    replay = lambda st, texts, lps: check_generation(st, texts, lps, inv_t_of(TEMPERATURE), atol=1e-6)       # noqa: E731
    _control(stage, _seeded(), _short_window(stage.model), replay)


@pytest.mark.parametrize("name", VERIFYING)
def test_control_target_pass_fed_one_position_late(manager, name):
    stage = manager.get_stage(name)
    _control(stage, _seeded(), _shifted_target_pass(stage))


def test_controls_fail_at_bf16_too(manager_bf16):
    """On "34b": at eps_x near 0.6 the bound is near 1.7, which the one-position shift exceeds at a few positions of 60 there
    (on "13b", whose draft is its own model, at one or none: not a control)."""
    stage = manager_bf16.get_stage("34b")
    _control(stage, _seeded(), _short_window(stage.model))
    _control(stage, _seeded(), _shifted_target_pass(stage))


def test_control_penalties_without_the_steps_proposals(manager):
    stage = manager.get_stage("13b")
    orig = stage.ops.penalty_rows
    kw = dict(_seeded(), logit_bias=RECUR_BIAS, **S.PENALTIES)
    _control(stage, kw, patched(stage.ops, penalty_rows=lambda logits, pen, step_tok=None, n_prev=0: orig(logits, pen, None, 0)))


def test_control_edit_without_the_position_inside_the_step(manager):
    """min_tokens live on a stop id that a bias makes likely.  Dropping `offset` from the DRAFT's calls alone cannot be seen in
    what is returned, and need not be: draft and verify then share a wrong proposal distribution, against which the chain is
    still lossless for the target's.  The control drops the position inside the step on every call, the target's rows too."""
    stage = manager.get_stage("13b")
    orig = stage.ops.logit_edit_rows

    def no_offset(logits, edits, seq_len, start, offset=0):
        for row in (logits.unbind(1) if logits.dim() == 3 else [logits]):
            orig(row, edits, seq_len, start, 0)
        return logits
    stop = text_ids(stage.generate(**_seeded())[0][0])[2]
    kw = dict(_seeded(), stop_token_ids=[stop], logit_bias={stop: 4.0}, min_tokens=[3, 6, 5, 4, 2])
    _control(stage, kw, patched(stage.ops, logit_edit_rows=no_offset))


@pytest.mark.parametrize("name", VERIFYING)
def test_control_bad_words_that_match_into_the_prompt(manager, name):
    stage = manager.get_stage(name)
    orig = stage.ops.bad_words_rows
    free = [text_ids(t) for t in stage.generate(**_seeded())[0]]
    words = [[(p[-1], g[0])] for p, g in zip(stage._encode(PROMPTS)[1], free)]     # the word's prefix ends the prompt
    kw = dict(_seeded(), bad_words_per_prompt=words)
    out = _control(stage, kw, patched(stage.ops, bad_words_rows=lambda lg, w, tokens, seq_len, start, cap, *a: orig(lg, w, tokens, seq_len, 0, cap, *a)))
    assert all(text_ids(t)[0] != g[0] for t, g in zip(out[0], free))              # the defect was live: the first token was banned


def test_control_commit_of_the_drafts_log_probs(manager):
    stage = manager.get_stage("13b")
    ops, seen = stage.ops, {}
    verify = ops.verify_accept

    def keep_lp_d(score, tok, lp_d, *a, **k):
        seen["lp_d"] = lp_d
        return verify(score, tok, lp_d, *a, **k)

    def swapped(name):
        orig = getattr(ops, name)
        return lambda tok, lp_tok, *a, **k: orig(tok, seen["lp_d"].clone(), *a, **k)
    free = text_ids(stage.generate(**_seeded())[0][0])
    for name, extra in (("commit_step_lp", {}), ("commit_step_stop", dict(stop_token_ids=[free[6]])),
                        ("commit_step_finish", dict(max_tokens=[12, 5, 9, 12, 7]))):
        _control(stage, dict(_seeded(), **extra), patched(ops, verify_accept=keep_lp_d, **{name: swapped(name)}))


@pytest.mark.parametrize("name", NAMES)
def test_control_another_rows_sampling_table(manager, name):
    stage = manager.get_stage(name)
    orig = stage.ops.pack_sampling_rows
    roll = lambda v: None if v is None else list(v[1:]) + list(v[:1])             # noqa: E731
    _control(stage, dict(_seeded(), **MIXED),
             patched(stage.ops, pack_sampling_rows=lambda inv_t, k, p, mp, *a: orig(roll(inv_t), roll(k), roll(p), roll(mp), *a)))


@pytest.mark.parametrize("name", VERIFYING)
def test_control_resolution_a_drawn_log_prob_off_by_a_hundredth(manager, name):
    stage = manager.get_stage(name)
    orig = stage.ops.residual_sample_lp

    def shifted(*a, **k):
        tok, lp = orig(*a, **k)
        return tok, lp - 0.01
    _control(stage, _seeded(), patched(stage.ops, residual_sample_lp=shifted))


# ---- guided rows, n-gram bans, prompt log-probs: defects of the plumbing that the features' own replays share with the loop
def _ngram_kw():
    return dict(prompts=PROMPTS, max_tokens=MAX_TOKENS, temperature=TEMPERATURE, seed=SEEDS, no_repeat_ngram_size=S.NGRAM_ROWS,
                logit_bias={S.NGRAM_RECUR: 4.0})


def test_control_ngram_without_the_steps_proposals(manager_v64):
    """A position inside a step bans from the committed tokens alone: one or more positions late.  "13b": proposals are
    accepted there, so the text holds tokens whose history had proposals in it."""
    stage = manager_v64.get_stage("13b")
    orig = stage.ops.no_repeat_ngram_rows
    blind = lambda logits, ng, tokens, seq_len, max_len, step_tok=None, n_prev=0: orig(logits, ng, tokens, seq_len, max_len, None, 0)  # noqa: E731
    _control(stage, _ngram_kw(), patched(stage.ops, no_repeat_ngram_rows=blind), match=DIFF_OR_REMOVED, live=_generated_differs)


@pytest.mark.parametrize("name", NAMES)
def test_control_ngram_with_the_padding_counted_as_history(manager_v64, name):
    """Every row is told its prompt is P ids long: at n = 1 the pad id 0 is banned on every shorter row, which still never
    repeats a token -- check_no_repeat passes -- and returns the log-probs of a smaller distribution."""
    from tests.ngram_ref import check_no_repeat, real_ids
    stage = manager_v64.get_stage(name)
    orig = stage.ops.pack_no_repeat_ngram
    kw = dict(_ngram_kw(), no_repeat_ngram_size=1)
    assert len({len(r) for r in real_ids(stage, PROMPTS)[0]}) > 1
    replay = lambda st, texts, lps: check_no_repeat(real_ids(st, PROMPTS)[0], texts, [1] * len(PROMPTS))     # noqa: E731
    _control(stage, kw, patched(stage.ops, pack_no_repeat_ngram=lambda ns, lens, P, dev: orig(ns, [P] * len(lens), P, dev)), replay,
             live=_generated_differs)


def _guided_kw(stage):
    """Every row under cycle3: each state allows another third of the vocabulary, so a state that is one transition off lets a
    forbidden token through or returns the log-prob of another restricted distribution."""
    return dict(_seeded(), guided_fsm=S.cycle3(stage.shape.vocab))


def test_control_guided_bonus_row_under_a_stale_state(manager):
    """fsm_advance is skipped behind the LAST proposal, so column K -- the bonus row's -- keeps what an earlier step left.  "13b":
    whole blocks pass there, so the bonus row is live."""
    stage = manager.get_stage("13b")
    orig, last = stage.ops.fsm_advance, stage.config.draft_len - 1
    _control(stage, _guided_kw(stage), patched(stage.ops, fsm_advance=lambda fsm, step_tok, k: None if k == last else orig(fsm, step_tok, k)),
             match=DIFF_OR_REMOVED, live=_generated_differs)


@pytest.mark.parametrize("name", NAMES)
def test_control_guided_commit_that_moves_nothing(manager, name):
    stage = manager.get_stage(name)
    _control(stage, _guided_kw(stage), patched(stage.ops, fsm_commit=lambda *a, **k: None), match=DIFF_OR_REMOVED, live=_generated_differs)


def test_control_guided_target_rows_all_under_column_0(manager):
    """Every one of the target's K + 1 rows is masked by the state behind the committed tokens, as if no proposal had moved the
    automaton.  Dropping `first` from the DRAFT's calls alone need not be visible in what is returned, for the reason
    test_control_edit_without_the_position_inside_the_step gives: draft and verify would share a wrong proposal distribution,
    against which the chain is still lossless for the target's.  The control is on the target's rows, and on "13b": "34b" accepts
    next to nothing, so all it ever commits comes from row 0, whose column IS column 0 -- the defect is not live there (its
    returned tokens and log-probs keep their bits)."""
    stage = manager.get_stage("13b")
    orig = stage.ops.fsm_mask_rows

    def column_0(logits, fsm, first=0):
        if logits.dim() == 2:
            return orig(logits, fsm, first)
        for j in range(logits.shape[1]):
            orig(logits[:, j], fsm, 0)
        return logits
    _control(stage, _guided_kw(stage), patched(stage.ops, fsm_mask_rows=column_0), match=DIFF_OR_REMOVED, live=_generated_differs)


def _prompt_replay(n):
    from tests.prompt_logprobs_ref import check_values
    return lambda st, stats: print(f"[control] prompt_logprobs_ref.check_values passes: {check_values(st, stats, n):.3e}")


@pytest.mark.parametrize("name", NAMES)
def test_control_prompt_prefill_fed_one_position_late(manager, name):
    """The prefill pass (T = P at stage 0, T = P - 1 at a verifying stage) is fed one position late.  The logits the loop kept
    are then self-consistent with the numbers it returned -- prompt_logprobs_ref.check_values passes -- and are not the model's
    for those prompt positions."""
    stage = manager.get_stage(name)
    P = stage.encode_prompts(PROMPTS).shape[1]
    orig, T = stage.model.forward_ragged, (P, P - 1)
    assert stage.config.draft_len + 1 not in T and min(T) > 2                     # no decode pass has that many rows
    late = lambda ids, pos0, window, *a, **k: orig(ids, *((pos0 + 1, window + 1) if ids.shape[1] in T else (pos0, window)), *a, **k)  # noqa: E731
    _control(stage, dict(_seeded(), prompt_logprobs=3), patched(stage.model, forward_ragged=late), match=r"prompt token .*\|diff\|",
             replay_stats=_prompt_replay(3), live=_prompt_numbers_differ)


@pytest.mark.parametrize("name", VERIFYING)
def test_control_prompt_prefill_with_a_short_window(manager, name):
    stage = manager.get_stage(name)
    _control(stage, dict(_seeded(), prompt_logprobs=3), _short_window(stage.model), match=r"prompt token .*\|diff\|",
             replay_stats=_prompt_replay(3), live=_prompt_numbers_differ)
