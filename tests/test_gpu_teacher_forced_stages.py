"""What Stage.generate RETURNS on distributed.HipOps against the f64 teacher-forced reference of tests/teacher_forced_ref.py: the
scenarios of tests/test_teacher_forced_stages.py (tests/teacher_forced_scenarios.py) through the real kernels -- samplers,
verify, residual draw, commits, mask, automata, bad words, n-gram bans, edits, penalties, top-N, prompt scores -- on the three
tiny stages of tests/stage_scenario.py in float32 (at vocabulary 64 for the n-gram rows), two two-stage runs at the full
vocabulary, and the default bfloat16 stages under the same formulas.

Every check starts from the returned text: a dense f64 forward over prompt + text, the processors and the truncation in f64, and
the bound 2 * inv_t * a * eps_x + 2e-5 with eps_x = 4 * max |dense forward in the stage's dtype on the GPU - f64| (the reference
side only; 2e-5 is tests/test_gpu_stages.py's bar for a kernel log-prob against f64 at its own row).  The SHARP check is the
float32 one: eps_x is a few 1e-5 there and a plumbing defect moves a log-prob by 1e-2 to 10 (the negative controls of the CPU
file).  At bfloat16 eps_x is near 0.5 and the bound near 1.5: that run shows only that the production dtype's casts break
nothing gross.

MEASURED on the MI355X (every test prints its figures; DESIGN.md 5.1 holds the same table).  eps_x / bound / worst |lp - f64| /
worst top-N log-prob / ambiguous positions:
  float32   defaults                      4.3e-5 .. 6.0e-5 / 1.4e-4 .. 1.9e-4 / 9.1e-6 / -               / 0 of 468
  float32   target top-k, top-p, min-p    4.2e-5 .. 6.3e-5 / 1.4e-4 .. 2.0e-4 / 1.3e-5 / -               / 0 of 480
  float32   rows route                    4.3e-5 .. 5.3e-5 / 1.9e-4 .. 2.3e-4 / 9.4e-6 / -               / 0 of 360
  float32   ragged ends                   4.4e-5 .. 5.8e-5 / 1.4e-4 .. 1.9e-4 / 1.1e-5 / -               / 0 of 615
  float32   everything on (+ V = 152064)  4.3e-5 .. 5.2e-5 / 2.0e-4 .. 2.9e-4 / 9.9e-6 / 1.5e-5, 0 swaps / 0 of 760
  float32   greedy                        4.7e-5 .. 5.8e-5 / 1.3e-4 .. 1.6e-4 / 6.2e-6 / -               / 0 of 150 (none inside the arg-max gap)
  float32   edges of the loop             3.6e-5 .. 6.1e-5 / 1.2e-4 .. 1.9e-4 / 9.4e-6 / -               / 1 of 876 (at most 1 of 60 in a call)
  bfloat16  defaults                      0.58 .. 0.71     / 1.7 .. 2.0       / 0.13   / -               / 0 of 180
  bfloat16  everything on                 0.50 .. 0.63     / 2.8 .. 3.6       / 0.13   / 0.22, 130 swaps / 0 of 352
(bfloat16: stage 0 at top_p = 1, tests/teacher_forced_scenarios.py::bf16 says why.)

GUIDED ROWS, N-GRAM BANS, PROMPT LOG-PROBS (fsm.hip, no_repeat_ngram.hip, prompt_logprobs.hip), the same columns and on a
second line the prompt's: worst |prompt lp - f64| / worst prompt-table log-prob / rank windows wider than one value:
  float32   guided rows, six ways         4.1e-5 .. 6.0e-5 / 1.1e-4 .. 2.2e-4 / 8.4e-6 / 1.6e-5, 0 swaps / 4 of 764 (at most 1 of 39 in a call)
  float32   n-gram rows, V = 64           3.4e-5 .. 4.8e-5 / 9.4e-5 .. 1.4e-4 / 8.0e-6 / -               / 0 of 480
            live bans per call (mass above the bound): n = 2 row 4 .. 5, n = 3 row 8 .. 12 (of 32 tokens), n = 1 row 11 .. 12
  float32   everything now (+ V = 152064) 4.3e-5 .. 5.2e-5 / 2.0e-4 .. 3.0e-4 / 1.1e-5 / 1.5e-5, 0 swaps / 0 of 748
            prompt: 4.8e-6 / 7.1e-6, 0 swaps / 16 of 166 (all 16 at V = 152064, 8 of 11 in a call; 0 of 144 at V = 1000)
  float32   prompt_logprobs 0, 3, 8       4.4e-5 .. 6.1e-5 / 1.1e-4 .. 3.7e-4 / 1.1e-5 / -               / 1 of 900 (at most 1 of 60 in a call)
            prompt: 4.8e-6 / 6.3e-6, 0 swaps / 0 of 180
  float32   edges of the loop, now        3.2e-5 .. 6.1e-5 / 1.1e-4 .. 1.9e-4 / 9.6e-6 / -               / 0 of 895
            prompt: 6.3e-6 / 3.8e-6, 0 swaps / 0 of 174
  bfloat16  everything now                0.53 .. 0.71     / 3.0 .. 4.1       / 0.14   / 0.20, 97 swaps  / 0 of 341
            prompt: 0.074 / 0.076, 22 swaps / 72 of 72
  bfloat16  prompt_logprobs 3             0.58 .. 0.71     / 1.7 .. 2.0       / 0.13   / -               / 0 of 180
            prompt: 0.074 / 0.075, 6 swaps / 36 of 36
No scenario failed on the kernels: the state columns, the bans' histories and the scored prefill are the reference's."""
import pytest
import torch

from tests import teacher_forced_scenarios as S
from tests.stage_scenario import MAX_TOKENS, NAMES, PROMPTS, stage_configs

pytestmark = pytest.mark.gpu

LP_BAR = 2e-5      # tests/test_gpu_stages.py's bar for a kernel lp against the f64 value at its row
VERIFYING = NAMES[1:]


def _manager(dtype=torch.float32, draft_len=None, **kw):
    from asd_amd.serving.stages import StageManager
    cfgs = stage_configs(dtype=dtype, **kw)
    for c in cfgs:
        c.draft_len = draft_len or c.draft_len
    return StageManager(cfgs)


@pytest.fixture(scope="module")
def manager():
    return _manager()


@pytest.fixture(scope="module")
def manager_bf16():
    return _manager(torch.bfloat16)


@pytest.mark.parametrize("seeded", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_defaults(manager, name, seeded):
    stage = manager.get_stage(name)
    rep = S.defaults(stage, LP_BAR, seeded)
    assert name == NAMES[0] or rep["ambiguous"] == 0                              # the untruncated target
    assert name != "13b" or stage.last_steps < MAX_TOKENS                         # its draft's weights are its own: blocks pass
    manager.ops.check_status()


@pytest.mark.parametrize("which", sorted(S.TARGET_TRUNCATION))
@pytest.mark.parametrize("name", VERIFYING)
def test_target_truncation(manager, name, which):
    S.target_truncation(manager.get_stage(name), LP_BAR, which)
    manager.ops.check_status()


@pytest.mark.parametrize("which", sorted(S.ROWS))
@pytest.mark.parametrize("name", NAMES)
def test_rows_route(manager, name, which):
    S.rows_route(manager.get_stage(name), LP_BAR, which)
    manager.ops.check_status()


@pytest.mark.parametrize("sync_every", [1, 4])
@pytest.mark.parametrize("name", NAMES)
def test_ragged_ends(manager, name, sync_every):
    S.ragged_ends(manager.get_stage(name), LP_BAR, sync_every)
    manager.ops.check_status()


@pytest.mark.parametrize("name", NAMES)
def test_everything_on(manager, name):
    S.everything(manager.get_stage(name), LP_BAR)
    manager.ops.check_status()


@pytest.mark.parametrize("name", NAMES)
def test_greedy_with_a_stop_id_and_penalties(manager, name):
    S.greedy(manager.get_stage(name), LP_BAR)
    manager.ops.check_status()


@pytest.mark.parametrize("name", NAMES)
def test_one_manager_calls_back_to_back(name):
    sm = _manager()
    S.back_to_back(sm.get_stage(name), LP_BAR)
    sm.ops.check_status()


@pytest.mark.parametrize("edge", sorted(S.EDGES))
def test_edges_of_the_loop(edge):
    sm, _ = S.edge(_manager, LP_BAR, edge)
    sm.ops.check_status()


def test_full_vocabulary_two_stage_run():
    """tiny(vocab=152064) in float32, B = 4, 8 tokens, two stages with a draft that differs from its target, everything on: a
    row is spread over workgroups and slices here."""
    from asd_amd.serving.stages import StageManager
    cfgs = stage_configs(vocab=152064, dtype=torch.float32)[:2]
    cfgs[1].model_seed = 1
    sm = StageManager(cfgs)
    S.everything(sm.get_stage(NAMES[1]), LP_BAR, PROMPTS[:4], 8)
    sm.ops.check_status()


@pytest.mark.parametrize("name", NAMES)
def test_bf16_defaults_and_everything_on(manager_bf16, name):
    """The production dtype under the same formulas: coarse (module docstring); the sharp check is the float32 one."""
    stage = manager_bf16.get_stage(name)
    S.bf16(stage, LP_BAR)
    manager_bf16.ops.check_status()


# ---- guided rows (fsm.hip), n-gram bans (no_repeat_ngram.hip), prompt log-probs (prompt_logprobs.hip)
@pytest.fixture(scope="module")
def manager_v64():
    return _manager(vocab=S.NGRAM_VOCAB)


@pytest.mark.parametrize("name,how", S.guided_cases(NAMES))
def test_guided_rows(manager, name, how):
    S.guided(manager.get_stage(name), LP_BAR, how)
    manager.ops.check_status()


@pytest.mark.parametrize("greedy", [False, True], ids=["sampled", "greedy"])
def test_ngram_rows_with_live_bans(manager_v64, greedy):
    """All three stages in one test: the n = 3 row's live bans are counted over the scenario."""
    reps = [S.ngram(manager_v64.get_stage(name), LP_BAR, greedy) for name in NAMES]
    assert sum(rep["ngram_live"][2] for rep in reps) >= 1, [rep["ngram_live"] for rep in reps]
    manager_v64.ops.check_status()


@pytest.mark.parametrize("name", NAMES)
def test_everything_now(manager, name):
    S.everything_now(manager.get_stage(name), LP_BAR)
    manager.ops.check_status()


@pytest.mark.parametrize("n,how", S.PROMPT_HOW)
@pytest.mark.parametrize("name", NAMES)
def test_prompt_logprobs(manager, name, n, how):
    S.prompt(manager.get_stage(name), LP_BAR, n, how)
    manager.ops.check_status()


@pytest.mark.parametrize("edge", sorted(S.EDGES))
def test_edges_of_the_loop_now(edge):
    sm, _ = S.edge_now(_manager, LP_BAR, edge)
    sm.ops.check_status()


@pytest.mark.parametrize("name", NAMES)
def test_one_manager_calls_back_to_back_now(name):
    sm = _manager()
    S.back_to_back_now(sm.get_stage(name), LP_BAR)
    sm.ops.check_status()


def test_full_vocabulary_two_stage_run_now():
    """test_full_vocabulary_two_stage_run's shape under everything_now: the automaton's state rows, the n-gram bans and the
    prompt's scoring pass at V = 152064."""
    from asd_amd.serving.stages import StageManager
    cfgs = stage_configs(vocab=152064, dtype=torch.float32)[:2]
    cfgs[1].model_seed = 1
    sm = StageManager(cfgs)
    S.everything_now(sm.get_stage(NAMES[1]), LP_BAR, PROMPTS[:4], 8)
    sm.ops.check_status()


@pytest.mark.parametrize("name", NAMES)
def test_bf16_everything_now_and_prompt(manager_bf16, name):
    """Coarse, as the other bfloat16 run is."""
    S.bf16_now(manager_bf16.get_stage(name), LP_BAR)
    manager_bf16.ops.check_status()
