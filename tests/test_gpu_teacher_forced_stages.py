"""What Stage.generate RETURNS on distributed.HipOps against the f64 teacher-forced reference of tests/teacher_forced_ref.py: the
scenarios of tests/test_teacher_forced_stages.py (tests/teacher_forced_scenarios.py) through the real kernels -- samplers,
verify, residual draw, commits, mask, bad words, edits, penalties, top-N -- on the three tiny stages of tests/stage_scenario.py
in float32, one two-stage run at the full vocabulary, and the default bfloat16 stages under the same formulas.

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
(bfloat16: stage 0 at top_p = 1, tests/teacher_forced_scenarios.py::bf16 says why.)"""
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
