"""Stage.generate with per-request temperature / top-k / top-p / min-p on distributed.HipOps (serving/stages.py, PER-REQUEST
SAMPLING): the three tiny stages of tests/stage_scenario.py.
  - the mixed call of tests/test_per_request_stages.py replays through check_generation with every row's own temperature and
    threshold (tests/per_request_ref.py) at the bar of tests/test_gpu_stages.py;
  - seeded and with every row truncated on both sides, row b of the mixed call is row b of the scalar call with row b's values,
    bit for bit in texts and log-probs;
  - a run with a stop set and logprobs = 3: every table row is the reference's at the row's own temperature;
  - one two-stage run at the full vocabulary."""
import numpy as np
import pytest
import torch

from tests.per_request_ref import MIXED, TRUNCATED, check_generation_rows, inv_t_of, own_values, row_values
from tests.stage_scenario import MAX_TOKENS, NAMES, PROMPTS, stage_configs, text_ids
from tests.top_logprobs_ref import LP_ATOL, ref_top_logprobs, step_rows

pytestmark = pytest.mark.gpu

ATOL = 2e-5        # tests/test_gpu_stages.py's bar for a kernel lp against the f64 value at its row
SEEDS = [11, 2 ** 64 - 1, 33, 0, 55]


@pytest.fixture(scope="module")
def manager():
    from asd_amd.serving.stages import StageManager
    return StageManager(stage_configs())


def _bonus_thr(ops, stage, values):
    """The bonus rows' thresholds by the select itself: one draw per row under the rows' own values (the threshold does not
    depend on the uniform)."""
    cols = list(zip(*values))

    def thr(bonus):
        lg = bonus.cuda().contiguous()
        table = ops.pack_sampling_rows(list(cols[0]), list(cols[1]), list(cols[2]), list(cols[3]), lg.shape[1], lg.dtype, lg.device)
        r = torch.full((lg.shape[0],), 0.5, dtype=torch.float32, device=lg.device)
        return ops.draft_sample_rows(lg, r, table)[2].cpu().numpy()
    return thr


def _run_kept(stage, **kw):
    stage.keep_inputs = True
    try:
        return stage.generate(**kw)
    finally:
        stage.keep_inputs = False


@pytest.mark.parametrize("name", NAMES)
def test_mixed_call_replays_with_every_rows_own_values(manager, name):
    stage = manager.get_stage(name)
    texts, lps, _ = _run_kept(stage, prompts=PROMPTS, max_tokens=MAX_TOKENS, **MIXED)
    values = own_values(stage, MIXED)
    worst = check_generation_rows(stage, texts, lps, values, atol=ATOL, bonus_thr=_bonus_thr(manager.ops, stage, values))
    print(f"[per-request] stage {name}: max |lp_drawn - f64| = {worst:.3e}")
    if name != "8b":
        V = stage.shape.vocab
        for s in stage.step_inputs:
            thr = s["t_thr"].cpu().numpy()
            for b, v in enumerate(values):
                off = not 0 < v[1] < V and not 0.0 < v[2] < 1.0 and not v[3] > 0.0
                assert np.isneginf(thr[b]).all() if off else np.isfinite(thr[b]).all()
    manager.ops.check_status()


@pytest.mark.parametrize("name", NAMES)
def test_seeded_row_b_is_the_scalar_call_with_row_bs_values(manager, name):
    stage = manager.get_stage(name)
    mixed = stage.generate(prompts=PROMPTS, max_tokens=MAX_TOKENS, seed=SEEDS, **TRUNCATED)
    sets = {}
    for b in range(len(PROMPTS)):
        sets.setdefault(tuple(sorted(row_values(TRUNCATED, b).items())), []).append(b)
    assert len(sets) == 4                                                  # rows 0 and 4 share a set
    for key, rows in sets.items():
        scal = stage.generate(prompts=PROMPTS, max_tokens=MAX_TOKENS, seed=SEEDS, **dict(key))
        for b in rows:
            assert scal[0][b] == mixed[0][b], (name, b)
            assert scal[1][b].tobytes() == mixed[1][b].tobytes(), (name, b)
    assert len(set(mixed[0])) == len(PROMPTS)
    manager.ops.check_status()


def test_stop_set_and_top_logprobs_at_every_rows_own_temperature(manager):
    stage = manager.get_stage("34b")
    plain, _, _ = stage.generate(prompts=PROMPTS, max_tokens=MAX_TOKENS, seed=SEEDS, **MIXED)
    stop = sorted({text_ids(t)[3] for t in plain})[:8]                     # ids the run is known to commit
    texts, lps, stats = _run_kept(stage, prompts=PROMPTS, max_tokens=MAX_TOKENS, seed=SEEDS, stop_token_ids=stop, logprobs=3,
                                  **MIXED)
    assert "stop" in stats["finish_reasons"]
    for t, lp, n, why, ids, tlp in zip(texts, lps, stats["n_tokens"], stats["finish_reasons"], stats["top_token_ids"],
                                       stats["top_logprobs"]):
        tk = text_ids(t)
        assert len(tk) == n == len(lp) and ids.shape == (n, 3) and tlp.shape == (n, 3)
        assert (why == "stop") == (tk[-1] in stop) and not any(i in stop for i in tk[:-1])
        assert np.isfinite(lp).all() and (np.diff(tlp, axis=1) <= 0).all()
        for i in range(n):                                                 # the table is the UNTRUNCATED distribution
            hit = np.nonzero(ids[i] == tk[i])[0]
            if hit.size:
                assert lp[i] >= tlp[i, hit[0]] - 1e-5
    worst, rows = 0.0, 0
    for s in stage.step_inputs:
        c = {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in s.items()}
        x = step_rows(c)
        for b, T in enumerate(MIXED["temperature"]):
            ref_id, ref_lp = ref_top_logprobs(x[b], 3, inv_t_of(T))
            assert np.array_equal(c["top_id"][b].numpy(), ref_id), b
            worst = max(worst, float(np.abs(c["top_lp"][b].numpy().astype(np.float64) - ref_lp).max()))
            rows += x.shape[1]
    assert rows > 0 and worst <= LP_ATOL, worst
    manager.ops.check_status()


def test_full_vocabulary_two_stage_run():
    from asd_amd.serving.stages import StageManager
    sm = StageManager(stage_configs(vocab=152064)[:2])
    stage = sm.get_stage(NAMES[1])
    params = {k: [v[4], v[1], v[2], v[3]] for k, v in MIXED.items()}          # row 0 truncates nothing
    texts, lps, _ = _run_kept(stage, prompts=PROMPTS[:4], max_tokens=10, **params)
    values = own_values(stage, params)
    check_generation_rows(stage, texts, lps, values, atol=ATOL, bonus_thr=_bonus_thr(sm.ops, stage, values), max_tokens=10)
    sm.ops.check_status()
