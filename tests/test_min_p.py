"""Min-p on CPU: the numpy reference (tests/min_p_ref.py) against the direct f64 statement "keep p_v >= min_p * p_max,
renormalise", and the stage loops of serving/stages.py on the oracle twin with min_p / target_min_p set."""
import numpy as np
import pytest
import torch

import asd_amd
from asd_amd.serving.stages import StageConfig, StageManager
from tests.min_p_ref import MinPOracleOps, combine, direct_min_p, min_p_delta, min_p_thresholds, x_mp_of
from tests.oracle_backend import OracleBackend
from tests.stage_scenario import MAX_TOKENS, NAMES, PROMPTS, TEMPERATURE, check_generation, ref_logprob, stage_configs

INV_T = float(np.float32(1 / TEMPERATURE))


@pytest.fixture(autouse=True)
def oracle_backend():
    asd_amd.set_backend(OracleBackend())
    yield
    asd_amd.set_backend(None)


def _rows():
    """Rows whose boundary is hit exactly: at T = 1 the logits ln(p) of probabilities on a binary grid, so that
    p_v / p_max is exact and equals min_p for some v (ties at the boundary), plus Gaussian rows."""
    rng = np.random.default_rng(5)
    grid = np.array([0.0, -1.0, -1.0, -2.0, -2.0, -2.0, -3.0, -5.0, -np.inf, 0.0], np.float32) * np.float32(np.log(2.0))
    return [grid, rng.standard_normal(64).astype(np.float32) * 3, np.full(16, 1.25, np.float32)]


@pytest.mark.parametrize("min_p", [1.0, 0.5, 0.25, 0.1, 1e-30])
def test_reference_is_the_direct_statement(min_p):
    for row in _rows():
        for inv_t in (1.0, INV_T):
            thr = combine(np.float32(-np.inf), x_mp_of(row[None, :], min_p, inv_t))[0][0]
            keep = row >= thr
            q, want = direct_min_p(row, inv_t, min_p)
            z = row.astype(np.float64) * float(np.float32(inv_t))
            ratio = np.exp(z - z.max())
            clear = np.abs(ratio / min_p - 1.0) > 1e-6          # a token within an f32 rounding of the boundary may differ
            assert (keep == want)[clear].all(), (min_p, inv_t)
            assert keep[np.argmax(row)] and keep[row == row.max()].all()
            if min_p == 1.0:
                assert thr == row.max() and (keep == (row == row.max())).all()      # only the maxima survive
            if min_p == 1e-30:
                assert (keep == (row > -np.inf)).all()                              # nothing removed
            if (keep == want).all():
                for tok in np.nonzero(keep)[0][:4]:
                    assert abs(ref_logprob(row, tok, inv_t, thr) - np.log(q[tok])) < 1e-12


def test_ties_at_the_boundary_are_kept():
    row = _rows()[0]
    thr = x_mp_of(row[None, :], 0.25, 1.0)[0]                   # p / p_max = 1/4 exactly at the three logits -2 ln 2
    keep = row >= thr
    if thr == row[3]:
        assert keep[3:6].all() and keep.sum() == 7
    assert keep[:3].all() and not keep[6:9].any()
    assert min_p_delta(1.0, INV_T) == 0.0 and min_p_delta(0.1, INV_T) < 0.0
    # behind top-k: the larger threshold wins, row by row
    t = torch.from_numpy(np.stack([row, row]))
    a = min_p_thresholds(t, 1.0, 2, 1.0, 1e-30)
    b = min_p_thresholds(t, 1.0, 0, 1.0, 0.5)
    assert a[0] == row[0] and b[0] == np.float32(row.max() + min_p_delta(0.5, 1.0))


def _manager(**kw):
    ops = MinPOracleOps()
    return StageManager(stage_configs(**kw), ops=ops), ops


@pytest.mark.parametrize("name", NAMES)
def test_stage_loops_commit_from_the_min_p_set(name):
    sm, ops = _manager(min_p=0.05, target_min_p=0.05)
    stage = sm.get_stage(name)
    stage.keep_inputs = True
    texts, lps, _ = stage.generate(prompts=PROMPTS, max_tokens=MAX_TOKENS, temperature=TEMPERATURE)
    cfg = stage.config
    names = [n for n, _ in ops.trace]
    assert "draft_sample_min_p" in names and "draft_sample" not in names
    assert ("verify_accept_min_p" in names) == (name != "8b") and "verify_accept" not in names
    thr_b = lambda bonus: ops.bonus_threshold(bonus, INV_T, cfg.target_top_k, cfg.target_top_p, 0.05)
    check_generation(stage, texts, lps, INV_T, atol=1e-6, thr_of_bonus=thr_b)
    # every committed draw lies in its row's kept set
    for s in stage.step_inputs:
        drawn = s["drawn"].numpy()
        for b in range(len(PROMPTS)):
            if "tok" in s:
                j, K = int(s["n_acc"][b]), s["tok"].shape[1]
                row, thr = (s["logits"][b, j], float(s["t_thr"][b, j])) if j < K else (s["bonus"][b], float(thr_b(s["bonus"])[b]))
            else:
                row, thr = s["logits"][b], float(s["thr"][b])
            x = row.float().numpy()
            assert thr >= np.float32(x.max()) + min_p_delta(0.05, INV_T)
            assert x[drawn[b]] >= thr


def test_generate_argument_overrides_and_min_p_zero_is_todays_calls():
    sm, ops = _manager()
    for name in NAMES:
        stage = sm.get_stage(name)
        ops.trace.clear()
        a = stage.generate(prompts=PROMPTS, max_tokens=MAX_TOKENS, temperature=TEMPERATURE)
        first = list(ops.trace)
        stage.gen.manual_seed(int(stage.config.seed))
        ops.trace.clear()
        b = stage.generate(prompts=PROMPTS, max_tokens=MAX_TOKENS, temperature=TEMPERATURE, min_p=0.0)
        assert ops.trace == first and a[0] == b[0]
        assert {n for n, _ in first} <= {"draft_sample", "verify_accept", "residual_sample_lp", "commit_step_lp"}
        assert not any("min_p" in kw for _, kw in first)
        stage.gen.manual_seed(int(stage.config.seed))
        ops.trace.clear()
        c = stage.generate(prompts=PROMPTS, max_tokens=MAX_TOKENS, temperature=TEMPERATURE, min_p=0.3)
        names = {n for n, _ in ops.trace}
        if name == "8b":
            assert "draft_sample_min_p" in names
        else:                                                       # the argument is the TARGET's min-p at a verifying stage
            assert "verify_accept_min_p" in names and "draft_sample_min_p" not in names
            assert ("residual_sample_lp", ("min_p",)) in ops.trace
        assert c[0] != a[0]                                          # the setting is live
    # greedy decoding ignores min-p
    stage = sm.get_stage("8b")
    ops.trace.clear()
    try:
        stage.generate(prompts=PROMPTS[:1], max_tokens=2, temperature=0.0, min_p=0.5)
    except AttributeError:
        pass                                                        # (the twin has no greedy op; the point is what was NOT called)
    assert not any("min_p" in n for n, _ in ops.trace)


@pytest.mark.parametrize("bad", [-0.1, 1.5, float("nan"), float("inf"), "0.1", True])
def test_bad_min_p_raises(bad):
    sm, _ = _manager()
    with pytest.raises(ValueError, match="min_p"):
        sm.get_stage("8b").generate(prompts=PROMPTS[:1], max_tokens=2, min_p=bad)
    for field in ("min_p", "target_min_p"):
        with pytest.raises(ValueError, match="min_p"):
            StageManager([StageConfig(**{**stage_configs()[0].__dict__, field: bad})], ops=MinPOracleOps())
    assert StageConfig().min_p == 0.0 and StageConfig().target_min_p == 0.0
