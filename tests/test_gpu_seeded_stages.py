"""Stage.generate(seed=...) on distributed.HipOps: which uniform reaches which kernel (a thin recording subclass of HipOps and
keep_inputs' recorded `u`, against the numpy Philox reference), repeated calls, seed=None, and the statistical losslessness of
the HIP draft / verify / commit chain on uniforms that come from asd_step_uniforms (tests/test_seeded_lossless.py's wrapper
around tests/test_gpu_lossless.py's HipChain)."""
from dataclasses import replace

import numpy as np
import pytest
import torch

from tests import lossless as L
from tests.philox_ref import check_wiring, step_uniforms_ref
from tests.stage_scenario import NAMES, PROMPTS, TEMPERATURE, stage_configs, text_ids

pytestmark = pytest.mark.gpu

MAX_TOKENS = 12
DRAFT_LEN = 3
SEEDS = [0, 1, 2 ** 32, 2 ** 63, 2 ** 64 - 1]
_UNIFORM_ARG = {"draft_sample": 1, "draft_sample_top_k": 1, "draft_sample_min_p": 1, "verify_accept": 3, "verify_accept_top_p": 3,
                "verify_accept_top_k": 3, "verify_accept_min_p": 3, "residual_sample_lp": 3}


def _recording_ops():
    from asd_amd.distributed import HipOps

    class RecordingHipOps(HipOps):
        """HipOps that logs, per sampling call, its name and a host copy of the uniforms it was handed (tests/philox_ref.py's
        log format), and every step_uniforms call with its arguments."""

        def __init__(self):
            super().__init__()
            self.log = []

        def step_uniforms(self, seeds, step, stage, K_draft, K_accept, commit=True, out=None):
            self.log.append(dict(name="step_uniforms", kw=(), uniform=None, seeds=seeds.cpu().numpy().view(np.uint64).copy(),
                                 step=int(step), stage=int(stage), K_draft=int(K_draft), K_accept=int(K_accept),
                                 commit=bool(commit)))
            return super().step_uniforms(seeds, step, stage, K_draft, K_accept, commit=commit, out=out)

    def recorded(name):
        def call(self, *a, **kw):
            self.log.append(dict(name=name, kw=tuple(sorted(kw)), uniform=a[_UNIFORM_ARG[name]].cpu().numpy().copy()))
            return getattr(HipOps, name)(self, *a, **kw)
        return call
    for n in _UNIFORM_ARG:
        setattr(RecordingHipOps, n, recorded(n))
    return RecordingHipOps()


@pytest.fixture(scope="module")
def manager():
    from asd_amd.serving.stages import StageManager
    return StageManager([replace(c, draft_len=DRAFT_LEN) for c in stage_configs()], ops=_recording_ops())


def _names(ops):
    return [e["name"] for e in ops.log]


def _same(a, b):
    assert a[0] == b[0] and all(x.tobytes() == y.tobytes() for x, y in zip(a[1], b[1]))
    assert a[2]["n_tokens"] == b[2]["n_tokens"] and a[2]["finish_reasons"] == b[2]["finish_reasons"]
    for key in ("top_token_ids", "top_logprobs"):
        if key in a[2]:
            assert all(x.tobytes() == y.tobytes() for x, y in zip(a[2][key], b[2][key]))


@pytest.mark.parametrize("name", NAMES)
def test_every_uniform_is_the_reference_slot_of_its_seed_step_and_stage(manager, name, monkeypatch):
    stage, ops = manager.get_stage(name), manager.ops
    index = NAMES.index(name)
    Kd = 0 if index == 0 else DRAFT_LEN
    ops.log.clear()
    state = stage.gen.get_state().clone()

    def boom(*a, **kw):
        raise AssertionError("torch.rand launched inside a seeded call")
    stage.keep_inputs = True
    try:
        with monkeypatch.context() as m:
            m.setattr(torch, "rand", boom)
            texts, lps, stats = stage.generate(prompts=PROMPTS, max_tokens=MAX_TOKENS, temperature=TEMPERATURE, seed=SEEDS)
    finally:
        stage.keep_inputs = False
    assert torch.equal(stage.gen.get_state(), state)
    steps = check_wiring(ops.log, SEEDS, index, Kd)                 # the kernel's uniforms ARE the reference's, at their calls
    assert steps == stage.last_steps == len(stage.step_inputs)
    for s, kept in enumerate(stage.step_inputs):                    # ... and what the step kept is what it consumed
        rd, u, rc = step_uniforms_ref(SEEDS, s, index, max(Kd, 1), Kd)
        assert kept["r_draft"].cpu().numpy().tobytes() == rd.tobytes()
        if Kd:
            assert kept["u"].cpu().numpy().tobytes() == u.tobytes() and kept["r_commit"].cpu().numpy().tobytes() == rc.tobytes()
    assert all(len(text_ids(t)) == MAX_TOKENS == len(lp) and np.isfinite(lp).all() for t, lp in zip(texts, lps))
    ops.check_status()


@pytest.mark.parametrize("name", NAMES[:2])
def test_a_repeated_call_is_bit_equal(manager, name):
    stage, ops = manager.get_stage(name), manager.ops
    free = stage.generate(prompts=PROMPTS, max_tokens=MAX_TOKENS, temperature=TEMPERATURE, seed=SEEDS)
    stop = sorted({text_ids(t)[3] for t in free[0]})[:8]            # ids the seeded run is known to commit
    kw = dict(prompts=PROMPTS, max_tokens=MAX_TOKENS, temperature=TEMPERATURE, seed=SEEDS, stop_token_ids=stop, logprobs=2)
    a = stage.generate(**kw)
    stage.generate(prompts=PROMPTS[:2], max_tokens=3, temperature=TEMPERATURE)           # an unseeded call in between
    stage.generate(prompts=PROMPTS, max_tokens=MAX_TOKENS, temperature=TEMPERATURE, seed=7)
    ops.log.clear()
    b = stage.generate(**kw)
    _same(a, b)
    assert "stop" in a[2]["finish_reasons"] and _names(ops).count("step_uniforms") == stage.last_steps
    for i, (t, lp) in enumerate(zip(a[0], a[1])):                   # the free seeded run, cut behind its first stop id
        n = a[2]["n_tokens"][i]
        assert text_ids(t) == text_ids(free[0][i])[:n] and lp.tobytes() == free[1][i][:n].tobytes()
    _same(free, stage.generate(prompts=PROMPTS, max_tokens=MAX_TOKENS, temperature=TEMPERATURE, seed=SEEDS))
    ops.check_status()


@pytest.mark.parametrize("name", NAMES[:2])
def test_seed_none_makes_no_step_uniforms_call(manager, name):
    stage, ops = manager.get_stage(name), manager.ops
    ops.log.clear()
    stage.generate(prompts=PROMPTS, max_tokens=4, temperature=TEMPERATURE)
    assert _names(ops) and "step_uniforms" not in _names(ops)
    ops.log.clear()
    stage.generate(prompts=PROMPTS, max_tokens=4, temperature=0.0, seed=SEEDS)           # greedy ignores the seed
    assert not ops.log


def test_hip_chain_on_kernel_uniforms_is_lossless():
    """V = 512, B = 4096, 50 steps, route b: every uniform of every step comes out of asd_step_uniforms."""
    from asd_amd import kernels
    from asd_amd.distributed import HipOps
    from tests.test_gpu_lossless import DRAW_SEED, PAD, ROW_SEED, HipChain, TorchOps
    from tests.test_seeded_lossless import SeededChain
    ops = HipOps()
    checked = []

    def uniforms(seeds, step, stage, K_draft, K_accept):
        out = ops.step_uniforms(torch.from_numpy(seeds).cuda(), step, stage, K_draft, K_accept)
        got = tuple(t.cpu().numpy() for t in out)
        if step in (0, L.SMALL.n_calls - 1):                        # the stream under test is the reference's
            ref = step_uniforms_ref(seeds, step, stage, K_draft, K_accept)
            checked.append(all(g.tobytes() == r.tobytes() for g, r in zip(got, ref)))
        return got
    route = L.ROUTES["b"]
    xt, xd = L.make_rows(L.SMALL, "bf16", ROW_SEED)
    ref = L.reference(xt, xd, route)
    inner = HipChain(kernels, L.SMALL, route, "bf16", xt, xd)
    chain = SeededChain(inner, uniforms=uniforms)
    counts = L.run_chain(chain, L.SMALL, DRAW_SEED, L.SMALL.V + PAD + 1, xp=TorchOps)
    torch.cuda.synchronize()
    assert inner.ds.status() == 0 and inner.rs.status() == 0 and inner.ws.status() == 0
    assert counts.n_seq == L.SMALL.B * L.SMALL.n_calls >= 200000 and checked == [True, True]
    L.assert_lossless(L.evaluate(counts, ref), "seeded HIP chain, V 512 B 4096, route b bf16")
