"""The ops calls of one step of Stage.generate, per route, against a recording (tests/stage_call_pattern.json) made from the
loops as they were BEFORE they were folded into two: serving/stages.py may be reorganised, the calls a step makes may not change.

For stage 0 and one verifying stage of tests/stage_scenario.py (vocabulary 1000, draft_len 4, two prompts, max_tokens 6) and every
route of ROUTES, each ops call the STAGE makes is reduced to its pattern: the name, the positional arguments and the keyword
arguments, an int / float / bool / str (or a list of them) by value, a tensor by shape and dtype, anything else by type name;
the `step` of step_uniforms is a placeholder.  Checked: the calls ahead of the first step (the packs), that EVERY step of the
call shows the route's one pattern, that there are stats["steps"] of them, and the calls behind the last.  How many steps a call
takes, and anything else that depends on which tokens were accepted, is not recorded: that may differ between CPUs.

Recording (only ever from a tree whose loops are known good): ASD_RECORD_STAGE_CALL_PATTERN=1 python -m tests.test_stage_call_pattern"""
import json
import os
from pathlib import Path

import numpy as np
import pytest
import torch

import asd_amd
from asd_amd.serving.stages import StageManager
from tests.logit_edit_ref import EditOracleOps
from tests.oracle_backend import OracleBackend
from tests.philox_ref import PhiloxOracleOps
from tests.stage_scenario import NAMES, PROMPTS, TEMPERATURE, stage_configs

FIXTURE = Path(__file__).with_name("stage_call_pattern.json")
RECORD_ENV = "ASD_RECORD_STAGE_CALL_PATTERN"
STAGES = (NAMES[0], NAMES[2])
TWO = PROMPTS[:2]
ROWS = dict(temperature=[0.7, 1.0], top_k=[0, 50])
FINISH = dict(max_tokens=[4, 6], stop_sequences=[[5, 9]])
ROUTES = {
    "plain": {},
    "top_k": dict(top_k=50),
    "min_p": dict(min_p=0.1),
    "rows": ROWS,
    "greedy": dict(temperature=0.0),
    "stop_ids": dict(stop_token_ids=[3, 7]),
    "finish": FINISH,
    "logprobs": dict(logprobs=2),
    "seeded": dict(seed=[11, 2 ** 64 - 1]),
    "edits": dict(logit_bias={5: 2.0}, banned_token_ids=[7], min_tokens=2, stop_token_ids=[3]),
    "combined": dict(ROWS, **FINISH, seed=[11, 2 ** 64 - 1], logprobs=2, logit_bias={5: 2.0}, banned_token_ids=[7]),
}


class PatternOracleOps(PhiloxOracleOps, EditOracleOps):
    """Every op of the stage loops on CPU tensors: the rows, edit, top-N, stop and finish twins + step_uniforms."""


class CallLog:
    """Stands between a Stage and its ops: logs the pattern of every call the stage makes (the calls a twin makes inside one
    of its own ops go to the twin itself and are not seen)."""

    def __init__(self, ops):
        self._ops, self.calls = ops, []

    def __getattr__(self, name):
        fn = getattr(self._ops, name)

        def call(*a, **kw):
            args = [_describe(v) for v in a]
            if name == "step_uniforms":
                args[1] = "<step>"
            self.calls.append(dict(name=name, args=args, kw={k: _describe(kw[k]) for k in sorted(kw)}))
            return fn(*a, **kw)
        return call


def _describe(v):
    if isinstance(v, torch.Tensor):
        return dict(shape=list(v.shape), dtype=str(v.dtype))
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    if isinstance(v, np.integer):
        return int(v)
    if isinstance(v, np.floating):
        return float(v)
    if isinstance(v, (list, tuple)):
        return [_describe(x) for x in v]
    if isinstance(v, (torch.dtype, torch.device)):
        return str(v)
    return type(v).__name__


def observe(name, route):
    """One generate call -> (packs, steps, tail, stats): the calls ahead of the first step, one list of calls per step (a step
    ends with its commit_step_* call and the commit_top_logprobs call that may follow it), and the calls behind the last."""
    log = CallLog(PatternOracleOps())
    stage = StageManager(stage_configs(), ops=log).get_stage(name)
    kw = dict(prompts=TWO, max_tokens=6, temperature=TEMPERATURE)
    kw.update(ROUTES[route])
    stats = stage.generate(**kw)[2]
    calls = log.calls
    n_packs = next(i for i, c in enumerate(calls) if not c["name"].startswith("pack_"))
    steps, cur = [], []
    for i, c in enumerate(calls[n_packs:], n_packs):
        cur.append(c)
        nxt = calls[i + 1]["name"] if i + 1 < len(calls) else None
        if c["name"] == "commit_top_logprobs" or (c["name"].startswith("commit_step") and nxt != "commit_top_logprobs"):
            steps.append(cur)
            cur = []
    return calls[:n_packs], steps, cur, stats


def dump(out):
    """The file's layout: one line per ops call."""
    calls = lambda cs: "[" + ",".join("\n   " + json.dumps(c, sort_keys=True) for c in cs) + "]"     # noqa: E731
    route = lambda v: ",\n".join(f'  "{part}": {calls(v[part])}' for part in ("packs", "step", "tail"))   # noqa: E731
    FIXTURE.write_text("{\n" + ",\n".join(f' {json.dumps(k)}: {{\n{route(v)}}}' for k, v in sorted(out.items())) + "\n}\n")


def record():
    out = {}
    for name in STAGES:
        for route in ROUTES:
            packs, steps, tail, stats = observe(name, route)
            assert steps and all(s == steps[0] for s in steps) and len(steps) == stats["steps"], (name, route)
            out[f"{name}/{route}"] = dict(packs=packs, step=steps[0], tail=tail)
    dump(out)


@pytest.fixture(autouse=True)
def oracle_backend():
    asd_amd.set_backend(OracleBackend())
    yield
    asd_amd.set_backend(None)


@pytest.fixture(scope="module")
def recorded():
    return json.loads(FIXTURE.read_text())


def test_the_recording_holds_every_route_of_both_stages(recorded):
    assert sorted(recorded) == sorted(f"{n}/{r}" for n in STAGES for r in ROUTES)


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("name", STAGES)
def test_every_step_makes_the_recorded_calls(recorded, name, route):
    want = recorded[f"{name}/{route}"]
    packs, steps, tail, stats = observe(name, route)
    as_json = lambda v: json.loads(json.dumps(v))                       # noqa: E731  (tuples -> lists, as the file holds them)
    assert as_json(packs) == want["packs"]
    assert len(steps) == stats["steps"] >= 1
    for i, s in enumerate(steps):
        assert as_json(s) == want["step"], (i, [c["name"] for c in s], [c["name"] for c in want["step"]])
    assert as_json(tail) == want["tail"]


if __name__ == "__main__":
    if os.environ.get(RECORD_ENV) != "1":
        raise SystemExit(f"set {RECORD_ENV}=1 to overwrite {FIXTURE.name}")
    asd_amd.set_backend(OracleBackend())
    record()
