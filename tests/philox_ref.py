"""The numpy statement of asd_step_uniforms (include/asd_hip.h, "Per-request seeds"): Philox4x32-10 written from the Random123
description, the step's uniforms by the header's counter layout, and the oracle ops twin that serves them to the stage loops
and records what every ops call was handed.

TEST INFRASTRUCTURE, like tests/min_p_ref.py: never importable from the package."""
import numpy as np
import torch

from tests.top_logprobs_ref import TopOracleOps

M0, M1 = 0xD2511F53, 0xCD9E8D57          # the round multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85          # the key increments (golden ratio, sqrt(3) - 1)
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter: 4 and key: 2 uint32 values (or arrays that broadcast against each other) -> uint32 [..., 4].
    Round: (c0, c1, c2, c3) -> (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)); the key is bumped between the
    10 rounds.  Products are taken in uint64 (both factors < 2^32: exact)."""
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(*[np.asarray(v, dtype=np.uint64) & MASK for v in (*counter, *key)])
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & MASK, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + np.uint64(W0)) & MASK, (k1 + np.uint64(W1)) & MASK
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def to_uniform(x):
    """float(x >> 8) * 2^-24 of uint32 words: exact in f32, in [0, 1)."""
    return ((np.asarray(x, np.uint32) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)


def as_u64(seeds):
    """Seeds as the kernel reads them: ints in [0, 2^64), or an int64 tensor / array (two's complement) -> uint64 [B]."""
    if isinstance(seeds, torch.Tensor):
        seeds = seeds.cpu().numpy()
    if isinstance(seeds, np.ndarray) and seeds.dtype == np.int64:
        return seeds.view(np.uint64).copy()
    return np.array([int(s) for s in seeds], dtype=np.uint64)


def step_uniforms_ref(seeds, step, stage, K_draft, K_accept):
    """-> (r_draft f32 [K_draft, B], u f32 [B, K_accept], r_commit f32 [B]): word 0 / word 1 of counter (step, k, stage, 0) under
    key (seed_lo, seed_hi) for slot k, word 2 of k = 0."""
    s = as_u64(seeds)
    B = s.shape[0]
    K = max(int(K_draft), int(K_accept), 1)
    k = np.arange(K, dtype=np.uint64)[None, :]
    w = philox4x32_10((np.uint64(step), k, np.uint64(stage), np.uint64(0)), (s[:, None] & MASK, s[:, None] >> np.uint64(32)))
    assert w.shape == (B, K, 4)
    f = to_uniform(w)
    return (np.ascontiguousarray(f[:, :K_draft, 0].T), np.ascontiguousarray(f[:, :K_accept, 1]),
            np.ascontiguousarray(f[:, 0, 2]))


# where every sampling op takes its uniforms (positional index; all are called positionally by the stage loops)
_UNIFORM_ARG = {"draft_sample": 1, "draft_sample_top_k": 1, "draft_sample_min_p": 1, "verify_accept": 3, "verify_accept_top_p": 3,
                "verify_accept_top_k": 3, "verify_accept_min_p": 3, "residual_sample_lp": 3}
_RECORDED = tuple(_UNIFORM_ARG) + ("commit_step_lp", "commit_step_stop", "top_logprobs", "commit_top_logprobs", "verify_greedy")


class RecordingOracleOps(TopOracleOps):
    """The CPU twin of distributed.HipOps for the stage loops (plain / stop / greedy / top-N ops) that logs every ops call:
    `log` holds dict(name=, kw= sorted keyword names, uniform= a copy of the uniform array the call was handed, or None)."""

    def __init__(self):
        super().__init__()
        self.log = []

    def names(self):
        return [e["name"] for e in self.log]

    def trace(self):
        return [(e["name"], e["kw"]) for e in self.log]


def _recorded(name):
    def call(self, *a, **kw):
        at = _UNIFORM_ARG.get(name)
        uni = None if at is None else a[at].detach().cpu().numpy().copy()
        self.log.append(dict(name=name, kw=tuple(sorted(kw)), uniform=uni))
        return getattr(super(RecordingOracleOps, self), name)(*a, **kw)
    call.__name__ = name
    return call


for _n in _RECORDED:
    if hasattr(TopOracleOps, _n):
        setattr(RecordingOracleOps, _n, _recorded(_n))


class PhiloxOracleOps(RecordingOracleOps):
    """RecordingOracleOps + step_uniforms on the reference above, with HipOps' contract: the outputs are views of `out`."""

    def step_uniforms(self, seeds, step, stage, K_draft, K_accept, commit=True, out=None):
        B = seeds.shape[0]
        self.log.append(dict(name="step_uniforms", kw=(), uniform=None, seeds=as_u64(seeds), step=int(step), stage=int(stage),
                             K_draft=int(K_draft), K_accept=int(K_accept), commit=bool(commit)))
        assert seeds.dtype == torch.int64 and 0 <= step < 2 ** 32 and 0 <= stage < 2 ** 32
        need = (K_draft + K_accept + 1) * B
        if out is None:
            out = torch.empty((need,), dtype=torch.float32)
        assert out.dtype == torch.float32 and out.dim() == 1 and out.numel() >= need
        rd, u, rc = step_uniforms_ref(seeds, step, stage, K_draft, K_accept)
        out[:need] = float("nan")                                         # what the kernel skips is not a uniform
        v_rd = v_u = v_rc = None
        if K_draft > 0:
            v_rd = out[:K_draft * B].view(K_draft, B)
            v_rd.copy_(torch.from_numpy(rd))
        if K_accept > 0:
            v_u = out[K_draft * B:(K_draft + K_accept) * B].view(B, K_accept)
            v_u.copy_(torch.from_numpy(u))
        if commit:
            v_rc = out[(K_draft + K_accept) * B:need]
            v_rc.copy_(torch.from_numpy(rc))
        return v_rd, v_u, v_rc


def check_wiring(log, seeds, stage_index, K):
    """Over the log of one generate call: exactly one step_uniforms call per step, numbered 0, 1, ... with the stage's index,
    and every uniform array handed to a draft_sample*, verify_accept* or residual_sample_lp call between two of them is the
    reference's slot of that step, bit for bit: proposal k of the step takes r_draft[k], the verify u, the commit draw
    r_commit.  K: draft_len of a verifying stage, 0 for stage 0.  -> the number of steps."""
    want_seeds = as_u64(seeds)
    step, k, ref = -1, 0, None
    seen = {"draft": 0, "verify": 0, "residual": 0}
    for e in log:
        n = e["name"]
        if n == "step_uniforms":
            assert ref is None or k == max(K, 1), "a step ended before it made all its proposals"
            step += 1
            assert e["step"] == step and e["stage"] == stage_index and np.array_equal(e["seeds"], want_seeds)
            assert (e["K_draft"], e["K_accept"], e["commit"]) == ((K, K, True) if K else (1, 0, False))
            ref = step_uniforms_ref(want_seeds, step, stage_index, e["K_draft"], e["K_accept"])
            k = 0
        elif n.startswith("draft_sample"):
            assert ref is not None and e["uniform"].tobytes() == ref[0][k].tobytes(), (step, k)
            k += 1
            seen["draft"] += 1
        elif n.startswith("verify_accept"):
            assert e["uniform"].tobytes() == ref[1].tobytes(), step
            seen["verify"] += 1
        elif n == "residual_sample_lp":
            assert e["uniform"].tobytes() == ref[2].tobytes(), step
            seen["residual"] += 1
    steps = step + 1
    assert steps >= 1 and seen["draft"] == steps * max(K, 1)
    assert (seen["verify"], seen["residual"]) == ((steps, steps) if K else (0, 0))
    return steps
