"""Top-k before top-p in the hierarchy loop on CPU (HierarchyConfig.top_k / target_top_k): HF's generate(do_sample=True, ...)
applies TopKLogitsWarper(50) before TopPLogitsWarper unless told otherwise, on the draft's scores and -- in assisted
generation -- on the target's.

The arithmetic is the oracle's through the masked-row recipe: x_k of a row is numpy's k-th largest (np.partition on the f32
view), the combined threshold is max(x_k, O.draft_sample(row masked below x_k).thr), and O.draft_sample / O.verify_accept /
O.residual_sample on rows stored with -inf below that threshold return exactly the top-k + top-p draw, lp_t and commit."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import oracle as O  # noqa: E402
from tests.oracle_backend import OracleOps, _np_store  # noqa: E402
from tests.test_target_top_p import (K, NEW, P, V, NucleusOracleOps, _leading_finite, _masked_tensor, _model,  # noqa: E402
                                     _predictor, _run)

TOP_K, TOP_P = 20, 0.9


def x_k_of(rows_f32, top_k):
    """The top_k-th largest value of every row counting multiplicity; -inf where fewer than top_k values are > -inf."""
    rows = np.asarray(rows_f32, np.float32)
    Vr = rows.shape[-1]
    if top_k <= 0 or top_k >= Vr:
        return np.full(rows.shape[0], -np.inf, np.float32)
    kth = np.partition(rows, Vr - top_k, axis=-1)[:, Vr - top_k]
    return np.where((rows > -np.inf).sum(-1) >= top_k, kth, -np.inf).astype(np.float32)


def top_k_thresholds(t, inv_temperature, top_k, top_p):
    """thr = max(x_k, x*_K) of every row of t [..., V]: x*_K is the oracle's nucleus threshold of the row masked below x_k."""
    store, dt = _np_store(t)
    rows = store.reshape(-1, store.shape[-1])
    R, Vr = rows.shape
    x_k = x_k_of(O.logits_as_f32(rows, dt), top_k)
    if not 0.0 < top_p < 1.0:
        return x_k
    masked, _ = _np_store(_masked_tensor(t.reshape(R, Vr), x_k))
    thr_p = O.draft_sample(masked, dt, np.full(R, 0.5, np.float32), R, Vr, inv_temperature, top_p)["thr"]
    return np.maximum(x_k, thr_p).astype(np.float32)


class TopKOracleOps(NucleusOracleOps):
    """NucleusOracleOps with the top-k entry points of distributed.HipOps, by the masked-row recipe."""

    def __init__(self):
        super().__init__()
        self.calls = {"draft": 0, "verify": 0, "residual": 0}

    def draft_sample_top_k(self, logits, r, inv_temperature=1.0, top_k=0, top_p=1.0):
        self.calls["draft"] += 1
        thr = top_k_thresholds(logits, inv_temperature, top_k, top_p)
        tok, lp, _ = self.draft_sample(_masked_tensor(logits, thr), r, inv_temperature, 1.0)
        return tok, lp, torch.from_numpy(thr)

    def verify_accept_top_k(self, logits, tok, lp_d, u, inv_temperature=1.0, top_k=0, top_p=1.0):
        self.calls["verify"] += 1
        Bv, Kv, Vv = logits.shape
        thr = top_k_thresholds(logits, inv_temperature, top_k, top_p)
        lp_t, acc, n_acc, bits = self.verify_accept(_masked_tensor(logits, thr), tok, lp_d, u, inv_temperature)
        return (lp_t, acc, n_acc, bits, torch.from_numpy(thr.reshape(Bv, Kv).copy()),
                torch.from_numpy(_leading_finite(lp_t.numpy())))

    def residual_sample_top_k(self, t_logits, d_logits, n_acc, r, bonus, inv_temperature=1.0, d_threshold=None,
                              t_threshold=None, top_k=0, top_p=1.0):
        self.calls["residual"] += 1
        b_thr = top_k_thresholds(bonus, inv_temperature, top_k, top_p)
        t_logits = _masked_tensor(t_logits, t_threshold.numpy())
        bonus = _masked_tensor(bonus, b_thr)
        tok = OracleOps.residual_sample(self, t_logits, d_logits, n_acc, r, bonus, inv_temperature, d_threshold)
        self.draws.append((t_logits.clone(), bonus.clone(), n_acc.clone(), tok.clone()))
        return tok


def test_x_k_keeps_ties_and_short_rows():
    x = np.array([[3.0, 1.0, 3.0, 2.0, 2.0, -np.inf], [1.0, -np.inf, -np.inf, -np.inf, -np.inf, -np.inf]], np.float32)
    assert x_k_of(x, 2).tolist() == [3.0, -np.inf]
    assert x_k_of(x, 3).tolist() == [2.0, -np.inf]
    assert ((x >= x_k_of(x, 3)[:, None]).sum(1) == [4, 6]).all()     # every tie at x_k is kept; a short row is kept whole


def test_defaults_are_off():
    from asd_amd.serving import hierarchy as H
    from asd_amd.serving.speculative import SpeculativeVerifier
    cfg = H.HierarchyConfig()
    assert cfg.top_k == 0 and cfg.target_top_k == 0
    names = SpeculativeVerifier.__init__.__code__.co_names            # (constructing one needs a GPU)
    assert "top_k" in names and "target_top_k" in names


def test_hierarchy_commits_from_the_top_k_set():
    ops = TopKOracleOps()
    tr, ts = _run(ops, top_k=TOP_K, target_top_k=TOP_K, target_top_p=TOP_P)
    assert (tr.seq_len == P + NEW).all()
    assert ops.calls["draft"] > 0 and ops.calls["verify"] > 0 and ops.calls["residual"] > 0
    inv_t = float(np.float32(1.0 / 0.7))
    checked = accepted = 0
    for rec in tr.records:
        for s, (v, drawn) in rec["tiers"].items():
            inp = v.inputs
            lp_t, n_acc = inp["lp_t"].numpy(), inp["n_acc"].numpy()
            thr = inp["t_nucleus_logit"].numpy()
            logits = inp["logits"].float().numpy()
            want = top_k_thresholds(inp["logits"], inv_t, TOP_K, TOP_P).reshape(thr.shape)
            assert thr.tobytes() == want.tobytes()
            # the kept set is at most top_k tokens plus the ties at x_k
            x_k = x_k_of(logits.reshape(-1, V), TOP_K).reshape(thr.shape)
            assert (thr >= x_k).all()
            assert ((logits >= thr[..., None]).sum(-1) <= ((logits >= x_k[..., None]).sum(-1))).all()
            tok = inp["tok"].numpy()
            inside = np.take_along_axis(logits, tok[..., None].astype(np.int64), 2)[..., 0] >= thr
            assert (np.isfinite(lp_t) == inside).all()
            assert (n_acc <= inp["n_finite"].numpy()).all()
            accepted += int(n_acc.sum())
            stop = v.stop.numpy()[v.idx.numpy()] == 1
            for i in np.nonzero(stop)[0]:
                b, j = int(v.idx[i]), int(n_acc[i])
                row = logits[i, j] if j < K else inp["bonus_logits"][i].float().numpy()
                bound = thr[i, j] if j < K else top_k_thresholds(inp["bonus_logits"][i:i + 1], inv_t, TOP_K, TOP_P)[0]
                assert row[int(drawn[b])] >= bound, (s, b, j)
                checked += 1
    assert checked > 10 and accepted > 0


def test_top_k_zero_leaves_the_committed_stream_unchanged():
    ops = TopKOracleOps()
    a, _ = _run(OracleOps(), keep=False)
    b, _ = _run(ops, keep=False, top_k=0, target_top_k=0)
    assert torch.equal(a.tokens, b.tokens) and a.tier_counts == b.tier_counts
    assert ops.calls == {"draft": 0, "verify": 0, "residual": 0}       # the top-k entry points are not called at all
    c, _ = _run(TopKOracleOps(), keep=False, top_k=TOP_K, target_top_k=TOP_K, target_top_p=TOP_P)
    d, _ = _run(NucleusOracleOps(), keep=False, target_top_p=TOP_P)
    assert not torch.equal(c.tokens, d.tokens)           # the setting is live: top-k changes what is committed


def test_fused_head_with_target_top_k_takes_the_logits_route():
    from asd_amd.serving import hierarchy as H
    a, _ = _run(TopKOracleOps(), keep=False, target_top_k=TOP_K)
    b, ts = _run(TopKOracleOps(), heads=("fused", "fused"), keep=False, target_top_k=TOP_K)
    assert all(isinstance(t.head, H.LogitsHead) for t in ts)
    assert torch.equal(a.tokens, b.tokens)


def test_sharded_head_and_target_refuse_target_top_k():
    from asd_amd.serving import hierarchy as H
    cfg = H.HierarchyConfig(draft_len=K, target_top_k=50)
    head = H.ShardedHead.__new__(H.ShardedHead)            # (no process group is needed to be refused)
    prompt = torch.zeros((2, P), dtype=torch.int64)
    with pytest.raises(ValueError, match="target_top_k"):
        H.VerifyRole(_model(0, 0), 1, cfg, OracleOps(), prompt, NEW, _predictor(), head=head)
    with pytest.raises(ValueError, match="target_top_k"):
        H.ShardedTargetRole(_model(0, 0), cfg, OracleOps(), prompt, NEW, _predictor(), head, 0, 2)
