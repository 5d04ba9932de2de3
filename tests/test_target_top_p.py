"""Target-side top-p in the hierarchy loop on CPU (HierarchyConfig.target_top_p): the verifying tiers score and commit against
the target's nucleus p^N, as HF's assisted generation warps the target's scores too (generate_training_data.py:110-119).

The arithmetic is the oracle's (tests/oracle_backend.py: OracleOps) through the masked-row recipe: x* of a row is
O.draft_sample's threshold, and O.verify_accept / O.residual_sample on rows stored with -inf below x* return exactly the
nucleus lp_t and the nucleus residual / bonus draw."""
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

V, B, P, NEW, K = 1000, 6, 5, 24, 4
LAM_MIX = 25.0
TOP_P_T = 0.9
NEG_INF_STORE = {O.DT_F32: np.float32(-np.inf), O.DT_BF16: np.uint16(0xFF80), O.DT_F16: np.uint16(0xFC00)}


def _masked_tensor(t, thr):
    """t [..., V] with every entry below its row's threshold set to -inf (in t's storage dtype)."""
    store, dt = _np_store(t)
    shape = store.shape
    rows = store.reshape(-1, shape[-1]).copy()
    below = O.logits_as_f32(rows, dt) < np.asarray(thr, np.float32).reshape(-1, 1)
    rows[below] = NEG_INF_STORE[dt]
    rows = rows.reshape(shape)
    if dt == O.DT_F32:
        return torch.from_numpy(rows)
    return torch.from_numpy(rows.view(np.int16)).view(torch.bfloat16 if dt == O.DT_BF16 else torch.float16)


def _thresholds(t, inv_temperature, top_p):
    store, dt = _np_store(t)
    rows = store.reshape(-1, store.shape[-1])
    R = rows.shape[0]
    return O.draft_sample(rows, dt, np.full(R, 0.5, np.float32), R, rows.shape[1], inv_temperature, top_p)["thr"]


def _leading_finite(lp):
    fin = np.isfinite(lp)
    return np.where(fin.all(axis=1), lp.shape[1], np.argmin(fin, axis=1)).astype(np.int32)


class NucleusOracleOps(OracleOps):
    """OracleOps with the target-nucleus entry points of distributed.HipOps, by the masked-row recipe; records every draw."""

    def __init__(self):
        super().__init__()
        self.draws = []

    def verify_accept_top_p(self, logits, tok, lp_d, u, inv_temperature=1.0, top_p=1.0):
        Bv, Kv, Vv = logits.shape
        if 0.0 < top_p < 1.0:
            thr = _thresholds(logits, inv_temperature, top_p)
            logits = _masked_tensor(logits, thr)
        else:
            thr = np.full(Bv * Kv, -np.inf, np.float32)
        lp_t, acc, n_acc, bits = self.verify_accept(logits, tok, lp_d, u, inv_temperature)
        return (lp_t, acc, n_acc, bits, torch.from_numpy(thr.reshape(Bv, Kv).copy()),
                torch.from_numpy(_leading_finite(lp_t.numpy())))

    def residual_sample(self, t_logits, d_logits, n_acc, r, bonus, inv_temperature=1.0, d_threshold=None, t_threshold=None,
                        top_p=1.0):
        if 0.0 < top_p < 1.0:
            b_thr = _thresholds(bonus, inv_temperature, top_p)
            t_logits = _masked_tensor(t_logits, t_threshold.numpy())
            bonus = _masked_tensor(bonus, b_thr)
            tok = super().residual_sample(t_logits, d_logits, n_acc, r, bonus, inv_temperature, d_threshold)
            self.draws.append((t_logits.clone(), bonus.clone(), n_acc.clone(), tok.clone()))
            return tok
        return super().residual_sample(t_logits, d_logits, n_acc, r, bonus, inv_temperature, d_threshold)

    def predictor_stop(self, pred, lp, feat, p_hist, stage_idx, costs, lam, risk_adjustment=True, n_obs=100, alpha=1.0,
                       beta=1.0, stats_col=5, n_valid=None):
        if n_valid is None:
            return super().predictor_stop(pred, lp, feat, p_hist, stage_idx, costs, lam, risk_adjustment, n_obs, alpha, beta,
                                          stats_col)
        # asd_predictor_stop with n_valid: the statistics of the leading n_valid[b] log-probs only
        w1, b1, w2, b2 = pred
        lpn = np.asarray(lp.numpy(), dtype=np.float32)
        x = np.array(feat.numpy(), dtype=np.float32, copy=True)
        stats = O.logprob_stats(lpn, n_valid.numpy().astype(np.int32), K=lpn.shape[1])
        if stats_col >= 0:
            x[:, stats_col:stats_col + 5] = stats.astype(np.float32)
        score = O.mlp_predict(x, w1, b1, np.asarray(w2).reshape(-1), b2)
        p = score.astype(np.float64)
        if risk_adjustment:
            p = O.bayes_adjust(p, n_obs, alpha, beta)
        hist = p_hist.numpy().copy()
        hist[:, stage_idx] = p
        k_star, _ = O.optimal_stopping(hist, np.asarray(costs.numpy(), dtype=np.float64), float(lam))
        p_hist.copy_(torch.from_numpy(hist))
        return torch.from_numpy(score), torch.from_numpy(k_star), p_hist


def _model(noise, seed):
    from asd_amd.serving.synthetic_lm import SyntheticLM, tiny
    m = SyntheticLM(tiny(vocab=V), dtype=torch.float32, device="cpu", seed=1, logit_scale=4.0)
    if noise:
        g = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            m.lm_head.weight.add_(torch.randn(m.lm_head.weight.shape, generator=g) * noise)
    return m


def _predictor():
    from asd_amd.minimal_adaptive_decoder import MinimalQualityPredictor
    torch.manual_seed(0)
    pred = MinimalQualityPredictor().eval()
    with torch.no_grad():
        for p in pred.parameters():
            p.mul_(3.0)
    return pred


def _run(ops, heads=("logits", "logits"), keep=True, **cfg_kw):
    from asd_amd.serving import hierarchy as H
    cfg = H.HierarchyConfig(draft_len=K, temperature=0.7, top_p=0.9, lambda_value=LAM_MIX, seed=3, **cfg_kw)
    pred = _predictor()
    prompt = torch.randint(0, V, (B, P), generator=torch.Generator().manual_seed(7))
    d = H.DraftRole(_model(0, 0), cfg, ops, prompt, NEW, pred)
    ts = []
    for s, (noise, seed, hd) in enumerate(zip((0.02, 0.04), (5, 6), heads), start=1):
        m = _model(noise, seed)
        head = H.FusedHead(m, ops) if hd == "fused" else H.LogitsHead(m, ops)
        ts.append(H.VerifyRole(m, s, cfg, ops, prompt, NEW, pred, head=head, keep_inputs=keep))
    return H.generate_hierarchical(d, ts, keep_inputs=keep), ts


def test_hierarchy_commits_from_the_target_nucleus():
    ops = NucleusOracleOps()
    tr, ts = _run(ops, target_top_p=TOP_P_T)
    assert (tr.seq_len == P + NEW).all()
    inv_t = float(np.float32(1.0 / 0.7))
    checked = accepted = 0
    saw_out_of_nucleus_draft = False
    for rec in tr.records:
        for s, (v, drawn) in rec["tiers"].items():
            inp = v.inputs
            lp_t, n_acc = inp["lp_t"].numpy(), inp["n_acc"].numpy()
            thr = inp["t_nucleus_logit"].numpy()
            logits = inp["logits"].float().numpy()
            # x* is the draft sampler's select on each verified row; lp_t is finite exactly inside the nucleus
            want_thr = _thresholds(inp["logits"], inv_t, TOP_P_T).reshape(thr.shape)
            assert thr.tobytes() == want_thr.tobytes()
            tok = inp["tok"].numpy()
            inside = np.take_along_axis(logits, tok[..., None].astype(np.int64), 2)[..., 0] >= thr
            assert (np.isfinite(lp_t) == inside).all()
            saw_out_of_nucleus_draft |= bool((~inside).any())
            assert (inp["n_finite"].numpy() == _leading_finite(lp_t)).all()
            assert (n_acc <= inp["n_finite"].numpy()).all()      # an accepted token is inside the nucleus
            accepted += int(n_acc.sum())
            # every token this tier COMMITS by a draw lies in the nucleus of its row
            stop = v.stop.numpy()[v.idx.numpy()] == 1
            for i in np.nonzero(stop)[0]:
                b, j = int(v.idx[i]), int(n_acc[i])
                row = logits[i, j] if j < K else inp["bonus_logits"][i].float().numpy()
                x_star = thr[i, j] if j < K else _thresholds(inp["bonus_logits"][i:i + 1], inv_t, TOP_P_T)[0]
                assert row[int(drawn[b])] >= x_star, (s, b, j)
                checked += 1
    assert checked > 10 and accepted > 0 and ops.draws
    assert saw_out_of_nucleus_draft                       # the nucleus made a difference somewhere


def test_target_top_p_one_leaves_the_committed_stream_unchanged():
    a, _ = _run(OracleOps(), keep=False)
    b, _ = _run(OracleOps(), keep=False, target_top_p=1.0)
    assert torch.equal(a.tokens, b.tokens) and a.tier_counts == b.tier_counts


def test_default_config_keeps_the_full_softmax():
    from asd_amd.serving import hierarchy as H
    assert H.HierarchyConfig().target_top_p == 1.0
    a, _ = _run(NucleusOracleOps(), keep=False, target_top_p=TOP_P_T)
    b, _ = _run(OracleOps(), keep=False, target_top_p=1.0)
    assert not torch.equal(a.tokens, b.tokens)           # the setting is live: the nucleus changes what is committed


def test_fused_head_with_target_top_p_takes_the_logits_route():
    a, _ = _run(NucleusOracleOps(), keep=False, target_top_p=TOP_P_T)
    b, ts = _run(NucleusOracleOps(), heads=("fused", "fused"), keep=False, target_top_p=TOP_P_T)
    from asd_amd.serving import hierarchy as H
    assert all(isinstance(t.head, H.LogitsHead) for t in ts)
    assert torch.equal(a.tokens, b.tokens)


def test_sharded_target_refuses_target_top_p():
    from asd_amd.serving import hierarchy as H
    cfg = H.HierarchyConfig(draft_len=K, target_top_p=TOP_P_T)
    head = H.ShardedHead.__new__(H.ShardedHead)            # (no process group is needed to be refused)
    prompt = torch.zeros((2, P), dtype=torch.int64)
    with pytest.raises(ValueError, match="target_top_p"):
        H.VerifyRole(_model(0, 0), 1, cfg, OracleOps(), prompt, NEW, _predictor(), head=head)
    with pytest.raises(ValueError, match="target_top_p"):
        H.ShardedTargetRole(_model(0, 0), cfg, OracleOps(), prompt, NEW, _predictor(), head, 0, 2)
