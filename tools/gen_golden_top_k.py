"""Writes tests/golden/speculative_sampling_top_k.npz: transformers' speculative sampling with top-k before top-p on both score sets.

    python tools/gen_golden_top_k.py

The reference calls generate(do_sample=True, temperature=0.7, top_p=0.9) and passes no top_k (src/training/
generate_training_data.py:110-119), so transformers applies its default top_k = 50: the warper chain is
TemperatureLogitsWarper -> TopKLogitsWarper -> TopPLogitsWarper, on the candidate scores and on the target scores before
`_speculative_sampling`.  The rows are those of oracle/gen_golden.py::spec_full_rows (V = 152064, bf16 / f16 storage,
K = 4 / 8; regenerated from (seed, case) by tests/helpers.py::spec_full_cases).  Two settings: (top_k, top_p) = (50, 0.9), the
reference's effective call, and (20, 0.8), where a small k binds more often.  The warpers of the installed transformers and
`_speculative_sampling` are called unmodified, its uniforms supplied and its multinomial input recorded.

Stored: seeds and results only -- drafted tokens, log q, per-row x_k and kept-set sizes, the combined thresholds (draft rows and
the K + 1 target rows), n_matches, residual tokens -- and, per case, what the SAME drafts and uniforms give under top-p alone
(n_matches_top_p, the target rows' top-p-only kept-set sizes): the pinning test asserts that the top-p-only entry points
disagree with these results."""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.gen_golden import spec_full_rows  # noqa: E402  (the row recipe tests/helpers.py::spec_full_cases regenerates)

OUT = os.path.join(ROOT, "tests", "golden", "speculative_sampling_top_k.npz")
SEED = 20261017
SETTINGS = ((50, 0.9), (20, 0.8))


def _spec(ids, u, cand_w, new_w, K):
    """transformers' _speculative_sampling, unmodified, with its uniforms supplied -> (n_matches, residual distribution)."""
    import transformers.generation.utils as U
    got = {}
    real_rand_like, real_multinomial = torch.rand_like, torch.multinomial

    def fake_rand_like(t, *a, **k):
        return torch.from_numpy(u.copy()).to(t.dtype).reshape(t.shape)

    def fake_multinomial(p, num_samples=1, **k):
        got["p"] = p.detach().clone()
        return torch.zeros((p.shape[0], num_samples), dtype=torch.long)

    torch.rand_like, torch.multinomial = fake_rand_like, fake_multinomial
    try:
        _, n = U._speculative_sampling(torch.from_numpy(ids)[None, :], cand_w[None], K, new_w[None], False)
    finally:
        torch.rand_like, torch.multinomial = real_rand_like, real_multinomial
    return int(n), got["p"][0].double().numpy()


def main():
    from transformers.generation.logits_process import TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper
    V, T = 152064, 0.7
    cases = []
    c = 0
    for (top_k, top_p) in SETTINGS:
        for storage in ("bf16", "f16"):
            for K in (4, 8):
                for scale, spread in ((3.0, 0.5), (2.0, 0.1)):
                    cases.append((c, K, scale, spread, storage, top_k, top_p))
                    c += 1
    rec = dict(case=[], K=[], scale=[], spread=[], storage=[], top_k=[], top_p=[], off=[0], u=[], ids=[], lq=[], thr=[], x_k=[],
               n_keep=[], ties_removed=[], t_ties_removed=[], pick_margin=[], n_matches=[], n_matches_top_p=[], r=[], tok=[], margin=[], t_thr=[], t_x_k=[], t_n_keep=[],
               t_n_keep_top_p=[])
    rng = np.random.default_rng(SEED)

    for (case, K, scale, spread, storage, top_k, top_p) in cases:
        cand, new, pick = spec_full_rows(SEED, case, K, V, scale, spread, storage)

        def warp(x, with_k=True):
            s = TemperatureLogitsWarper(T)(None, torch.from_numpy(x.copy()))
            if with_k:
                s = TopKLogitsWarper(top_k)(None, s)
            return TopPLogitsWarper(top_p)(None, s)

        cand_w, new_w = warp(cand), warp(new)
        keep = torch.isfinite(cand_w).numpy()
        thr = np.array([cand[k][keep[k]].min() for k in range(K)], np.float32)
        x_k = np.array([np.sort(cand[k])[::-1][top_k - 1] for k in range(K)], np.float32)
        lq_all = torch.log_softmax(cand_w.double(), dim=-1).numpy()
        ids = np.empty(K, np.int64)
        pm = np.empty(K)
        for k in range(K):
            q = np.exp(lq_all[k])
            cum = np.cumsum(q)
            target = float(pick[k]) * cum[-1]
            t = int(np.searchsorted(cum, target, side="right"))
            while t < V - 1 and q[t] <= 0.0:
                t += 1
            ids[k] = min(t, V - 1)
            lo = cum[ids[k] - 1] if ids[k] > 0 else 0.0
            pm[k] = min(target - lo, cum[ids[k]] - target) / cum[-1]
        lq = lq_all[np.arange(K), ids]
        lp = torch.log_softmax(new_w[:K].double(), dim=-1).numpy()[np.arange(K), ids]      # -inf outside the target's kept set
        ratio = lp - lq
        u = rng.uniform(0, 1, K)
        for _ in range(100):
            with np.errstate(invalid="ignore"):
                bad = np.abs(np.log(u) - ratio) < 1e-3
            if not bad.any():
                break
            u[bad] = rng.uniform(0, 1, int(bad.sum()))
        u = u.astype(np.float32)
        n, pp = _spec(ids, u, cand_w, new_w, K)
        # the same drafts and uniforms when both score sets are warped by top-p alone (what the top-p-only path computes)
        cand_p, new_p = warp(cand, False), warp(new, False)
        n_p, _ = _spec(ids, u, cand_p, new_p, K)
        cum = np.cumsum(pp)
        total = cum[-1]
        for r in rng.uniform(0, 1, 3).astype(np.float32):
            target = float(r) * total
            t = int(np.searchsorted(cum, target, side="right"))
            while t < V - 1 and pp[t] <= 0.0:
                t += 1
            t = min(t, V - 1)
            lo = cum[t - 1] if t > 0 else 0.0
            rec["r"].append(r)
            rec["tok"].append(t)
            rec["margin"].append(min(target - lo, cum[t] - target) / total)
        rec["case"].append(case); rec["K"].append(K); rec["scale"].append(scale); rec["spread"].append(spread)
        rec["storage"].append(storage); rec["top_k"].append(top_k); rec["top_p"].append(top_p); rec["off"].append(rec["off"][-1] + K)
        rec["u"].append(u); rec["ids"].append(ids.astype(np.int32)); rec["lq"].append(lq); rec["thr"].append(thr); rec["x_k"].append(x_k)
        rec["n_keep"].append(keep.sum(1).astype(np.int32)); rec["pick_margin"].append(pm)
        # scores EQUAL to the threshold that the top-p warper's sort dropped (the kernels keep every tie by contract)
        rec["ties_removed"].append(np.array([int(((cand[k] == thr[k]) & ~keep[k]).sum()) for k in range(K)], np.int32))
        rec["n_matches"].append(n); rec["n_matches_top_p"].append(n_p)
        tkeep = torch.isfinite(new_w).numpy()
        tthr = np.array([new[k][tkeep[k]].min() for k in range(K + 1)], np.float32)
        rec["t_thr"].append(tthr)
        rec["t_ties_removed"].append(np.array([int(((new[k] == tthr[k]) & ~tkeep[k]).sum()) for k in range(K + 1)], np.int32))
        rec["t_x_k"].append(np.array([np.sort(new[k])[::-1][top_k - 1] for k in range(K + 1)], np.float32))
        rec["t_n_keep"].append(tkeep.sum(1).astype(np.int32))
        rec["t_n_keep_top_p"].append(torch.isfinite(new_p).numpy().sum(1).astype(np.int32))
        print(f"  case {case}: {storage} K={K} scale={scale} spread={spread} top_k={top_k} top_p={top_p} n_matches {n} "
              f"(top-p only {n_p}) target kept {tkeep.sum(1).tolist()} (top-p only {rec['t_n_keep_top_p'][-1].tolist()})")
    i32 = lambda k: np.concatenate(rec[k]).astype(np.int32)          # noqa: E731
    f32 = lambda k: np.concatenate(rec[k]).astype(np.float32)        # noqa: E731
    np.savez_compressed(OUT, seed=np.int64(SEED), V=np.int32(V), T=np.float32(T), top_p=np.float32(SETTINGS[0][1]),
                        case=np.array(rec["case"], np.int32), K=np.array(rec["K"], np.int32),
                        scale=np.array(rec["scale"], np.float32), spread=np.array(rec["spread"], np.float32),
                        storage=np.array(rec["storage"]), case_top_k=np.array(rec["top_k"], np.int32),
                        case_top_p=np.array(rec["top_p"], np.float32), off=np.array(rec["off"], np.int64),
                        u=f32("u"), ids=i32("ids"), lq=np.concatenate(rec["lq"]).astype(np.float64), thr=f32("thr"), x_k=f32("x_k"),
                        n_keep=i32("n_keep"), ties_removed=i32("ties_removed"), t_ties_removed=i32("t_ties_removed"),
                        pick_margin=np.concatenate(rec["pick_margin"]).astype(np.float64),
                        n_matches=np.array(rec["n_matches"], np.int32), n_matches_top_p=np.array(rec["n_matches_top_p"], np.int32),
                        r=np.array(rec["r"], np.float32).reshape(-1, 3), tok=np.array(rec["tok"], np.int32).reshape(-1, 3),
                        margin=np.array(rec["margin"], np.float64).reshape(-1, 3),
                        t_thr=f32("t_thr"), t_x_k=f32("t_x_k"), t_n_keep=i32("t_n_keep"), t_n_keep_top_p=i32("t_n_keep_top_p"),
                        t_off=np.cumsum([0] + [k + 1 for k in rec["K"]]).astype(np.int64))
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
