"""Writes tests/golden/speculative_sampling_target_top_p.npz: transformers' speculative sampling with the TARGET warped too.

    python tools/gen_golden_target_top_p.py

HF's assisted generation runs the same logits processors on the candidate scores and on the target scores before
`_speculative_sampling`; the reference asks for T = 0.7, top_p = 0.9 on every model (src/training/generate_training_data.py:
110-119, src/serving/real_model_pipeline.py:60,326,378).  The cases are those of oracle/gen_golden.py::gen_speculative_sampling_full
(V = 152064, bf16 / f16 storage, K = 4 / 8; rows regenerated from (seed, case) by tests/helpers.py::spec_full_cases), but here
BOTH score sets go through TemperatureLogitsWarper(0.7) + TopPLogitsWarper(0.9) -- the classes of the installed transformers,
called unmodified -- and `_speculative_sampling` is called unmodified with its uniforms supplied and its multinomial input
recorded.  Stored: seeds and results only (the fields of speculative_sampling_full.npz, plus the target rows' nucleus
thresholds t_thr / t_ties_removed, K + 1 per case from t_off)."""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.gen_golden import spec_full_rows  # noqa: E402  (the row recipe tests/helpers.py::spec_full_cases regenerates)

OUT = os.path.join(ROOT, "tests", "golden", "speculative_sampling_target_top_p.npz")
SEED = 20261016


def main():
    import transformers.generation.utils as U
    from transformers.generation.logits_process import TemperatureLogitsWarper, TopPLogitsWarper
    V, T, TOP_P = 152064, 0.7, 0.9
    cases = []
    c = 0
    for storage in ("bf16", "f16"):
        for K in (4, 8):
            for scale, spread in ((3.0, 0.5), (4.0, 1.5), (2.0, 0.1), (6.0, 1.0)):
                cases.append((c, K, scale, spread, storage))
                c += 1
    rec = dict(case=[], K=[], scale=[], spread=[], storage=[], off=[0], u=[], ids=[], lq=[], thr=[], n_keep=[], ties_removed=[],
               pick_margin=[], n_matches=[], r=[], tok=[], margin=[], t_thr=[], t_ties_removed=[])
    rng = np.random.default_rng(SEED)
    real_rand_like, real_multinomial = torch.rand_like, torch.multinomial

    def warp(x):
        return TopPLogitsWarper(TOP_P)(None, TemperatureLogitsWarper(T)(None, torch.from_numpy(x.copy())))

    for (case, K, scale, spread, storage) in cases:
        cand, new, pick = spec_full_rows(SEED, case, K, V, scale, spread, storage)
        cand_w, new_w = warp(cand), warp(new)
        keep = torch.isfinite(cand_w).numpy()
        thr = np.array([cand[k][keep[k]].min() for k in range(K)], np.float32)
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
        lp = torch.log_softmax(new_w[:K].double(), dim=-1).numpy()[np.arange(K), ids]      # -inf outside the target's nucleus
        ratio = lp - lq
        u = rng.uniform(0, 1, K)
        for _ in range(100):
            with np.errstate(invalid="ignore"):
                bad = np.abs(np.log(u) - ratio) < 1e-3
            if not bad.any():
                break
            u[bad] = rng.uniform(0, 1, int(bad.sum()))
        u = u.astype(np.float32)
        got = {}

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
        n = int(n)
        pp = got["p"][0].double().numpy()
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
        rec["storage"].append(storage); rec["off"].append(rec["off"][-1] + K)
        rec["u"].append(u); rec["ids"].append(ids.astype(np.int32)); rec["lq"].append(lq); rec["thr"].append(thr)
        rec["n_keep"].append(keep.sum(1).astype(np.int32)); rec["pick_margin"].append(pm); rec["n_matches"].append(n)
        rec["ties_removed"].append(np.array([int(((cand[k] == thr[k]) & ~keep[k]).sum()) for k in range(K)], np.int32))
        # the TARGET's nucleus per row (K verified rows + the bonus row), in raw score units, and the ties its sort order dropped:
        # where a kernel's x* differs (top_p within rounding of a cumulative-mass step), the committed token is not compared
        tkeep = torch.isfinite(new_w).numpy()
        tthr = np.array([new[k][tkeep[k]].min() for k in range(K + 1)], np.float32)
        rec["t_thr"].append(tthr)
        rec["t_ties_removed"].append(np.array([int(((new[k] == tthr[k]) & ~tkeep[k]).sum()) for k in range(K + 1)], np.int32))
        print(f"  case {case}: {storage} K={K} scale={scale} spread={spread} n_matches {n} "
              f"target nucleus {torch.isfinite(new_w).sum(1).tolist()}")
    np.savez(OUT, seed=np.int64(SEED), V=np.int32(V), T=np.float32(T),
             top_p=np.float32(TOP_P), case=np.array(rec["case"], np.int32), K=np.array(rec["K"], np.int32),
             scale=np.array(rec["scale"], np.float32), spread=np.array(rec["spread"], np.float32),
             storage=np.array(rec["storage"]), off=np.array(rec["off"], np.int64), u=np.concatenate(rec["u"]).astype(np.float32),
             ids=np.concatenate(rec["ids"]), lq=np.concatenate(rec["lq"]).astype(np.float64),
             thr=np.concatenate(rec["thr"]).astype(np.float32), n_keep=np.concatenate(rec["n_keep"]),
             ties_removed=np.concatenate(rec["ties_removed"]),
             pick_margin=np.concatenate(rec["pick_margin"]).astype(np.float64), n_matches=np.array(rec["n_matches"], np.int32),
             r=np.array(rec["r"], np.float32).reshape(-1, 3), tok=np.array(rec["tok"], np.int32).reshape(-1, 3),
             margin=np.array(rec["margin"], np.float64).reshape(-1, 3),
             t_thr=np.concatenate(rec["t_thr"]).astype(np.float32), t_ties_removed=np.concatenate(rec["t_ties_removed"]),
             t_off=np.cumsum([0] + [k + 1 for k in rec["K"]]).astype(np.int64))
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
