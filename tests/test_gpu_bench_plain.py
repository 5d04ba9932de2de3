"""The plain benchmark line (`bench.py --gpus 1 --steps K --warmup W`) and --dump-outputs: the line holds the headline keys and
nothing measured on the side, and the dumped arrays are what the path computes for the buffer of the last timed step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


@pytest.mark.gpu
def test_plain_line_and_dumped_outputs(tmp_path):
    import torch

    import bench
    from asd_amd import kernels as K

    out_dir = tmp_path / "outputs"
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "MASTER_ADDR")}
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "20", "--warmup", "5", "--dump-outputs", str(out_dir)],
                       capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    assert d["metric"] == "verified_tokens_per_s" and d["unit"] == "tokens/s" and d["higher_is_better"] is True
    assert d["dtype"] == "bf16" and d["steps"] == 20 and d["warmup"] == 5 and d["value"] > 0 and d["ms_per_step"] > 0
    for key in ("roofline", "loop", "cpu_baseline", "sharded_verify"):
        assert key not in d, key

    got = {f[:-4]: np.load(out_dir / f) for f in os.listdir(out_dir)}
    assert sorted(got) == ["accept", "accept_bits", "k_star", "lp_target", "n_acc", "p_hist", "score", "stop"]
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 << 20

    # rebuild the inputs in this process (same seed) and run the same step on the buffer of the last timed step
    B, Kd, V, _ = bench.WORKLOADS["c3"]
    nbuf, G = d["config"]["rotating_buffers"], d["config"]["steps_per_graph"]
    last = (d["warmup"] + (G if d["config"]["launch_mode"] != "eager" else d["steps"]) - 1) % nbuf
    dev = torch.device("cuda", 0)
    ws, bufs = bench.build_inputs(torch, K, B, Kd, V, nbuf, dev, seed=1234)
    buf = bufs[last]
    feat = torch.from_numpy((np.random.default_rng(7).standard_normal((B, 64)) * 0.3).astype(np.float32)).to(dev)
    p_hist = torch.ones((B, bench.N_STAGES), dtype=torch.float64, device=dev)
    v, s = K.verify_accept_fused(buf["logits"], buf["tok"], buf["lp_d"], buf["u"], ws, feat,
                                 K.pack_mlp_weights(*bench.predictor_weights(np), device=dev), 64, 32, stage_idx=0,
                                 L=bench.N_STAGES, stats_col=5, risk_adjustment=True, n_obs=100, p_hist=p_hist,
                                 Cc=torch.tensor(bench.STAGE_COSTS, dtype=torch.float64, device=dev), lam=1.0)
    torch.cuda.synchronize()
    want = {"lp_target": v.lp_target, "accept": v.accept, "n_acc": v.n_acc, "accept_bits": v.accept_bits,
            "score": s.score, "k_star": s.k_star, "stop": s.stop, "p_hist": p_hist}
    for name, t in want.items():
        w = t.cpu().numpy()
        assert got[name].shape == w.shape, name
        assert np.array_equal(got[name], w.astype(got[name].dtype)), name
