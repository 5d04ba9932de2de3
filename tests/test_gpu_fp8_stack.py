"""Weight-only FP8 through the decoder stack and the Stage API: HipDecoder(weights="fp8") equals the composition of its exported
parts bit for bit, frees the bf16 matrices, and StageConfig(quantized=True) generates through it."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BF = torch.bfloat16


def _shape():
    from asd_amd.serving.synthetic_lm import LMShape
    return LMShape("fp8-tiny", 256, 2, 2, 1, 512, vocab=1000, rope_theta=1.0e6)


@pytest.mark.parametrize("Bn,T", [(2, 1), (3, 9)])
def test_fp8_decoder_equals_the_composition_of_its_parts(Bn, T):
    from asd_amd import _binding as Bd
    from asd_amd import kernels as K
    from asd_amd.serving.synthetic_lm import SyntheticLM
    lib, shape, dt = K._lib(), _shape(), Bd.DTYPE_BF16
    lm = SyntheticLM(shape, dtype=BF, device="cuda", seed=6)
    g = torch.Generator(device="cuda").manual_seed(21)
    with torch.no_grad():
        for p in lm.parameters():
            if p.dim() == 1:                                        # norm weights and biases off their 1 / 0 defaults
                p.add_((torch.randn(p.shape, generator=g, device="cuda") * 0.1).to(BF))
    lm.enable_hip_layers(weights="fp8")
    hd = lm._hip
    for blk in lm.blocks:
        assert all(m.weight.numel() == 0 for m in (blk.q, blk.k, blk.v, blk.o, blk.gate, blk.up, blk.down))
    with pytest.raises(RuntimeError):
        lm.enable_hip_layers(False)
    t_max, M, H, kv, I = 64, Bn * T, shape.hidden, shape.kv_heads * 128, shape.intermediate
    lm.alloc_ragged(Bn, t_max)
    ids = torch.randint(0, shape.vocab, (Bn, T), generator=g, device="cuda")
    pos0 = torch.randint(0, t_max - T, (Bn,), generator=g, device="cuda")
    x = lm.embed(ids).view(M, H).clone()
    pos = (pos0[:, None] + torch.arange(T, device="cuda")).reshape(M).to(torch.int32)
    ws = K.LinearWorkspace("cuda")

    def norm(w, out):
        Bd.check("asd_rmsnorm", lib.asd_rmsnorm(x.data_ptr(), H, w.data_ptr(), shape.rms_eps, dt, M, H, out.data_ptr(), H, None))
    for i, blk in enumerate(lm.blocks):
        qkv_i, o_i, gu_i, down_i = hd._images[i]
        kc, vt = torch.zeros_like(hd.k_cache[i]), torch.zeros_like(hd.vt_cache[i])
        hn = torch.empty_like(x)
        norm(blk.ln1.weight, hn)
        qkv = K.linear_fp8(hn, qkv_i, H + 2 * kv, hd._fused[i][1], workspace=ws)
        Bd.check("asd_rope_kv_store", lib.asd_rope_kv_store(qkv.data_ptr(), qkv.stride(0), pos.data_ptr(), None, hd.inv_freq.data_ptr(), dt, Bn, T,
                                                            shape.heads, shape.kv_heads, 128, kc.data_ptr(), vt.data_ptr(), hd.t_max, None))
        attn = torch.empty(M, H, dtype=BF, device="cuda")
        Bd.check("asd_attn_ragged", lib.asd_attn_ragged(qkv.data_ptr(), qkv.stride(0), kc.data_ptr(), vt.data_ptr(), pos.data_ptr(), None, dt, Bn, T,
                                                        shape.heads, shape.kv_heads, 128, hd.t_max, attn.data_ptr(), H, None))
        K.linear_fp8(attn, o_i, H, workspace=ws, out=x, residual=x)
        norm(blk.ln2.weight, hn)
        gu = K.linear_fp8(hn, gu_i, 2 * I, workspace=ws)
        act = torch.empty(M, I, dtype=BF, device="cuda")
        Bd.check("asd_silu_mul", lib.asd_silu_mul(gu.data_ptr(), gu.stride(0), dt, M, I, act.data_ptr(), I, None))
        K.linear_fp8(act, down_i, H, workspace=ws, out=x, residual=x)
    want = torch.empty_like(x)
    norm(lm.norm.weight, want)
    got = lm.forward_ragged(ids, pos0, t_max, return_hidden=True)
    assert bool(torch.isfinite(want.float()).all()) and torch.equal(got.view(M, H), want)


def test_quantized_stage_generates_through_the_fp8_stack():
    from asd_amd.distributed import HipOps
    from asd_amd.serving.stages import StageConfig, StageManager
    from asd_amd.serving.synthetic_lm import tiny
    stage = StageManager([StageConfig(quantized=True, shape=_shape())], ops=HipOps()).get_stage("8b")
    assert stage.model.execution == "hip_decoder"
    info = stage.get_model_info()
    assert info["quantized"] is True and info["weight_dtype"] == "fp8_e4m3"
    for temperature in (0.0, 0.7):
        texts, lps, _ = stage.generate(prompts=["a b c", "d e"], max_tokens=6, temperature=temperature, return_logprobs=True)
        assert all(len(t.split()) == 6 for t in texts)
        got_lp = np.stack(lps)
        assert got_lp.shape == (2, 6) and bool(np.isfinite(got_lp).all())
    with pytest.raises(ValueError, match="quantized"):
        StageManager([StageConfig(quantized=True, shape=tiny())], ops=HipOps())
