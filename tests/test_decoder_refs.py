"""The checkers of tests/decoder_ref.py have teeth (CPU): a plain f32 restatement of k_attn_ragged's algorithm satisfies the
assertion of every attention case of tests/test_gpu_decoder_edges.py, and each of six single defects of that algorithm -- a
causal mask off by one either way, a dropped key, two exchanged V rows, a missing accumulator rescale, an unscaled merge of the
four streams -- fails at least one case.  That is what makes a pass of the GPU test say something about the kernel."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import decoder_ref as R  # noqa: E402

CASES = R.attn_cases()


def _run(c, defect=None):
    case = R.build_attn_case(c)
    out = R.attn_emulated(case["q"], case["k"], case["v"], case["pos"], case["row_of"], defect=defect)
    return R.attn_violations(out, case)


def test_case_table():
    assert len(CASES) == 20 and len({R.case_id(c) for c in CASES}) == 20
    assert {c.kind for c in CASES} == set(R.KINDS) and sum(1 for c in CASES if c.rows) == len(R.KINDS)
    for c in CASES:
        rep_rows = c.H // c.KVH * c.T
        assert c.t_max == 4096 and rep_rows in (20, 63)
        case = R.build_attn_case(c)
        n_tiles = int(case["pos"].max()) // 32 + 1
        assert c.pos0[0] == 0 or (n_tiles % 4 != 0 and (int(case["pos"].max()) + 1) % 32 != 0)   # ragged last tile
    seen = set()
    for c in CASES:
        if c.kind == "needle":
            case = R.build_attn_case(c)
            seen |= {i for i, n in enumerate(case["count"]) if n > 0}
    assert seen == set(range(len(R.NEEDLES)))                     # every needle is chosen by a row of some case


@pytest.mark.parametrize("c", CASES, ids=R.case_id)
def test_clean_emulation_satisfies_every_case(c):
    bad, worst = _run(c)
    print(f"{R.case_id(c)}: worst |err| / bound {worst:.3f}")
    assert bad == 0, (bad, worst)


@torch.no_grad()
def _chain(lm, ids, pos0, caches, inv_freq):
    """The decoder stack of `lm` as a chain of decoder_ref's single-op references, all f64: ids [B, T] at positions pos0[b] ..
    pos0[b] + T - 1, caches = one (k, v) pair [B, KVH, t_max, 128] per layer, written in place.  Returns (final norm, residual
    stream), both [B * T, hidden]."""
    s = lm.shape
    Bn, T = ids.shape
    M, kv = Bn * T, s.kv_heads * 128
    pos = (pos0[:, None] + torch.arange(T)).reshape(M)
    seq = torch.arange(M) // T
    x = lm.embed.weight[ids.reshape(M)].double()
    for blk, (kc, vc) in zip(lm.blocks, caches):
        hn = R.rmsnorm_ref(x, blk.ln1.weight, s.rms_eps)
        qkv = R.linear_ref(hn, torch.cat([blk.q.weight, blk.k.weight, blk.v.weight]), torch.cat([blk.q.bias, blk.k.bias, blk.v.bias]))
        qkv = qkv.view(M, s.heads + 2 * s.kv_heads, 128)
        q = R.rope_ref(qkv[:, :s.heads], pos, inv_freq)
        kc[seq, :, pos] = R.rope_ref(qkv[:, s.heads:s.heads + s.kv_heads], pos, inv_freq)
        vc[seq, :, pos] = qkv[:, s.heads + s.kv_heads:]
        attn, _ = R.attn_ref(q, kc, vc, pos, seq.tolist())
        x = R.linear_ref(attn.reshape(M, s.hidden), blk.o.weight, None, x)
        hn = R.rmsnorm_ref(x, blk.ln2.weight, s.rms_eps)
        act = R.silu_mul_ref(R.linear_ref(hn, torch.cat([blk.gate.weight, blk.up.weight])))
        x = R.linear_ref(act, blk.down.weight, None, x)
    return R.rmsnorm_ref(x, lm.norm.weight, s.rms_eps), x


def test_reference_chain_has_the_models_wiring():
    """The single-op references, chained, against SyntheticLM's own forward_ragged in f64 on the CPU, with random biases and norm
    weights: a prefill of 7 tokens for 2 sequences, then 3 tokens at ragged positions (sequence 0 rolled back by two).  Agreement
    to 1e-9 of the largest magnitude (both sides are f64 evaluations of the same formulas in other orders: 1e-13 would do; a
    missing residual, a bias on the wrong projection, the (i, i + 1) rope pairing or a wrong GQA head mapping are errors of order
    one) -- so what tests/test_gpu_decoder_widths.py leans on has the model's wiring, and randomize_affine's values reach it."""
    from importlib import import_module
    SL = import_module("adaptive-speculative-decoding_amd.serving.synthetic_lm")
    shape = SL.LMShape("chain", 256, 2, 2, 1, 512, vocab=100, rope_theta=1.0e6)
    lm = SL.SyntheticLM(shape, dtype=R.BF, device="cpu", seed=3)
    plain = [p.clone() for p in lm.parameters()]
    R.randomize_affine(lm, 11)
    twin = SL.SyntheticLM(shape, dtype=R.BF, device="cpu", seed=3)
    R.randomize_affine(twin, 11)
    n_changed = 0
    for (name, p), q, before in zip(lm.named_parameters(), twin.parameters(), plain):
        assert torch.equal(p, q) and p.dtype == R.BF                    # one seed, one set of values, in the model's dtype
        assert torch.equal(p, before) == (p.dim() == 2), name           # matrices untouched, every bias and norm weight moved
        if p.dim() == 1:
            n_changed += 1
            z = p.detach().float() - (0.0 if name.endswith(".bias") else 1.0)
            sd = 1.0 if name.endswith(".bias") else 0.25
            assert abs(float(z.mean())) < 0.3 * sd and 0.7 * sd < float(z.std()) < 1.3 * sd, name        # >= 128 draws each
    assert n_changed == 2 * (2 + 3) + 1                                  # per layer: ln1, ln2, three biases; the final norm
    lm = lm.double()
    t_max = 32
    lm.alloc_ragged(2, t_max)
    inv_freq = 1.0 / (shape.rope_theta ** (torch.arange(0, 128, 2, dtype=torch.float32) / 128))
    caches = [(torch.zeros(2, 1, t_max, 128, dtype=torch.float64), torch.zeros(2, 1, t_max, 128, dtype=torch.float64)) for _ in range(2)]
    g = torch.Generator().manual_seed(5)
    for T, pos0 in ((7, torch.tensor([0, 0])), (3, torch.tensor([5, 7]))):
        ids = torch.randint(0, shape.vocab, (2, T), generator=g)
        want = lm.forward_ragged(ids, pos0, int(pos0.max()) + T, return_hidden=True).view(2 * T, shape.hidden)
        got, _ = _chain(lm, ids, pos0, caches, inv_freq)
        assert want.dtype == torch.float64 and got.dtype == torch.float64
        err, scale = float((got - want).abs().max()), float(want.abs().max())
        print(f"T = {T}, pos0 = {pos0.tolist()}: max |chain - model| = {err:.3e} at scale {scale:.3f}")
        assert err <= 1e-9 * scale
        for (kc, vc), (kb, vb) in zip(caches, lm._ragged):
            assert float((kc - kb).abs().max()) <= 1e-9 * float(kb.abs().max())
            assert float((vc - vb).abs().max()) <= 1e-9 * float(vb.abs().max())


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_each_defect_fails_a_case(defect):
    caught = []
    for c in CASES:
        bad, worst = _run(c, defect)
        if bad:
            caught.append((R.case_id(c), bad, round(worst, 2)))
    print(f"{defect}: caught by {len(caught)} of {len(CASES)} cases: {caught}")
    assert caught
