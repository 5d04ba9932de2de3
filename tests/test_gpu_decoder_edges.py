"""The decoder-stack kernels (csrc/decoder.hip) where they go wrong: asd_attn_ragged at 4096 keys (128 tiles, 32 per wave, ragged
last tiles, row tiles that mix positions and heads) against assertions without slack for a dropped, duplicated or leaked key;
asd_rope_kv_store at positions up to 32766 in a 32768-slot cache; and KV rollback as an exact statement -- cache entries past a
sequence's committed length contribute exactly nothing.  References, bounds and case builders: tests/decoder_ref.py, whose
assertions tests/test_decoder_refs.py shows to fail six single defects of the attention algorithm."""
import os
import sys
from importlib import import_module

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import decoder_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

BF = torch.bfloat16


def _lib():
    return import_module("adaptive-speculative-decoding_amd.kernels")._lib()


def _B():
    return import_module("adaptive-speculative-decoding_amd._binding")


@pytest.mark.parametrize("c", R.attn_cases(), ids=R.case_id)
def test_attn_ragged_long_context(c):
    """Every element of every query row against the case's own assertion (decoder_ref.build_attn_case): uniform -- relative
    2^-8 + 2^-20, exact zeros; needle -- 2^-40 absolute; rising and gaussian -- attn_bound.  The whole cache is filled, the
    masked tail included, so a leaked key shows."""
    case = R.build_attn_case(c)
    M, width = c.Bn * c.T, (c.H + 2 * c.KVH) * 128
    qkv = torch.randn(M, width, generator=torch.Generator().manual_seed(5)).to(BF)          # live k | v columns: never read
    qkv[:, : c.H * 128] = case["q"].reshape(M, c.H * 128)
    qkv = qkv.cuda()
    kc = case["k"].cuda()
    vt = case["v"].cuda().transpose(2, 3).contiguous()
    pos = case["pos"].cuda()
    rows = torch.tensor(c.rows, dtype=torch.int32, device="cuda") if c.rows else None
    out = torch.full((M, c.H * 128), 7.0, dtype=BF, device="cuda")
    rc = _lib().asd_attn_ragged(qkv.data_ptr(), width, kc.data_ptr(), vt.data_ptr(), pos.data_ptr(),
                                None if rows is None else rows.data_ptr(), _B().DTYPE_BF16, c.Bn, c.T, c.H, c.KVH, 128, c.t_max,
                                out.data_ptr(), c.H * 128, None)
    _B().check("asd_attn_ragged", rc)
    got = out.cpu().float().view(M, c.H, 128)
    bad, worst = R.attn_violations(got, case)
    print(f"asd_attn_ragged {R.case_id(c)}: worst |err| / bound {worst:.4f}")
    assert bad == 0, (bad, worst)


_ROPE_T_MAX = 32768
_rope_pattern = {}


def _rope_caches():
    """The pre-filled caches of the rope test (a fixed pattern of live values), built once."""
    if not _rope_pattern:
        g = torch.Generator(device="cuda").manual_seed(77)
        _rope_pattern["k"] = torch.randn(2, 2, _ROPE_T_MAX, 128, generator=g, device="cuda").to(BF)
        _rope_pattern["vt"] = torch.randn(2, 2, 128, _ROPE_T_MAX, generator=g, device="cuda").to(BF)
    return _rope_pattern["k"], _rope_pattern["vt"]


@pytest.mark.parametrize("theta", [1.0e6, 1.0e4])
@pytest.mark.parametrize("pos0", [(0, 4094), (30, 32764)], ids=["pos0_4094", "pos30_32764"])
def test_rope_kv_store_long_positions(theta, pos0):
    """Positions 0-2 | 4094-4096 and 30-32 | 32764-32766 (the last real slot; slot t_max - 1 is the trash slot and stays out) in a
    32768-slot cache: angles up to 32766 rad, cache offsets of 2^23 elements.  Bound of test_rope_kv_store."""
    Bn, T, H, KVH, t_max = 2, 3, 4, 2, _ROPE_T_MAX
    M, heads = Bn * T, H + 2 * KVH
    width = heads * 128
    g = torch.Generator().manual_seed(int(theta) // 1000 + pos0[0])
    qkv0 = torch.randn(M, width, generator=g).to(BF)
    pos = (torch.tensor(pos0)[:, None] + torch.arange(T)).reshape(M).to(torch.int32)
    assert int(pos.max()) < t_max - 1
    inv = (1.0 / (theta ** (torch.arange(0, 128, 2, dtype=torch.float32) / 128))).contiguous()
    k0, vt0 = _rope_caches()
    kc, vt = k0.clone(), vt0.clone()
    qkv, pos_d, inv_d = qkv0.cuda(), pos.cuda(), inv.cuda()
    rc = _lib().asd_rope_kv_store(qkv.data_ptr(), width, pos_d.data_ptr(), None, inv_d.data_ptr(), _B().DTYPE_BF16, Bn, T, H,
                                  KVH, 128, kc.data_ptr(), vt.data_ptr(), t_max, None)
    _B().check("asd_rope_kv_store", rc)
    o = qkv0.view(M, heads, 128)
    q_ref = R.rope_ref(o[:, :H], pos, inv)
    k_ref = R.rope_ref(o[:, H:H + KVH], pos, inv)
    got = qkv.cpu().view(M, heads, 128)
    assert torch.equal(got[:, H:], o[:, H:])                                               # k, v columns untouched
    seq = torch.arange(M) // T
    got_k = kc[seq.cuda(), :, pos.long().cuda()].cpu()                                     # [M, KVH, 128]
    got_v = vt[seq.cuda(), :, :, pos.long().cuda()].cpu()
    err_q = (got[:, :H].double() - q_ref).abs()
    err_k = (got_k.double() - k_ref).abs()
    worst = max(float((err_q / R.rope_bound(q_ref)).max()), float((err_k / R.rope_bound(k_ref)).max()))
    print(f"asd_rope_kv_store theta {theta:g} pos0 {pos0}: worst |err| / bound {worst:.4f}, worst |err| {max(float(err_q.max()), float(err_k.max())):.3e}")
    assert bool((err_q <= R.rope_bound(q_ref)).all()) and bool((err_k <= R.rope_bound(k_ref)).all())
    assert torch.equal(got_v, o[:, H + KVH:])                                              # v: bit for bit, transposed
    # nothing else changed: put the pattern back into the written slots and compare the whole caches
    kc[seq.cuda(), :, pos.long().cuda()] = k0[seq.cuda(), :, pos.long().cuda()]
    vt[seq.cuda(), :, :, pos.long().cuda()] = vt0[seq.cuda(), :, :, pos.long().cuda()]
    assert torch.equal(kc, k0) and torch.equal(vt, vt0)


def test_kv_rollback_is_exact():
    """Two models with the same weights and the same committed tokens, whose caches differ only in entries PAST the committed
    lengths (the rejected suffixes of two different drafts, inside live 32-key tiles): every later pass gives the same bits."""
    SL = import_module("adaptive-speculative-decoding_amd.serving.synthetic_lm")
    shape = SL.LMShape("small", 512, 3, 4, 2, 1024, vocab=1000, rope_theta=1.0e6)
    g = torch.Generator().manual_seed(12)
    V = shape.vocab
    ids = torch.randint(0, V, (3, 20), generator=g).cuda()
    keep = torch.tensor([0, 2, 5])
    X = torch.randint(0, V, (3, 5), generator=g)
    Xp = (X + 1 + torch.randint(0, V - 1, (3, 5), generator=g)) % V                        # differs from X everywhere ...
    Xp = torch.where(torch.arange(5)[None, :] < keep[:, None], X, Xp)                      # ... but in the kept prefix of each row
    assert bool(((X != Xp) == (torch.arange(5)[None, :] >= keep[:, None])).all())
    Y = torch.randint(0, V, (3, 3), generator=g).cuda()
    Z = torch.randint(0, V, (3, 1), generator=g).cuda()
    S = torch.randint(0, V, (2, 4), generator=g).cuda()
    sub = torch.tensor([2, 0], device="cuda")
    outs, caches = [], []
    for feed in (X, Xp):
        lm = SL.SyntheticLM(shape, dtype=BF, device="cuda", seed=4)
        R.randomize_affine(lm, 21)
        lm.enable_hip_layers()
        lm.alloc_ragged(3, 96)
        length = torch.zeros(3, dtype=torch.int64, device="cuda")
        lm.forward_ragged(ids, length, 20)
        length += 20
        first = lm.forward_ragged(feed.cuda(), length, 25)
        length += keep.cuda()                                                              # rollback: rows keep 0, 2 and 5 tokens
        mine = [lm.forward_ragged(Y, length, 28)]
        length += torch.tensor([1, 3, 2], device="cuda")                                   # a second rollback, the same in both
        mine.append(lm.forward_ragged(Z, length, 30))
        length += 1
        caches.append([c.clone() for c in lm._hip.k_cache])
        mine.append(lm.forward_ragged(S, length[sub], 36, rows=sub))
        outs.append((first, mine))
    (fa, a), (fb, b) = outs
    assert not torch.equal(fa, fb)                                                         # the drafts did differ
    assert any(not torch.equal(x, y) for x, y in zip(*caches))                             # ... and left different stale entries
    for x, y in zip(a, b):
        assert x.dtype == BF and bool(torch.isfinite(x.float()).all())
        assert torch.equal(x, y)
