"""The decoder stack at the widths the benchmark runs (the Qwen2.5 7B / 14B / 32B / 72B projections, two layers each), with
random biases and norm weights, row-major and packed tile-major weights.

tests/test_gpu_decoder.py holds asd_decoder_forward to the composition of its parts at hidden 512 only, where every sliced
projection has exactly four slices, the second piece of k_rmsnorm<true> (D > 4096) does not exist, and -- with SyntheticLM's
bias = 0, norm weight = 1 -- a wrong bias or weight index changes nothing.  Here the slab consumers (k_rope_kv_store<true>,
k_rmsnorm<true>, k_silu_mul<true>) run with 3 .. 18 slices at N up to 59136, every op of the composition is held element by
element to the f64 reference of its own rounded inputs (tests/decoder_ref.py, whose chain tests/test_decoder_refs.py holds to
the model's f64 forward), the fused forward to the composition bit for bit, and the packed layout to the row-major one."""
import ctypes as C
import os
import sys
import time
from importlib import import_module

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import decoder_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
T_MAX = 64
PROJECTIONS = ("q|k|v", "o", "gate|up", "down")
WIDTHS = {                                  # hidden, heads, kv_heads, intermediate (the Qwen2.5 model cards)
    "7B": (3584, 28, 4, 18944), "14B": (5120, 40, 8, 13824), "32B": (5120, 40, 8, 27648), "72B": (8192, 64, 8, 29568),
}
# (widths, sequences, tokens per sequence, form of the linear launcher at M = Bn * T, the T = 1 pass feeds every sequence)
CASES = [
    ("7B", 3, 5, "skinny", False), ("7B", 13, 5, "tile", False), ("14B", 3, 5, "skinny", False),
    ("32B", 32, 9, "tall", True), ("72B", 3, 5, "skinny", False), ("72B", 33, 9, "two_row_blocks", False),
]


def _case_id(c):
    return f"{c[0]}-M{c[1] * c[2]}-{c[3]}"


def _K():
    return import_module("adaptive-speculative-decoding_amd.kernels")


def _B():
    return import_module("adaptive-speculative-decoding_amd._binding")


def _check(rc, name):
    _B().check(name, rc)


def _shape(widths):
    SL = import_module("adaptive-speculative-decoding_amd.serving.synthetic_lm")
    hidden, heads, kv_heads, intermediate = WIDTHS[widths]
    return SL.LMShape(widths, hidden, 2, heads, kv_heads, intermediate, vocab=1000, rope_theta=1.0e6)


def _plans(shape, M):
    """slice counts of q|k|v, o, gate|up, down at M rows, from the launcher's own plan"""
    lib, kv = _K()._lib(), shape.kv_heads * 128
    return [lib.asd_linear_slices(M, N, D) for N, D in ((shape.hidden + 2 * kv, shape.hidden), (shape.hidden, shape.hidden),
                                                        (2 * shape.intermediate, shape.hidden), (shape.hidden, shape.intermediate))]


def _model(shape, pack, cache_rows):
    SL = import_module("adaptive-speculative-decoding_amd.serving.synthetic_lm")
    lm = SL.SyntheticLM(shape, dtype=BF, device="cuda", seed=6)
    R.randomize_affine(lm, 17)
    lm.enable_hip_layers(pack_weights=pack)
    lm.alloc_ragged(cache_rows, T_MAX)
    return lm


class _Worst:
    """worst |err| / bound and number of elements outside their bound, per op kind"""

    def __init__(self):
        self.ratio, self.bad = {}, {}

    def hold(self, kind, got, ref, bound):
        err = (got.double() - ref).abs()
        self.ratio[kind] = max(self.ratio.get(kind, 0.0), float((err / bound).max()))
        self.bad[kind] = self.bad.get(kind, 0) + int((~(err <= bound)).sum())          # NaN counts as outside


@torch.no_grad()
def _composition(lm, ids, pos0, worst):
    """The exported parts called one by one on fresh zeroed caches, asd_linear_ex's own reduce kernel after every sliced
    projection; every op's output goes to worst.hold with the f64 reference of the op's own inputs.  Returns (final norm,
    residual stream, [(k cache, vt cache) per layer])."""
    K_, Bd, lib = _K(), _B(), _K()._lib()
    s, hd = lm.shape, lm._hip
    Bn, T = ids.shape
    M, H, KVH, h, I = Bn * T, s.heads, s.kv_heads, s.hidden, s.intermediate
    heads = H + 2 * KVH
    x = lm.embed(ids).view(M, h).clone()
    pos = (pos0[:, None] + torch.arange(T, device="cuda")).reshape(M).to(torch.int32)
    seq = torch.arange(M, device="cuda") // T
    ws = K_.LinearWorkspace("cuda")
    caches = []

    def norm(weight):
        out = torch.empty_like(x)
        _check(lib.asd_rmsnorm(x.data_ptr(), h, weight.data_ptr(), s.rms_eps, Bd.DTYPE_BF16, M, h, out.data_ptr(), h, None), "asd_rmsnorm")
        ref = R.rmsnorm_ref(x, weight, s.rms_eps)
        worst.hold("rmsnorm", out, ref, R.elementwise_bound(ref))
        return out

    def project(inp, w, bias=None, residual=False):
        ref = R.linear_ref(inp, w, bias, x if residual else None)
        out = K_.linear(inp, w, bias, workspace=ws, out=x, residual=x) if residual else K_.linear(inp, w, bias, workspace=ws)
        worst.hold("linear", out, ref, R.linear_bound(ref))
        return out

    for i, blk in enumerate(lm.blocks):
        qkv_w, qkv_b, gu_w = hd._fused[i]
        kc, vt = torch.zeros_like(hd.k_cache[i]), torch.zeros_like(hd.vt_cache[i])
        qkv = project(norm(blk.ln1.weight), qkv_w, qkv_b)
        o = qkv.clone().view(M, heads, 128)
        _check(lib.asd_rope_kv_store(qkv.data_ptr(), qkv.stride(0), pos.data_ptr(), None, hd.inv_freq.data_ptr(), Bd.DTYPE_BF16, Bn, T,
                                     H, KVH, 128, kc.data_ptr(), vt.data_ptr(), hd.t_max, None), "asd_rope_kv_store")
        q = qkv.view(M, heads, 128)[:, :H].contiguous()
        for got, part in ((q, o[:, :H]), (kc[seq, :, pos.long()], o[:, H:H + KVH])):
            ref = R.rope_ref(part, pos, hd.inv_freq)
            worst.hold("rope", got, ref, R.rope_bound(ref))
        assert torch.equal(qkv.view(M, heads, 128)[:, H:], o[:, H:])                         # k, v columns untouched
        assert torch.equal(vt[seq, :, :, pos.long()], o[:, H + KVH:])                        # v: bit for bit, transposed
        attn = torch.empty(M, h, dtype=BF, device="cuda")
        _check(lib.asd_attn_ragged(qkv.data_ptr(), qkv.stride(0), kc.data_ptr(), vt.data_ptr(), pos.data_ptr(), None, Bd.DTYPE_BF16, Bn, T,
                                   H, KVH, 128, hd.t_max, attn.data_ptr(), h, None), "asd_attn_ragged")
        ref, A = R.attn_ref(q, kc, vt.transpose(2, 3), pos, seq.tolist())
        worst.hold("attention", attn.view(M, H, 128), ref, R.attn_bound(ref, A))
        del ref, A
        project(attn, blk.o.weight, residual=True)
        gu = project(norm(blk.ln2.weight), gu_w)
        act = torch.empty(M, I, dtype=BF, device="cuda")
        _check(lib.asd_silu_mul(gu.data_ptr(), gu.stride(0), Bd.DTYPE_BF16, M, I, act.data_ptr(), I, None), "asd_silu_mul")
        ref = R.silu_mul_ref(gu)
        worst.hold("silu_mul", act, ref, R.elementwise_bound(ref))
        del ref
        project(act, blk.down.weight, residual=True)
        caches.append((kc, vt))
    return norm(lm.norm.weight), x, caches


def _forward_direct(lm, x, pos, Bn, T, final_norm):
    """asd_decoder_forward through ctypes, as HipDecoder.forward calls it, on the caller's x [M, hidden] (updated in place: the
    residual stream).  Returns the final norm's output, or None without one."""
    hd, s = lm._hip, lm.shape
    scratch = hd._scratch_for(Bn * T)
    base = (scratch.data_ptr() + 255) // 256 * 256
    hn = torch.empty_like(x) if final_norm else None
    rc = hd.lib.asd_decoder_forward(hd._layers, s.layers, C.byref(hd._shape), x.data_ptr(), x.stride(0), pos.data_ptr(), None, Bn, T,
                                    lm.norm.weight.data_ptr() if final_norm else None, hn.data_ptr() if final_norm else None,
                                    hn.stride(0) if final_norm else 0, base, scratch.numel() - (base - scratch.data_ptr()),
                                    _K()._stream())
    _check(rc, "asd_decoder_forward")
    return hn


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_decoder_stack_at_benchmarked_widths(case):
    """One case of the table: (a) composition with per-op f64 checks, (b) fused forward = composition, (c) the same without a
    final norm, (d) packed twin.  Measured on an MI355X (256 CUs), worst |err| / bound over the six cases: attention 0.900,
    linear 0.983, rmsnorm 0.996, rope 0.995, silu * up 0.995 (DESIGN 4.9 has the table)."""
    widths, Bn, T, form, decode_all = case
    torch.cuda.empty_cache()
    if torch.cuda.mem_get_info()[0] < 24 * 10 ** 9:
        pytest.skip("less than 24 GB of device memory free")
    t0 = time.perf_counter()
    shape = _shape(widths)
    M = Bn * T
    plans = _plans(shape, M)
    print(f"{_case_id(case)}: slices of {', '.join(PROJECTIONS)} = {plans}")
    assert max(plans) > 1                                                      # fused consumers really run
    lm = _model(shape, False, Bn)
    hd = lm._hip
    assert not hd.packed
    g = torch.Generator(device="cuda").manual_seed(2)
    ids = torch.randint(0, shape.vocab, (Bn, T), generator=g, device="cuda")
    pos0 = torch.randint(0, T_MAX - T, (Bn,), generator=g, device="cuda")             # <= t_max - T - 1: the trash slot stays out
    pos0[0] = 0
    pos = (pos0[:, None] + torch.arange(T, device="cuda")).reshape(M).to(torch.int32)

    # a. the composition, every op against the f64 reference of its own inputs
    worst = _Worst()
    want, x_want, caches = _composition(lm, ids, pos0, worst)
    print(f"{_case_id(case)}: worst |err| / bound  " + "  ".join(f"{k} {v:.4f}" for k, v in sorted(worst.ratio.items())))
    assert set(worst.ratio) == {"rmsnorm", "linear", "rope", "attention", "silu_mul"}
    assert all(n == 0 for n in worst.bad.values()), (worst.bad, worst.ratio)

    # b. the fused forward equals the composition: final norm, residual stream, caches
    got = lm.forward_ragged(ids, pos0, T_MAX, return_hidden=True)
    assert torch.equal(got.view(M, shape.hidden), want)
    x = lm.embed(ids).view(M, shape.hidden).clone()
    hn = _forward_direct(lm, x, pos, Bn, T, final_norm=True)                   # the same positions: the same cache values again
    assert torch.equal(hn, want) and torch.equal(x, x_want)
    for i, (kc, vt) in enumerate(caches):
        assert torch.equal(hd.k_cache[i], kc) and torch.equal(hd.vt_cache[i], vt)

    # c. without a final norm a norm launch of its own finishes the last residual connection
    x = lm.embed(ids).view(M, shape.hidden).clone()
    assert _forward_direct(lm, x, pos, Bn, T, final_norm=False) is None
    assert torch.equal(x, x_want)
    del caches, x, hn, x_want

    # d. the packed twin: equal bits on the same pass and on a T = 1 pass behind it
    twin = _model(shape, True, Bn)
    assert twin._hip.packed
    assert torch.equal(twin.forward_ragged(ids, pos0, T_MAX, return_hidden=True).view(M, shape.hidden), want)
    rows = None if decode_all else torch.tensor([Bn - 1, 0], device="cuda")
    n1 = Bn if decode_all else 2
    ids1 = torch.randint(0, shape.vocab, (n1, 1), generator=g, device="cuda")
    pos1 = (pos0 + T) if decode_all else (pos0 + T)[rows]
    print(f"{_case_id(case)}: T = 1 pass over {n1} sequences, slices = {_plans(shape, n1)}")
    a = lm.forward_ragged(ids1, pos1, T_MAX, return_hidden=True, rows=rows)
    b = twin.forward_ragged(ids1, pos1, T_MAX, return_hidden=True, rows=rows)
    assert bool(torch.isfinite(a.float()).all()) and torch.equal(a, b)
    torch.cuda.synchronize()
    del lm, twin, hd, got, want, a, b
    torch.cuda.empty_cache()
    print(f"{_case_id(case)}: {time.perf_counter() - t0:.1f} s")


def test_the_cases_cover_the_slab_consumers():
    """What the case table is for, stated on the launcher's own plans on this device: if a condition fails (another CU count,
    another cost model), change the table -- M or widths -- not the condition."""
    plans = {_case_id(c): _plans(_shape(c[0]), c[1] * c[2]) for c in CASES}
    print(plans)
    for j, name in enumerate(PROJECTIONS):
        counts = [p[j] for p in plans.values()]
        assert any(k > 1 for k in counts), name                                # sliced in at least one case
        assert any(k > 1 and k % 4 != 0 for k in counts), name                 # a remainder of the unroll-by-4 slab loops
    assert any(max(p) > 8 for p in plans.values())                             # a third group of four
    for c in CASES:
        p = plans[_case_id(c)]
        assert max(p) > 1
        if WIDTHS[c[0]][0] == 8192:                                            # k_rmsnorm<true>'s second piece (t + 1024) after o and down
            assert p[1] > 1 and p[3] > 1
    assert any(WIDTHS[c[0]][0] == 8192 for c in CASES)
