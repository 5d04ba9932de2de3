"""asd_logit_edit_rows on the GPU against tests/logit_edit_ref.py::ref_logit_edit.  The WHOLE allocation -- a guard band in
front, the tensor with its row padding, a guard band behind -- is compared bit for bit, so a stray write anywhere fails.
bf16 / f16 / f32; B = 3, K1 in {1, 5}, V in {1000, 1003} (the odd one with padded rows: ld_row > V); a [:, :4] slice of a
[3, 5, V] tensor (ld_seq != K1 * ld_row); rows with 0, 1 and 1024 entries; the shared list (row_first = NULL) and the per-row
form; ids 0 and V - 1 and ids outside [0, V); `until` on both sides of g at one position and across positions; bias 0; the
launcher's status codes; and the existing samplers on an edited tensor."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.logit_edit_ref import FOREVER, ref_logit_edit
from tests.stage_scenario import ref_logprob

pytestmark = pytest.mark.gpu

B = 3
GUARD = 256                                      # elements of the tensor's dtype on either side
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
SEQ_LEN, START, OFFSET = [7, 9, 12], 5, 1        # g = seq_len - start + offset + j = 3 + j, 5 + j, 8 + j
LP_ATOL = 2e-5                                   # tests/test_gpu_stages.py's bar for a kernel lp against the f64 value at its row


@pytest.fixture(scope="module")
def K_():
    from asd_amd import kernels
    return kernels


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16).numpy().tobytes()


def _arena(dtype, K1, V, pad, seed, rows_alloc=None):
    """-> (buf: the whole allocation on the CPU, view(buf) -> the [B, K1, V] logits inside it, row stride V + pad)."""
    rows_alloc = K1 if rows_alloc is None else rows_alloc
    g = torch.Generator().manual_seed(seed)
    n = B * rows_alloc * (V + pad)
    buf = (torch.randn(n + 2 * GUARD, generator=g) * 4.0).to(dtype)

    def view(b):
        return b[GUARD:GUARD + n].view(B, rows_alloc, V + pad)[:, :K1, :V]
    return buf, view


def _entries(ids, g0, rng):
    """One entry per id with a mix of what an entry can do: a plain bias, bias 0 (nothing), a permanent ban, and `until` at
    g0 .. g0 + 3 -- with g = g0 + j that is banned / not banned at j = 0 and flips inside K1 = 5 positions."""
    out = []
    for i, t in enumerate(ids):
        kind = i % 7
        bias = float(np.float32(rng.uniform(-100.0, 100.0)))
        if kind == 0:
            out.append((t, bias, 0))
        elif kind == 1:
            out.append((t, 0.0, 0))                                  # stores nothing
        elif kind == 2:
            out.append((t, bias, FOREVER))
        else:
            out.append((t, bias if i % 2 else 0.0, g0 + kind - 3))   # until = g0, g0 + 1, g0 + 2, g0 + 3
    return out


def _rows(form, V, rng):
    g0 = [s - START + OFFSET for s in SEQ_LEN]
    if form == "shared":                                             # one list for every row: row_first = NULL
        ids = [0, V - 1, -1, V, V + 5, -2 ** 31, 2 ** 31 - 1] + [int(t) for t in rng.choice(np.arange(1, V - 1), 33, replace=False)]
        return [_entries(ids, g0[1], rng)] * B
    if form == "shared1024":
        return [_entries(list(range(-10, 1014)), g0[0], rng)] * B
    # per row: 0 entries, 1 entry, 1024 entries (distinct ids: all of [0, V) and some outside it)
    return [[], [(V - 1, -3.25, g0[1] + 1)], _entries(list(range(-10, 1014)), g0[2], rng)]


def _run(K_, dtype, K1, V, pad, form, seed, rows_alloc=None):
    rng = np.random.default_rng(seed)
    buf, view = _arena(dtype, K1, V, pad, seed, rows_alloc)
    rows = _rows(form, V, rng)
    want = buf.clone()
    ref_logit_edit(view(want), rows, SEQ_LEN, START, OFFSET)
    dev = buf.cuda()
    packed = K_.pack_logit_edits(rows, "cuda")
    assert (packed.row_first is None) == form.startswith("shared")
    x = view(dev)
    out = K_.logit_edit_rows(x, packed, torch.tensor(SEQ_LEN, dtype=torch.int32, device="cuda"), START, OFFSET)
    torch.cuda.synchronize()
    assert out is x
    assert _bits(dev) == _bits(want)
    changed = int((view(want) != view(buf)).sum() + (torch.isneginf(view(want)) & ~torch.isneginf(view(buf))).sum())
    assert changed > 0 and torch.isneginf(view(want)).any()
    return view(buf), view(want), rows


@pytest.mark.parametrize("form", ["shared", "rows"])
@pytest.mark.parametrize("V", [1000, 1003])
@pytest.mark.parametrize("K1", [1, 5])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16", "f32"])
def test_kernel_matches_the_reference_bit_for_bit(K_, dtype, K1, V, form):
    before, after, rows = _run(K_, dtype, K1, V, 0 if V == 1000 else 9, form, seed=K1 * 10000 + V)
    if form == "rows":
        assert _bits(after[0]) == _bits(before[0])                   # the row without entries
        # the one entry of row 1: until = g + 1 at j = 0 (banned), g at j = 1 (the bias)
        assert torch.isneginf(after[1, 0, V - 1])
        if K1 > 1:
            assert after[1, 1, V - 1] == (before[1, 1, V - 1].float() - 3.25).to(dtype)
    else:
        # ids 0 and V - 1 are entries 0 (a bias) and 1 (bias 0: the bits stay)
        assert after[0, 0, 0] == (before[0, 0, 0].float() + torch.tensor(rows[0][0][1])).to(dtype)
        assert _bits(after[:, :, V - 1]) == _bits(before[:, :, V - 1])


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16", "f32"])
def test_shared_list_of_1024_entries_and_a_non_contiguous_slice(K_, dtype):
    _run(K_, dtype, 5, 1000, 0, "shared1024", seed=7)
    # a [:, :4] slice of a [3, 5, V] tensor: ld_seq = 5 V, K1 = 4; row 4 of every sequence is not touched
    before, after, _ = _run(K_, dtype, 4, 1003, 0, "rows", seed=8, rows_alloc=5)
    assert before.stride(0) == 5 * 1003 and before.shape == (B, 4, 1003)


def test_until_flips_inside_one_tensor(K_):
    """g = seq_len - start + offset + j: with until = 10 and seq_len = 12, start = 5, offset = 1 the positions j = 0, 1 are
    banned (g = 8, 9 = until - 1) and j = 2, 3, 4 carry the bias (g = until, ...)."""
    x = torch.zeros((1, 5, 16), dtype=torch.float32, device="cuda")
    packed = K_.pack_logit_edits([[(3, 1.5, 10)]], "cuda")
    K_.logit_edit_rows(x, packed, torch.tensor([12], dtype=torch.int32, device="cuda"), 5, 1)
    got = x[0, :, 3].cpu().tolist()
    assert got == [float("-inf"), float("-inf"), 1.5, 1.5, 1.5]
    assert int((x != 0).sum()) == 5


def test_nothing_is_touched_without_rows_or_entries(K_):
    from asd_amd import _binding
    lib = _binding.load_library()
    x = torch.randn((B, 2, 64), device="cuda")
    keep = x.clone()
    seq = torch.tensor(SEQ_LEN, dtype=torch.int32, device="cuda")
    empty = K_.pack_logit_edits([[], [], []], "cuda")
    assert empty.n == 0 and empty.row_first is None
    K_.logit_edit_rows(x, empty, seq, START, 0)
    e = K_.pack_logit_edits([[(1, 1.0, 0)]] * B, "cuda")
    args = lambda Bv, K1, n, first=None: (x.data_ptr(), 0, 128, 64, Bv, K1, 64, e.edit_id.data_ptr(), e.edit_bias.data_ptr(),   # noqa: E731
                                          e.edit_until.data_ptr(), first, n, seq.data_ptr(), START, 0, None)
    assert lib.asd_logit_edit_rows(*args(0, 2, 1)) == 0
    assert lib.asd_logit_edit_rows(*args(B, 0, 1)) == 0
    assert lib.asd_logit_edit_rows(*args(B, 2, 0)) == 0
    # ... before the pointers are looked at: B == 0 with nothing else valid
    assert lib.asd_logit_edit_rows(None, 0, 0, 0, 0, 1, 64, None, None, None, None, 1, None, 0, 0, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(x, keep)
    # per-row form with rows that own nothing and indices that would leave the arrays: clamped, nothing written
    first = torch.tensor([0, 0, 0, 0], dtype=torch.int32, device="cuda")
    assert lib.asd_logit_edit_rows(*args(B, 2, 1, first.data_ptr())) == 0
    wild = torch.tensor([-5, 7, 9, 2], dtype=torch.int32, device="cuda")
    assert lib.asd_logit_edit_rows(*args(B, 2, 1, wild.data_ptr())) == 0
    torch.cuda.synchronize()
    assert torch.equal(x, keep)


def test_argument_errors_return_their_codes(K_):
    from asd_amd import _binding
    lib = _binding.load_library()
    INVALID, UNSUPPORTED, ALIGNMENT = -1, -2, -5
    x = torch.randn((B, 2, 64), device="cuda")
    keep = x.clone()
    seq = torch.tensor(SEQ_LEN, dtype=torch.int32, device="cuda")
    e = K_.pack_logit_edits([[(1, 1.0, 0)]] * B, "cuda")
    good = dict(logits=x.data_ptr(), dtype=0, ld_seq=128, ld_row=64, B=B, K1=2, V=64, id=e.edit_id.data_ptr(),
                bias=e.edit_bias.data_ptr(), until=e.edit_until.data_ptr(), first=None, n=1, seq=seq.data_ptr(), start=START,
                offset=0, stream=None)

    def call(**kw):
        return lib.asd_logit_edit_rows(*{**good, **kw}.values())
    for kw in (dict(B=-1), dict(K1=-1), dict(V=-1), dict(n=-1)):
        assert call(**kw) == INVALID, kw
    for kw in (dict(logits=None), dict(id=None), dict(bias=None), dict(until=None), dict(seq=None), dict(ld_row=63),
               dict(ld_seq=127)):
        assert call(**kw) == INVALID, kw
    assert call(dtype=7) == UNSUPPORTED and call(dtype=-1) == UNSUPPORTED
    assert call(n=1025) == UNSUPPORTED                                # row_first == NULL: every row would own 1025 entries
    assert call(logits=x.data_ptr() + 2) == ALIGNMENT
    torch.cuda.synchronize()
    assert torch.equal(x, keep)
    assert call() == 0
    torch.cuda.synchronize()
    assert int((x != keep).sum()) == B * 2
    # the wrapper's own checks
    with pytest.raises(ValueError):
        K_.logit_edit_rows(x.cpu(), e, seq, START)
    with pytest.raises(ValueError):
        K_.logit_edit_rows(x[:2], e, seq[:2], START)
    with pytest.raises(ValueError):
        K_.logit_edit_rows(x.transpose(1, 2), e, seq, START)
    for bad in ([[(1, 1.0, 0), (1, 2.0, 0)]], [[(1, float("nan"), 0)]], [[(1, 1.0, -1)]], [[(t, 1.0, 0) for t in range(1025)]]):
        with pytest.raises(ValueError):
            K_.pack_logit_edits(bad, "cuda")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
def test_existing_samplers_on_an_edited_tensor(K_, dtype):
    """The unchanged kernels on the new input class: about 50 -inf entries per row from the edit kernel itself, then
    draft_sample, verify_accept and residual_sample_lp through HipOps at the bar of tests/test_gpu_stages.py (every returned
    log-prob within 2e-5 of the f64 value on the edited row), and no banned id is ever returned."""
    from asd_amd.distributed import HipOps
    ops = HipOps()
    V, K = 1000, 4
    inv_t = float(np.float32(1 / 0.7))
    rng = np.random.default_rng(5)
    g = torch.Generator().manual_seed(5)
    t_out = (torch.randn((B, K + 1, V), generator=g) * 3.0).to(dtype).cuda()
    d_all = (t_out.float() + 0.5 * torch.randn((B, K + 1, V), generator=g).cuda()).to(dtype)[:, :K].contiguous()
    banned = [sorted(int(t) for t in rng.choice(V, 50, replace=False)) for _ in range(B)]
    # ban the most likely token of every row of row b as well: the samplers would otherwise rarely meet a banned id
    for b in range(B):
        banned[b] = sorted(set(banned[b]) | {int(t) for t in t_out[b].float().argmax(-1).tolist()}
                           | {int(t) for t in d_all[b].float().argmax(-1).tolist()})
    seq = torch.tensor(SEQ_LEN, dtype=torch.int32, device="cuda")
    packed = ops.pack_logit_edits([[(t, 0.0, FOREVER) for t in ids] for ids in banned], "cuda")
    ops.logit_edit_rows(t_out, packed, seq, START, 0)
    ops.logit_edit_rows(d_all, packed, seq, START, 0)
    for b in range(B):
        assert int(torch.isneginf(t_out[b, 0]).sum()) == len(banned[b]) >= 50
    toks, lpd, thrs = [], [], []
    for k in range(K):
        dl = d_all[:, k].contiguous()
        tok, lp, thr = ops.draft_sample(dl, torch.rand((B,), generator=g).cuda(), inv_t, 0.9)
        toks.append(tok), lpd.append(lp), thrs.append(thr)
        for b in range(B):
            assert int(tok[b]) not in banned[b]
            ref = ref_logprob(dl[b].float().cpu().numpy(), int(tok[b]), inv_t, float(thr[b]))
            assert abs(float(lp[b]) - ref) <= LP_ATOL
    tok32 = torch.stack(toks, 1).to(torch.int32).contiguous()
    tok32[0, 1] = banned[0][0]                                       # a banned proposal (never made by the loop): lp_t = -inf, rejected
    lp_d = torch.stack(lpd, 1).contiguous()
    d_thr = torch.stack(thrs, 1).contiguous()
    score, bonus = t_out[:, :K].contiguous(), t_out[:, K].contiguous()
    u = torch.rand((B, K), generator=g).cuda()
    lp_t, accept, n_acc, _ = ops.verify_accept(score, tok32, lp_d, u, inv_t)
    for b in range(B):
        for k in range(K):
            ref = ref_logprob(score[b, k].float().cpu().numpy(), int(tok32[b, k]), inv_t)
            if np.isneginf(ref):
                assert np.isneginf(float(lp_t[b, k])) and int(accept[b, k]) == 0
            else:
                assert abs(float(lp_t[b, k]) - ref) <= LP_ATOL
                margin = np.log(max(float(u[b, k]), 1e-300)) - (ref - float(lp_d[b, k]))
                if abs(margin) > 1e-4:
                    assert int(accept[b, k]) == int(margin <= 0)
    assert np.isneginf(float(lp_t[0, 1])) and int(n_acc[0]) <= 1
    drawn, lp_drawn = ops.residual_sample_lp(score, d_all, n_acc, torch.rand((B,), generator=g).cuda(), bonus, inv_t,
                                             d_threshold=d_thr, t_threshold=None)
    for b in range(B):
        assert int(drawn[b]) not in banned[b] and 0 <= int(drawn[b]) < V
        row = score[b, int(n_acc[b])] if int(n_acc[b]) < K else bonus[b]
        assert abs(float(lp_drawn[b]) - ref_logprob(row.float().cpu().numpy(), int(drawn[b]), inv_t)) <= LP_ATOL
    ops.check_status()
