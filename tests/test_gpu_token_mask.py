"""asd_logit_mask_rows on the GPU against tests/token_mask_ref.py::ref_logit_mask.  The WHOLE allocation -- a guard band in
front, the tensor with its row padding, a guard band behind (the arena of tests/test_gpu_logit_edit.py) -- is compared bit for
bit, so a stray write anywhere fails.  bf16 / f16 / f32; B = 3, K1 in {1, 5}, V in {5, 32, 1000, 1003} with ld_row = V and
ld_row = V + 13 (row bases of every alignment); a view one element into the arena; the [:, :4] slice of a [3, 5, V] tensor;
V = 152064 at (B, K1) = (1, 1) and (2, 3) (a row cut into slices).  Masks: all set, all clear, one kept id at 0 and at V - 1,
0x55555555, random at density 1/2, runs on and off the 8- and 32-element boundaries, garbage of both kinds in the tail bits of
the last word.  mask_row: NULL, two sequences on one mask, -1 and R.  Then: mask and edit commute, the launcher's status
codes, and the existing samplers on a masked tensor."""
import numpy as np
import pytest
import torch

from tests.logit_edit_ref import FOREVER, ref_logit_edit
from tests.stage_scenario import ref_logprob
from tests.token_mask_ref import ref_logit_mask, ref_pack_bits

pytestmark = pytest.mark.gpu

B = 3
GUARD = 256                                      # elements of the tensor's dtype on either side
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
DTYPE_IDS = ["bf16", "f16", "f32"]
LP_ATOL = 2e-5                                   # tests/test_gpu_logit_edit.py's, taken from tests/test_gpu_stages.py
RUNS = [(0, 8), (13, 16), (24, 37), (40, 64), (64, 71), (95, 129), (130, 131), (160, 192), (250, 263)]


@pytest.fixture(scope="module")
def K_():
    from asd_amd import kernels
    return kernels


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16).numpy().tobytes()


def _arena(dtype, K1, V, pad, seed, rows_alloc=None, shift=0, nb=B):
    """-> (buf: the whole allocation on the CPU, view(buf) -> the [nb, K1, V] logits inside it, row stride V + pad, the first
    element `shift` elements behind the front guard band)."""
    rows_alloc = K1 if rows_alloc is None else rows_alloc
    g = torch.Generator().manual_seed(seed)
    n = nb * rows_alloc * (V + pad)
    buf = (torch.randn(n + shift + 2 * GUARD, generator=g) * 4.0).to(dtype)

    def view(b):
        return b[GUARD + shift:GUARD + shift + n].view(nb, rows_alloc, V + pad)[:, :K1, :V]
    return buf, view


def _mask(kind, V, rng, garbage):
    """One mask as uint32 [W] words.  `garbage`: what the bits at v >= V of the last word hold (True: set, False: clear)."""
    keep = np.zeros(V, dtype=bool)
    if kind == "all_set":
        keep[:] = True
    elif kind == "first":
        keep[0] = True
    elif kind == "last":
        keep[V - 1] = True
    elif kind == "0x55":
        keep[0::2] = True                                             # 0x55555555 throughout: every chunk is mixed
    elif kind == "random":
        keep = rng.random(V) < 0.5
    elif kind == "runs":
        for lo, hi in RUNS + [(V - 9, V)]:
            keep[max(lo, 0):min(hi, V)] = True
    else:
        assert kind == "all_clear"
    words = ref_pack_bits([np.nonzero(keep)[0].tolist()], V)[0]
    if V % 32 and garbage:
        words[-1] |= np.uint32((0xFFFFFFFF << (V % 32)) & 0xFFFFFFFF)
    return words, keep


# three masks per launch, one per sequence; between them every kind, and tail garbage of both kinds
MASK_SETS = {"set_clear_first": [("all_set", False), ("all_clear", True), ("first", True)],
             "last_55_random": [("last", False), ("0x55", True), ("random", False)],
             "runs_random_clear": [("runs", True), ("random", True), ("all_clear", False)]}


def _packed(K_, words, mask_row, V, nb=B):
    bits = torch.from_numpy(np.stack(words).view(np.int32)).cuda()
    row = None if mask_row is None else torch.tensor(mask_row, dtype=torch.int32, device="cuda")
    return K_.TokenMasks(bits, row, len(words), nb, V)


def _run(K_, dtype, K1, V, pad, masks, seed, mask_row=(0, 1, 2), rows_alloc=None, shift=0, nb=B):
    rng = np.random.default_rng(seed)
    buf, view = _arena(dtype, K1, V, pad, seed, rows_alloc, shift, nb)
    made = [_mask(kind, V, rng, garbage) for kind, garbage in masks]
    words = [w for w, _ in made]
    want = buf.clone()
    ref_logit_mask(view(want), np.stack(words), mask_row)
    dev = buf.cuda()
    x = view(dev)
    out = K_.logit_mask_rows(x, _packed(K_, words, None if mask_row is None else list(mask_row), V, nb))
    torch.cuda.synchronize()
    assert out is x
    assert _bits(dev) == _bits(want)
    # the reference itself did what the header says, independently of its bit arithmetic: -inf exactly off the kept set
    for b in range(nb):
        r = 0 if mask_row is None else mask_row[b]
        if 0 <= r < len(made):
            keep = torch.from_numpy(made[r][1])
            assert torch.isneginf(view(want)[b][:, ~keep]).all() and _bits(view(want)[b][:, keep]) == _bits(view(buf)[b][:, keep])
        else:
            assert _bits(view(want)[b]) == _bits(view(buf)[b])
    return view(buf), view(want)


@pytest.mark.parametrize("masks", list(MASK_SETS), ids=list(MASK_SETS))
@pytest.mark.parametrize("pad", [0, 13])
@pytest.mark.parametrize("V", [5, 32, 1000, 1003])
@pytest.mark.parametrize("K1", [1, 5])
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_kernel_matches_the_reference_bit_for_bit(K_, dtype, K1, V, pad, masks):
    before, after = _run(K_, dtype, K1, V, pad, MASK_SETS[masks], seed=K1 * 10000 + V + pad)
    if masks == "set_clear_first":
        assert _bits(after[0]) == _bits(before[0])                   # all set: nothing written
        assert torch.isneginf(after[1]).all()                        # all clear: the whole row, legal for the kernel
        assert torch.isneginf(after[2][:, 1:]).all() and _bits(after[2][:, 0]) == _bits(before[2][:, 0])
    elif masks == "last_55_random":
        assert torch.isneginf(after[0][:, :V - 1]).all() and _bits(after[0][:, V - 1]) == _bits(before[0][:, V - 1])


@pytest.mark.parametrize("V", [1000, 1003])
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_an_offset_view_and_a_non_contiguous_slice(K_, dtype, V):
    # a view that starts one element into the arena: every row base is off the 16-byte grid, also with ld_row = V even
    for masks in MASK_SETS.values():
        _run(K_, dtype, 5, V, 0, masks, seed=V + 1, shift=1)
    # the [:, :4] slice of a [3, 5, V] tensor: ld_seq = 5 V, K1 = 4; row 4 of every sequence is not touched
    before, _ = _run(K_, dtype, 4, V, 0, MASK_SETS["runs_random_clear"], seed=V + 2, rows_alloc=5)
    assert before.stride(0) == 5 * V and before.shape == (B, 4, V)


@pytest.mark.parametrize("mask_row", [None, (1, 0, 1), (-1, 0, 2), (1, -2 ** 31, 2 ** 31 - 1)], ids=["null", "shared", "none_and_R", "wild"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
def test_which_mask_a_sequence_uses(K_, dtype, mask_row):
    masks = [("random", True), ("runs", False)]                      # R = 2: index 2 is R, "never leaves the array"
    before, after = _run(K_, dtype, 5, 1003, 13, masks, seed=77, mask_row=mask_row)
    where = [torch.isneginf(after[b]).numpy().tobytes() for b in range(B)]
    if mask_row is None:
        assert where[0] == where[1] == where[2]
    elif mask_row == (1, 0, 1):
        assert where[0] == where[2] != where[1]
    elif mask_row == (-1, 0, 2):
        assert _bits(after[0]) == _bits(before[0]) and _bits(after[2]) == _bits(before[2]) and torch.isneginf(after[1]).any()
    else:
        assert _bits(after[1]) == _bits(before[1]) and _bits(after[2]) == _bits(before[2]) and torch.isneginf(after[0]).any()


@pytest.mark.parametrize("shape", [(1, 1), (2, 3)], ids=["1x1", "2x3"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_full_vocabulary_rows_are_cut_into_slices(K_, dtype, shape):
    """V = 152064: 4752 mask words per row, cut into slices of whole words by the launcher; an allow-list of 4 (the stream of
    16-byte stores), a random mask (every chunk mixed), and a view one element off the 16-byte grid."""
    nb, K1 = shape
    V = 152064
    for shift, pad in ((0, 0), (1, 3)):
        buf, view = _arena(dtype, K1, V, pad, 5, shift=shift, nb=nb)
        rng = np.random.default_rng(5)
        four = ref_pack_bits([[0, 4127, 4128, V - 1]], V)[0]          # (4127 | 4128: either side of a slice boundary at B = 1)
        words = [four, _mask("random", V, rng, False)[0]][:nb]
        want = buf.clone()
        ref_logit_mask(view(want), np.stack(words), list(range(nb)))
        dev = buf.cuda()
        K_.logit_mask_rows(view(dev), _packed(K_, words, list(range(nb)), V, nb))
        torch.cuda.synchronize()
        assert _bits(dev) == _bits(want)
        assert int((~torch.isneginf(view(want)[0])).sum()) == 4 * K1


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
def test_mask_and_edit_commute(K_, dtype):
    V, K1 = 1003, 5
    rng = np.random.default_rng(3)
    buf, view = _arena(dtype, K1, V, 13, 3)
    made = [_mask("random", V, rng, True), _mask("runs", V, rng, False), _mask("0x55", V, rng, True)]
    masks = _packed(K_, [w for w, _ in made], [0, 1, 2], V)
    seq_len, start = [7, 9, 12], 5
    ids = [int(t) for t in rng.choice(V, 120, replace=False)]       # kept and masked ids alike: biases, bans, min_tokens-style bans
    rows = [[(t, float(np.float32(rng.uniform(-100, 100))) if i % 3 else 0.0, (0, FOREVER, 4 + b)[i % 3]) for i, t in enumerate(ids)]
            for b in range(B)]
    edits = K_.pack_logit_edits(rows, "cuda")
    seq = torch.tensor(seq_len, dtype=torch.int32, device="cuda")
    a, b = buf.cuda(), buf.cuda()
    K_.logit_edit_rows(K_.logit_mask_rows(view(a), masks), edits, seq, start)
    K_.logit_mask_rows(K_.logit_edit_rows(view(b), edits, seq, start), masks)
    torch.cuda.synchronize()
    assert _bits(a) == _bits(b)
    want = buf.clone()
    ref_logit_edit(ref_logit_mask(view(want), np.stack([w for w, _ in made]), [0, 1, 2]), rows, seq_len, start)
    assert _bits(a) == _bits(want) and _bits(a) != _bits(buf)


def test_nothing_is_touched_without_rows_or_masks(K_):
    from asd_amd import _binding
    lib = _binding.load_library()
    x = torch.randn((B, 2, 64), device="cuda")
    keep = x.clone()
    bits = torch.zeros((1, 2), dtype=torch.int32, device="cuda")     # all clear: a launch would write everything
    args = lambda Bv, K1, V, R: (x.data_ptr(), 0, 128, 64, Bv, K1, V, bits.data_ptr(), R, None, None)      # noqa: E731
    assert lib.asd_logit_mask_rows(*args(0, 2, 64, 1)) == 0
    assert lib.asd_logit_mask_rows(*args(B, 0, 64, 1)) == 0
    assert lib.asd_logit_mask_rows(*args(B, 2, 0, 1)) == 0
    assert lib.asd_logit_mask_rows(*args(B, 2, 64, 0)) == 0
    # ... before the pointers and the dtype are looked at
    assert lib.asd_logit_mask_rows(None, 99, 0, 0, 0, 1, 64, None, 1, None, None) == 0
    # every row without a list: pack_token_masks uploads no mask, the call launches nothing
    none = K_.pack_token_masks([None] * B, 64, "cuda")
    assert none.R == 0 and none.mask_row.tolist() == [-1] * B
    K_.logit_mask_rows(x, none)
    torch.cuda.synchronize()
    assert torch.equal(x, keep)
    assert lib.asd_logit_mask_rows(*args(B, 2, 64, 1)) == 0
    torch.cuda.synchronize()
    assert torch.isneginf(x).all()


def test_argument_errors_return_their_codes(K_):
    from asd_amd import _binding
    lib = _binding.load_library()
    INVALID, UNSUPPORTED, ALIGNMENT = -1, -2, -5
    x = torch.randn((B, 2, 64), device="cuda")
    keep = x.clone()
    m = K_.pack_token_masks([(1, 2, 63)] * B, 64, "cuda")
    assert m.R == 1 and m.mask_row is None and tuple(m.bits.shape) == (1, 2)
    good = dict(logits=x.data_ptr(), dtype=0, ld_seq=128, ld_row=64, B=B, K1=2, V=64, bits=m.bits.data_ptr(), R=1, row=None,
                stream=None)

    def call(**kw):
        return lib.asd_logit_mask_rows(*{**good, **kw}.values())
    for kw in (dict(B=-1), dict(K1=-1), dict(V=-1), dict(R=-1)):
        assert call(**kw) == INVALID, kw
    for kw in (dict(logits=None), dict(bits=None), dict(ld_row=63), dict(ld_seq=127)):
        assert call(**kw) == INVALID, kw
    assert call(dtype=7) == UNSUPPORTED and call(dtype=-1) == UNSUPPORTED
    assert call(B=2 ** 31 - 1, K1=2, ld_seq=128) == UNSUPPORTED         # B * K1 > INT32_MAX
    assert call(logits=x.data_ptr() + 2) == ALIGNMENT
    assert call(bits=m.bits.data_ptr() + 2) == ALIGNMENT
    torch.cuda.synchronize()
    assert torch.equal(x, keep)
    assert call() == 0
    torch.cuda.synchronize()
    assert int(torch.isneginf(x).sum()) == B * 2 * 61 and torch.equal(x[:, :, [1, 2, 63]], keep[:, :, [1, 2, 63]])
    # the wrapper's own checks
    with pytest.raises(ValueError):
        K_.logit_mask_rows(x.cpu(), m)
    with pytest.raises(ValueError):
        K_.logit_mask_rows(x[:2], m)                                  # packed for 3 rows
    with pytest.raises(ValueError):
        K_.logit_mask_rows(x[:, :, :63], m)                           # packed for V = 64
    with pytest.raises(ValueError):
        K_.logit_mask_rows(x.transpose(1, 2), m)
    for bad in ([(0, 64)], [(-1,)]):
        with pytest.raises(ValueError):
            K_.pack_token_masks(bad, 64, "cuda")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
def test_existing_samplers_on_a_masked_tensor(K_, dtype):
    """The unchanged kernels on the new input class: 950 of 1000 logits of every row -inf from the mask kernel itself, then
    draft_sample and verify_accept through HipOps: draft_sample returns only kept ids, lp_t of a masked proposal is -inf and
    of a kept one within 2e-5 of the f64 log-prob over the kept set."""
    from asd_amd.distributed import HipOps
    ops = HipOps()
    V, K = 1000, 4
    inv_t = float(np.float32(1 / 0.7))
    rng = np.random.default_rng(5)
    g = torch.Generator().manual_seed(5)
    t_out = (torch.randn((B, K + 1, V), generator=g) * 3.0).to(dtype).cuda()
    d_all = (t_out.float() + 0.5 * torch.randn((B, K + 1, V), generator=g).cuda()).to(dtype)[:, :K].contiguous()
    lists = [tuple(sorted(int(t) for t in rng.choice(V, 50, replace=False))) for _ in range(B)]
    masks = ops.pack_token_masks(lists, V, "cuda")
    assert masks.R == B
    ops.logit_mask_rows(t_out, masks)
    ops.logit_mask_rows(d_all, masks)
    for b in range(B):
        assert int((~torch.isneginf(t_out[b])).sum()) == 50 * (K + 1) and int((~torch.isneginf(d_all[b])).sum()) == 50 * K
    toks, lpd = [], []
    for k in range(K):
        dl = d_all[:, k].contiguous()
        tok, lp, thr = ops.draft_sample(dl, torch.rand((B,), generator=g).cuda(), inv_t, 0.9)
        toks.append(tok), lpd.append(lp)
        for b in range(B):
            assert int(tok[b]) in lists[b]
            assert abs(float(lp[b]) - ref_logprob(dl[b].float().cpu().numpy(), int(tok[b]), inv_t, float(thr[b]))) <= LP_ATOL
    tok32 = torch.stack(toks, 1).to(torch.int32).contiguous()
    masked = next(t for t in range(V) if t not in lists[0])
    tok32[0, 1] = masked                                             # a masked proposal (never made by the loop): lp_t = -inf, rejected
    lp_d = torch.stack(lpd, 1).contiguous()
    score = t_out[:, :K].contiguous()
    u = torch.rand((B, K), generator=g).cuda()
    lp_t, accept, n_acc, _ = ops.verify_accept(score, tok32, lp_d, u, inv_t)
    n_kept = 0
    for b in range(B):
        for k in range(K):
            ref = ref_logprob(score[b, k].float().cpu().numpy(), int(tok32[b, k]), inv_t)       # -inf logits add nothing: the kept set
            if (b, k) == (0, 1):
                assert np.isneginf(ref) and np.isneginf(float(lp_t[b, k])) and int(accept[b, k]) == 0
            else:
                assert np.isfinite(ref) and abs(float(lp_t[b, k]) - ref) <= LP_ATOL
                n_kept += 1
    assert n_kept == B * K - 1 and int(n_acc[0]) <= 1
    ops.check_status()
