"""asd_penalty_rows and asd_penalty_commit on the GPU against tests/penalty_ref.py (numpy float32, the header's operation
order), bit for bit.  The WHOLE allocation -- a guard band in front, the tensor with its row padding, a guard band behind (the
arena of tests/test_gpu_logit_edit.py) -- is compared, so a stray write anywhere fails; for the commit kernel the whole seen /
counts allocations, guard bands included.  bf16 / f16 / f32; B = 3, K1 in {1, 5}, V in {1000, 1003} (the odd V with padded
rows); the [:, :4] slice of a [3, 5, V] tensor; V = 152064 at B = 2, K1 = 3 (a row cut into slices, seen ids on both sides of
every 4096-token boundary).  Row 1 of every launch is neutral."""
import numpy as np
import pytest
import torch

from tests.penalty_ref import ref_penalty, ref_penalty_commit, ref_seen_bits

pytestmark = pytest.mark.gpu

B = 3
GUARD = 256                                      # elements on either side
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
DTYPE_IDS = ["bf16", "f16", "f32"]
# rep > 1 with positive presence / frequency; the neutral row; rep < 1 with negative presence / frequency
PARAMS = np.array([[1.5, 0.75, 0.3], [1.0, 0.0, 0.0], [0.5, -1.0, -0.5]], dtype=np.float32)
UNSEEN = 5                                       # proposed by rows 0 and 2 alike, twice by row 0; in no row's state


@pytest.fixture(scope="module")
def K_():
    from asd_amd import kernels
    return kernels


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16).numpy().tobytes()


def _arena(dtype, K1, V, pad, seed, rows_alloc=None, nb=B):
    rows_alloc = K1 if rows_alloc is None else rows_alloc
    g = torch.Generator().manual_seed(seed)
    n = nb * rows_alloc * (V + pad)
    buf = (torch.randn(n + 2 * GUARD, generator=g) * 4.0).to(dtype)

    def view(b):
        return b[GUARD:GUARD + n].view(nb, rows_alloc, V + pad)[:, :K1, :V]
    return buf, view


def _state(V, seed, nb=B, extra=()):
    """-> (seen ids per row, counts int32 [nb, V]): ids 0, 31, 32, V - 1 and a few dozen random ones; 31 and half of the random
    ones are prompt-only (bit set, count 0); counts of 1 (id 0), 300 (id 32), 2 (V - 1) and 1..4."""
    rng = np.random.default_rng(seed)
    ids, counts = [], np.zeros((nb, V), dtype=np.int32)
    for b in range(nb):
        rand = [int(t) for t in rng.choice(np.arange(40, V - 1), 48, replace=False)]
        row = sorted({0, 31, 32, V - 1, *rand, *extra} - {UNSEEN, 7})
        ids.append(row)
        counts[b, 0], counts[b, 32], counts[b, V - 1] = 1, 300, 2
        for t in rand[::2]:
            counts[b, t] = int(rng.integers(1, 5))
    return ids, counts


def _fill(x, ids, dtype):
    """Logits of every kind at seen and proposed ids: positive, negative, 0.0, -inf; the f16 clamp at row 2."""
    V = x.shape[2]
    x[:, :, 0] = 3.25
    x[:, :, 31] = -2.5
    x[:, :, 32] = 0.0
    x[:, :, V - 1] = float("-inf")
    x[:, :, UNSEEN] = 1.75
    x[:, :, 7] = -0.0
    clamp = next(t for t in ids[2] if t > 40)
    x[2, :, clamp] = 60000.0                     # rep = 0.5: 120000, +inf in f16 -> stored as 65504
    return clamp


def _step_tok(V):
    # row 0: unseen, seen already, the same unseen id again, outside the vocabulary; row 1 (neutral): anything; row 2: the id
    # row 0 proposes, a negative id, another unseen id twice
    return np.array([[UNSEEN, 0, UNSEEN, V], [UNSEEN, UNSEEN, 0, 31], [UNSEEN, -1, 7, 7]], dtype=np.int32)


def _pen(K_, ids, counts, params, V):
    seen = ref_seen_bits(ids, V)
    return K_.Penalties(torch.from_numpy(seen.view(np.int32)).cuda(), torch.from_numpy(counts).cuda(),
                        torch.from_numpy(np.ascontiguousarray(params)).cuda(), len(ids), V), seen


def _run(K_, dtype, K1, V, pad, n_prev, seed, with_tok=True, rows_alloc=None):
    buf, view = _arena(dtype, K1, V, pad, seed, rows_alloc)
    ids, counts = _state(V, seed)
    clamp = _fill(view(buf), ids, dtype)
    pen, seen = _pen(K_, ids, counts, PARAMS, V)
    tok = _step_tok(V) if with_tok else None
    want = buf.clone()
    ref_penalty(view(want), seen, counts, PARAMS, tok, n_prev)
    dev = buf.cuda()
    x = view(dev)
    # (step_tok as a [:, :4] slice of a wider buffer: ld_tok > n_tok)
    tok_dev = None if tok is None else torch.from_numpy(np.concatenate([tok, np.full((B, 3), 9, np.int32)], 1)).cuda()[:, :4]
    out = K_.penalty_rows(x, pen, tok_dev, n_prev)
    torch.cuda.synchronize()
    assert out is x
    assert _bits(dev) == _bits(want)
    # the state is read, never written
    assert np.array_equal(pen.seen.cpu().numpy().view(np.uint32), seen) and np.array_equal(pen.counts.cpu().numpy(), counts)
    before, after = view(buf), view(want)
    # the reference did what the header says, independently of its arithmetic
    assert _bits(after[1]) == _bits(before[1])                                    # the neutral row
    assert torch.isneginf(after[:, :, V - 1]).all()                               # -inf stays -inf
    untouched = np.ones(V, dtype=bool)
    untouched[ids[0]] = False
    untouched[[UNSEEN, 0]] = False
    assert _bits(after[0][:, untouched]) == _bits(before[0][:, untouched])        # nothing but seen or proposed ids
    if dtype == torch.float16:
        assert float(after[2, 0, clamp]) == 65504.0                              # 120000 or more: the largest finite f16
    else:
        assert 110000.0 < float(after[2, 0, clamp]) < 130000.0
    if not with_tok:                                                             # id 0 of row 0, c = 1: the header's three steps
        y = np.float32(np.float32(np.float32(3.25) / np.float32(1.5)) - np.float32(np.float32(0.3) * np.float32(1.0))) - np.float32(0.75)
        assert float(after[0, 0, 0]) == float(torch.tensor(y).to(dtype))
    return before, after


@pytest.mark.parametrize("V,pad", [(1000, 0), (1003, 13)])
@pytest.mark.parametrize("K1,n_prev", [(1, 3), (5, 0)])
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_kernel_matches_the_reference_bit_for_bit(K_, dtype, K1, n_prev, V, pad):
    before, after = _run(K_, dtype, K1, V, pad, n_prev, seed=K1 * 10000 + V)
    f = lambda t: t.float().numpy()                                               # noqa: E731
    # an unseen proposal is seen by the positions behind it only: row 0 proposes UNSEEN at slots 0 and 2
    if K1 == 5:
        assert _bits(after[0, 0, UNSEEN]) == _bits(before[0, 0, UNSEEN])          # position 0 sees no proposal
        got = f(after[0, :, UNSEEN])
        assert got[1] == got[2] and got[3] < got[2] and got[4] == got[3]          # c = 1, 1, 2, 2 at positions 1..4
        assert _bits(after[2, 1, 7]) == _bits(before[2, 1, 7])                    # row 2 proposes 7 at slots 2 and 3
        assert f(after[2, 4, 7]) > f(after[2, 3, 7]) > 0                          # -0.0 * 0.5 + 0.5 c + 1.0: negative penalties
    else:
        assert f(after[0, 0, UNSEEN]) < f(before[0, 0, UNSEEN])                   # n_prev = 3 sees slots 0..2: c = 2
        assert _bits(after[2, 0, 7]) != _bits(before[2, 0, 7])                    # slot 2 is seen, slot 3 is not: c = 1


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_no_proposals_and_a_non_contiguous_slice(K_, dtype):
    for V, pad in ((1000, 0), (1003, 13)):
        _run(K_, dtype, 1, V, pad, 0, seed=V + 1, with_tok=False)                 # stage 0's call: step_tok NULL
        _run(K_, dtype, 5, V, pad, 0, seed=V + 2, with_tok=False)
    # the [:, :4] slice of a [3, 5, V] tensor: ld_seq = 5 V, K1 = 4; row 4 of every sequence is not touched
    before, _ = _run(K_, dtype, 4, 1000, 0, 0, seed=77, rows_alloc=5)
    assert before.stride(0) == 5 * 1000 and before.shape == (B, 4, 1000)


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_full_vocabulary_rows_are_cut_into_slices(K_, dtype):
    """V = 152064: 4752 mask words per row, cut into slices of whole words by the launcher; seen ids on both sides of every
    4096-token boundary (every slice boundary the launcher can choose is one), 2048 random ones, proposals seen and unseen."""
    V, nb, K1 = 152064, 2, 3
    rng = np.random.default_rng(9)
    edges = [t for k in range(1, V // 4096 + 1) for t in (k * 4096 - 1, k * 4096)]
    buf, view = _arena(dtype, K1, V, 3, 9, nb=nb)
    ids, counts = [], np.zeros((nb, V), dtype=np.int32)
    for b in range(nb):
        row = sorted({0, V - 1, *edges, *(int(t) for t in rng.choice(V, 2048, replace=False))} - {8193, 100001})
        ids.append(row)
        counts[b, row[::3]] = rng.integers(1, 300, len(row[::3]))
    params = np.array([[1.2, 0.5, 0.25], [0.75, -0.5, 1.5]], dtype=np.float32)
    tok = np.array([[8191, 8193], [100001, 100001]], dtype=np.int32)              # seen | unseen, across a boundary; one id twice
    pen, seen = _pen(K_, ids, counts, params, V)
    want = buf.clone()
    ref_penalty(view(want), seen, counts, params, tok, 0)
    dev = buf.cuda()
    K_.penalty_rows(view(dev), pen, torch.from_numpy(tok).cuda(), 0)
    torch.cuda.synchronize()
    assert _bits(dev) == _bits(want) and _bits(want) != _bits(buf)
    for t in (4095, 4096, 8191, 8192, 147455, 147456, V - 1):
        assert _bits(view(want)[0, :, t]) != _bits(view(buf)[0, :, t])
    assert _bits(view(want)[0, 0, 8193]) == _bits(view(buf)[0, 0, 8193]) and _bits(view(want)[0, 2, 8193]) != _bits(view(buf)[0, 2, 8193])


def test_a_damaged_repetition_penalty_reads_as_one(K_):
    V = 1000
    ids, counts = _state(V, 3)
    for rep in (0.0, -1.5, float("nan")):
        params = np.array([[rep, 0.5, 0.25]] * B, dtype=np.float32)
        pen, seen = _pen(K_, ids, counts, params, V)
        buf, view = _arena(torch.float32, 2, V, 0, 3)
        want = buf.clone()
        ref_penalty(view(want), seen, counts, np.array([[1.0, 0.5, 0.25]] * B, dtype=np.float32))
        dev = buf.cuda()
        K_.penalty_rows(view(dev), pen)
        torch.cuda.synchronize()
        assert _bits(dev) == _bits(want) and _bits(want) != _bits(buf)


# ------------------------------------------------------------------------------------------ asd_penalty_commit
def _guarded(a, fill):
    """-> (the whole allocation on the device, the view of `a` inside it)."""
    flat = np.full(a.size + 2 * GUARD, fill, dtype=a.dtype)
    flat[GUARD:GUARD + a.size] = a.reshape(-1)
    dev = torch.from_numpy(flat).cuda()
    return dev, dev[GUARD:GUARD + a.size].view(*a.shape)


def test_commit_counts_every_token_once_and_sets_its_bit(K_):
    V, nb, cap = 1000, 4, 16
    rng = np.random.default_rng(4)
    tokens = rng.integers(0, V, (nb, cap)).astype(np.int32)
    seq_len = np.array([5, 9, 12, 16], dtype=np.int32)
    n_commit = np.array([0, 1, 3, 5], dtype=np.int32)
    tokens[2, 9:12] = [40, 7, 40]                                                 # one id twice in a step
    tokens[3, 11:16] = [64, 65, 64, V, 95]                                        # three ids of mask word 2; an id outside [0, V)
    prompt = [[1, 2, 3], [31, 32], [40], [V - 1, 0]]
    seen = ref_seen_bits(prompt, V)
    counts = np.zeros((nb, V), dtype=np.int32)
    counts[2, 40] = 299                                                           # (its bit is set: the prompt holds it)
    seen_dev, seen_view = _guarded(seen.view(np.int32), -1)
    counts_dev, counts_view = _guarded(counts, 7)
    pen = K_.Penalties(seen_view, counts_view, torch.zeros((nb, 3), device="cuda"), nb, V)
    tok_dev = torch.from_numpy(tokens).cuda()
    for call in range(2):                                                         # two consecutive steps
        K_.penalty_commit(tok_dev, torch.from_numpy(seq_len).cuda(), torch.from_numpy(n_commit).cuda(), pen, cap)
        torch.cuda.synchronize()
        ref_penalty_commit(tokens, seq_len, n_commit, V, cap, seen, counts)
        got_seen, got_counts = seen_dev.cpu().numpy(), counts_dev.cpu().numpy()
        assert (got_seen[:GUARD] == -1).all() and (got_seen[-GUARD:] == -1).all()
        assert (got_counts[:GUARD] == 7).all() and (got_counts[-GUARD:] == 7).all()
        assert np.array_equal(got_seen[GUARD:-GUARD].view(np.uint32).reshape(nb, -1), seen)
        assert np.array_equal(got_counts[GUARD:-GUARD].reshape(nb, V), counts)
        if call == 0:
            assert counts[0].sum() == 0 and counts[1].sum() == 1 and counts[2, 40] == 301 and counts[2, 7] == 1
            assert counts[3, 64] == 2 and counts[3].sum() == 4 and int(seen[3, 2]) == 0b11 | (1 << 31)
            # the next step: row 0 commits now, row 3 has finished (n_commit 0: its state must not move), row 1 repeats a token
            tokens[0, 5:7] = [500, 500]
            tokens[1, 9:11] = [tokens[1, 8], 31]
            seq_len = np.array([7, 11, 14, 16], dtype=np.int32)
            n_commit = np.array([2, 2, 2, 0], dtype=np.int32)
            tok_dev = torch.from_numpy(tokens).cuda()
    assert counts[0, 500] == 2 and counts[1, tokens[1, 8]] == 2 and counts[3].sum() == 4


# ------------------------------------------------------------------------------------------ status codes
def test_argument_errors_return_their_codes(K_):
    from asd_amd import _binding
    lib = _binding.load_library()
    INVALID, UNSUPPORTED, ALIGNMENT = -1, -2, -5
    V = 64
    x = torch.randn((B, 2, V), device="cuda")
    keep = x.clone()
    pen = K_.pack_penalties([1.5] * B, [0.5] * B, [0.25] * B, [[1, 2, 63]] * B, V, "cuda")
    assert tuple(pen.seen.shape) == (B, 2) and tuple(pen.counts.shape) == (B, V) and not pen.counts.any()
    assert np.array_equal(pen.seen.cpu().numpy().view(np.uint32), ref_seen_bits([[1, 2, 63]] * B, V))
    tok = torch.zeros((B, 4), dtype=torch.int32, device="cuda")
    good = dict(logits=x.data_ptr(), dtype=0, ld_seq=2 * V, ld_row=V, B=B, K1=2, V=V, seen=pen.seen.data_ptr(),
                counts=pen.counts.data_ptr(), params=pen.params.data_ptr(), tok=tok.data_ptr(), ld_tok=4, n_tok=4, n_prev=3,
                stream=None)

    def call(**kw):
        return lib.asd_penalty_rows(*{**good, **kw}.values())
    for kw in (dict(B=-1), dict(K1=-1), dict(V=-1), dict(n_tok=-1), dict(n_prev=-1)):
        assert call(**kw) == INVALID, kw
    # nothing to do: ASD_OK before the pointers and the dtype are looked at
    assert call(B=0) == 0 and call(K1=0) == 0 and call(V=0) == 0
    assert lib.asd_penalty_rows(None, 99, 0, 0, 0, 1, V, None, None, None, None, 0, 0, 0, None) == 0
    assert call(dtype=7) == UNSUPPORTED and call(dtype=-1) == UNSUPPORTED
    assert call(n_tok=65, ld_tok=65) == UNSUPPORTED
    for kw in (dict(logits=None), dict(seen=None), dict(counts=None), dict(params=None), dict(ld_row=V - 1), dict(ld_seq=2 * V - 1),
               dict(tok=None), dict(n_prev=4), dict(n_tok=3, ld_tok=3), dict(ld_tok=3)):
        assert call(**kw) == INVALID, kw          # (tok NULL with n_prev 3; position 1 would see 5 of 4, or 4 of 3; ld_tok < n_tok)
    for name in ("logits", "seen", "counts", "params", "tok"):
        assert call(**{name: good[name] + 2}) == ALIGNMENT, name
    torch.cuda.synchronize()
    assert torch.equal(x, keep)
    assert call() == 0 and call(tok=None, n_prev=0) == 0
    torch.cuda.synchronize()
    assert not torch.equal(x[:, :, [1, 2, 63]], keep[:, :, [1, 2, 63]])
    others = [v for v in range(V) if v not in (0, 1, 2, 63)]                       # (0: the proposals of `tok`)
    assert torch.equal(x[:, :, others], keep[:, :, others])

    tokens = torch.zeros((B, 8), dtype=torch.int32, device="cuda")
    seq = torch.full((B,), 4, dtype=torch.int32, device="cuda")
    n = torch.ones((B,), dtype=torch.int32, device="cuda")
    good_c = dict(tokens=tokens.data_ptr(), ld=8, seq=seq.data_ptr(), n=n.data_ptr(), B=B, V=V, cap=8, seen=pen.seen.data_ptr(),
                  counts=pen.counts.data_ptr(), stream=None)

    def commit(**kw):
        return lib.asd_penalty_commit(*{**good_c, **kw}.values())
    for kw in (dict(B=-1), dict(V=-1), dict(cap=-1)):
        assert commit(**kw) == INVALID, kw
    assert commit(B=0) == 0 and commit(V=0) == 0 and commit(cap=0) == 0
    assert lib.asd_penalty_commit(None, 0, None, None, 0, V, 8, None, None, None) == 0
    for kw in (dict(tokens=None), dict(seq=None), dict(n=None), dict(seen=None), dict(counts=None), dict(ld=7)):
        assert commit(**kw) == INVALID, kw
    for name in ("tokens", "seq", "n", "seen", "counts"):
        assert commit(**{name: good_c[name] + 2}) == ALIGNMENT, name
    torch.cuda.synchronize()
    assert not pen.counts.any()
    assert commit() == 0
    torch.cuda.synchronize()
    assert pen.counts[:, 0].tolist() == [1] * B and int(pen.counts.sum()) == B and (pen.seen[:, 0] & 1).tolist() == [1] * B

    # the wrappers' own checks
    with pytest.raises(ValueError):
        K_.penalty_rows(x.cpu(), pen)
    with pytest.raises(ValueError):
        K_.penalty_rows(x[:2], pen)                                   # packed for 3 rows
    with pytest.raises(ValueError):
        K_.penalty_rows(x[:, :, :63], pen)                            # packed for V = 64
    with pytest.raises(ValueError):
        K_.penalty_rows(x, pen, None, 1)                              # n_prev without step_tok
    with pytest.raises(ValueError):
        K_.penalty_rows(x, pen, tok, 4)                               # position 1 would see 5 proposals of 4
    with pytest.raises(ValueError):
        K_.penalty_rows(x, pen, tok.to(torch.int64), 0)
    with pytest.raises(ValueError):
        K_.penalty_commit(tokens[:2], seq, n, pen, 8)
    for bad in (dict(prompt_ids=[[V]] * B), dict(prompt_ids=[[-1]] * B), dict(rep=[0.0] * B), dict(freq=[float("nan")] * B),
                dict(rep=[1.0] * 2)):
        args = dict(rep=[1.5] * B, pres=[0.5] * B, freq=[0.25] * B, prompt_ids=[[1]] * B)
        args.update(bad)
        with pytest.raises(ValueError):
            K_.pack_penalties(args["rep"], args["pres"], args["freq"], args["prompt_ids"], V, "cuda")
