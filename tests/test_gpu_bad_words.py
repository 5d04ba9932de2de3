"""asd_bad_words_rows on the GPU against tests/bad_words_ref.py (numpy, the header's text), bit for bit.  The WHOLE allocation --
a guard band in front, the tensor with its row padding, a guard band behind (the arena of tests/test_gpu_penalty.py) -- is
compared, so a stray write anywhere fails.  bf16 / f16 / f32; B = 3, K1 in {1, 5}, V in {1000, 1003} (the odd V with padded
rows); the [:, :4] slice of a [3, 5, V] tensor; V = 152064 at B = 2, K1 = 3.  Row 1 of every per-row launch has no word.

The history (START = 6 prompt tokens, which are NOT history; MAX_LEN = 20 of LD_TOKENS = 24):
    row 0   prompt 1 2 3 4 10 77 | generated 20 21 22 23 24 25 26 10 | proposals 30 31 32 33
    row 2   prompt 9 9 9 60 61 62 | generated 50                      | proposals 51 52 53 54
Every index the kernel forms is clamped by contract: no case here can leave an array."""
import numpy as np
import pytest
import torch

from tests.bad_words_ref import ref_bad_words

pytestmark = pytest.mark.gpu

B = 3
GUARD = 256                                      # elements on either side
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
DTYPE_IDS = ["bf16", "f16", "f32"]
START, MAX_LEN, LD_TOKENS = 6, 20, 24
SEQ_LEN = [14, 9, 7]
STEP_TOK = np.array([[30, 31, 32, 33], [30, 31, 32, 33], [51, 52, 53, 54]], dtype=np.int32)


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


def _tokens():
    t = np.full((B, LD_TOKENS), 999, dtype=np.int32)                 # 999 behind every row's end: never history
    t[0, :14] = [1, 2, 3, 4, 10, 77, 20, 21, 22, 23, 24, 25, 26, 10]
    t[1, :9] = [1, 2, 3, 4, 5, 6, 30, 31, 32]
    t[2, :7] = [9, 9, 9, 60, 61, 62, 50]
    return t


def _words(V):
    row0 = [(5,),                                # one token: always
            (10, 11), (26, 10, 11),              # entirely in `tokens`; two words ending in one id
            (26, 10, 12),
            (10, 30, 40),                        # straddling `tokens` and the proposals: position 1
            (30, 31, 32, 41),                    # entirely in the proposals: position 3, not position 2
            (21, 22, 23, 24, 25, 26, 10, 42),    # 8 tokens, in `tokens`
            (24, 25, 26, 10, 30, 31, 32, 43),    # 8 tokens, straddling: position 3
            (10, V - 1),                         # the last element of the row
            (10, V), (10, -1),                   # a last id outside [0, V): skipped
            (-1, 44), (V, 45),                   # prefix ids outside the vocabulary: compared as integers, never matched
            (77, 10, 46),                        # 77 ends the prompt and 10 the generated tokens: not neighbours in the history
            (4, 10, 47)]                         # the prompt's 4 10: not history
    row2 = [(62, 50, 51),                        # would match only by reading the prompt token 62: a history shorter than the prefix
            (61, 62, 50, 55),
            (50, 56),                            # position 0
            (50, 51, 52),                        # straddling: position 1
            (9, 9, 9, 60, 61, 62, 50, 57),       # 8 tokens, the whole prompt in front: never
            (51, 52, 53, 58)]                    # position 3
    return [row0, [], row2]


def _run(K_, dtype, K1, V, pad, n_prev, seed, rows=None, rows_alloc=None, seq_len=None, with_tok=True):
    rows = _words(V) if rows is None else rows
    seq_len = SEQ_LEN if seq_len is None else seq_len
    buf, view = _arena(dtype, K1, V, pad, seed, rows_alloc)
    view(buf)[0, :, 5] = float("-inf")                               # an element that is -inf already
    view(buf)[2, :, 56] = float("-inf")
    tokens = _tokens()
    tok = STEP_TOK if with_tok else None
    want = buf.clone()
    ref_bad_words(view(want), rows, tokens, seq_len, START, MAX_LEN, tok, n_prev)
    dev = buf.cuda()
    x = view(dev)
    words = K_.pack_bad_words(rows, "cuda")
    # (step_tok as a [:, :4] slice of a wider buffer: ld_tok > n_tok)
    tok_dev = None if tok is None else torch.from_numpy(np.concatenate([tok, np.full((B, 3), 10, np.int32)], 1)).cuda()[:, :4]
    out = K_.bad_words_rows(x, words, torch.from_numpy(tokens).cuda(), torch.tensor(seq_len, dtype=torch.int32).cuda(), START,
                            MAX_LEN, tok_dev, n_prev)
    torch.cuda.synchronize()
    assert out is x
    assert _bits(dev) == _bits(want)
    return view(buf), view(want), words


def _banned(before, after, b, j):
    """The ids the reference banned at (b, j): -inf now, finite before."""
    return set(torch.nonzero(torch.isneginf(after[b, j]) & ~torch.isneginf(before[b, j])).flatten().tolist())


@pytest.mark.parametrize("V,pad", [(1000, 0), (1003, 13)])
@pytest.mark.parametrize("K1,n_prev", [(1, 3), (5, 0)])
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_kernel_matches_the_reference_bit_for_bit(K_, dtype, K1, n_prev, V, pad):
    before, after, words = _run(K_, dtype, K1, V, pad, n_prev, seed=K1 * 10000 + V)
    assert words.row_first is not None and words.row_first.tolist() == [0, 15, 15, 21]
    # the reference did what the header says, whatever its code
    assert _bits(after[1]) == _bits(before[1])                                    # the row without a word
    if K1 == 5:
        assert _banned(before, after, 0, 0) == {11, 12, 42, V - 1}                # (5 was -inf already)
        assert _banned(before, after, 0, 1) == {40} and _banned(before, after, 0, 2) == set()
        assert _banned(before, after, 0, 3) == {41, 43} and _banned(before, after, 0, 4) == set()
        assert [_banned(before, after, 2, j) for j in range(5)] == [set(), {52}, set(), {58}, set()]   # (56 was -inf already)
    else:                                                                         # one proposal row, which sees 3 proposals
        assert _banned(before, after, 0, 0) == {41, 43} and _banned(before, after, 2, 0) == {58}
    assert torch.isneginf(after[0, :, 5]).all() and torch.isneginf(after[2, 0, 56])


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_no_proposals_a_shared_list_and_a_non_contiguous_slice(K_, dtype):
    for V, pad in ((1000, 0), (1003, 13)):
        before, after, _ = _run(K_, dtype, 1, V, pad, 0, seed=V + 1, with_tok=False)     # stage 0's call: step_tok NULL
        assert _banned(before, after, 0, 0) == {11, 12, 42, V - 1} and _banned(before, after, 2, 0) == set()
        # one list for every row: row_first NULL.  Row 1's history 30 31 32 now completes row 0's word (30, 31, 32, 41)
        before, after, words = _run(K_, dtype, 5, V, pad, 0, seed=V + 2, rows=[_words(V)[0]] * B)
        assert words.row_first is None and words.n == 15
        assert _banned(before, after, 1, 0) == {5, 41} and _banned(before, after, 2, 0) == {5}
    # the [:, :4] slice of a [3, 5, V] tensor: ld_seq = 5 V, K1 = 4; row 4 of every sequence is not touched
    before, after, _ = _run(K_, dtype, 4, 1000, 0, 0, seed=77, rows_alloc=5)
    assert before.stride(0) == 5 * 1000 and before.shape == (B, 4, 1000) and _banned(before, after, 0, 3) == {41, 43}


def test_a_row_with_256_words_and_a_damaged_seq_len(K_):
    V = 1000
    # 255 one-token words and, on the last lane, the bigram that the history completes
    many = [(t,) for t in range(100, 355)] + [(10, 11)]
    before, after, words = _run(K_, torch.bfloat16, 5, V, 0, 0, seed=5, rows=[many, [], _words(V)[2]])
    assert words.row_first.tolist() == [0, 256, 256, 262]
    assert _banned(before, after, 0, 0) == set(range(100, 355)) | {11} and _banned(before, after, 0, 1) == set(range(100, 355))
    # seq_len beyond max_len is clamped to it (the history then ends in 999 999), below start to start (no committed history)
    rows = [[(999, 999, 60), (10, 11)], [(61,), (30, 62)], [(50, 56), (51, 63)]]
    before, after, _ = _run(K_, torch.float32, 5, V, 0, 0, seed=6, rows=rows, seq_len=[2 ** 31 - 1, -5, 3])
    assert _banned(before, after, 0, 0) == {60} and _banned(before, after, 1, 0) == {61}
    assert _banned(before, after, 1, 1) == {61, 62} and _banned(before, after, 2, 0) == set() and _banned(before, after, 2, 1) == {63}


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_full_vocabulary(K_, dtype):
    V, nb, K1 = 152064, 2, 3
    buf, view = _arena(dtype, K1, V, 3, 9, nb=nb)
    tokens = np.zeros((nb, 16), dtype=np.int32)
    tokens[0, 4:8] = [V - 1, 4096, 4095, 151000]
    tokens[1, 4:6] = [7, 8]
    seq_len = [8, 6]
    tok = np.array([[V - 2, 0], [8, 8]], dtype=np.int32)
    rows = [[(151000, V - 1), (4095, 151000, 0), (V - 1,), (151000, V - 2, 131072), (V - 2, 0, 65536), (151000, V)],
            [(8, 8, 8, 100000), (7, 8, 4096), (8, 4095)]]
    want = buf.clone()
    ref_bad_words(view(want), rows, tokens, seq_len, 4, 16, tok, 0)
    dev = buf.cuda()
    K_.bad_words_rows(view(dev), K_.pack_bad_words(rows, "cuda"), torch.from_numpy(tokens).cuda(),
                      torch.tensor(seq_len, dtype=torch.int32).cuda(), 4, 16, torch.from_numpy(tok).cuda(), 0)
    torch.cuda.synchronize()
    assert _bits(dev) == _bits(want)
    before, after = view(buf), view(want)
    assert [_banned(before, after, 0, j) for j in range(3)] == [{V - 1, 0}, {V - 1, 131072}, {V - 1, 65536}]
    assert [_banned(before, after, 1, j) for j in range(3)] == [{4096, 4095}, {4095}, {4095, 100000}]


def test_argument_errors_return_their_codes(K_):
    from asd_amd import _binding
    lib = _binding.load_library()
    INVALID, UNSUPPORTED, ALIGNMENT = -1, -2, -5
    V = 64
    x = torch.randn((B, 2, V), device="cuda")
    keep = x.clone()
    words = K_.pack_bad_words([[(1, 2), (3,)]] * B, "cuda")
    first = torch.tensor([0, 2, 2, 2], dtype=torch.int32, device="cuda")
    tokens = torch.ones((B, 8), dtype=torch.int32, device="cuda")
    seq = torch.full((B,), 5, dtype=torch.int32, device="cuda")
    tok = torch.zeros((B, 4), dtype=torch.int32, device="cuda")
    good = dict(logits=x.data_ptr(), dtype=0, ld_seq=2 * V, ld_row=V, B=B, K1=2, V=V, word_tok=words.word_tok.data_ptr(),
                word_n=words.word_n.data_ptr(), row_first=first.data_ptr(), n=2, tokens=tokens.data_ptr(), ld_tokens=8,
                seq_len=seq.data_ptr(), start=4, max_len=8, tok=tok.data_ptr(), ld_tok=4, n_tok=4, n_prev=3, stream=None)

    def call(**kw):
        return lib.asd_bad_words_rows(*{**good, **kw}.values())
    for kw in (dict(B=-1), dict(K1=-1), dict(V=-1), dict(n=-1), dict(n_tok=-1), dict(n_prev=-1), dict(start=-1), dict(max_len=-1),
               dict(B=0, n_prev=-1)):                                             # ... before the empty batch
        assert call(**kw) == INVALID, kw
    # nothing to do: ASD_OK before the pointers and the dtype are looked at
    assert call(B=0) == 0 and call(K1=0) == 0 and call(V=0) == 0 and call(n=0) == 0
    assert lib.asd_bad_words_rows(None, 99, 0, 0, 0, 1, V, None, None, None, 1, None, 0, None, 0, 0, None, 0, 0, 0, None) == 0
    assert call(dtype=7) == UNSUPPORTED and call(dtype=-1) == UNSUPPORTED
    assert call(row_first=None, n=257) == UNSUPPORTED and call(n=257, ld_row=V - 1) == INVALID   # only a shared list is bounded here
    assert call(n_tok=65, ld_tok=65) == UNSUPPORTED
    assert call(dtype=7, logits=None) == UNSUPPORTED                             # unsupported comes before the NULL checks
    for kw in (dict(logits=None), dict(word_tok=None), dict(word_n=None), dict(tokens=None), dict(seq_len=None), dict(ld_row=V - 1),
               dict(ld_seq=2 * V - 1), dict(ld_tokens=7), dict(start=9), dict(tok=None), dict(n_prev=4), dict(n_tok=3, ld_tok=3),
               dict(ld_tok=3)):
        assert call(**kw) == INVALID, kw          # (tok NULL with n_prev 3; position 1 would see 5 of 4, or 4 of 3; ld_tok < n_tok)
    assert call(logits=good["logits"] + 2, ld_row=V - 1) == INVALID               # invalid comes before alignment
    for name in ("logits", "word_tok", "word_n", "row_first", "tokens", "seq_len", "tok"):
        assert call(**{name: good[name] + 2}) == ALIGNMENT, name
    torch.cuda.synchronize()
    assert torch.equal(x, keep)                                                   # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    # row 0 alone owns the words; (3,) always; (1, 2) not: behind the committed 1 both positions see three proposals, all 0
    assert torch.isneginf(x[0, :, 3]).all() and torch.equal(x[1:], keep[1:]) and torch.equal(x[0, :, 2], keep[0, :, 2])
    assert call(row_first=None, tok=None, n_prev=0) == 0                          # every row, and no position sees a proposal
    torch.cuda.synchronize()
    assert torch.isneginf(x[:, :, 3]).all() and torch.isneginf(x[:, :, 2]).all()   # (1, 2): the history ends in the committed 1
    others = [v for v in range(V) if v not in (2, 3)]
    assert torch.equal(x[:, :, others], keep[:, :, others])

    # the wrappers' own checks
    with pytest.raises(ValueError):
        K_.bad_words_rows(x.cpu(), words, tokens, seq, 4, 8)
    with pytest.raises(ValueError):
        K_.bad_words_rows(x[:2], words, tokens[:2], seq[:2], 4, 8)               # packed for 3 rows
    with pytest.raises(ValueError):
        K_.bad_words_rows(x, words, tokens, seq, 4, 9)                            # max_len beyond the token rows
    with pytest.raises(ValueError):
        K_.bad_words_rows(x, words, tokens, seq, 9, 8)                            # start beyond max_len
    with pytest.raises(ValueError):
        K_.bad_words_rows(x, words, tokens, seq, 4, 8, None, 1)                   # n_prev without step_tok
    with pytest.raises(ValueError):
        K_.bad_words_rows(x, words, tokens, seq, 4, 8, tok, 4)                    # position 1 would see 5 proposals of 4
    with pytest.raises(ValueError):
        K_.bad_words_rows(x, words, tokens, seq, 4, 8, tok.to(torch.int64), 0)
    for bad in ([[()]], [[tuple(range(9))]], [[(1,)] * 257], [[(2 ** 31,)]]):
        with pytest.raises(ValueError):
            K_.pack_bad_words(bad, "cuda")
