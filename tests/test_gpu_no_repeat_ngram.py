"""asd_no_repeat_ngram_rows on the GPU against tests/ngram_ref.py (numpy, the header's text), bit for bit.  The WHOLE allocation
-- a guard band in front, the tensor with its row padding (ld_row = V + 13), a guard band behind -- is compared, so a stray write
anywhere fails.  bf16 / f16 / f32; V = 70 with ids drawn from 3 to 4 symbols, so that matches are dense; K1 = 1 with n_prev 0
(no proposal buffer) and 3, K1 = 5 with n_prev 0; n in {1, 2, 3, 8}, a per-row mix that includes 0, 9 and -1, and one n for every
row.  ONE launch covers every history length: the rows of the batch differ.  For every n the committed history has 0, n-2, n-1,
n, n+1 tokens and -1, 0, +1, n-2, n-1, n tokens around 256 (the workgroup's lanes) and around every slice boundary the launcher
forms (ASD_NGRAM_SLICE n-gram starts per workgroup; MAX_LEN gives three slices), so both the history length and the number of
n-gram starts pass every boundary.  The reference's ban masks are computed once per (K1, n_prev) and shared by the dtypes.

Hand-written rows (START = 8 prompt slots, of which row_start marks the real ones):
    "prompt"     real prompt 5 6 5                      n = 2: 6 is banned by the prompt alone
    "padding"    slots 0 0 0 0 0 0 7 0, row_start 6     n = 2: H = 7 0; the pad 0 in front of 7 would complete 0 -> 7 and 0 -> 0
    "generated"  no prompt, generated 5 6 5             n = 2: 6
    "proposals"  nothing committed, proposals 5 6 5 9   n = 2: 6 at the position that sees three proposals, nothing elsewhere
    "seams"      prompt 5, generated 6 8 5, proposals 6 ..  n = 3: 8 once the first proposal is seen
    "one symbol" generated 4 x 10                       n = 3: 4 (the first n-gram of H, and the last, which overlaps the suffix)
    "odd ids"    generated -1 70 -1 3 -1                n = 2: 3; 70 = V is never a store index
Every index the kernel forms is clamped by contract: no case here can leave an array."""
import functools

import numpy as np
import pytest
import torch

from tests.ngram_ref import ref_no_repeat_ngram

pytestmark = pytest.mark.gpu

V, PAD = 70, 13
GUARD = 256                                      # elements on either side
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
DTYPE_IDS = ["bf16", "f16", "f32"]
START = 8                                        # the padded prompt length
N_TOK = 4
SYMBOLS = (3, 17, 42, 69)                        # 69 = V - 1: the last element of a row
CONFIGS = [(1, 0, False), (1, 3, True), (5, 0, True)]            # (K1, n_prev, with step_tok)


@pytest.fixture(scope="module")
def K_():
    from asd_amd import kernels
    return kernels


def _slice():
    from asd_amd import _binding
    return _binding.NGRAM_SLICE


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16).numpy().tobytes()


def _arena(dtype, nb, K1, v, pad, seed, rows_alloc=None):
    rows_alloc = K1 if rows_alloc is None else rows_alloc
    g = torch.Generator().manual_seed(seed)
    n = nb * rows_alloc * (v + pad)
    buf = (torch.randn(n + 2 * GUARD, generator=g) * 4.0).to(dtype)

    def view(b):
        return b[GUARD:GUARD + n].view(nb, rows_alloc, v + pad)[:, :K1, :v]
    return buf, view


@functools.lru_cache(maxsize=None)
def _batch():
    """-> (names, ns, tokens [B, LD], seq_len, row_start, step_tok [B, N_TOK], max_len): the rows of the one launch."""
    S = _slice()
    max_len = START + 2 * S + 40                                                     # three slices: (max_len + N_TOK) / S = 2.03
    assert (max_len + N_TOK + S - 1) // S == 3
    rng = np.random.default_rng(7)
    rows = []                                                                        # (name, n, prompt slots (START), generated, seq_len, row_start, proposals)

    def add(name, n, real, gen, proposals=None, seq_len=None, row_start=None):
        slots = [0] * (START - len(real)) + list(real)
        rows.append((name, n, slots, list(gen), START + len(gen) if seq_len is None else seq_len,
                     START - len(real) if row_start is None else row_start,
                     rng.choice(SYMBOLS[:3], size=N_TOK).tolist() if proposals is None else proposals))

    for n in (1, 2, 3, 8):
        lengths = sorted({max(0, n - 2), n - 1, n, n + 1, 0} |
                         {c + d for c in (256, S, 2 * S) for d in (-1, 0, 1, n - 2, n - 1, n)})
        for k, length in enumerate(lengths):
            syms = SYMBOLS[:3 + k % 2]
            if n == 8:                                                               # a block of 9 ids, tiled, one id in 50 redrawn:
                block = rng.choice(syms, size=9)                                     # 8-grams repeat, which random ids would not
                H = np.resize(block, length)
                redraw = rng.random(length) < 0.02
                redraw[max(0, length - 16):] = False                                 # (not at the end, where the suffix is taken)
                H[redraw] = rng.choice(syms, size=int(redraw.sum()))
                proposals = [int(block[(length + k) % 9]) for k in range(N_TOK)]     # the proposals go on with the block: matches
            else:                                                                    # across the seam
                H, proposals = rng.choice(syms, size=length), None
            n_real = min(length, int(rng.integers(0, START + 1)))                    # the history begins in the prompt slots
            add(f"n{n}-len{length}", n, H[:n_real].tolist(), H[n_real:].tolist(), proposals)
    add("prompt", 2, [5, 6, 5], [], proposals=[60, 61, 62, 63])
    add("padding", 2, [7, 0], [], proposals=[60, 61, 62, 63])
    add("generated", 2, [], [5, 6, 5], proposals=[60, 61, 62, 63])
    add("proposals", 2, [], [], proposals=[5, 6, 5, 9])
    add("seams", 3, [5], [6, 8, 5], proposals=[6, 60, 61, 62])
    add("one symbol", 3, [], [4] * 10, proposals=[60, 61, 62, 63])
    add("odd ids", 2, [], [-1, V, -1, 3, -1], proposals=[60, 61, 62, 63])
    # the per-row mix: rows that are off, and damaged device data
    mixed = rng.choice(SYMBOLS[:3], size=40).tolist()
    add("off", 0, mixed[:4], mixed[4:])
    add("n = 9", 9, mixed[:4], mixed[4:])
    add("n = -1", -1, mixed[:4], mixed[4:])
    add("seq_len below start", 2, [3, 17, 3], mixed, seq_len=-5)                     # H = the prompt alone: 17
    add("seq_len above max_len", 1, [], [3] * 10, seq_len=2 ** 31 - 1)               # H runs to max_len: the 0s behind the row's end, too
    add("row_start negative", 2, [17, 0], [], row_start=-3)                          # the eight slots count: 0 0 0 0 0 0 17 0 -> 0, 17
    add("row_start above start", 2, [42, 17, 3], [42, 3, 42], row_start=START + 5)   # H = 42 3 42 -> 3 (with the prompt: 17 as well)
    ld = max_len + 3
    tokens = np.zeros((len(rows), ld), dtype=np.int32)
    for b, (_, _, slots, gen, _, _, _) in enumerate(rows):
        tokens[b, :START] = slots
        tokens[b, START:START + len(gen)] = gen
    return ([r[0] for r in rows], [r[1] for r in rows], tokens, [r[4] for r in rows], [r[5] for r in rows],
            np.array([r[6] for r in rows], dtype=np.int32), max_len)


@functools.lru_cache(maxsize=None)
def _mask(K1, n_prev, with_tok, shared_n=None, no_row_start=False, every=1):
    """The reference's ban mask [B, K1, V] (bool) of the launch, computed once."""
    _, ns, tokens, seq_len, row_start, step, max_len = _batch()
    pick = slice(None, None, every)
    x = torch.zeros((len(ns[pick]), K1, V))
    ref_no_repeat_ngram(x, ns[pick] if shared_n is None else shared_n, tokens[pick], seq_len[pick],
                        None if no_row_start else row_start[pick], START, max_len, step[pick] if with_tok else None, n_prev)
    return torch.isneginf(x)


def _launch(K_, dtype, K1, n_prev, with_tok, seed, shared_n=None, no_row_start=False, every=1, rows_alloc=None):
    """One launch on the arena against the reference's mask, the whole allocation bit for bit -> (before, after) views."""
    _, ns, tokens, seq_len, row_start, step, max_len = _batch()
    pick = slice(None, None, every)
    mask = _mask(K1, n_prev, with_tok, shared_n, no_row_start, every)
    nb = mask.shape[0]
    buf, view = _arena(dtype, nb, K1, V, PAD, seed, rows_alloc)
    view(buf)[:, :, 17] = torch.where(torch.arange(nb)[:, None] % 2 == 0, float("-inf"), 1.0).to(dtype)   # elements that are -inf already
    want = buf.clone()
    view(want)[mask] = float("-inf")
    dev = buf.cuda()
    x = view(dev)
    dv = lambda a: torch.tensor(a, dtype=torch.int32).cuda()                         # noqa: E731
    packed = K_.NoRepeatNgram(None if shared_n is not None else dv(ns[pick]), None if no_row_start else dv(row_start[pick]),
                              0 if shared_n is None else shared_n, START, nb)
    # (step_tok as a [:, :N_TOK] slice of a wider buffer: ld_tok > n_tok)
    tok_dev = torch.from_numpy(np.concatenate([step[pick], np.full((nb, 3), 3, np.int32)], 1)).cuda()[:, :N_TOK] if with_tok else None
    tok_in = torch.from_numpy(tokens[pick].copy()).cuda()
    out = K_.no_repeat_ngram_rows(x, packed, tok_in, dv(seq_len[pick]), max_len, tok_dev, n_prev)
    torch.cuda.synchronize()
    assert out is x
    assert _bits(dev) == _bits(want)
    assert np.array_equal(tok_in.cpu().numpy(), tokens[pick])                        # `tokens` is only read
    return view(buf), view(want)


def _banned(mask, name, j=0):
    return set(mask[_batch()[0].index(name), j].nonzero().flatten().tolist())


def test_the_reference_bans_in_at_least_half_of_the_positions_and_what_the_header_says():
    """On the CPU side of this file: the batch is dense, and the hand-written rows get the bans the module docstring lists."""
    names, ns, tokens, seq_len, row_start, step, max_len = _batch()
    S = _slice()
    assert max_len + N_TOK > 2 * S and len(names) == len(set(names))
    for K1, n_prev, with_tok in CONFIGS:
        m = _mask(K1, n_prev, with_tok)
        assert 2 * int(m.any(-1).sum()) >= m.shape[0] * K1, (K1, n_prev, int(m.any(-1).sum()), m.shape)
        for n in (1, 2, 3, 8):                                                       # ... in the rows behind the last slice boundary too
            assert _banned(m, f"n{n}-len{2 * S + n}"), n
    m = _mask(1, 0, False)
    assert _banned(m, "prompt") == {6} and _banned(m, "padding") == set() and _banned(m, "generated") == {6}
    assert _banned(m, "proposals") == set() and _banned(m, "seams") == set() and _banned(m, "one symbol") == {4}
    assert _banned(m, "odd ids") == {3} and _banned(m, "seq_len below start") == {17} and _banned(m, "seq_len above max_len") == {3, 0}
    assert _banned(m, "row_start negative") == {17, 0} and _banned(m, "row_start above start") == {3}
    assert not (_banned(m, "off") or _banned(m, "n = 9") or _banned(m, "n = -1"))
    assert _banned(m, "n1-len0") == set() and _banned(m, "n2-len1") == set() and _banned(m, "n8-len7") == set()
    m = _mask(5, 0, True)
    assert [_banned(m, "proposals", j) for j in range(5)] == [set(), set(), set(), {6}, set()]    # - | 5 | 5 6 | 5 6 5 -> 6 | 5 6 5 9
    assert [_banned(m, "seams", j) for j in range(5)] == [set(), {8}, set(), set(), set()]
    assert _banned(m, "one symbol", 0) == {4} and _banned(m, "one symbol", 1) == set()            # 4 .. 4 | 4 .. 4 60
    m = _mask(1, 3, True)
    assert _banned(m, "proposals") == {6} and _banned(m, "prompt") == set()                       # H = 5 6 5 60 61 62


@pytest.mark.parametrize("K1,n_prev,with_tok", CONFIGS)
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_kernel_matches_the_reference_bit_for_bit(K_, dtype, K1, n_prev, with_tok):
    before, after = _launch(K_, dtype, K1, n_prev, with_tok, seed=K1 * 100 + n_prev)
    off = _batch()[0].index("off")
    assert _bits(after[off]) == _bits(before[off]) and torch.isneginf(after[::2, :, 17]).all()


@pytest.mark.parametrize("n", [1, 2, 3, 8])
def test_one_n_for_every_row_and_no_row_start(K_, n):
    """ngram_n == NULL with n_shared = n, on every fourth row of the batch; then row_start == NULL as well: the prompt slots are no
    history.  And the [:, :4] slice of a [B, 5, V] tensor."""
    _launch(K_, torch.bfloat16, 5, 0, True, seed=n, shared_n=n, every=4)
    _launch(K_, torch.float32, 1, 3, True, seed=n + 10, shared_n=n, no_row_start=True, every=4)
    before, _ = _launch(K_, torch.float16, 4, 0, True, seed=n + 20, shared_n=n, every=4, rows_alloc=5)
    assert before.stride(0) == 5 * (V + PAD) and before.shape[1] == 4


def test_full_vocabulary(K_):
    Vf, nb, K1 = 152064, 2, 9
    S = _slice()
    max_len = S + 120
    rng = np.random.default_rng(3)
    syms = np.array([0, Vf - 1, 131072, 65536])
    tokens = np.zeros((nb, max_len), dtype=np.int32)
    seq_len = [300, S + 100]
    for b in range(nb):
        tokens[b, :seq_len[b]] = rng.choice(syms, size=seq_len[b])
    step = rng.choice(syms, size=(nb, 8)).astype(np.int32)
    ns, row_start = [3, 2], [2, 0]
    buf, view = _arena(torch.bfloat16, nb, K1, Vf, 3, 9)
    want = buf.clone()
    ref_no_repeat_ngram(view(want), ns, tokens, seq_len, row_start, 4, max_len, step, 0)
    assert torch.isneginf(view(want)).any(-1).all()
    dev = buf.cuda()
    packed = K_.pack_no_repeat_ngram(ns, [2, 4], 4, "cuda")
    assert packed.ngram_n.tolist() == ns and packed.row_start.tolist() == row_start and packed.P == 4
    K_.no_repeat_ngram_rows(view(dev), packed, torch.from_numpy(tokens).cuda(), torch.tensor(seq_len, dtype=torch.int32).cuda(),
                            max_len, torch.from_numpy(step).cuda(), 0)
    torch.cuda.synchronize()
    assert _bits(dev) == _bits(want)


def test_the_packed_form_on_the_device(K_):
    p = K_.pack_no_repeat_ngram([2, 0, 3], [3, 1, 5], 5, "cuda")
    assert p.ngram_n.tolist() == [2, 0, 3] and p.row_start.tolist() == [2, 4, 0] and (p.n_shared, p.P, p.B) == (0, 5, 3)
    p = K_.pack_no_repeat_ngram([3, 3, 3], [0, 0, 0], 5, "cuda")                   # one n, no prompt id: no table at all
    assert p.ngram_n is None and p.row_start is None and (p.n_shared, p.P, p.B) == (3, 5, 3)


def test_argument_errors_return_their_codes(K_):
    from asd_amd import _binding
    lib = _binding.load_library()
    INVALID, UNSUPPORTED, ALIGNMENT = -1, -2, -5
    B, v = 3, 64
    x = torch.randn((B, 2, v), device="cuda")
    keep = x.clone()
    ns = torch.tensor([2, 0, 0], dtype=torch.int32, device="cuda")
    first = torch.tensor([4, 4, 4], dtype=torch.int32, device="cuda")
    tokens = torch.ones((B, 8), dtype=torch.int32, device="cuda")
    seq = torch.full((B,), 6, dtype=torch.int32, device="cuda")
    tok = torch.full((B, 4), 7, dtype=torch.int32, device="cuda")
    good = dict(logits=x.data_ptr(), dtype=0, ld_seq=2 * v, ld_row=v, B=B, K1=2, V=v, ngram_n=ns.data_ptr(), n_shared=0,
                row_start=first.data_ptr(), tokens=tokens.data_ptr(), ld_tokens=8, seq_len=seq.data_ptr(), start=4, max_len=8,
                tok=tok.data_ptr(), ld_tok=4, n_tok=4, n_prev=3, stream=None)

    def call(**kw):
        return lib.asd_no_repeat_ngram_rows(*{**good, **kw}.values())
    for kw in (dict(B=-1), dict(K1=-1), dict(V=-1), dict(n_shared=-1), dict(n_tok=-1), dict(n_prev=-1), dict(start=-1), dict(max_len=-1),
               dict(B=0, n_prev=-1)):                                             # ... before the empty batch
        assert call(**kw) == INVALID, kw
    # nothing to do: ASD_OK before the pointers and the dtype are looked at
    assert call(B=0) == 0 and call(K1=0) == 0 and call(V=0) == 0 and call(ngram_n=None, n_shared=0) == 0
    assert lib.asd_no_repeat_ngram_rows(None, 99, 0, 0, 0, 1, v, None, 2, None, None, 0, None, 0, 0, None, 0, 0, 0, None) == 0
    assert lib.asd_no_repeat_ngram_rows(None, 99, 0, 0, B, 1, v, None, 0, None, None, 0, None, 0, 0, None, 0, 0, 0, None) == 0
    assert call(dtype=7) == UNSUPPORTED and call(dtype=-1) == UNSUPPORTED
    assert call(ngram_n=None, n_shared=9) == UNSUPPORTED and call(n_shared=9, ld_row=v - 1) == INVALID   # only a shared n is bounded here
    assert call(n_tok=65, ld_tok=65) == UNSUPPORTED
    assert call(max_len=2 ** 31 - 200, ld_tokens=2 ** 31) == UNSUPPORTED                      # the scan counts in int32
    assert call(dtype=7, logits=None) == UNSUPPORTED                             # unsupported comes before the NULL checks
    for kw in (dict(logits=None), dict(tokens=None), dict(seq_len=None), dict(ld_row=v - 1), dict(ld_seq=2 * v - 1), dict(ld_tokens=7),
               dict(start=9), dict(tok=None), dict(n_prev=4), dict(n_tok=3, ld_tok=3), dict(ld_tok=3)):
        assert call(**kw) == INVALID, kw          # (tok NULL with n_prev 3; position 1 would see 5 of 4, or 4 of 3; ld_tok < n_tok)
    assert call(logits=good["logits"] + 2, ld_row=v - 1) == INVALID               # invalid comes before alignment
    for name in ("logits", "ngram_n", "row_start", "tokens", "seq_len", "tok"):
        assert call(**{name: good[name] + 2}) == ALIGNMENT, name
    torch.cuda.synchronize()
    assert torch.equal(x, keep)                                                   # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    # row 0 alone is on: H = 1 1 | 7 7 7 (position 0) bans 7 (7 -> 7), position 1 likewise; 1 -> 1 is no match for the suffix 7
    assert torch.isneginf(x[0, :, 7]).all() and torch.equal(x[1:], keep[1:])
    others = [t for t in range(v) if t != 7]
    assert torch.equal(x[0][:, others], keep[0][:, others])
    x.copy_(keep)
    assert call(ngram_n=None, n_shared=2, row_start=None, tok=None, n_prev=0) == 0            # every row: H = 1 1 bans 1
    torch.cuda.synchronize()
    assert torch.isneginf(x[:, :, 1]).all()
    others = [t for t in range(v) if t != 1]
    assert torch.equal(x[:, :, others], keep[:, :, others])

    # the wrappers' own checks
    packed = K_.pack_no_repeat_ngram([2, 0, 0], [0, 0, 0], 4, "cuda")
    with pytest.raises(ValueError):
        K_.no_repeat_ngram_rows(x.cpu(), packed, tokens, seq, 8)
    with pytest.raises(ValueError):
        K_.no_repeat_ngram_rows(x[:2], packed, tokens[:2], seq[:2], 8)           # packed for 3 rows
    with pytest.raises(ValueError):
        K_.no_repeat_ngram_rows(x, packed, tokens, seq, 9)                        # max_len beyond the token rows
    with pytest.raises(ValueError):
        K_.no_repeat_ngram_rows(x, K_.pack_no_repeat_ngram([2, 0, 0], [0, 0, 0], 9, "cuda"), tokens, seq, 8)   # start beyond max_len
    with pytest.raises(ValueError):
        K_.no_repeat_ngram_rows(x, packed, tokens, seq, 8, None, 1)               # n_prev without step_tok
    with pytest.raises(ValueError):
        K_.no_repeat_ngram_rows(x, packed, tokens, seq, 8, tok, 4)                # position 1 would see 5 proposals of 4
    with pytest.raises(ValueError):
        K_.no_repeat_ngram_rows(x, packed, tokens, seq, 8, tok.to(torch.int64), 0)
    for bad in (([9], [0], 4), ([2], [5], 4), ([2, 2], [0], 4)):
        with pytest.raises(ValueError):
            K_.pack_no_repeat_ngram(*bad, "cuda")
