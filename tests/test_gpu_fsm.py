"""asd_fsm_mask_rows, asd_fsm_advance and asd_fsm_commit on the GPU against tests/fsm_ref.py (numpy, the header's text), bit for
bit.  The WHOLE allocation -- a guard band in front, the tensor with its row padding, a guard band behind (the arena of
tests/test_gpu_bad_words.py) -- is compared, for the logits and for the state columns alike, so a stray write anywhere fails.
bf16 / f16 / f32; B = 3 with row 1 unguided (-1), K1 in {1, 5}, V in {1000, 1003} (the odd V with padded rows); the [:, :4]
slice of a [3, 5, V] tensor; V = 152064 at B = 2, K1 = 3, one launch per kernel.

Every case stays inside its arrays by contract: states outside [0, S), tokens outside [0, V), n_commit above ld_state and seq_len
outside [1, max_len] are values the kernels clamp or compare, never indices they follow."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests.fsm_ref import ref_delta, ref_fsm_advance, ref_fsm_commit, ref_fsm_mask, ref_state_bits, tables_of
from tests.test_gpu_bad_words import B, DTYPE_IDS, DTYPES, GUARD, _arena, _bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def K_():
    from asd_amd import kernels
    return kernels


def _fsm(first, tok, nxt, other, starts, V):
    i32 = lambda a: np.asarray(a, dtype=np.int32).reshape(-1)                       # noqa: E731
    return SimpleNamespace(state_first=i32(first), edge_tok=i32(tok), edge_next=i32(nxt), state_other=i32(other), starts=list(starts), V=V)


def _state_arena(K_, packed, values):
    """Put the state columns into a guard-banded arena of their own -> (the arena on the device, its view, the host copy)."""
    values = np.asarray(values, dtype=np.int32)
    host = np.full(values.size + 2 * GUARD, -77, dtype=np.int32)
    host[GUARD:GUARD + values.size] = values.reshape(-1)
    dev = torch.from_numpy(host.copy()).cuda()
    packed.pos_state = dev[GUARD:GUARD + values.size].view(values.shape)
    packed.B, packed.ld_state = values.shape
    return dev, host


# ------------------------------------------------------------------------------------------ the mask
def _mask_states(V):
    """State 0 allows one token; 1 all but one; 2 everything; 3 nothing; 4 exactly the first and the last mask word (all-set
    words there, all-clear words between); 5 everything but the first and the last mask word; 6 a scattered set."""
    last = ((V - 1) >> 5) << 5
    ends = list(range(32)) + list(range(last, V))
    scattered = sorted({0, 31, 32, 33, V - 1, V - 2, 500, 511, 512} | set(range(64, 200, 3)))
    states = [([V // 2], [0], -1), ([V - 1], [-1], 1), ([], [], 2), ([], [], -1), (ends, [4] * len(ends), -1),
              (ends, [-1] * len(ends), 5), (scattered, [6] * len(scattered), -1)]
    first = np.cumsum([0] + [len(s[0]) for s in states])
    return _fsm(first, np.concatenate([np.asarray(s[0], dtype=np.int64) for s in states]),
                np.concatenate([np.asarray(s[1], dtype=np.int64) for s in states]), [s[2] for s in states], [0, -1, 0], V)


def _run_mask(K_, dtype, K1, V, pad, first, seed, rows_alloc=None, nb=B, small=True):
    fsm = _mask_states(V)
    packed = K_.pack_fsm(fsm, first + K1 + 1, "cuda")
    t = tables_of(fsm.state_first, fsm.edge_tok, fsm.edge_next, fsm.state_other, V)
    bits = packed.state_bits.cpu().numpy().view(np.uint32)
    if small:                                                    # the packed bits are the reference's, built from the header's sentence
        assert np.array_equal(bits, ref_state_bits(t))
    S = t.S
    # a distinct state per position; row 1 has no automaton; states outside [0, S) leave their position alone
    pool = [0, 1, 2, 3, 4, 5, 6, S, 1, -2, 4, 2 ** 30, 6, 0, 5, 3, 2]
    pos = np.array([[pool[(3 * b + c) % len(pool)] for c in range(first + K1 + 1)] for b in range(nb)], dtype=np.int32)
    pos[1] = -1
    state_dev, state_host = _state_arena(K_, packed, pos)
    buf, view = _arena(dtype, K1, V, pad, seed, rows_alloc, nb)
    view(buf)[0, :, V // 2] = float("-inf")                      # an element that is -inf already
    want = buf.clone()
    ref_fsm_mask(view(want), bits, pos, first)
    dev = buf.cuda()
    x = view(dev)
    out = K_.fsm_mask_rows(x, packed, first)
    torch.cuda.synchronize()
    assert out is x
    assert _bits(dev) == _bits(want)
    assert np.array_equal(state_dev.cpu().numpy(), state_host)   # the mask kernel writes no state
    return view(buf), view(want), pos


@pytest.mark.parametrize("V,pad", [(1000, 0), (1003, 13)])
@pytest.mark.parametrize("K1,first", [(1, 0), (1, 3), (5, 0), (5, 2)])
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_mask_matches_the_reference_bit_for_bit(K_, dtype, K1, first, V, pad):
    before, after, pos = _run_mask(K_, dtype, K1, V, pad, first, seed=K1 * 10000 + V + first)
    assert _bits(after[1]) == _bits(before[1])                   # the row without an automaton
    last = ((V - 1) >> 5) << 5
    for b in (0, 2):                                             # the reference did what the header says, whatever its code
        for j in range(K1):
            s, neg = int(pos[b, first + j]), torch.isneginf(after[b, j])
            if s == 0:
                assert int((~neg).sum()) == (0 if b == 0 else 1) and (b == 0 or not neg[V // 2])   # (row 0's was -inf already)
            elif s == 1:
                assert neg[V - 1] and int(neg.sum()) == 1 + (b == 0)
            elif s == 3:
                assert neg.all()
            elif s == 4:
                assert not neg[:32].any() and not neg[last:].any() and neg[32:last].all()
            elif s == 5:
                assert neg[:32].all() and neg[last:].all() and int(neg[32:last].sum()) == (b == 0)
            elif s in (2, 7, -2, 2 ** 30):
                assert _bits(after[b, j]) == _bits(before[b, j])


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_mask_on_a_non_contiguous_slice(K_, dtype):
    # the [:, :4] slice of a [3, 5, V] tensor: ld_seq = 5 V, K1 = 4; row 4 of every sequence is not touched
    before, after, _ = _run_mask(K_, dtype, 4, 1000, 0, 1, seed=77, rows_alloc=5)
    assert before.stride(0) == 5 * 1000 and before.shape == (B, 4, 1000)


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_mask_full_vocabulary(K_, dtype):
    _run_mask(K_, dtype, 3, 152064, 3, 1, seed=9, nb=2, small=False)


# ------------------------------------------------------------------------------------------ the transition
def _edge_states(V):
    """Two states (other = -1, other = a state) per edge count: 0, 1, 63, 64, 65, 4096, 4097 (where V has room) and V -- the
    round boundaries of the cooperative search.  Fewer than V edges: the ids 1, 3, 5, ... (0 lies below, the even ids between,
    2 n and up above); V edges: every id.  The middle edge of every state leads to -1."""
    counts = [n for n in (0, 1, 63, 64, 65, 4096, 4097) if 2 * n < V] + [V]
    S = 2 * len(counts)
    states = []
    for n in counts:
        ids = np.arange(V, dtype=np.int64) if n == V else 1 + 2 * np.arange(n, dtype=np.int64)
        for other in (-1, (len(states) + 3) % S):
            nxt = (len(states) + 1 + np.arange(n, dtype=np.int64)) % S
            if n:
                nxt[n // 2] = -1
            states.append((ids, nxt, other))
    first = np.cumsum([0] + [len(s[0]) for s in states])
    fsm = _fsm(first, np.concatenate([s[0] for s in states]), np.concatenate([s[1] for s in states]), [s[2] for s in states], [0], V)
    return fsm, states


def _cases(V, states):
    """(state, token) pairs: hits at the first, the last and the forbidden middle edge, at ids 0 and V - 1; misses below,
    between and above the edges under both kinds of `other`; tokens outside [0, V); states outside [0, S)."""
    S, out = len(states), []
    for s, (ids, _, _) in enumerate(states):
        n = len(ids)
        toks = [0, 2, V - 1, V - 2, -1, V, 2 ** 31 - 1, -2 ** 31]
        if n:
            toks += [int(ids[0]), int(ids[-1]), int(ids[n // 2]), int(ids[-1]) + 1 if int(ids[-1]) + 1 < V else V - 1, int(ids[n // 3])]
        if n > 64:
            toks += [int(ids[63]), int(ids[64]), int(ids[64]) + 1, int(ids[n - 2])]
        out += [(s, t) for t in toks]
    out += [(-1, 5), (S, 5), (2 ** 30, 1), (-2 ** 31, 0)]
    return out


@pytest.fixture(scope="module", params=[1000, 1003, 152064])
def edge_setup(request, K_):
    V = request.param
    fsm, states = _edge_states(V)
    return V, fsm, states, tables_of(fsm.state_first, fsm.edge_tok, fsm.edge_next, fsm.state_other, V), _cases(V, states)


def test_the_reference_transition_is_the_headers(edge_setup):
    V, _, states, t, _ = edge_setup
    S = len(states)
    for s, (ids, nxt, other) in enumerate(states):
        n = len(ids)
        stay_or = lambda to: s if to < 0 else to                                  # noqa: E731
        assert ref_delta(t, s, -1) == s == ref_delta(t, s, V)
        if n == V:
            assert ref_delta(t, s, 0) == stay_or(int(nxt[0])) and ref_delta(t, s, V - 1) == stay_or(int(nxt[-1]))
        else:
            assert ref_delta(t, s, 0) == stay_or(other) == ref_delta(t, s, 2) == ref_delta(t, s, V - 1 if 2 * n < V - 1 else 0)
        if n:
            assert ref_delta(t, s, int(ids[n // 2])) == s and ref_delta(t, s, int(ids[-1])) == stay_or(int(nxt[-1]))
    assert ref_delta(t, S, 5) == S and ref_delta(t, -1, 5) == -1


def test_advance_matches_the_reference(K_, edge_setup):
    V, fsm, states, t, cases = edge_setup
    nb, ld_state, k = len(cases), 4, 1
    packed = K_.pack_fsm(fsm, ld_state, "cuda")
    pos = np.full((nb, ld_state), -5, dtype=np.int32)
    pos[:, k] = [np.int64(s).astype(np.int32) for s, _ in cases]
    tok = np.full((nb, 5), 7, dtype=np.int32)                                    # step_tok as a [:, :3] slice: ld_tok > n_tok
    tok[:, k] = [np.int64(x).astype(np.int32) for _, x in cases]
    state_dev, host = _state_arena(K_, packed, pos)
    want = pos.copy()
    ref_fsm_advance(t, want, k, tok)
    assert len(set(want[:, k + 1].tolist())) > len(states) // 2                   # the cases reach most states
    K_.fsm_advance(packed, torch.from_numpy(tok).cuda()[:, :3], k)
    torch.cuda.synchronize()
    host[GUARD:GUARD + want.size] = want.reshape(-1)
    got = state_dev.cpu().numpy()
    bad = np.nonzero(got != host)[0]
    assert bad.size == 0, [(cases[(i - GUARD) // ld_state], int(got[i]), int(host[i])) for i in bad[:8] if GUARD <= i < GUARD + want.size]


def test_commit_matches_the_reference(K_, edge_setup):
    V, fsm, states, t, cases = edge_setup
    Kd, max_len, ld_tokens = 4, 12, 16
    ld_state = Kd + 1
    # every (state, token) case once, under a rotating n_commit: 1, draft_len + 1, above ld_state (clamped), 2, and 0 (frozen)
    commits = [1, Kd + 1, Kd + 9, 2, 0, 2 ** 31 - 1, -3]
    seqs = [5, max_len, 1, max_len + 7, 0, -5, 2 ** 31 - 1, 3]                   # outside [1, max_len]: clamped
    nb = len(cases)
    n_commit = np.array([commits[b % len(commits)] for b in range(nb)], dtype=np.int32)
    seq_len = np.array([seqs[b % len(seqs)] for b in range(nb)], dtype=np.int32)
    pos = np.full((nb, ld_state), -1, dtype=np.int32)
    tokens = np.full((nb, ld_tokens), 3, dtype=np.int32)
    for b, (s, x) in enumerate(cases):
        c = min(max(int(n_commit[b]), 1), ld_state)
        L = min(max(int(seq_len[b]), 1), max_len)
        pos[b, :] = np.int64(s).astype(np.int32) if b % 2 else -1                 # (odd rows: every column; even rows: the one that is read)
        pos[b, c - 1] = np.int64(s).astype(np.int32)
        tokens[b, L - 1] = np.int64(x).astype(np.int32)
    packed = K_.pack_fsm(fsm, ld_state, "cuda")
    state_dev, host = _state_arena(K_, packed, pos)
    want = pos.copy()
    ref_fsm_commit(t, want, tokens, seq_len, n_commit, max_len)
    frozen = n_commit <= 0
    assert frozen.any() and np.array_equal(want[frozen], pos[frozen]) and (want[~frozen, 0] != pos[~frozen, 0]).any()
    K_.fsm_commit(packed, torch.from_numpy(tokens).cuda(), torch.from_numpy(seq_len).cuda(), torch.from_numpy(n_commit).cuda(), max_len)
    torch.cuda.synchronize()
    host[GUARD:GUARD + want.size] = want.reshape(-1)
    assert np.array_equal(state_dev.cpu().numpy(), host)


def test_a_step_of_advances_then_a_commit(K_):
    """The loop's own sequence on a trie: draft_len advances fill the columns 1 .. draft_len, the commit moves column 0."""
    V, Kd = 1000, 4
    # 0 -5-> 1 -6-> 2 -7-> 3 -8-> 4 -9-> 5; every state also 1 -> 0
    fsm = _fsm([0, 2, 4, 6, 8, 10, 11], [1, 5, 1, 6, 1, 7, 1, 8, 1, 9, 1], [0, 1, 0, 2, 0, 3, 0, 4, 0, 5, 0], [-1] * 6, [0, -1, 1], V)
    t = tables_of(fsm.state_first, fsm.edge_tok, fsm.edge_next, fsm.state_other, V)
    packed = K_.pack_fsm(fsm, Kd + 1, "cuda")
    assert packed.pos_state.tolist() == [[0] * 5, [-1] * 5, [1] * 5]
    tok = np.array([[5, 6, 7, 1], [5, 6, 7, 8], [6, 7, 400, 8]], dtype=np.int32)    # row 2: 400 is forbidden in state 3: it stays
    want = packed.pos_state.cpu().numpy().copy()
    tok_dev = torch.from_numpy(tok).cuda()
    for k in range(Kd):
        K_.fsm_advance(packed, tok_dev, k)
        ref_fsm_advance(t, want, k, tok)
    torch.cuda.synchronize()
    assert packed.pos_state.tolist() == want.tolist() == [[0, 1, 2, 3, 0], [-1] * 5, [1, 2, 3, 3, 4]]
    # row 0 commits 3 tokens (two accepted proposals and the drawn 1), row 1 is unguided, row 2 is finished (n_commit 0)
    tokens = np.zeros((3, 12), dtype=np.int32)
    tokens[0, 2:5] = [5, 6, 1]
    seq_len, n_commit = [5, 5, 4], [3, 3, 0]
    ref_fsm_commit(t, want, tokens, seq_len, n_commit, 12)
    K_.fsm_commit(packed, torch.from_numpy(tokens).cuda(), torch.tensor(seq_len, dtype=torch.int32).cuda(),
                  torch.tensor(n_commit, dtype=torch.int32).cuda(), 12)
    torch.cuda.synchronize()
    assert packed.pos_state.tolist() == want.tolist() == [[0, 1, 2, 3, 0], [-1] * 5, [1, 2, 3, 3, 4]]
    tokens[0, 4] = 7                                              # ... and with the drawn token 7 in place of 1: state 3
    K_.fsm_commit(packed, torch.from_numpy(tokens).cuda(), torch.tensor(seq_len, dtype=torch.int32).cuda(),
                  torch.tensor(n_commit, dtype=torch.int32).cuda(), 12)
    torch.cuda.synchronize()
    assert packed.pos_state[:, 0].tolist() == [3, -1, 1]


def test_argument_errors_return_their_codes(K_):
    from asd_amd import _binding
    lib = _binding.load_library()
    INVALID, UNSUPPORTED, ALIGNMENT = -1, -2, -5
    V, Kd = 64, 4
    fsm = _fsm([0, 1, 2], [3, 4], [1, 0], [-1, -1], [0] * B, V)
    f = K_.pack_fsm(fsm, Kd + 1, "cuda")
    x = torch.randn((B, 2, V), device="cuda")
    keep, keep_state = x.clone(), f.pos_state.clone()
    tok = torch.zeros((B, Kd), dtype=torch.int32, device="cuda")
    tokens = torch.ones((B, 8), dtype=torch.int32, device="cuda")
    seq = torch.full((B,), 5, dtype=torch.int32, device="cuda")
    nc = torch.ones((B,), dtype=torch.int32, device="cuda")
    tabs = dict(first=f.state_first.data_ptr(), tok=f.edge_tok.data_ptr(), nxt=f.edge_next.data_ptr(), other=f.state_other.data_ptr(),
                S=2, E=2, V=V, pos=f.pos_state.data_ptr(), ld_state=Kd + 1, B=B)

    mask = dict(logits=x.data_ptr(), dtype=0, ld_seq=2 * V, ld_row=V, B=B, K1=2, V=V, bits=f.state_bits.data_ptr(), S=2,
                pos=f.pos_state.data_ptr(), ld_state=Kd + 1, first=1, stream=None)
    call = lambda **kw: lib.asd_fsm_mask_rows(*{**mask, **kw}.values())            # noqa: E731
    for kw in (dict(B=-1), dict(K1=-1), dict(V=-1), dict(S=-1), dict(first=-1), dict(ld_state=-1), dict(B=0, first=-1)):
        assert call(**kw) == INVALID, kw
    assert call(B=0) == 0 and call(K1=0) == 0 and call(V=0) == 0 and call(S=0) == 0
    assert call(dtype=7) == UNSUPPORTED and call(dtype=7, logits=None) == UNSUPPORTED
    for kw in (dict(logits=None), dict(bits=None), dict(pos=None), dict(ld_row=V - 1), dict(ld_seq=2 * V - 1), dict(first=4), dict(ld_state=2)):
        assert call(**kw) == INVALID, kw
    assert call(logits=mask["logits"] + 2, ld_row=V - 1) == INVALID
    for name in ("logits", "bits", "pos"):
        assert call(**{name: mask[name] + 2}) == ALIGNMENT, name

    adv = dict(tabs, k=1, step_tok=tok.data_ptr(), ld_tok=Kd, n_tok=Kd, stream=None)
    call = lambda **kw: lib.asd_fsm_advance(*{**adv, **kw}.values())               # noqa: E731
    for kw in (dict(B=-1), dict(S=-1), dict(E=-1), dict(V=-1), dict(k=-1), dict(n_tok=-1), dict(ld_state=-1), dict(B=0, k=-1)):
        assert call(**kw) == INVALID, kw
    assert call(B=0) == 0 and call(B=0, first=None, pos=None, step_tok=None) == 0
    assert call(n_tok=65, ld_tok=65) == UNSUPPORTED
    for kw in (dict(first=None), dict(other=None), dict(tok=None), dict(nxt=None), dict(pos=None), dict(step_tok=None), dict(k=Kd),
               dict(ld_state=2), dict(n_tok=1), dict(ld_tok=Kd - 1)):
        assert call(**kw) == INVALID, kw
    assert call(tok=None, nxt=None, E=0) == 0                                     # no edge: the tables may be NULL
    for name in ("first", "tok", "nxt", "other", "pos", "step_tok"):
        assert call(**{name: adv[name] + 2}) == ALIGNMENT, name

    com = dict(tabs, tokens=tokens.data_ptr(), ld_tokens=8, seq_len=seq.data_ptr(), n_commit=nc.data_ptr(), max_len=8, stream=None)
    call = lambda **kw: lib.asd_fsm_commit(*{**com, **kw}.values())                # noqa: E731
    for kw in (dict(B=-1), dict(S=-1), dict(E=-1), dict(V=-1), dict(max_len=-1), dict(ld_state=-1), dict(B=0, max_len=-1)):
        assert call(**kw) == INVALID, kw
    assert call(B=0) == 0
    for kw in (dict(first=None), dict(other=None), dict(tok=None), dict(pos=None), dict(tokens=None), dict(seq_len=None), dict(n_commit=None),
               dict(ld_state=0), dict(max_len=0), dict(ld_tokens=7)):
        assert call(**kw) == INVALID, kw
    for name in ("first", "tok", "nxt", "other", "pos", "tokens", "seq_len", "n_commit"):
        assert call(**{name: com[name] + 2}) == ALIGNMENT, name
    torch.cuda.synchronize()
    # nothing was launched by a refused call; the accepted E = 0 advance moved nothing either (no edge, other = -1: the state stays)
    assert torch.equal(x, keep) and torch.equal(f.pos_state, keep_state)

    # the wrappers' own checks
    with pytest.raises(ValueError):
        K_.fsm_mask_rows(x.cpu(), f)
    with pytest.raises(ValueError):
        K_.fsm_mask_rows(x[:2], f)                                                # packed for 3 rows
    with pytest.raises(ValueError):
        K_.fsm_mask_rows(x, f, 4)                                                 # positions 4, 5 of 5 columns
    with pytest.raises(ValueError):
        K_.fsm_advance(f, tok, Kd)
    with pytest.raises(ValueError):
        K_.fsm_advance(f, tok.to(torch.int64), 0)
    with pytest.raises(ValueError):
        K_.fsm_commit(f, tokens, seq, nc, 9)                                      # max_len beyond the token rows
    for bad in (dict(state_first=[0, 1, 3]), dict(edge_tok=[3, 64]), dict(edge_next=[2, 0]), dict(state_other=[-2, 0]), dict(starts=[2])):
        with pytest.raises(ValueError):
            K_.pack_fsm(SimpleNamespace(**{**vars(fsm), **bad}), 1, "cuda")
