"""asd_lookup_propose on the GPU against tests/lookup_ref.py: `tok` and `matched` as integers, the one-hot draft rows bit for bit
over the WHOLE allocation (guard bands and row padding included), over two successive calls on changed histories so that the
second one unsets the first one's proposals; and the residual draw on such rows against the f64 inverse CDF.

The rows of one launch: histories of 1, 2, N, N + 1, tile - 1, tile, tile + 1 and 2 tile + 3 tokens over two symbols (matches
of every length up to N occur, and ties go to the most recent), an all-equal one, one whose only match ends at len - 1 (a
period-1 copy), an empty one, and the halo trap: H = [0, 1, 0] behind a padding that ends in [0, 1] -- read past row_start, its
match would be 3 tokens long, not 1.  Every row has its own row_start; the padding in front and the slots behind seq_len hold
symbols of the same alphabet.  The second call moves every seq_len up by 3; one row's then lies beyond max_len and is clamped."""
import functools

import numpy as np
import pytest
import torch

from tests.lookup_ref import onehot_image, propose_rows

pytestmark = pytest.mark.gpu

START, V, GUARD, PAD = 8, 64, 96, 5
TILE = 4096                                              # ASD_LOOKUP_TILE (asserted below)
PARAMS = [(1, 1), (3, 1), (3, 3), (8, 2)]


@functools.lru_cache(maxsize=None)
def _scenario(N, n0, K):
    """-> (tokens [B, cap], row_start [B], max_len, [(seq_len, tok, matched) of call 0 and of call 1])."""
    rng = np.random.default_rng(N * 100 + n0)
    lens = [1, 2, N, N + 1, TILE - 1, TILE, TILE + 1, 2 * TILE + 3, 40, 6, 0, 3]
    Bn = len(lens)
    cap = START + max(lens) + 8
    max_len = cap - 2
    tokens = rng.integers(0, 2, size=(Bn, cap)).astype(np.int32)
    row_start = np.array([max(START - n, 0) if n < START else b % 6 for b, n in enumerate(lens)], dtype=np.int32)
    tokens[8, :] = 1                                     # the all-equal row
    tokens[9, row_start[9]:row_start[9] + 6] = [10, 11, 12, 13, 14, 14]         # the only match ends at len - 1
    tokens[11, row_start[11] - 2:row_start[11] + 3] = [0, 1, 0, 1, 0]           # the halo trap
    calls = []
    for extra in (0, 3):
        seq_len = np.array([s + n + extra for s, n in zip(row_start, lens)], dtype=np.int32)
        if extra:
            seq_len[7] = max_len + 100                   # damaged: clamped to max_len
        assert (seq_len >= START).all()
        tok, matched = propose_rows(tokens, row_start, np.minimum(seq_len, max_len), K, N, n0)
        calls.append((seq_len, tok, matched))
    return tokens, row_start, max_len, calls


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("K", [1, 4, 16])
@pytest.mark.parametrize("N,n0", PARAMS)
def test_proposals_and_onehot_rows_equal_the_reference(N, n0, K, dtype):
    from asd_amd import _binding, kernels as K_
    assert _binding.LOOKUP_TILE == TILE
    tokens, row_start, max_len, calls = _scenario(N, n0, K)
    Bn = len(tokens)
    ld_row = V + PAD
    buf = torch.full((2 * GUARD + Bn * K * ld_row,), 1.0, dtype=dtype).cuda()
    onehot = buf[GUARD:GUARD + Bn * K * ld_row].view(Bn, K, ld_row)[:, :, :V]
    onehot.fill_(float("-inf"))                          # (the view writes through) once per call, as the loop does
    tok = torch.full((Bn, K), -1, dtype=torch.int32).cuda()
    matched = torch.full((Bn,), -7, dtype=torch.int32).cuda()
    counter = torch.zeros((Bn,), dtype=torch.int32).cuda()
    want_count = np.zeros(Bn, dtype=np.int32)
    for seq_len, want_tok, want_matched in calls:
        out = K_.lookup_propose(torch.from_numpy(tokens).cuda(), torch.from_numpy(seq_len).cuda(), START, max_len, tok, matched, N, n0,
                                torch.from_numpy(row_start).cuda(), counter, onehot)
        assert out is tok
        assert np.array_equal(tok.cpu().numpy(), want_tok)
        assert np.array_equal(matched.cpu().numpy(), want_matched)
        want_count += want_matched > 0
        assert np.array_equal(counter.cpu().numpy(), want_count)
        image = np.ones(buf.numel(), dtype=np.float32)
        image[GUARD:GUARD + Bn * K * ld_row].reshape(Bn, K, ld_row)[:, :, :V] = onehot_image(want_tok, V)
        assert buf.float().cpu().numpy().tobytes() == image.tobytes()
    assert calls[0][2][11] == (n0 == 1) and calls[0][2][8] == N and (calls[0][1][9] == 14).all() and (calls[0][1][10] == 0).all()
    # greedy: no one-hot rows, the same proposals; no row_start: the history begins at `start`
    seq_len = calls[0][0]
    tok2 = torch.full((Bn, K), -1, dtype=torch.int32).cuda()
    K_.lookup_propose(torch.from_numpy(tokens).cuda(), torch.from_numpy(seq_len).cuda(), START, max_len, tok2, matched, N, n0)
    want = propose_rows(tokens, np.full(Bn, START), seq_len, K, N, n0)
    assert np.array_equal(tok2.cpu().numpy(), want[0]) and np.array_equal(matched.cpu().numpy(), want[1])


def test_the_residual_draw_on_onehot_rows_is_the_target_without_the_proposal():
    """256 rows share one f32 logits row and one proposal, lp_d = 0.  verify_accept accepts exactly where u < p_t(tok) (f64; the
    uniforms lie at least 1e-4 from that edge); on the rejected rows residual_sample_lp with the kernel's one-hot rows never
    returns the proposal and returns the f64 inverse CDF of p_t without it at r_i = (i + 0.5) / 256 (a neighbour only where r_i
    lies within 1e-5 of an edge of that CDF)."""
    from asd_amd import kernels as K_
    from asd_amd.distributed import HipOps
    ops, Bn = HipOps(), 256
    x = torch.randn(V, generator=torch.Generator().manual_seed(5)) * 2.0
    x[9] = x.max()                                       # a proposal likely enough that rows are accepted and rows are rejected
    hist = torch.tensor([[3, 9, 3]], dtype=torch.int32).repeat(Bn, 1).cuda()    # "3" was followed by 9: the proposal
    tok = torch.full((Bn, 1), -1, dtype=torch.int32).cuda()
    onehot = torch.full((Bn, 1, V), float("-inf")).cuda()
    K_.lookup_propose(hist, torch.full((Bn,), 3, dtype=torch.int32).cuda(), 0, 3, tok, torch.zeros(Bn, dtype=torch.int32).cuda(),
                      3, 1, torch.zeros(Bn, dtype=torch.int32).cuda(), None, onehot)
    assert (tok.cpu().numpy() == 9).all()
    p = np.exp(x.double().numpy() - x.double().numpy().max())
    p /= p.sum()
    r = (np.arange(Bn) + 0.5) / Bn
    u = np.where(np.abs(r - p[9]) < 1e-4, r + 2e-4, r)
    score = x.repeat(Bn, 1, 1).cuda()
    dev = lambda a: torch.from_numpy(a.astype(np.float32)).cuda()               # noqa: E731
    _, _, n_acc, _ = ops.verify_accept(score, tok, torch.zeros((Bn, 1)).cuda(), dev(u[:, None]))
    assert np.array_equal(n_acc.cpu().numpy() == 1, u.astype(np.float32) < p[9]) and 0 < int(n_acc.sum()) < Bn
    drawn, _ = ops.residual_sample_lp(score, onehot, n_acc, dev(r), x.repeat(Bn, 1).cuda(), 1.0,
                                      d_threshold=torch.full((Bn, 1), float("-inf")).cuda())
    q = p.copy()
    q[9] = 0.0
    edges = np.cumsum(q / q.sum())
    drawn = drawn.cpu().numpy()
    for i in np.flatnonzero(n_acc.cpu().numpy() == 0):
        t, want = int(drawn[i]), int(np.searchsorted(edges, np.float32(r[i]), side="right"))
        assert t != 9
        near = np.abs(edges - np.float32(r[i])).min() < 1e-5
        assert t == want or (near and abs(t - want) <= 2 and t != 9), (i, t, want)
