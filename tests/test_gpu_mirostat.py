"""asd_mirostat_rows / asd_mirostat_commit on the GPU against tests/mirostat_ref.py (numpy f64) on the stored values.  The WHOLE
allocation is compared, guard bands and row padding included: a cut element is -inf, everything else keeps its bits.  The kept
set is exact outside the window w around mu_{b,j} and mu_path lies within dmu of the reference (mirostat_ref.bounds, DESIGN
section 5); every case asserts ON THE REFERENCE ALONE that no token lies inside a window (inputs on a grid of 2^-6; seeds
checked on the CPU).  V = 3 (under one vector), 64, 4099 (past the workgroup's first 1024 f32 vectors), 32781 (past a lane's
first unrolled trip); K1 = 1 and 9; three dtypes; contiguous and strided at an odd element offset; B = 3, sequence 1 off."""
import numpy as np
import pytest
import torch

from tests.mirostat_ref import U, bounds, ref_commit, ref_mirostat

pytestmark = pytest.mark.gpu

GUARD = 257                                      # odd: the strided view starts at an odd element offset
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
INV_T = float(np.float32(1.0 / 0.7))
TABLE = [(INV_T, 5.0, 0.1), (INV_T, 0.0, 0.0), (float(np.float32(1.0 / 1.3)), 3.0, 0.5)]       # sequence 1 is off


@pytest.fixture(scope="module")
def K_():
    from asd_amd import kernels
    return kernels


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16).numpy()


def _arena(dtype, nb, k1, v, strided, seed):
    """-> (buf, view): a flat buffer with guard bands and the [nb, k1, v] view into it; N(0, 3^2) on a grid of 2^-6."""
    g = torch.Generator().manual_seed(seed)
    ld_row, pad_seq = (v + 5, 3) if strided else (v, 0)
    ld_seq = k1 * ld_row + pad_seq
    buf = (torch.round(torch.randn(nb * ld_seq + 2 * GUARD, generator=g) * 3.0 * 64.0) / 64.0).to(dtype)
    return buf, (lambda b: b[GUARD:GUARD + nb * ld_seq].view(nb, ld_seq)[:, :k1 * ld_row].view(nb, k1, ld_row)[:, :, :v])


def _run(K_, buf, view, table, tok, mu0=None):
    """The kernel on a device copy of the arena -> (the arena afterwards, mu_path), on the CPU."""
    dev = buf.cuda()
    x = view(dev)
    miro = K_.pack_mirostat([t for t, _, _ in table], [a for _, a, _ in table], [e for _, _, e in table], "cuda")
    if mu0 is not None:
        miro.mu.copy_(torch.tensor(mu0, dtype=torch.float32))
    mu_in = miro.mu.clone()
    k1 = x.shape[1]
    path = K_.mirostat_rows(x[:, 0] if k1 == 1 else x, miro, None if k1 == 1 else torch.from_numpy(tok).cuda())
    torch.cuda.synchronize()
    assert torch.equal(miro.mu, mu_in)                                       # mu moves in the commit only
    return dev.cpu(), path.cpu().numpy()


def _check(buf, view, table, tok, mu0, after, path, what):
    """The reference's own condition first (no token inside a window), then the arena and mu_path against it."""
    x0 = view(buf).double().numpy()
    cut, want, gap, kk = ref_mirostat(x0, table, mu0, tok)
    per_vec = 4 if buf.dtype == torch.float32 else 8
    finite = np.where(np.isfinite(x0), np.abs(x0), 0.0)
    for b, (inv_t, tau, eta) in enumerate(table):
        if not tau > 0:
            continue
        w, dmu = bounds(x0.shape[2], per_vec, finite[b].max() * inv_t / np.log(2.0), want[b], kk[b], eta)
        assert (gap[b] > w).all(), (what, b, "a token inside the window: pick another seed", gap[b], w)
        assert (np.abs(path[b] - want[b]) <= dmu + U * np.abs(want[b])).all(), (what, b, path[b], want[b], dmu)
    expect = buf.clone()
    view(expect)[torch.from_numpy(cut)] = float("-inf")
    assert np.array_equal(_bits(expect), _bits(after)), (what, "the allocation differs from the reference's")
    return cut, want


@pytest.mark.parametrize("strided", [False, True], ids=["contiguous", "strided"])
@pytest.mark.parametrize("dtype", list(DTYPES), ids=list(DTYPES))
@pytest.mark.parametrize("K1", [1, 9])
@pytest.mark.parametrize("V", [3, 64, 4099, 32781])
def test_random_rows(K_, V, K1, dtype, strided):
    buf, view = _arena(DTYPES[dtype], len(TABLE), K1, V, strided, 7000 + V + K1)
    x = view(buf).float()
    g = torch.Generator().manual_seed(V)
    rank = torch.randint(0, min(3, V), (len(TABLE), max(K1 - 1, 1)), generator=g)        # a proposal among the row's three best
    tok = x[:, :max(K1 - 1, 1)].argsort(-1, descending=True).gather(-1, rank[:, :, None])[:, :, 0].to(torch.int32).numpy()
    mu0 = [2.0 * a for _, a, _ in TABLE]
    after, path = _run(K_, buf, view, TABLE, tok)
    cut, want = _check(buf, view, TABLE, tok, mu0, after, path, (V, K1, dtype, strided))
    if V >= 64:
        assert cut[0].any() and cut[2].any() and not cut[1].any()            # the cut is live; the off sequence is untouched
    if K1 > 1 and V >= 64:
        assert len(set(want[0].tolist())) == K1                              # ... and so is the chain (V = 3: a proposal is cut)
    again, path2 = _run(K_, buf, view, TABLE, tok)                           # the same call on a fresh copy: equal bytes
    assert np.array_equal(_bits(again), _bits(after)) and path2[[0, 2]].tobytes() == path[[0, 2]].tobytes()


def test_designed_rows(K_):
    """One call, f32, V = 4099 (every wave holds a vector), K1 = 9, one design per sequence."""
    V, K1, nb = 4099, 9, 7
    buf, view = _arena(torch.float32, nb, K1, V, True, 99)
    x = view(buf)
    x.clamp_(max=8.0)
    ties = [5, 70, 2000, 4098]                                               # the scalar head, two waves, the tail
    x[0][:, ties] = 9.0                                                      # 0: mu below the arg-max's surprise: only the ties survive
    x[4, 2, 17] = float("nan")                                               # 4: a NaN row and an all -inf row in mid-chain
    x[4, 4] = float("-inf")
    x[5] = float("-inf")                                                     # 5: one finite value per row
    x[5][:, 1234] = 1.5
    x[6, 3, 11] = float("inf")                                               # 6: a +inf row
    tok = view(buf).float().argmax(-1)[:, :K1 - 1].to(torch.int32).numpy()   # the arg-max: always kept ...
    tok[2, 2] = int(x[2, 2].argmin())                                        # 2: ... but a proposal that is cut at row 2
    x[3, 1, tok[3, 1]] = float("-inf")                                       # 3: a proposal that is -inf on entry at row 1
    tok[5] = 1234
    table = [(INV_T, 5.0, 0.1)] * nb
    mu0 = [0.01, 1.0e4, 10.0, 10.0, 10.0, 10.0, 10.0]                        # 1: mu so large that nothing is written
    after, path = _run(K_, buf, view, table, tok, mu0)
    cut, want = _check(buf, view, table, tok, mu0, after, path, "designed")
    keep0 = ~cut[0] & np.isfinite(x[0].numpy())
    assert (keep0.sum(-1) == len(ties)).all() and keep0[:, ties].all()
    assert not cut[1].any() and not cut[5].any()
    assert cut[2, :3].any() and not cut[2, 3:].any() and (path[2, 3:] == path[2, 2]).all()
    assert cut[3, :2].any() and not cut[3, 2:].any() and (path[3, 2:] == path[3, 1]).all()
    assert not cut[4, 2].any() and path[4, 3] == path[4, 2] and path[4, 5] == path[4, 4] and cut[4, 5].any()
    assert np.allclose(np.diff(path[5]), 0.1 * 5.0, rtol=1e-6)                # surprise 0 under a one-token row: mu rises by eta tau
    assert not cut[6, 3].any() and path[6, 4] == path[6, 3] and cut[6, 4].any()


@pytest.mark.parametrize("n_acc,n_commit", [(0, 1), (3, 4), (8, 9), (5, 0), (5, 2)], ids=["none", "mid", "all", "finished", "ended"])
def test_commit(K_, n_acc, n_commit):
    nb, K1, cap = 3, 9, 40
    rng = np.random.default_rng(n_acc)
    path = rng.uniform(1.0, 12.0, (nb, K1)).astype(np.float32)
    lp = np.array([-0.5, -2.0, -7.25], np.float32)
    seq_len = np.array([20, 31, 40], np.int32)
    acc, com = np.full(nb, n_acc, np.int32), np.full(nb, n_commit, np.int32)
    miro = K_.pack_mirostat([t for t, _, _ in TABLE], [a for _, a, _ in TABLE], [e for _, _, e in TABLE], "cuda")
    mu, out = miro.mu.cpu().numpy().copy(), np.full((nb, cap), np.nan, np.float32)
    ref_commit(path, acc, lp, seq_len, com, TABLE, mu, out)
    got = torch.full((nb, cap), float("nan"), device="cuda")
    K_.mirostat_commit(miro, *(torch.from_numpy(a).cuda() for a in (path, acc, lp, seq_len, com)), got)
    assert got.cpu().numpy().tobytes() == out.tobytes()
    assert (np.abs(miro.mu.cpu().numpy() - mu) <= 2 * U * np.abs(mu)).all()
    assert (miro.mu.cpu().numpy() != 2.0 * np.array([5.0, 0.0, 3.0], np.float32))[[0, 2]].all() == (n_commit == n_acc + 1)
