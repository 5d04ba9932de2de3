"""asd_typical_accept on the GPU (csrc/typical_accept.hip) against the numpy f64 reference on the stored logits
(tests/typical_accept_ref.py): lp_t within DESIGN 2's 2e-5, the entropy within the token statistics' bar, and -- every row of
the reference being at least 1e-3 nats from its threshold, asserted first -- accept_bits and n_acc exactly, on every row."""
from functools import lru_cache

import numpy as np
import pytest
import torch

from tests.token_stats_ref import H_ATOL, H_RTOL
from tests.typical_accept_ref import ref_typical_accept

pytestmark = pytest.mark.gpu

LP_ATOL, MARGIN = 2e-5, 1e-3
EPS, ALPHA = 0.09, 0.3
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
INF = float("inf")


def _table(inv_t, eps=EPS, alpha=ALPHA):
    return [(float(np.float32(t)), float(np.float32(np.log(eps))), float(np.float32(np.log(alpha)))) for t in inv_t]


def _packed(table, device="cuda"):
    from asd_amd import kernels as K
    rec = np.array([(*r, 0.0) for r in table], dtype=np.float32)
    return K.TypicalAccept(torch.from_numpy(rec.view(np.uint8).reshape(len(table), 16).copy()).to(device), len(table))


@lru_cache(maxsize=None)
def _case(V, dtype, B, K):
    """Logits 3 N(0, 1) rounded to the dtype; two tokens of three from the row's own softmax, the rest uniform; T in {0.7, 1};
    the reference, computed once for both values of `splits`."""
    g = torch.Generator().manual_seed(V + 31 * B + K)
    x = (3.0 * torch.randn((B, K, V), generator=g)).to(DTYPES[dtype])
    table = _table([1.0 / (0.7, 1.0)[b % 2] for b in range(B)])
    inv_t = torch.tensor([t[0] for t in table])[:, None, None]
    own = torch.multinomial(torch.softmax(x.float() * inv_t, -1).reshape(B * K, V), 1, generator=g).reshape(B, K)
    uni = torch.randint(0, V, (B, K), generator=g)
    tok = torch.where(torch.arange(B * K).reshape(B, K) % 3 < 2, own, uni).to(torch.int32)
    ref = ref_typical_accept(x.float().numpy(), tok.numpy(), table)
    return x, tok, table, ref


def _check(got, ref, what):
    lp, H, thr, acc, bits, n_acc = ref
    fin = np.isfinite(lp)
    assert (np.abs(lp[fin] - thr[fin]) > MARGIN).all(), (what, "the reference's own margin")      # before any kernel output
    g_lp, g_H, g_bits, g_n = (t.cpu().numpy() for t in got)
    assert np.array_equal(np.isnan(g_lp), np.isnan(lp)) and np.array_equal(np.isnan(g_H), np.isnan(H)), what
    assert np.array_equal(np.isneginf(g_lp), np.isneginf(lp)), what
    err_lp = np.abs(g_lp[fin] - lp[fin]).max() if fin.any() else 0.0
    ok = ~np.isnan(H)
    err_H = np.abs(g_H[ok] - H[ok])
    print(what, "lp_t err", float(err_lp), "entropy err", float(err_H.max()) if ok.any() else 0.0)
    assert err_lp <= LP_ATOL, (what, err_lp)
    assert (err_H <= H_ATOL + H_RTOL * np.abs(H[ok])).all(), (what, float(err_H.max()))
    assert np.array_equal(g_bits.view(np.uint64), bits) and np.array_equal(g_n, n_acc), (what, g_bits, bits, g_n, n_acc)


@pytest.mark.parametrize("splits", [1, 3])
@pytest.mark.parametrize("B,K", [(1, 1), (4, 5), (2, 16)])
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("V", [1003, 4099, 152064])
def test_against_the_f64_reference(V, dtype, B, K, splits):
    from asd_amd import kernels as Kn
    x, tok, table, ref = _case(V, dtype, B, K)
    got = Kn.typical_accept(x.cuda(), tok.cuda(), _packed(table), splits=splits)
    _check(got, ref, (V, dtype, B, K, splits))


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_a_view_with_an_odd_element_offset_and_padded_rows(dtype):
    from asd_amd import kernels as Kn
    B, K, V, pad = 3, 5, 4099, 6
    x, tok, table, ref = _case(V, dtype, 4, 5)
    x, tok, table, ref = x[:B], tok[:B], table[:B], tuple(r[:B] for r in ref)
    flat = torch.full((B * K * (V + pad) + 1,), float("nan"), dtype=DTYPES[dtype], device="cuda")     # the gaps: never read
    view = flat[1:].view(B, K, V + pad)[:, :, :V]
    view.copy_(x)
    for splits in (0, 1, 3):
        got = Kn.typical_accept(view, tok.cuda(), _packed(table), splits=splits)
        _check(got, ref, ("view", dtype, splits))
        again = Kn.typical_accept(view, tok.cuda(), _packed(table), splits=splits)   # the same call twice: bit-equal
        assert all(p.cpu().numpy().tobytes() == q.cpu().numpy().tobytes() for p, q in zip(got, again))


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_constructed_rows(dtype):
    from asd_amd import kernels as Kn
    B, K, V = 6, 8, 1003                                                         # odd V: rows start at every 16-byte phase
    g = torch.Generator().manual_seed(7)
    x = (3.0 * torch.randn((B, K, V), generator=g)).to(DTYPES[dtype])
    tok = torch.randint(8, V - 8, (B, K), generator=g).to(torch.int32)
    for b in range(B):
        for k in range(K):
            x[b, k, tok[b, k]] = 24.0                                            # every proposal dominates its row: accepted ...
    # ... but for sequence 0's special rows
    tok[0, 0] = V - 1; x[0, 0, V - 1] = 24.0                                     # the last element (a scalar tail, or the body's end)
    tok[0, 1] = 0; x[0, 1, 0] = 24.0                                             # row 1 starts off a 16-byte boundary: the scalar head
    x[0, 2, tok[0, 2]] = -INF                                                    # the token at -inf
    tok[0, 3] = V                                                                # out of range
    x[0, 4, 500] = float("nan")                                                  # a NaN row: its neighbours stay
    x[0, 5] = -INF; x[0, 5, 17] = 3.0; tok[0, 5] = 17                            # one-hot, the hot token: H = 0, accepted
    x[0, 6] = -INF; x[0, 6, 17] = 3.0; tok[0, 6] = 18                            # one-hot, another token
    x[0, 7, 3] = INF                                                             # a +inf element
    x[1, 0, tok[1, 0]] = -24.0                                                   # sequence 1: a reject at k = 0, then accepts
    tok[2, 2] = -1; x[2, 5] = -INF                                               # sequence 2: below range; no finite element
    table = _table([1.0, 1.0 / 0.7, 1.0, 1.0, 0.0, 1.0])                         # sequence 3: all accepted; 4: inv_t = 0 rejects
    table[5] = (1.0, -INF, table[5][2])                                          # sequence 5: a non-finite ln_eps rejects
    ref = ref_typical_accept(x.float().numpy(), tok.numpy(), table)
    for splits in (1, 3):
        got = Kn.typical_accept(x.cuda(), tok.cuda(), _packed(table), splits=splits)
        _check(got, ref, ("constructed", dtype, splits))
        lp, H, bits, n_acc = (t.cpu().numpy() for t in got)
        assert bits.tolist() == [0b00100011, 0b11111110, 0b11011011, 0b11111111, 0, 0] and n_acc.tolist() == [2, 0, 2, 8, 0, 0]
        assert np.isneginf(lp[0, [2, 3, 6]]).all() and np.isnan(lp[0, [4, 7]]).all() and np.isnan(H[0, [4, 7]]).all()
        assert 0.0 <= H[0, 5] <= H_ATOL and 0.0 <= H[0, 6] <= H_ATOL and np.isnan(lp[2, 5]) and np.isnan(lp[4:]).all()

