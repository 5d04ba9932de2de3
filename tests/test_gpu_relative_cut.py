"""asd_relative_cut_rows on the GPU against tests/relative_cut_ref.py (numpy f64, the header's text) over the WHOLE allocation
(a guard band in front and behind, ld_row = V + 13, an odd element offset: the arena of tests/test_gpu_entropy_cut.py), and
asd_step_uniforms_ex against the numpy Philox.  Only the tokens inside the reference's window are excused, and every test
asserts on the reference alone, before it looks at the kernel, that at most 2 % of its rows hold one.

V, after the kernel's geometry (1024 lanes, 16-byte vectors, 19 resident vectors per lane): 3 (under one vector), 64, 4099 (past
a lane's first vector in f32), 8203 (past it in 16 bits), the two sides of the residency bound (77827 | 77828 in f32,
155655 | 155656 in 16 bits: the streaming kernel's rows also pass a lane's first unrolled trip), and one case at 152064."""
import functools

import numpy as np
import pytest
import torch

from tests.philox_ref import philox4x32_10, step_uniforms_ref, to_uniform
from tests.relative_cut_ref import OFF, TOP_A, TOP_N_SIGMA, XTC, assert_cap, check_rel_cut, ref_relative_cut
from tests.test_gpu_entropy_cut import DTYPE_IDS, DTYPES, INV_T, _arena, _bits, _esz, f32

pytestmark = pytest.mark.gpu

MIX = [(TOP_N_SIGMA, 1.0, 0.0), (TOP_N_SIGMA, 2.5, 0.0), (TOP_A, 0.2, 0.0), (TOP_A, 1.0, 0.0), (OFF, 0.0, 0.0),
       (XTC, 0.02, 0.5), (XTC, 0.1, 1.0), (XTC, 0.005, 0.5)]
B, K1 = len(MIX), 3
COINS = np.tile(np.array([0.25, 0.5, 0.75], np.float32), (B, 1))             # under q, equal to q = 0.5 ("no"), above it
BOUND = {4: 77827, 2: 155655}                                                # the last V of the resident kernel, by element size
SEEDS = {(155655, "f16"): 1, (77827, "f32"): 1}                              # (V, dtype id) -> seed, picked on the CPU for the cap; else 0


@pytest.fixture(scope="module")
def K_():
    from asd_amd import kernels
    return kernels


def _table(rows, inv_t=INV_T):
    return [(f32(inv_t), m, f32(a), f32(b)) for m, a, b in rows]


def _raw(K_, table):
    """The device table without the host's checks: a damaged record must reach the kernel."""
    rec = np.array([tuple(r) for r in table], dtype=K_._RELCUT_REC)
    t = torch.from_numpy(rec.view(np.uint8).reshape(len(rec), 16).copy()).cuda()
    return K_.RelativeCut(t, tuple(int(r[1]) for r in table), len(table))


def _launch(K_, buf, view, table, coins, squeeze=False):
    dev = buf.cuda()
    x = view(dev)
    wide = torch.full((coins.shape[0], coins.shape[1] + 2), 2.0, dtype=torch.float32)      # coins with a leading dimension of their own
    wide[:, :coins.shape[1]] = torch.from_numpy(coins)
    out = K_.relative_cut_rows(x[:, 0] if squeeze else x, _raw(K_, table), wide.cuda()[:, :coins.shape[1]])
    assert out.data_ptr() == x.data_ptr()
    torch.cuda.synchronize()
    return dev.cpu()


@functools.lru_cache(maxsize=None)
def _case(V, dtype, k1, seed=0):
    buf, view = _arena(dtype, B, k1, V, 2000 + seed)
    table, coins = _table(MIX), COINS[:, :k1]
    return buf, view, table, coins, ref_relative_cut(view(buf).float().numpy(), table, coins, _esz(dtype))[1]


def _run_case(K_, V, dtype, k1s=(1, K1)):
    cases = [_case(V, dtype, k1, SEEDS.get((V, DTYPE_IDS[DTYPES.index(dtype)]), 0)) for k1 in k1s]
    assert_cap(np.concatenate([c[4].reshape(-1, V) for c in cases]), (V, dtype))       # on the reference alone, first
    live = False
    for (buf, view, table, coins, _), k1 in zip(cases, k1s):
        after = _launch(K_, buf, view, table, coins, squeeze=k1 == 1)
        outside = torch.ones(buf.shape, dtype=torch.bool)
        view(outside)[:] = False
        assert np.array_equal(_bits(buf)[outside.numpy()], _bits(after)[outside.numpy()]), "a write outside the rows"
        changed = _bits(view(buf)) != _bits(view(after))
        x1 = view(after).float().numpy()
        assert np.isneginf(x1[changed]).all()                                    # a kept token keeps its BITS
        keep, _, touched = check_rel_cut(view(buf).float().numpy(), x1, table, coins, _esz(dtype), (V, dtype, k1))
        assert (x1 > -np.inf).any(axis=-1).all()                                 # no row is emptied
        assert not touched[5, 1:].any() and not touched[7, 1:].any() and not touched[4].any()   # coin >= q, and off
        live |= bool((~keep).any())
        again = _launch(K_, buf, view, table, coins, squeeze=k1 == 1)            # the same call on a fresh copy: equal bytes
        assert np.array_equal(_bits(again), _bits(after))
    assert live or V < 64


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("V", [3, 64, 4099, 8203])
def test_random_rows_all_modes_mixed(K_, V, dtype):
    _run_case(K_, V, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("past", [0, 1], ids=["resident", "streaming"])
def test_both_sides_of_the_residency_bound(K_, past, dtype):
    _run_case(K_, BOUND[_esz(dtype)] + past, dtype, k1s=(K1,))


def test_full_vocabulary(K_):
    _run_case(K_, 152064, torch.bfloat16, k1s=(2,))


def _designed():
    """-> (x f64 [R, V], records, coins, names): the constructed rows; every expected pattern is exact (no window)."""
    V = 2500
    low = np.full(V, -20.0)
    xs, recs, coins, names = [], [], [], []

    def add(name, x, mode, a, b=0.0, coin=0.0, inv_t=1.0):
        xs.append(np.asarray(x, np.float64)); recs.append((f32(inv_t), mode, f32(a), f32(b))); coins.append(coin); names.append(name)
    for mode, a, b in ((TOP_N_SIGMA, 1.0, 0.0), (TOP_A, 1.0, 0.0), (XTC, 1e-4, 1.0)):
        add(f"flat {mode}", np.full(V, 1.5), mode, a, b)                         # nothing is cut in any mode; sigma = 0
    two = np.full(V, -np.inf)
    two[[5, 2100]] = 0.0
    add("two maxima", two, XTC, 0.5, 1.0)                                        # p = 0.5 each, t = 0.5: both stay
    three = low.copy()
    three[[7, 900, 2400]] = [3.0, 2.0, 2.0]
    add("tied minimum", three, XTC, 0.1, 1.0)                                    # the tie stays, the top goes
    add("coin equals q", three, XTC, 0.1, 0.5, coin=0.5)                         # c == q is "no"
    one = low.copy()
    one[7] = 5.0
    add("one above t", one, XTC, 0.1, 1.0)
    pair = np.full(V, -np.inf)
    pair[[5, 2100]] = [1.0, 0.4]
    add("pair sigma", pair, TOP_N_SIGMA, 0.5)                                    # mu = 0.7, sigma = 0.3 over the TWO elements: 0.4 goes
    add("pair xtc", pair, XTC, 0.2, 1.0)                                         # both in A: the arg-max goes
    add("pair top-a", pair, TOP_A, 1.0)                                          # p = (0.65, 0.35), bound 0.42: 0.4 goes
    nan = np.linspace(-3, 3, V)
    nan[1234] = np.nan
    add("nan", nan, TOP_N_SIGMA, 1.0)
    add("no finite", np.full(V, -np.inf), TOP_A, 0.5)
    for name, rec in (("bad mode", (1.0, 7, 0.5, 0.5)), ("bad inv_t", (-1.0, TOP_N_SIGMA, 1.0, 0.0)), ("bad a", (1.0, TOP_A, 2.0, 0.0)),
                      ("bad q", (1.0, XTC, 0.1, 1.5))):
        add(name, np.linspace(-3, 3, V), rec[1], rec[2], rec[3], inv_t=rec[0])
    return np.stack(xs), recs, np.array(coins, np.float32)[:, None], names


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_constructed_rows_are_exact(K_, dtype):
    x64, recs, coins, names = _designed()
    x = torch.from_numpy(x64).to(torch.float32).to(dtype)
    x0 = x.float().numpy()
    keep, _, touched = ref_relative_cut(x0, recs, coins, _esz(dtype))
    at = names.index
    cut_ids = lambda n: np.nonzero(~keep[at(n)])[0].tolist()                     # noqa: E731
    assert cut_ids("tied minimum") == [7] and cut_ids("pair sigma") == [2100] and cut_ids("pair xtc") == [5]
    assert cut_ids("pair top-a") == [2100]
    still = ["flat 1", "flat 2", "flat 3", "two maxima", "coin equals q", "one above t", "nan", "no finite", "bad mode", "bad inv_t",
             "bad a", "bad q"]
    assert all(keep[at(n)].all() for n in still)
    out = K_.relative_cut_rows(x.cuda(), _raw(K_, recs), torch.from_numpy(coins).cuda())
    torch.cuda.synchronize()
    bits0, bits1, x1 = _bits(x), _bits(out), out.cpu().float().numpy()
    for n in still:
        assert np.array_equal(bits0[at(n)], bits1[at(n)]), n                     # bit-equal, the NaN's payload included
    want_cut = ~keep | np.isneginf(x0)
    assert np.array_equal(np.isneginf(x1), want_cut)                             # exactly the reference's pattern, no window
    assert np.array_equal(bits0[~want_cut], bits1[~want_cut])


def test_step_uniforms_ex_adds_coins_and_moves_nothing(K_):
    Bn, K = 37, 5
    vals = [(i * 0x9E3779B97F4A7C15 + 11) % 2 ** 64 for i in range(Bn)]
    seeds = torch.tensor([v - 2 ** 64 if v >= 2 ** 63 else v for v in vals], dtype=torch.int64).cuda()
    new = lambda *shape: torch.full(shape, -1.0, dtype=torch.float32, device="cuda")   # noqa: E731
    old = new(K, Bn), new(Bn, K), new(Bn)
    K_.step_uniforms(seeds, 9, 2, *old)
    ex0 = new(K, Bn), new(Bn, K), new(Bn)
    rc = K_._lib().asd_step_uniforms_ex(seeds.data_ptr(), 9, 2, Bn, K, K, *[t.data_ptr() for t in ex0], None, 0, None)
    ex = new(K, Bn), new(Bn, K), new(Bn), new(Bn, K + 1)
    K_.step_uniforms(seeds, 9, 2, *ex)
    torch.cuda.synchronize()
    assert rc == 0
    for a, b, c in zip(old, ex0, ex):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() == c.cpu().numpy().tobytes()
    assert all(np.array_equal(a.cpu().numpy(), r) for a, r in zip(old, step_uniforms_ref(vals, 9, 2, K, K)))
    s = np.array(vals, dtype=np.uint64)[:, None]
    k = np.arange(K + 1, dtype=np.uint64)[None, :]
    words = philox4x32_10((np.uint64(9), k, np.uint64(2), np.uint64(0)), (s & np.uint64(0xFFFFFFFF), s >> np.uint64(32)))
    assert np.array_equal(ex[3].cpu().numpy(), to_uniform(words[..., 3]))
