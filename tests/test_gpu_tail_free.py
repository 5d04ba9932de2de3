"""asd_tail_free_rows on the GPU against tests/tail_free_ref.py (numpy f64, the header's text) over the WHOLE allocation (a guard
band in front and behind, ld_row = V + 13, an odd element offset: the arena of tests/test_gpu_entropy_cut.py).  Only the tokens
inside the reference's window are excused, and every test asserts on the reference alone, before it looks at the kernel, that
at most 2 % of its rows hold one.  Every launch gets a workspace poisoned with a pattern of its own.  V, after the kernel's
geometry: 3 (one d2), 64, 1024 | 1025 (a wave's slice of ceil(n / 16) keys passes its first 64 and a lane's chunk of
ceil(n / 1024) its first key), 4099 | 8203 (past a lane's first vector in f32 | 16 bits), one bf16 case at 152064.  The row is
never resident: there is no residency bound."""
import functools

import numpy as np
import pytest
import torch

from tests.tail_free_ref import assert_cap, check_tail_free, ref_tail_free
from tests.test_gpu_entropy_cut import DTYPE_IDS, DTYPES, INV_T, _arena, _bits, f32

pytestmark = pytest.mark.gpu

MIX = [0.5, 0.9, 0.95, 1.0, 0.99, 0.2]                                       # row 3 is off
B, K1 = len(MIX), 3


@pytest.fixture(scope="module")
def K_():
    from asd_amd import kernels
    return kernels


def _raw(K_, table):
    """The device table without the host's checks: a damaged record must reach the kernel."""
    rec = np.array([tuple(r) for r in table], dtype=K_._TFS_REC)
    return K_.TailFree(torch.from_numpy(rec.view(np.uint8).reshape(len(rec), 8).copy()).cuda(), tuple(r[1] for r in table), len(table))


def _launch(K_, buf, view, table, poison, squeeze=False):
    dev = buf.cuda()
    x = view(dev)
    ws = torch.full((K_.tail_free_workspace_bytes(*x.shape, x.dtype),), poison, dtype=torch.uint8, device="cuda")
    out = K_.tail_free_rows(x[:, 0] if squeeze else x, _raw(K_, table), ws)
    assert out.data_ptr() == x.data_ptr()
    torch.cuda.synchronize()
    return dev.cpu()


@functools.lru_cache(maxsize=None)
def _case(V, dtype, k1):
    buf, view = _arena(dtype, B, k1, V, 3000)                                    # (seed 3000 meets the cap at every shape below)
    table = [(f32(INV_T), f32(z)) for z in MIX]
    return buf, view, table, ref_tail_free(view(buf).float().numpy(), table)[1]


def _run_case(K_, V, dtype, k1s=(1, K1)):
    cases = [_case(V, dtype, k1) for k1 in k1s]
    assert_cap(np.concatenate([c[3].reshape(-1, V) for c in cases]), (V, dtype))       # on the reference alone, first
    live = False
    for (buf, view, table, _), k1 in zip(cases, k1s):
        after = _launch(K_, buf, view, table, 0xAA, squeeze=k1 == 1)
        outside = torch.ones(buf.shape, dtype=torch.bool)
        view(outside)[:] = False
        assert np.array_equal(_bits(buf)[outside.numpy()], _bits(after)[outside.numpy()]), "a write outside the rows"
        changed = _bits(view(buf)) != _bits(view(after))
        x1 = view(after).float().numpy()
        assert np.isneginf(x1[changed]).all()                                    # a kept token keeps its BITS
        keep, _, touched = check_tail_free(view(buf).float().numpy(), x1, table, (V, dtype, k1))
        assert (x1 > -np.inf).any(axis=-1).all() and not touched[3].any()        # no row is emptied; the off row
        live |= bool((~keep).any())
        again = _launch(K_, buf, view, table, 0x55, squeeze=k1 == 1)             # a fresh copy, another poison: equal bytes
        assert np.array_equal(_bits(again), _bits(after))
    assert live


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("V", [3, 64, 1024, 1025, 4099, 8203])
def test_random_rows_mixed_z(K_, V, dtype):
    _run_case(K_, V, dtype)


def test_full_vocabulary(K_):
    _run_case(K_, 152064, torch.bfloat16, k1s=(2,))


def _designed():
    """-> (x f64 [R, V], records, names): the constructed rows; every expected pattern is exact (no window)."""
    V = 4104
    p5 = np.full(V, -np.inf)
    p5[[9, 700, 2049, 3000, 4100]] = np.log([0.5, 0.3, 0.1, 0.06, 0.04])     # d2 = (0, 0.16, 0.02): 5 finite among 4099 -inf
    xs, recs, names = [], [], []

    def add(name, x, z, inv_t=1.0):
        xs.append(np.asarray(x, np.float64)); recs.append((f32(inv_t), f32(z))); names.append(name)
    add("p5 z=0.5", p5, 0.5)                                                     # c = (0, 0.16, 0.18), 0.09: i* = 1, 2 tokens stay
    add("p5 z=0.95", p5, 0.95)                                                   # 0.171: i* = 2, 3 tokens stay
    tie = np.full(V, -np.inf)
    tie[[3, 11, 1500, 2600, 4000, 4101]] = [4.0, 2.0, 2.0, 2.0, 0.0, -1.0]       # i* lands on the value 2.0: all three stay
    add("tie", tie, 0.85)                                                        # c / S = (0.795, 0.795, 0.903, 1)
    add("flat", np.full(V, 1.5), 0.5)
    two = np.full(V, -np.inf)
    two[[5, 2100]] = [1.0, 0.4]
    add("two finite", two, 0.5)
    for name, where, value in (("nan", 1234, np.nan), ("+inf", 77, np.inf)):
        row = np.linspace(-3, 3, V)
        row[where] = value
        add(name, row, 0.5)
    add("no finite", np.full(V, -np.inf), 0.5)
    add("off", np.linspace(-3, 3, V), 1.0)
    for name, (inv_t, z) in (("z=1.5", (1.0, 1.5)), ("z=0", (1.0, 0.0)), ("inv_t=0", (0.0, 0.5)), ("inv_t<0", (-1.0, 0.5))):
        add(name, np.linspace(-3, 3, V), z, inv_t)
    return np.stack(xs), recs, names


def test_constructed_rows_are_exact(K_):
    x64, recs, names = _designed()
    x = torch.from_numpy(x64).to(torch.float32)
    x0 = x.numpy()
    keep, und, _ = ref_tail_free(x0, recs)
    at = names.index
    kept = lambda n: np.nonzero(keep[at(n)] & np.isfinite(x0[at(n)]))[0].tolist()      # noqa: E731
    assert not und.any()
    assert kept("p5 z=0.5") == [9, 700] and kept("p5 z=0.95") == [9, 700, 2049] and kept("tie") == [3, 11, 1500, 2600]
    still = [n for n in names if n not in ("p5 z=0.5", "p5 z=0.95", "tie")]
    assert all(keep[at(n)].all() for n in still)
    out = K_.tail_free_rows(x.cuda(), _raw(K_, recs))
    torch.cuda.synchronize()
    bits0, bits1, x1 = _bits(x), _bits(out), out.cpu().numpy()
    for n in still:
        assert np.array_equal(bits0[at(n)], bits1[at(n)]), n                     # bit-equal, the NaN's payload included
    want_cut = ~keep | np.isneginf(x0)
    assert np.array_equal(np.isneginf(x1), want_cut)                             # exactly the reference's pattern, no window
    assert np.array_equal(bits0[~want_cut], bits1[~want_cut])
