"""asd_logit_shape_rows on the GPU against tests/logit_shape_ref.py (numpy f64, the header's text) over the WHOLE allocation (a
guard band in front and behind, ld_row = V + 13, an odd element offset: the arena of tests/test_gpu_entropy_cut.py).  EVERY
element must lie in its interval; on the 16-bit types every test first asserts, on the reference alone, that no interval of a
sharp element spans more than two adjacent values.  V follows the kernel's geometry (1024 lanes, 16-byte vectors, 19 resident
per lane): under one vector, past a lane's first vector, and the two sides of the residency bound of each element size."""
import numpy as np
import pytest
import torch

from asd_amd import kernels as K_
from tests.logit_shape_ref import DYNATEMP, OFF, QUADRATIC, ref_logit_shape, value_steps
from tests.test_gpu_entropy_cut import DTYPE_IDS, DTYPES, _arena, _bits, _esz, f32

pytestmark = pytest.mark.gpu

MIX = [(DYNATEMP, 0.7, 0.3, 0.5), (DYNATEMP, 1.0, 0.5, 1.0), (DYNATEMP, 1.5, 1.0, 2.0),
       (DYNATEMP, 0.7, float(np.nextafter(np.float32(0.7), np.float32(0))), 1.0),      # a range just under T
       (QUADRATIC, 0.0, 0.3, 1.0), (QUADRATIC, 0.0, 0.3, 2.0), (QUADRATIC, 0.0, 0.2, 3.0), (OFF, 0.0, 0.0, 0.0),
       (7, 1.0, 0.5, 1.0), (DYNATEMP, 0.5, 0.7, 1.0)]                                   # damaged: the mode; a range above T
B = len(MIX)
BOUND = {4: 77827, 2: 155655}                                                # the last V of the resident kernel, by element size


def _raw(table):                                                         # no host checks: a damaged record must reach the kernel
    rec = np.array([(m, f32(t), f32(a), f32(b)) for m, t, a, b in table], dtype=K_._SHAPE_REC)
    return K_.LogitShape(torch.from_numpy(rec.view(np.uint8).reshape(len(rec), 16).copy()).cuda(), tuple(r[0] for r in table), len(table))


def _check(before, after, table, dtype, what):
    """before / after: CPU tensors [B, K1, V] -> (touched per row, changed per element); every element in its interval."""
    x0, x1 = before.float().numpy(), after.float().numpy()
    lo, hi, touched, sharp = ref_logit_shape(x0, table, dtype)
    if dtype != torch.float32:                                               # on the reference alone, first
        assert (value_steps(lo, hi, dtype)[sharp] <= 1).all(), (what, "an interval of more than two values")
        assert sharp.mean() >= 0.98, (what, "the cancellation band of the quadratic rows holds more than 2 % of the elements")
    fin = np.isfinite(x0)
    same = _bits(before) == _bits(after)
    assert same[~fin].all() and same[~touched].all(), (what, "a -inf element or an untouched row changed")
    assert np.isfinite(x1[fin]).all(), (what, "a finite element became inf or NaN")
    bad = fin & ~((x1 >= lo) & (x1 <= hi))
    assert not bad.any(), (what, np.argwhere(bad)[:5], x0[bad][:5], x1[bad][:5], lo[bad][:5], hi[bad][:5])
    for b, rec in enumerate(table):
        for j in range(x0.shape[1] if rec[0] == QUADRATIC else 0):
            order = np.argsort(x0[b, j][fin[b, j]], kind="stable")
            assert (np.diff(x1[b, j][fin[b, j]][order]) >= 0).all(), (what, b, j, "the order of a quadratic row is inverted")
    return touched, ~same


def _run_case(V, dtype, k1):
    buf, view = _arena(dtype, B, k1, V, 3000)
    outs = []
    for _ in range(2):                                                       # the same call on a fresh copy: equal bytes
        dev = buf.cuda()
        x = view(dev)
        out = K_.logit_shape_rows(x[:, 0] if k1 == 1 else x, _raw(MIX))
        assert out.data_ptr() == x.data_ptr()
        torch.cuda.synchronize()
        outs.append(dev.cpu())
    after = outs[0]
    assert np.array_equal(_bits(after), _bits(outs[1]))
    outside = torch.ones(buf.shape, dtype=torch.bool)
    view(outside)[:] = False
    assert np.array_equal(_bits(buf)[outside.numpy()], _bits(after)[outside.numpy()]), "a write outside the rows"
    touched, changed = _check(view(buf), view(after), MIX, dtype, (V, dtype, k1))
    assert not touched[7:].any() and (touched[:7].all() or V < 2)            # off and damaged records: skipped
    assert V < 64 or all(changed[b].any() for b in range(7))                 # the pass is live on every row that is on


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("k1", [1, 3])
@pytest.mark.parametrize("V", [1, 3, 64, 4099, 8203, "resident", "streaming"])
def test_random_rows_all_modes_mixed(V, k1, dtype):
    if isinstance(V, str):                                                   # the two sides of the residency bound
        V = BOUND[_esz(dtype)] + (V == "streaming")
    _run_case(V, dtype, k1)


def _designed():
    V = 2500
    rng = np.random.default_rng(5)
    xs, recs, names = [], [], []

    def add(name, x, rec):
        xs.append(np.asarray(x, np.float64)); recs.append(rec); names.append(name)
    one = np.where(np.arange(V) == 1234, 2.5, -np.inf)
    nan, pinf = np.linspace(-3, 3, V), np.linspace(-3, 3, V)
    nan[77], pinf[2222] = np.nan, np.inf
    for tag, rec in (("dyn", (DYNATEMP, 1.0, 0.5, 1.0)), ("quad", (QUADRATIC, 0.0, 0.3, 2.0))):
        add(f"n == 1 {tag}", one, rec)
        add(f"n == 0 {tag}", np.full(V, -np.inf), rec)
        add(f"nan {tag}", nan, rec)
        add(f"+inf {tag}", pinf, rec)
        holes = rng.standard_normal(V) * 3
        holes[rng.random(V) < 0.3] = -np.inf
        add(f"holes {tag}", holes, rec)
    flat = np.where(np.arange(V) % 7 == 0, -np.inf, 4.0)                     # x c2 is exact for a power of two: s == n, u == 0, h == 1
    add("uniform", flat, (DYNATEMP, 1.5, 0.5, 2.0))                          # T_dyn = 1 + 2 * 0.5 = 2, g = 0.75: 3.0 exactly
    peak = np.where(np.arange(V) == 5, 60000.0, -60000.0)
    add("overflow", peak, (DYNATEMP, 1.5, 0.5, 1.0))                         # h = 0: g = 1.5, +-90000 leaves f16's range
    add("g == 1", rng.standard_normal(V) * 3, (DYNATEMP, 0.7, 1e-9, 1.0))    # |T_dyn - T| <= 1e-9: g rounds to 1, no write sweep
    return np.stack(xs), recs, names


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_constructed_rows(dtype):
    x64, recs, names = _designed()
    x = torch.from_numpy(x64).to(torch.float32).to(dtype)[:, None]
    out = K_.logit_shape_rows(x.cuda(), _raw(recs)).cpu()
    touched, changed = _check(x, out, recs, dtype, dtype)
    at = names.index
    for n in ("n == 1", "n == 0", "nan", "+inf"):
        assert not changed[at(f"{n} dyn")].any() and not changed[at(f"{n} quad")].any(), n   # bit-equal, the NaN's payload included
    assert touched[at("g == 1")].all() and not changed[at("g == 1")].any()
    assert changed[at("holes dyn")].any() and changed[at("holes quad")].any()
    flat = out[at("uniform"), 0].float().numpy()
    assert set(flat.tolist()) == {3.0, -np.inf} and np.array_equal(np.isneginf(flat), np.isneginf(x64[at("uniform")]))
    if dtype == torch.float16:                                               # clamped to the finite range, never inf
        peak = out[at("overflow"), 0].float().numpy()
        assert peak[5] == 65504.0 and (np.delete(peak, 5) == -65504.0).all()
