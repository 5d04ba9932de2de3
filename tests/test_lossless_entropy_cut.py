"""Statistical losslessness with an entropy cut, on the CPU: tests/lossless_entropy_cut.py's case through the oracle twin's
entropy_cut_rows (tests/entropy_cut_ref.py) and the oracle chain of tests/test_lossless.py, on the bars of tests/lossless.py.
One negative control: the target rows left uncut must fail the same bars."""
import numpy as np
import torch

from tests import lossless as L
from tests import lossless_entropy_cut as C
from tests.entropy_cut_ref import EntropyCutOracleOps
from tests.test_lossless import OracleChain


def _twin_cut(x, m):
    ops = EntropyCutOracleOps()
    return C.cut_by(ops.entropy_cut_rows, ops.pack_entropy_cut, x, m, lambda t: t.numpy(), torch.from_numpy)


def test_typical_keep_on_hand_made_rows():
    row = np.zeros(8, np.float32)
    row[0] = np.log(0.3 / (0.7 / 7))                                         # p_0 = 0.3 over a uniform tail
    assert C.typical_keep(row, 1.0, 0.2).tolist() == [False] + [True] * 7    # every tie of the tail is kept, the arg-max is cut
    assert C.typical_keep(row, 1.0, 0.8).all()
    assert C.typical_keep(np.array([2.0, 1.0, 0.0, -1.0]), 1.0, 0.999999).all()


def test_cut_chain_is_lossless_against_the_cut_target():
    xt, xd, ref, ct, cd = C.rows_and_reference()
    got_t, got_d = _twin_cut(xt, C.M_TARGET), _twin_cut(xd, C.M_DRAFT)
    assert np.array_equal(np.isfinite(got_t), np.isfinite(ct)) and np.array_equal(np.isfinite(got_d), np.isfinite(cd))
    counts = L.run_chain(OracleChain(C.GEOM, C.ROUTE, "f32", got_t, got_d), C.GEOM, C.DRAW_SEED, C.GEOM.V + 1)
    L.assert_lossless(L.evaluate(counts, ref), "oracle chain behind the twin's cut, V 64")


def test_control_uncut_target_fails():
    xt, xd, ref, ct, cd = C.rows_and_reference()
    counts = L.run_chain(OracleChain(C.GEOM, C.ROUTE, "f32", xt, _twin_cut(xd, C.M_DRAFT)), C.GEOM, C.DRAW_SEED, C.GEOM.V + 1)
    assert L.failures(L.evaluate(counts, ref), statistical_only=True)
