"""Statistical losslessness with an entropy cut, on the GPU beside tests/test_gpu_lossless.py: tests/lossless_entropy_cut.py's
case -- V = 64, the draft rows cut with one typical_p and the target rows with another by asd_entropy_cut_rows -- through
DraftSampler, verify_accept and ResidualSampler, on the harness and bars of tests/lossless.py."""
import numpy as np
import pytest

from tests import lossless as L
from tests import lossless_entropy_cut as C
from tests.entropy_cut_ref import assert_cap, ref_entropy_cut
from tests.test_gpu_lossless import PAD, HipChain, TorchOps

pytestmark = pytest.mark.gpu


def test_cut_chain_is_lossless_against_the_cut_target():
    import torch
    from asd_amd import kernels as K_
    xt, xd, ref, ct, cd = C.rows_and_reference()
    for x, m in ((xt, C.M_TARGET), (xd, C.M_DRAFT)):                         # on the reference alone: no row has a token at a boundary
        und = ref_entropy_cut(x, [(L.INV_T, C.TYPICAL, float(np.float32(m)))] * x.shape[0])[2]
        assert assert_cap(und, "lossless rows") == 0
    dev = lambda a: torch.from_numpy(a).cuda()                               # noqa: E731
    got_t = C.cut_by(K_.entropy_cut_rows, K_.pack_entropy_cut, xt, C.M_TARGET, lambda t: t.cpu().numpy(), dev)
    got_d = C.cut_by(K_.entropy_cut_rows, K_.pack_entropy_cut, xd, C.M_DRAFT, lambda t: t.cpu().numpy(), dev)
    # the kernel's kept sets are the definition's (no token of these rows lies at a boundary), and kept values keep their bits
    assert np.array_equal(got_t.view(np.uint32), ct.view(np.uint32)) and np.array_equal(got_d.view(np.uint32), cd.view(np.uint32))
    chain = HipChain(K_, C.GEOM, C.ROUTE, "f32", got_t, got_d)
    counts = L.run_chain(chain, C.GEOM, C.DRAW_SEED, C.GEOM.V + PAD + 1, xp=TorchOps)
    torch.cuda.synchronize()
    assert chain.ds.status() == 0 and chain.rs.status() == 0 and chain.ws.status() == 0
    L.assert_lossless(L.evaluate(counts, ref), "HIP chain behind asd_entropy_cut_rows, V 64")
