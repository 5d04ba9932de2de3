"""Statistical losslessness of the draft / verify / commit chain on the uniforms of asd_step_uniforms (CPU: the oracle chain of
tests/test_lossless.py on the numpy Philox reference).

tests/lossless.run_chain hands a backend fresh numpy uniforms per call.  `SeededChain` wraps a backend and ignores them: call
number c of the run is step c of B requests with seeds base + 0 .. base + B - 1 at stage 1, and the three stages of the chain
take the step's words by the layout of include/asd_hip.h -- proposal j of sequence b word 0 of slot j, the accept uniform word
1 of slot j, the commit draw word 2 of slot 0.  The driver, the case tables, the reference distribution and ALPHA are
tests/lossless.py's, unchanged: what is tested is that 2e5 sequences drawn this way are distributed as the target's, i.e. that
no two draws of a step share a word they must not share.  The negative control wires the accept uniform to the PROPOSAL word of
the same slot (u = r: a proposal from the low end of the draft's CDF is then always accepted) and must be noticed."""
import numpy as np
import pytest

from tests import lossless as L
from tests.philox_ref import step_uniforms_ref
from tests.test_lossless import DRAW_SEED, ROW_SEED, OracleChain

SEED_BASE = 2 ** 40 + 12345
STAGE = 1


class SeededChain:
    """A lossless.run_chain backend over another one (`inner`: draft / verify / residual, B, K) that substitutes the step's
    uniforms.  uniforms(seeds int64 [B], step, stage, K_draft, K_accept) -> numpy (r_draft [K, B], u [B, K], r_commit [B]):
    the reference here, the kernel in tests/test_gpu_seeded_stages.py.  wiring: "ok", or "accept_is_proposal" (the control)."""

    def __init__(self, inner, uniforms=step_uniforms_ref, wiring="ok", base=SEED_BASE):
        self.inner, self.uniforms, self.wiring = inner, uniforms, wiring
        self.seeds = (base + np.arange(inner.B)).astype(np.int64)
        self.step = -1

    def draft(self, r):
        B, K = self.inner.B, self.inner.K
        self.step += 1                                               # one call of the chain = one step of every request
        rd, u, rc = self.uniforms(self.seeds, self.step, STAGE, K, K)
        assert rd.shape == (K, B) and u.shape == (B, K) and rc.shape == (B,) and r.shape == (B * K,)
        if self.wiring == "accept_is_proposal":
            u = np.ascontiguousarray(rd.T)
        self.u, self.rc = u, rc
        return self.inner.draft(np.ascontiguousarray(rd.T).reshape(-1))      # r[b * K + j]: the proposal word of slot j

    def verify(self, tok, lp_d, u):
        return self.inner.verify(tok, lp_d, self.u)

    def residual(self, n_acc, r, d_thr, t_thr):
        return self.inner.residual(n_acc, self.rc, d_thr, t_thr)


def _run(wiring):
    route = L.ROUTES["b"]
    xt, xd = L.make_rows(L.SMALL, "bf16", ROW_SEED)
    ref = L.reference(xt, xd, route)
    chain = SeededChain(OracleChain(L.SMALL, route, "bf16", xt, xd), wiring=wiring)
    counts = L.run_chain(chain, L.SMALL, DRAW_SEED, L.SMALL.V + 1)
    assert chain.step == L.SMALL.n_calls - 1
    return L.evaluate(counts, ref), counts


def test_seeded_oracle_chain_is_lossless():
    assert L.ALPHA == 1e-6
    findings, counts = _run("ok")
    assert counts.n_seq >= 200000
    L.assert_lossless(findings, "seeded oracle chain, route b bf16")


def test_accept_uniform_wired_to_the_proposal_word_is_noticed():
    findings, _ = _run("accept_is_proposal")
    bad = L.failures(findings, statistical_only=True)
    print(f"[lossless] control accept_is_proposal: {len(bad)} checks failed; "
          + " | ".join(f"{f.what} class {f.cls} j {f.j}: {f.error}" for f in bad[:3]))
    assert bad and all(isinstance(f.error, L.HistogramError) for f in bad)
    assert all(f.what != "draft" for f in bad)                  # the proposals themselves are still the draft's
    with pytest.raises(L.HistogramError):                       # (evaluate collects the errors: the first, as raised)
        raise bad[0].error
