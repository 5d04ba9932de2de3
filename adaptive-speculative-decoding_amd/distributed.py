"""Multi-GPU forms of the verify step: one process per GPU, torch.distributed (backend "nccl" = RCCL
over xGMI on the GPU box, "gloo" in the CPU tests).  The reference has no collective of its own
(TP lives inside vLLM); these are the three placements SURVEY.md §8e derives from
the north star, and the rule they share is that FULL LOGITS NEVER CROSS A LINK:

  batch-parallel replicas   every rank verifies its own slice of the batch; no data-path
                            collective at all (optional all-gather of n_acc, 4 B per sequence).
  tiers on different GPUs   the verify kernel runs where the target logits are produced; the draft
                            rank ships tok + lp_d ([B,K] i32 + f32 = 2 KB at B=32, K=8) and gets
                            accept + n_acc back (~400 B): `TierLink`, point-to-point send/recv.
  vocab-sharded target      each rank reduces its [B,K,V/R] slice to (m2, s, g) triples
                            (asd_lse_partial), ONE all-gather of [B,K,3] f32 per rank (3 KB at B=32),
                            then every rank combines them in rank order (asd_accept_from_partials):
                            `VocabShardedVerifier`.  Moving the logits instead would cost 77.9 MB /
                            153 GB/s = 0.5 ms per hop against a ~17 us kernel.

The compute is reached through a small `ops` object so that the CPU test-suite can drive the
exchange logic over gloo with the oracle (tests/oracle_backend.py: OracleOps); the default is the
HIP kernels and there is no other implementation in this package.
"""
from __future__ import annotations

from typing import Tuple

import torch
import torch.distributed as dist

from .trace import traced


def shard_bounds(total: int, world: int, rank: int) -> Tuple[int, int]:
    """Contiguous, balanced [start, end) of `total` items for `rank` of `world`."""
    return total * rank // world, total * (rank + 1) // world


class HipOps:
    """The product: device tensors through libasd_hip.so.

    Re-entrant: the reference serves requests from a pool of up to 100 threads (src/serving/pipeline.py:83,155), so the
    scratch a call needs -- verify workspaces, sampler mailboxes, lm_head partial buffers -- is kept PER CALLING THREAD
    (a workspace must never be shared by calls that may overlap; each thread launches on its own current stream).  Only
    the packed lm_head images are shared between threads: they are read-only snapshots of a weight matrix."""

    def __init__(self, pack_lm_head: bool = True, profile: bool = False):
        """profile: bracket every verify step (verify_accept / verify_stop / lm_head_verify) with a HIP event pair on the
        calling thread's stream; `stats()` then reports `kernel_us` / `hbm_gbps` of the last one (the keys SURVEY §5 adds
        to the reference's get_stats(), pipeline.py:346-370).  Off by default: an event pair costs 5-15 us on this stack.
        pack_lm_head: lm_head matrices handed to lm_head_verify / lm_head_partial are re-laid out once, tile-major
        (asd_lm_head_pack_weights: 3-12 % faster streaming, bit-identical results).  COST: one more copy of every such
        matrix in HBM (+V*D*2 bytes: +2.5 GB for the 152064 x 8192 head of the 72B tier, +1.1 GB for the 7B one); pass
        False where that memory is needed for KV or batch."""
        import threading
        from . import kernels
        self.K = kernels
        self._tls = threading.local()
        self._packed = {}                    # weight key -> packed image (shared, read-only)
        self._lock = threading.Lock()
        self.pack_lm_head = bool(pack_lm_head)
        self.profile = bool(profile)

    def _timed_step(self, what, nbytes, fn):
        if not self.profile:
            return fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        self._tls.last = (e0, e1, int(nbytes), what)       # per calling thread, like the scratch: stats() reports THIS thread's step
        return out

    def stats(self):
        """{"kernel_us", "hbm_gbps", "step"} of the last verify step the CALLING THREAD profiled (waits for it to finish); {} if none."""
        last = getattr(self._tls, "last", None)
        if last is None:
            return {}
        e0, e1, nbytes, what = last
        e1.synchronize()
        us = 1e3 * e0.elapsed_time(e1)
        return {"kernel_us": us, "hbm_gbps": nbytes / (us * 1e-6) / 1e9 if us > 0 else 0.0, "step": what,
                "algorithmic_bytes": nbytes}

    @property
    def _ws(self):
        d = getattr(self._tls, "ws", None)
        if d is None:
            d = self._tls.ws = {}
        return d

    def check_status(self) -> None:
        """The sticky status words (include/asd_hip.h: asd_workspace_status) of every hand-off workspace the CALLING THREAD has
        used -- verify workspaces, the draft and residual samplers' mailboxes -- in ONE synchronising read.  A kernel whose bounded
        wait for a hand-off word ran out poisoned what depended on it (lp_t = NaN and reject; score = NaN, k* = L - 1; tok = -1) and
        raised the word: this raises kernels.LostHandoffError for it, after re-initialising every workspace that reported a loss
        (the late word was never handed back empty, so such a workspace is no longer all-zero between calls).  The loop drivers
        call it once per step, at a point where they synchronise anyway."""
        wss = [w for w in self._ws.values() if isinstance(w, self.K._StatusWorkspace)]
        if not wss:
            return
        by_dev = {}
        for w in wss:
            by_dev.setdefault(w.buf.device, []).append(w)
        dirty = []
        for group in by_dev.values():
            words = torch.stack([w.status_word for w in group])
            if int(words.max().item()) != 0:
                dirty += [w for w, v in zip(group, words.tolist()) if v != 0]
        if dirty:
            names = ", ".join(f"{type(w).__name__} (status 0x{int(w.status_word.item()):x})" for w in dirty)
            for w in dirty:
                w.reset()
            raise self.K.LostHandoffError(f"a hand-off word never arrived in: {names}; the affected results were poisoned and the "
                                          "workspaces have been re-initialised")

    def _workspace(self, B, K, V, dtype, device):
        key = (B, K, str(dtype), str(device))
        ws = self._ws.get(key)
        if ws is None or ws.V < V:
            ws = self._ws[key] = self.K.VerifyWorkspace(B, K, V, dtype, device)
        return ws

    @traced("verify_accept")
    def verify_accept(self, logits, tok, lp_d, u, inv_temperature: float = 1.0):
        B, K = tok.shape
        ws = self._workspace(B, K, logits.shape[-1], logits.dtype, logits.device)
        nbytes = B * K * logits.shape[-1] * logits.element_size() + 17 * B * K + 12 * B
        r = self._timed_step("asd_verify_accept", nbytes,
                             lambda: self.K.verify_accept(logits, tok, lp_d, u, ws, inv_temperature=inv_temperature))
        return r.lp_target, r.accept, r.n_acc, r.accept_bits

    @traced("verify_accept_top_p")
    def verify_accept_top_p(self, logits, tok, lp_d, u, inv_temperature: float = 1.0, top_p: float = 1.0):
        """Verify against the TARGET's nucleus (asd_verify_accept_top_p) -> (lp_t, accept, n_acc, bits, x* [B,K], n_finite [B]);
        top_p outside (0, 1) is asd_verify_accept_ex (the same bits)."""
        B, K = tok.shape
        ws = None if 0.0 < top_p < 1.0 else self._workspace(B, K, logits.shape[-1], logits.dtype, logits.device)
        nbytes = B * K * logits.shape[-1] * logits.element_size() + 21 * B * K + 16 * B
        r = self._timed_step("asd_verify_accept_top_p", nbytes, lambda: self.K.verify_accept_top_p(
            logits, tok, lp_d, u, ws, inv_temperature=inv_temperature, top_p=top_p))
        return r.lp_target, r.accept, r.n_acc, r.accept_bits, r.t_nucleus_logit, r.n_finite

    @traced("verify_accept_top_k")
    def verify_accept_top_k(self, logits, tok, lp_d, u, inv_temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0):
        """Verify against the TARGET's Temperature -> TopK -> TopP set (asd_verify_accept_top_k) -> (lp_t, accept, n_acc, bits,
        thr [B,K], n_finite [B]); top_k <= 0 or >= V is verify_accept_top_p (the same bits)."""
        B, K = tok.shape
        V = logits.shape[-1]
        off = not (0 < top_k < V) and not (0.0 < top_p < 1.0)
        ws = self._workspace(B, K, V, logits.dtype, logits.device) if off else None
        nbytes = B * K * V * logits.element_size() + 21 * B * K + 16 * B
        r = self._timed_step("asd_verify_accept_top_k", nbytes, lambda: self.K.verify_accept_top_k(
            logits, tok, lp_d, u, ws, inv_temperature=inv_temperature, top_k=top_k, top_p=top_p))
        return r.lp_target, r.accept, r.n_acc, r.accept_bits, r.t_nucleus_logit, r.n_finite

    @traced("verify_accept_min_p")
    def verify_accept_min_p(self, logits, tok, lp_d, u, inv_temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0,
                            min_p: float = 0.0):
        """Verify against the TARGET's Temperature -> TopK -> TopP -> MinP set (asd_verify_accept_min_p) -> (lp_t, accept,
        n_acc, bits, thr [B,K], n_finite [B]); min_p <= 0 is verify_accept_top_k (the same bits)."""
        B, K = tok.shape
        V = logits.shape[-1]
        off = not (0 < top_k < V) and not (0.0 < top_p < 1.0) and not min_p > 0.0
        ws = self._workspace(B, K, V, logits.dtype, logits.device) if off else None
        nbytes = B * K * V * logits.element_size() + 21 * B * K + 16 * B
        r = self._timed_step("asd_verify_accept_min_p", nbytes, lambda: self.K.verify_accept_min_p(
            logits, tok, lp_d, u, ws, inv_temperature=inv_temperature, top_k=top_k, top_p=top_p, min_p=min_p))
        return r.lp_target, r.accept, r.n_acc, r.accept_bits, r.t_nucleus_logit, r.n_finite

    @traced("verify_stop")
    def verify_stop(self, logits, tok, lp_d, u, inv_temperature, pred, feat, p_hist, stage_idx, costs, lam,
                    risk_adjustment=True, n_obs=100, alpha=1.0, beta=1.0, stats_col=5):
        """ONE launch per tier step (asd_verify_accept_fused_ex): verify + accept, then -- inside the same kernel, by the
        wave that completes each sequence -- statistics of the K target log-probs -> predictor -> Bayes -> DP rule
        (pipeline.py:225-261).  Returns ((lp_t, accept, n_acc, bits), (score, k_star, p_hist)); p_hist is updated in
        place.  Bit-identical to verify_accept followed by predictor_stop (tests/test_gpu_predictor.py)."""
        B, K = tok.shape
        ws = self._workspace(B, K, logits.shape[-1], logits.dtype, logits.device)
        packed, in_dim, hidden = pred
        nbytes = B * K * logits.shape[-1] * logits.element_size() + 17 * B * K + 12 * B
        v, r = self._timed_step("asd_verify_accept_fused_ex", nbytes, lambda: self.K.verify_accept_fused(
            logits, tok, lp_d, u, ws, feat, packed, in_dim, hidden, stage_idx=stage_idx, L=p_hist.shape[1], stats_col=stats_col,
            risk_adjustment=risk_adjustment, n_obs=n_obs, alpha=alpha, beta=beta, p_hist=p_hist, Cc=costs, lam=lam,
            inv_temperature=inv_temperature))
        return (v.lp_target, v.accept, v.n_acc, v.accept_bits), (r.score, r.k_star, p_hist)

    @traced("lse_partial")
    def lse_partial(self, logits_shard, tok, v_offset, inv_temperature: float = 1.0):
        B, K = tok.shape
        ws = self._workspace(B, K, logits_shard.shape[-1], logits_shard.dtype, logits_shard.device)
        return self.K.lse_partial(logits_shard, tok, v_offset, ws, inv_temperature=inv_temperature)

    @traced("accept_from_partials")
    def accept_from_partials(self, msg_all, lp_d, u, inv_temperature: float = 1.0):
        r = self.K.accept_from_partials(msg_all, lp_d, u, inv_temperature=inv_temperature)
        return r.lp_target, r.accept, r.n_acc, r.accept_bits

    @staticmethod
    def _weight_key(w):
        """Identity of a weight matrix AS DATA: address, geometry, dtype and torch's in-place version counter.  The address
        alone is not enough: an in-place update (`w.add_`, a checkpoint reload into the same storage) keeps it,
        and a row slice of a larger matrix shares it."""
        return (w.data_ptr(), tuple(w.shape), tuple(w.stride()), str(w.dtype), str(w.device), int(w._version))

    def _lm_head(self, weight, B, K):
        wkey = self._weight_key(weight)
        key = ("lmh", wkey[0], K)
        ver = self._ws.get(key)
        if ver is not None and (ver.wkey != wkey or ver.B < B):
            ver = None                           # the matrix changed in place (repack), or a larger batch than it was sized for
        if ver is None:
            image = None
            can_pack = self.pack_lm_head and weight.shape[1] % 64 == 0
            if can_pack:
                with self._lock:
                    for k2 in [k2 for k2 in self._packed if k2[:5] == wkey[:5] and k2 != wkey]:
                        del self._packed[k2]     # older versions of this very matrix (a row slice at the same address is its own entry)
                    image = self._packed.get(wkey)
            ver = self.K.LmHeadVerifier(weight, B, K, packed=can_pack and image is None, packed_image=image)
            ver.wkey = wkey
            if can_pack and image is None:
                with self._lock:
                    self._packed.setdefault(wkey, ver.packed)
            self._ws[key] = ver
        return ver

    @traced("lm_head_partial")
    def lm_head_partial(self, hidden, weight_shard, tok, v_offset, inv_temperature: float = 1.0):
        B, K = tok.shape
        return self._lm_head(weight_shard, B, K).partial(hidden, tok, v_offset, inv_temperature)

    @traced("lm_head_verify")
    def lm_head_verify(self, hidden, weight, tok, lp_d, u, inv_temperature: float = 1.0):
        """N2: verify from hidden states [n,K,D] and the [V,D] lm_head matrix (logits stay in MFMA accumulators)."""
        B, K = tok.shape
        ver = self._lm_head(weight, B, K)
        nbytes = weight.numel() * weight.element_size() + B * K * weight.shape[1] * weight.element_size()
        r = self._timed_step("asd_lm_head_verify", nbytes, lambda: ver(hidden, tok, lp_d, u, inv_temperature=inv_temperature))
        return r.lp_target, r.accept, r.n_acc, r.accept_bits

    # -- the rest of a tier step (serving/hierarchy.py): stop decision, proposal, commit draw, bookkeeping
    def pack_predictor(self, predictor, device):
        """predictor: MinimalQualityPredictor-like (weights_numpy / input_dim / hidden_dim) -> opaque handle."""
        return (self.K.pack_mlp_weights(*predictor.weights_numpy(), device=device), predictor.input_dim, predictor.hidden_dim)

    @traced("predictor_stop")
    def predictor_stop(self, pred, lp, feat, p_hist, stage_idx, costs, lam, risk_adjustment=True, n_obs=100, alpha=1.0,
                       beta=1.0, stats_col=5, n_valid=None):
        """asd_predictor_stop on [n] sequences: p_hist [n,L] f64 is updated in place (column stage_idx) and returned
        with (score f32 [n], k_star i32 [n]).  n_valid [n] i32: leading lp entries the statistics use (None: all K)."""
        packed, in_dim, hidden = pred
        r = self.K.predictor_stop(feat, packed, in_dim, hidden, stage_idx=stage_idx, L=p_hist.shape[1], lp=lp, n_valid=n_valid,
                                  stats_col=stats_col, risk_adjustment=risk_adjustment, n_obs=n_obs, alpha=alpha, beta=beta,
                                  p_hist=p_hist, Cc=costs, lam=lam)
        return r.score, r.k_star, p_hist

    def _sampler(self, kind, B, V, dtype, device):
        key = (kind, V, str(dtype), str(device))
        s = self._ws.get(key)
        if s is None or s.B < B:
            cls = self.K.DraftSampler if kind == "draft" else self.K.ResidualSampler
            s = self._ws[key] = cls(B, V, dtype, device)
        return s

    @traced("draft_sample")
    def draft_sample(self, logits, r, inv_temperature: float = 1.0, top_p: float = 1.0):
        """X1: logits [B,V] -> (tok i32 [B], log q(tok) f32 [B], nucleus threshold f32 [B])."""
        d = self._sampler("draft", logits.shape[0], logits.shape[1], logits.dtype, logits.device)(logits, r, inv_temperature, top_p)
        return d.tok, d.lp, d.thr

    @traced("draft_sample_top_k")
    def draft_sample_top_k(self, logits, r, inv_temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0):
        """X1 under Temperature -> TopK -> TopP (asd_draft_sample_top_k): logits [B,V] -> (tok i32 [B], log q(tok) f32 [B],
        threshold max(x_k, x*_K) f32 [B])."""
        s = self._sampler("draft", logits.shape[0], logits.shape[1], logits.dtype, logits.device)
        d = s.top_k(logits, r, inv_temperature, top_k=top_k, top_p=top_p)
        return d.tok, d.lp, d.thr

    @traced("draft_sample_min_p")
    def draft_sample_min_p(self, logits, r, inv_temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0,
                           min_p: float = 0.0):
        """X1 under Temperature -> TopK -> TopP -> MinP (asd_draft_sample_min_p): logits [B,V] -> (tok i32 [B], log q(tok)
        f32 [B], threshold max(thr_kp, x_max + T ln(min_p)) f32 [B])."""
        s = self._sampler("draft", logits.shape[0], logits.shape[1], logits.dtype, logits.device)
        d = s.min_p(logits, r, inv_temperature, min_p=min_p, top_k=top_k, top_p=top_p)
        return d.tok, d.lp, d.thr

    @traced("residual_sample")
    def residual_sample(self, t_logits, d_logits, n_acc, r, bonus, inv_temperature: float = 1.0, d_threshold=None,
                        t_threshold=None, top_p: float = 1.0):
        """t_logits / d_logits [n,K,V], bonus [n,V], n_acc i32 [n], r f32 [n] -> committed token i32 [n].
        0 < top_p < 1: against the TARGET's nucleus (asd_residual_sample_top_p; t_threshold [n,K] = the verify's x*)."""
        s = self._sampler("residual", t_logits.shape[0], t_logits.shape[2], t_logits.dtype, t_logits.device)
        if 0.0 < top_p < 1.0:
            return s.top_p(t_logits, d_logits, n_acc, r, bonus, inv_temperature, top_p=top_p, t_threshold=t_threshold,
                           d_threshold=d_threshold)
        return s(t_logits, d_logits, n_acc, r, bonus, inv_temperature, d_threshold=d_threshold)

    @traced("residual_sample_top_k")
    def residual_sample_top_k(self, t_logits, d_logits, n_acc, r, bonus, inv_temperature: float = 1.0, d_threshold=None,
                              t_threshold=None, top_k: int = 0, top_p: float = 1.0):
        """The committed token against the TARGET's top-k + top-p set (asd_residual_sample_top_k; t_threshold [n,K] = the
        thresholds of verify_accept_top_k).  top_k <= 0 or >= V is the top-p route (the same bits)."""
        s = self._sampler("residual", t_logits.shape[0], t_logits.shape[2], t_logits.dtype, t_logits.device)
        return s.top_k(t_logits, d_logits, n_acc, r, bonus, inv_temperature, top_k=top_k, top_p=top_p, t_threshold=t_threshold,
                       d_threshold=d_threshold)

    @traced("residual_sample_lp")
    def residual_sample_lp(self, t_logits, d_logits, n_acc, r, bonus, inv_temperature: float = 1.0, d_threshold=None,
                           t_threshold=None, top_k: int = 0, top_p: float = 1.0, min_p: float = 0.0):
        """The committed token and its target log-prob (asd_residual_sample_lp) -> (token i32 [n], lp f32 [n]); the token is
        residual_sample's / residual_sample_top_k's on the same arguments, lp = log p_t^N(token).  min_p > 0: against the
        target's min-p set as well (asd_residual_sample_lp_min_p; t_threshold = the thresholds of verify_accept_min_p)."""
        s = self._sampler("residual", t_logits.shape[0], t_logits.shape[2], t_logits.dtype, t_logits.device)
        if min_p > 0.0:
            return s.lp_min_p(t_logits, d_logits, n_acc, r, bonus, inv_temperature, top_k=top_k, top_p=top_p, min_p=min_p,
                              t_threshold=t_threshold, d_threshold=d_threshold)
        return s.lp(t_logits, d_logits, n_acc, r, bonus, inv_temperature, top_k=top_k, top_p=top_p, t_threshold=t_threshold,
                    d_threshold=d_threshold)

    # -- per-request sampling parameters (serving/stages.py, PER-REQUEST SAMPLING): one packed table per generate call
    def pack_sampling_rows(self, inv_temperature, top_k, top_p, min_p, V, dtype, device):
        """The packed per-sequence table of the *_rows ops (asd_sampling_rows_pack), uploaded once: inv_temperature / top_k /
        top_p / min_p hold one value per sequence (top_k / top_p / min_p may be None = off) -> opaque handle."""
        return self.K.SamplingRows(inv_temperature, top_k, top_p, min_p, V=V, dtype=dtype, device=device)

    @traced("draft_sample_rows")
    def draft_sample_rows(self, logits, r, rows):
        """X1 with every sequence's own Temperature -> TopK -> TopP -> MinP (asd_draft_sample_rows): logits [B,V] -> (tok i32
        [B], log q(tok) f32 [B], threshold f32 [B]); sequence b has the bits of draft_sample_min_p with its values."""
        d = self._sampler("draft", logits.shape[0], logits.shape[1], logits.dtype, logits.device).rows(logits, r, rows)
        return d.tok, d.lp, d.thr

    @traced("verify_accept_rows")
    def verify_accept_rows(self, logits, tok, lp_d, u, rows):
        """Verify against every sequence's own target distribution (asd_verify_accept_rows) -> (lp_t, accept, n_acc, bits,
        thr [B,K], n_finite [B]); a sequence that truncates nothing is scored by the same select kernel (thr = -inf)."""
        B, K = tok.shape
        nbytes = B * K * logits.shape[-1] * logits.element_size() + 21 * B * K + 16 * B + 32 * B
        r = self._timed_step("asd_verify_accept_rows", nbytes, lambda: self.K.verify_accept_rows(logits, tok, lp_d, u, rows))
        return r.lp_target, r.accept, r.n_acc, r.accept_bits, r.t_nucleus_logit, r.n_finite

    @traced("residual_sample_lp_rows")
    def residual_sample_lp_rows(self, t_logits, d_logits, n_acc, r, bonus, rows, d_threshold=None, t_threshold=None):
        """The committed token and its target log-prob with every sequence's own parameters (asd_residual_sample_lp_rows) ->
        (token i32 [n], lp f32 [n]); t_threshold = the thresholds of verify_accept_rows."""
        s = self._sampler("residual", t_logits.shape[0], t_logits.shape[2], t_logits.dtype, t_logits.device)
        return s.lp_rows(t_logits, d_logits, n_acc, r, bonus, rows=rows, t_threshold=t_threshold, d_threshold=d_threshold)

    @traced("top_logprobs_rows")
    def top_logprobs_rows(self, logits, n, rows, splits: int = 0):
        """top_logprobs with every sequence's own temperature (asd_top_logprobs_rows; rows: the pack_sampling_rows handle)."""
        return self._top_logprobs(logits, n, rows.inv_t, splits)

    @traced("verify_greedy")
    def verify_greedy(self, logits, tok=None, inv_temperature: float = 1.0, splits: int = 0):
        """Greedy decoding's step (asd_verify_greedy): logits [B,K+1,V] read in place (or [B,V] with tok = None: K = 0), tok i32
        [B,K] -> (lp_t [B,K], n_acc [B], drawn [B], lp_drawn [B], argmax [B,K+1], lp_argmax [B,K+1]).  One verifier (workspace)
        per shape and calling thread, like `_sampler`."""
        K = 0 if tok is None else tok.shape[1]
        Bv, V = logits.shape[0], logits.shape[-1]
        key = ("greedy", K, V, str(logits.dtype), str(logits.device))
        g = self._ws.get(key)
        if g is None or g.B < Bv:
            g = self._ws[key] = self.K.GreedyVerifier(Bv, K, V, logits.dtype, logits.device)
        r = g(logits, tok, inv_temperature, splits)
        return r.lp_target, r.n_acc, r.drawn, r.lp_drawn, r.argmax, r.lp_argmax

    @traced("top_logprobs")
    def top_logprobs(self, logits, n, inv_temperature: float = 1.0, splits: int = 0):
        """The `n` most likely tokens of every row and their log-probs over the whole vocabulary (asd_top_logprobs): logits
        [B,K1,V] -- a strided view is read in place, nothing is copied -- or [B,V] -> (top_id i32 [B,K1,n], top_lp f32 [B,K1,n]),
        value descending then id ascending, (-1, -inf) in slots that cannot be filled.  One workspace per shape and calling
        thread, like `verify_greedy`."""
        return self._top_logprobs(logits, n, inv_temperature, splits)

    def _top_logprobs(self, logits, n, inv_temperature, splits):
        K1 = 1 if logits.dim() == 2 else logits.shape[1]
        Bv, V = logits.shape[0], logits.shape[-1]
        key = ("top_logprobs", K1, V, int(n), str(logits.dtype), str(logits.device))
        t = self._ws.get(key)
        if t is None or t.B < Bv:
            t = self._ws[key] = self.K.TopLogprobs(Bv, K1, V, logits.dtype, int(n), logits.device)
        return t(logits, inv_temperature, splits)

    @traced("prompt_logprobs")
    def prompt_logprobs(self, logits, target, first, n, inv_temperature: float = 1.0, splits: int = 0):
        """The log-prob and the rank of target[b, t] in every row of [B,T,V] logits and, with n >= 1, the rows' top-n tables
        (asd_prompt_logprobs) -> (lp f32 [B,T], rank i32 [B,T], top_id i32 [B,T,n] | None, top_lp f32 [B,T,n] | None).  logits
        and target may be strided views, nothing is copied; rows with t < first[b] are skipped.  One workspace per shape and
        calling thread, like `top_logprobs`."""
        Bv, T, V = logits.shape
        key = ("prompt_logprobs", Bv, T, V, int(n), int(splits), str(logits.dtype), str(logits.device))
        t = self._ws.get(key)
        if t is None:
            t = self._ws[key] = self.K.PromptLogprobs(Bv, T, V, logits.dtype, int(n), int(splits), logits.device)
        return t(logits, target, first, inv_temperature)

    @traced("token_stats")
    def token_stats(self, logits, tok, n_acc, drawn, n: int = 0, inv_temperature: float = 1.0, rows=None, splits: int = 0):
        """Per row of a step's [B,K1,V] (or [B,V]) logits that may be committed -- row j of sequence b while j <= n_acc[b], scoring
        tok[b, j] below n_acc[b] and drawn[b] at it -- the rank of that token, the arg-max and its log-prob, the entropy and,
        with n >= 1, the row's top-n table, in one streaming pass (asd_token_stats) -> (stat_id i32 [B,K1,2] (rank, arg-max id),
        stat_val f32 [B,K1,2] (entropy in nats, max log-prob), top_id i32 [B,K1,n] | None, top_lp f32 [B,K1,n] | None).  rows:
        the pack_sampling_rows handle, whose per-sequence temperatures then hold (as in top_logprobs_rows).  logits and tok may
        be strided views, nothing is copied.  One workspace per shape and calling thread, like `prompt_logprobs`."""
        K1 = 1 if logits.dim() == 2 else logits.shape[1]
        Bv, V = logits.shape[0], logits.shape[-1]
        key = ("token_stats", Bv, K1, V, int(n), int(splits), str(logits.dtype), str(logits.device))
        t = self._ws.get(key)
        if t is None:
            t = self._ws[key] = self.K.TokenStats(Bv, K1, V, logits.dtype, int(n), int(splits), logits.device)
        return t(logits, tok, n_acc, drawn, inv_temperature if rows is None else rows.inv_t)

    @traced("commit_top_logprobs")
    def commit_top_logprobs(self, top_id, top_lp, seq_len, n_commit, out_id, out_lp, max_len):
        """The step's top-N rows follow its commit (asd_commit_top_logprobs); runs behind commit_step_lp / commit_step_stop and
        reads the seq_len / n_commit they left."""
        self.K.commit_top_logprobs(top_id, top_lp, seq_len, n_commit, out_id, out_lp, max_len=max_len)

    @traced("step_uniforms")
    def step_uniforms(self, seeds, step, stage, K_draft, K_accept, commit: bool = True, out=None):
        """Every uniform of a seeded decoding step in ONE launch (asd_step_uniforms; Philox4x32-10 keyed by seeds[b] i64 [B],
        counter (step, k, stage, 0)) -> (r_draft f32 [K_draft, B] | None, u f32 [B, K_accept] | None, r_commit f32 [B] | None):
        r_draft[k] is the proposal uniform of slot k, u[:, k] the accept uniform of slot k.  An output whose K is 0 (and
        r_commit with commit=False) is None and not written.  The three are views of `out`, one f32 buffer of at least
        (K_draft + K_accept + 1) * B elements that a stage loop allocates once per generate call (None: a fresh one), so a
        step's uniforms are valid until the next call on the same buffer (stream order)."""
        Bv = seeds.shape[0]
        Kd, Ka = int(K_draft), int(K_accept)
        need = (Kd + Ka + 1) * Bv
        if out is None:
            out = torch.empty((need,), dtype=torch.float32, device=seeds.device)
        if out.dim() != 1 or out.numel() < need:
            raise ValueError(f"out must be a float32 vector of at least {need} elements")
        r_draft = out[:Kd * Bv].view(Kd, Bv) if Kd > 0 else None
        u = out[Kd * Bv:(Kd + Ka) * Bv].view(Bv, Ka) if Ka > 0 else None
        r_commit = out[(Kd + Ka) * Bv:need] if commit else None
        self.K.step_uniforms(seeds, step, stage, r_draft, u, r_commit)
        return r_draft, u, r_commit

    def pack_logit_edits(self, rows, device):
        """One list of (id, bias, until) per batch row -> the device arrays of logit_edit_rows (kernels.pack_logit_edits: checked
        on the host, uploaded once per generate call; equal lists are uploaded once, without row_first)."""
        return self.K.pack_logit_edits(rows, device)

    @traced("logit_edit_rows")
    def logit_edit_rows(self, logits, edits, seq_len, start, offset: int = 0):
        """The sparse in-place logit edit ahead of the samplers (asd_logit_edit_rows): logits [B, V] or [B, K1, V] (any strides
        with a unit last stride) -> the same tensor, edited: for every entry (id, bias, until) of row b at position j, with
        g = seq_len[b] - start + offset + j, element id is -inf while g < until and x + bias (one rounding) afterwards.  One
        launch, no workspace; a stage loop makes the call once per logits tensor and only when the call has an entry."""
        return self.K.logit_edit_rows(logits, edits, seq_len, start, offset)

    def pack_token_masks(self, rows, V, device):
        """One sorted tuple of allowed token ids (or None: no list) per batch row -> the device bitmasks of logit_mask_rows
        (kernels.pack_token_masks: built with numpy on the host, uploaded once per generate call; equal lists share one mask)."""
        return self.K.pack_token_masks(rows, V, device)

    @traced("logit_mask_rows")
    def logit_mask_rows(self, logits, masks):
        """The dense allow-list ahead of the samplers (asd_logit_mask_rows): logits [B, V] or [B, K1, V] (any strides with a
        unit last stride) -> the same tensor, masked: element v of every position of row b is -inf where bit v of the row's
        mask is clear; a row without a list is not touched.  One launch, a write stream, no workspace; a stage loop makes the
        call once per logits tensor, in front of logit_edit_rows, and only when some row of the call has a list."""
        return self.K.logit_mask_rows(logits, masks)

    def pack_penalties(self, rep, pres, freq, prompt_ids, V, device):
        """Every row's (repetition, presence, frequency) penalty and its unpadded prompt ids -> the device state of
        penalty_rows / penalty_commit (kernels.pack_penalties: the prompt's seen bits are built with numpy on the host and
        uploaded once per generate call; the counts start at zero)."""
        return self.K.pack_penalties(rep, pres, freq, prompt_ids, V, device)

    @traced("penalty_rows")
    def penalty_rows(self, logits, pen, step_tok=None, n_prev: int = 0):
        """The stateful penalties ahead of the samplers (asd_penalty_rows): logits [B, V] or [B, K1, V] (any strides with a
        unit last stride) -> the same tensor, penalised from the row's history: its prompt and committed tokens (the state) and
        the step's proposals step_tok[b, :n_prev + j] at position j.  One launch, no workspace; a stage loop makes the call once
        per logits tensor, behind logit_edit_rows, and only when some row of the call has a non-neutral penalty."""
        return self.K.penalty_rows(logits, pen, step_tok, n_prev)

    @traced("penalty_commit")
    def penalty_commit(self, tokens, seq_len, n_commit, pen, max_len):
        """The step's committed tokens enter the penalty state (asd_penalty_commit), behind the step's commit: a finished row
        (n_commit 0) keeps its state, and a rejected proposal was never in it."""
        self.K.penalty_commit(tokens, seq_len, n_commit, pen, max_len)

    def pack_fsm(self, fsm, ld_state: int, device):
        """The compiled automata of one generate call (serving/guided.py::compile_rows) -> the device tables and state columns
        of fsm_mask_rows / fsm_advance / fsm_commit (kernels.pack_fsm: state_bits is built on the host from the CSR tables; one
        upload per generate call).  ld_state: draft_len + 1 at a verifying stage, 1 at stage 0."""
        return self.K.pack_fsm(fsm, ld_state, device)

    @traced("fsm_mask_rows")
    def fsm_mask_rows(self, logits, fsm, first: int = 0):
        """The automaton's mask ahead of the samplers (asd_fsm_mask_rows): logits [B, V] or [B, K1, V] (any strides with a unit
        last stride) -> the same tensor, position j of row b at -inf outside what state pos_state[b, first + j] allows.  The
        write stream of logit_mask_rows with a mask index per (row, position); a stage loop makes the call once per logits
        tensor, directly behind logit_mask_rows, and only when some row of the call is guided."""
        return self.K.fsm_mask_rows(logits, fsm, first)

    @traced("fsm_advance")
    def fsm_advance(self, fsm, step_tok, k: int):
        """Behind proposal k of a step (asd_fsm_advance): pos_state[b, k + 1] = delta(pos_state[b, k], step_tok[b, k])."""
        self.K.fsm_advance(fsm, step_tok, k)

    @traced("fsm_commit")
    def fsm_commit(self, fsm, tokens, seq_len, n_commit, max_len):
        """Behind the step's commit (asd_fsm_commit): the state behind the committed tokens moves to column 0; a finished row
        (n_commit 0) keeps its state."""
        self.K.fsm_commit(fsm, tokens, seq_len, n_commit, max_len)

    def pack_bad_words(self, rows, device):
        """Every row's bad words (1..8 token ids each, at most 256 per row) -> the device tables of bad_words_rows
        (kernels.pack_bad_words: one upload per generate call; equal rows share one list)."""
        return self.K.pack_bad_words(rows, device)

    @traced("bad_words_rows")
    def bad_words_rows(self, logits, words, tokens, seq_len, start, max_len, step_tok=None, n_prev: int = 0):
        """Multi-token bans ahead of the samplers (asd_bad_words_rows): logits [B, V] or [B, K1, V] (any strides with a unit
        last stride) -> the same tensor, with the last id of every word of row b at -inf where the word's other ids end the
        row's history: its committed generated tokens tokens[b, start:seq_len[b]] and the step's proposals
        step_tok[b, :n_prev + j] at position j.  One launch, no workspace, no state; a stage loop makes the call once per logits
        tensor, behind logit_mask_rows and in front of logit_edit_rows, and only when some row of the call has a word."""
        return self.K.bad_words_rows(logits, words, tokens, seq_len, start, max_len, step_tok, n_prev)

    @traced("pack_no_repeat_ngram")
    def pack_no_repeat_ngram(self, ns, prompt_lens, P: int, device):
        """Every row's no_repeat_ngram_size (0: off) and its number of real prompt ids, which end at index P of the token
        buffer -> the device arguments of no_repeat_ngram_rows (kernels.pack_no_repeat_ngram: one upload per generate call)."""
        return self.K.pack_no_repeat_ngram(ns, prompt_lens, P, device)

    @traced("no_repeat_ngram_rows")
    def no_repeat_ngram_rows(self, logits, ngram, tokens, seq_len, max_len, step_tok=None, n_prev: int = 0):
        """HF generate's no_repeat_ngram_size ahead of the samplers (asd_no_repeat_ngram_rows): logits [B, V] or [B, K1, V] (any
        strides with a unit last stride) -> the same tensor, with every token at -inf that would repeat an n-gram of the row's
        history: its real prompt ids and committed tokens tokens[b, row_start[b]:seq_len[b]] and the step's proposals
        step_tok[b, :n_prev + j] at position j.  One launch, no workspace, no state; a stage loop makes the call once per logits
        tensor, behind bad_words_rows and in front of logit_edit_rows, and only when some row of the call has n > 0."""
        return self.K.no_repeat_ngram_rows(logits, ngram, tokens, seq_len, max_len, step_tok, n_prev)

    @traced("pack_entropy_cut")
    def pack_entropy_cut(self, inv_t, modes, values, device):
        """Every row's 1 / temperature, mode (0 off, 1 typical_p, 2 epsilon_cutoff, 3 eta_cutoff) and value -> the device table
        of entropy_cut_rows (kernels.pack_entropy_cut: one upload per generate call and side)."""
        return self.K.pack_entropy_cut(inv_t, modes, values, device)

    @traced("entropy_cut_rows")
    def entropy_cut_rows(self, logits, cut):
        """HF's typical_p / epsilon_cutoff / eta_cutoff ahead of the samplers (asd_entropy_cut_rows): logits [B, V] or
        [B, K1, V] (any strides with a unit last stride) -> the same tensor, with every token at -inf that the row's cut removes
        from softmax(x / T) of the row as it stands.  One launch, no workspace, no state; a stage loop makes the call once per
        logits tensor, behind penalty_rows and directly ahead of the draw, and only when some row of the call has a cut."""
        return self.K.entropy_cut_rows(logits, cut)

    @traced("commit_step")
    def commit_step(self, tok, n_acc, drawn, seq_len, tokens, n_commit, max_len):
        self.K.commit_step(tok, n_acc, drawn, seq_len, tokens, n_commit, max_len=max_len)

    @traced("commit_step_lp")
    def commit_step_lp(self, tok, lp_tok, n_acc, drawn, lp_drawn, seq_len, tokens, lps, n_commit, max_len):
        """commit_step with the log-probs scattered beside the tokens (asd_commit_step_lp); tok = lp_tok = None: K = 0."""
        self.K.commit_step_lp(tok, lp_tok, n_acc, drawn, lp_drawn, seq_len, tokens, lps, n_commit, max_len=max_len)

    @traced("commit_step_stop")
    def commit_step_stop(self, tok, lp_tok, n_acc, drawn, lp_drawn, seq_len, tokens, lps, n_commit, max_len, stop_ids, finished,
                         n_finished):
        """commit_step_lp that ends a row at a stop token (asd_commit_step_stop): stop_ids i32 [S], finished i32 [B] (0 / 1 stop /
        2 length), n_finished i32 [1] -- the counter the stage loop reads every few steps."""
        self.K.commit_step_stop(tok, lp_tok, n_acc, drawn, lp_drawn, seq_len, tokens, lps, finished, stop_ids=stop_ids,
                                n_finished=n_finished, n_commit=n_commit, max_len=max_len)

    @traced("commit_step_finish")
    def commit_step_finish(self, tok, lp_tok, n_acc, drawn, lp_drawn, seq_len, tokens, lps, n_commit, max_len, start, seq_tok, seq_n,
                           row_first, row_max_len, finished, n_finished, matched):
        """commit_step_stop with multi-token stop sequences, per-row lists and per-row limits (asd_commit_step_finish): seq_tok
        i32 [n, 8] / seq_n i32 [n] / row_first i32 [B+1] (kernels.pack_stop_sequences; None where a call has no sequences),
        row_max_len i32 [B] or None, start = the prompt length, matched i32 [B]: which of its sequences ended a row."""
        self.K.commit_step_finish(tok, lp_tok, n_acc, drawn, lp_drawn, seq_len, tokens, lps, finished, start, seq_tok=seq_tok,
                                  seq_n=seq_n, row_first=row_first, row_max_len=row_max_len, n_finished=n_finished,
                                  matched=matched, n_commit=n_commit, max_len=max_len)

    @traced("lambda_sweep")
    def lambda_sweep(self, p_hist, costs, lams):
        """N4: the DP rule for every (lambda, sequence) pair in one launch -> k_star [G, n] i32."""
        return self.K.lambda_sweep(p_hist, costs, lams)[0]


def _world(group) -> Tuple[int, int]:
    return dist.get_world_size(group), dist.get_rank(group)


def host_staged(group=None) -> bool:
    """True when the group's backend cannot move device tensors itself (gloo: the CPU tests, and the one-GPU
    rehearsal of the multi-rank paths); messages are then staged through host memory.  RCCL moves them directly."""
    return dist.get_backend(group) == "gloo"


def all_gather_any(parts_like: torch.Tensor, group=None):
    """all_gather of equally shaped tensors -> list in rank order; device tensors over gloo go through the host."""
    world = dist.get_world_size(group)
    if parts_like.is_cuda and host_staged(group):
        src = parts_like.cpu()
        parts = [torch.empty_like(src) for _ in range(world)]
        dist.all_gather(parts, src, group=group)
        return [p.to(parts_like.device) for p in parts]
    parts = [torch.empty_like(parts_like) for _ in range(world)]
    dist.all_gather(parts, parts_like.contiguous(), group=group)
    return parts


def all_to_all_rows(rows: torch.Tensor, counts, group=None) -> torch.Tensor:
    """rows [sum(counts), W]: rows [o_q, o_q + counts[q]) go to rank q; returns [world * counts[me], W] -- the pieces every rank
    held of MY rows, in rank order.  One all-to-all (RCCL: ncclSend / ncclRecv pairs in one group); over gloo through the host."""
    world, me = dist.get_world_size(group), dist.get_rank(group)
    counts = [int(c) for c in counts]
    staged = rows.is_cuda and host_staged(group)
    src = rows.contiguous().cpu() if staged else rows.contiguous()
    out = torch.empty((world * counts[me],) + tuple(src.shape[1:]), dtype=src.dtype, device=src.device)
    dist.all_to_all_single(out, src, output_split_sizes=[counts[me]] * world, input_split_sizes=counts, group=group)
    return out.to(rows.device) if staged else out


class VocabShardedVerifier:
    """Target lm_head split over the ranks of `group` along the vocabulary."""

    def __init__(self, vocab: int, ops=None, group=None, inv_temperature: float = 1.0):
        self.vocab = vocab
        self.inv_temperature = float(inv_temperature)
        self.ops = ops if ops is not None else HipOps()
        self.group = group
        self.world, self.rank = _world(group)
        self.v0, self.v1 = shard_bounds(vocab, self.world, self.rank)

    def verify(self, logits_shard: torch.Tensor, tok: torch.Tensor, lp_d: torch.Tensor, u: torch.Tensor):
        """logits_shard: [B,K,v1-v0] of THIS rank; tok: GLOBAL ids.  Returns (lp_t, accept, n_acc, bits),
        identical on every rank (fixed combine order)."""
        if logits_shard.shape[-1] != self.v1 - self.v0:
            raise ValueError(f"rank {self.rank} expects a shard of width {self.v1 - self.v0}")
        msg = self.ops.lse_partial(logits_shard, tok, self.v0, self.inv_temperature).contiguous()
        return self._finish(msg, lp_d, u)

    def verify_hidden(self, hidden: torch.Tensor, weight_shard: torch.Tensor, tok: torch.Tensor, lp_d: torch.Tensor,
                      u: torch.Tensor):
        """Tensor-parallel lm_head (N2): `weight_shard` [v1-v0, D] is THIS rank's rows of the lm_head matrix,
        `hidden` [B,K,D] is replicated.  Each rank reduces its shard to the (m2, s, g) message without forming
        logits (asd_lm_head_partial); the exchange and the result are those of `verify`."""
        if weight_shard.shape[0] != self.v1 - self.v0:
            raise ValueError(f"rank {self.rank} expects a weight shard of {self.v1 - self.v0} rows")
        msg = self.ops.lm_head_partial(hidden, weight_shard, tok, self.v0, self.inv_temperature).contiguous()
        return self._finish(msg, lp_d, u)

    def _finish(self, msg, lp_d, u):
        parts = all_gather_any(msg, self.group)                # the one exchange step: [B,K,3] per rank
        return self.ops.accept_from_partials(torch.stack(parts).contiguous(), lp_d, u, self.inv_temperature)


class BatchShardedVerifier:
    """Batch-parallel replicas: rank r owns sequences [b0, b1); no data-path collective."""

    def __init__(self, batch: int, ops=None, group=None):
        self.ops = ops if ops is not None else HipOps()
        self.group = group
        self.world, self.rank = _world(group)
        self.batch = batch
        self.b0, self.b1 = shard_bounds(batch, self.world, self.rank)

    def verify_local(self, logits, tok, lp_d, u, inv_temperature: float = 1.0):
        """Arguments are THIS rank's rows [b0:b1)."""
        return self.ops.verify_accept(logits, tok, lp_d, u, inv_temperature)

    def gather_n_acc(self, n_acc_local: torch.Tensor) -> torch.Tensor:
        """Optional [B] view of the accepted lengths on every rank (token accounting)."""
        sizes = [shard_bounds(self.batch, self.world, r) for r in range(self.world)]
        width = max(e - s for s, e in sizes)
        pad = torch.zeros(width, dtype=n_acc_local.dtype, device=n_acc_local.device)
        pad[: n_acc_local.numel()] = n_acc_local
        parts = [torch.empty_like(pad) for _ in range(self.world)]
        dist.all_gather(parts, pad, group=self.group)
        return torch.cat([p[: e - s] for p, (s, e) in zip(parts, sizes)])


class TierLink:
    """Point-to-point hand-off between the rank that drafts and the rank that holds the target."""

    def __init__(self, draft_rank: int, target_rank: int, group=None):
        self.draft_rank, self.target_rank, self.group = draft_rank, target_rank, group

    # draft side --------------------------------------------------------------------------
    def send_draft(self, tok: torch.Tensor, lp_d: torch.Tensor) -> None:
        """tok [B,K] i32 + lp_d [B,K] f32 as ONE message (bit-cast into an i32 [2,B,K] buffer)."""
        buf = torch.stack([tok.to(torch.int32), lp_d.to(torch.float32).view(torch.int32)]).contiguous()
        dist.send(buf, dst=self.target_rank, group=self.group)

    def recv_verdict(self, B: int, K: int, device) -> Tuple[torch.Tensor, torch.Tensor]:
        buf = torch.empty(B * K + B, dtype=torch.int32, device=device)
        dist.recv(buf, src=self.target_rank, group=self.group)
        return buf[: B * K].view(B, K).to(torch.uint8), buf[B * K:].clone()

    # target side -------------------------------------------------------------------------
    def recv_draft(self, B: int, K: int, device) -> Tuple[torch.Tensor, torch.Tensor]:
        buf = torch.empty((2, B, K), dtype=torch.int32, device=device)
        dist.recv(buf, src=self.draft_rank, group=self.group)
        return buf[0].contiguous(), buf[1].contiguous().view(torch.float32)

    def send_verdict(self, accept: torch.Tensor, n_acc: torch.Tensor) -> None:
        buf = torch.cat([accept.reshape(-1).to(torch.int32), n_acc.reshape(-1).to(torch.int32)]).contiguous()
        dist.send(buf, dst=self.draft_rank, group=self.group)

    # generic small messages (committed tokens; ONE draft-logits row per sequence after a rejection)
    def send_to_target(self, t: torch.Tensor) -> None:
        dist.send(t.contiguous(), dst=self.target_rank, group=self.group)

    def send_to_draft(self, t: torch.Tensor) -> None:
        dist.send(t.contiguous(), dst=self.draft_rank, group=self.group)

    def recv_from_draft(self, shape, dtype, device) -> torch.Tensor:
        buf = torch.empty(shape, dtype=dtype, device=device)
        dist.recv(buf, src=self.draft_rank, group=self.group)
        return buf

    def recv_from_target(self, shape, dtype, device) -> torch.Tensor:
        buf = torch.empty(shape, dtype=dtype, device=device)
        dist.recv(buf, src=self.target_rank, group=self.group)
        return buf
