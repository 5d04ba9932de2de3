"""Device-tensor front end of libasd_hip.so: torch CUDA tensors in, torch CUDA tensors out.

torch is plumbing here (device memory + the current HIP stream); every function below is one
call through the C ABI with raw device pointers.  Nothing synchronises; outputs are valid in
stream order.  All of them raise if the tensors are not on a GPU -- there is no CPU path.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

from . import _binding as B

_DTYPE_CODE = {torch.float32: B.DTYPE_F32, torch.bfloat16: B.DTYPE_BF16, torch.float16: B.DTYPE_F16}


def _lib():
    return B.load_library()


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


# test infrastructure: `with kernels.test_hooks() as lib:` routes THIS thread's calls through lib/libasd_hip_test.so (the
# -DASD_TEST_HOOKS build, which alone has the asd_debug_* switches; `lib` is its ctypes handle)
test_hooks = B.use_test_library


def _dev(t: torch.Tensor, name: str, dtype=None) -> int:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError(f"{name} must be a CUDA (HIP) tensor; this package has no CPU path")
    if dtype is not None and t.dtype != dtype:
        raise ValueError(f"{name} must be {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    return t.data_ptr()


def _opt(t: Optional[torch.Tensor], name: str, dtype=None) -> Optional[int]:
    return None if t is None else _dev(t, name, dtype)


def version() -> int:
    return _lib().asd_version()


def device_cu_count(device: int = 0) -> int:
    n = _lib().asd_device_cu_count(device)
    if n < 0:
        B.check("asd_device_cu_count", n)
    return n


# ------------------------------------------------------------------------------- verify + accept
class LostHandoffError(RuntimeError):
    """A kernel's bounded wait for a hand-off word of this workspace ran out (ASD_WS_LOST_HANDOFF): the rows / sequences that
    depended on it came back POISONED (NaN / reject / tok = -1), and the workspace has been re-initialised."""


class _StatusWorkspace:
    """What every hand-off workspace shares (include/asd_hip.h, asd_workspace_status): `buf`, whose first 32-bit word is the
    sticky status the kernels or into when a bounded poll gives up."""

    buf: torch.Tensor
    bytes: int

    def reset(self) -> None:
        B.check("asd_workspace_init", _lib().asd_workspace_init(self.buf.data_ptr(), self.bytes, _stream()))

    @property
    def status_word(self) -> torch.Tensor:
        """0-d int32 view of the status word: read it together with whatever the caller synchronises on anyway."""
        return self.buf[:4].view(torch.int32)[0]

    def status(self) -> int:
        """Synchronising read of the status word through the C ABI (asd_workspace_status)."""
        out = C.c_uint32(0)
        B.check("asd_workspace_status", _lib().asd_workspace_status(self.buf.data_ptr(), C.addressof(out), _stream()))
        return int(out.value)

    def check(self) -> None:
        """Raise LostHandoffError (after re-initialising the workspace) if a hand-off was lost since the last reset."""
        st = self.status()
        if st != 0:
            self.reset()
            raise LostHandoffError(f"{type(self).__name__}: status 0x{st:x} (a hand-off word never arrived; results poisoned, "
                                   "workspace re-initialised)")


class VerifyWorkspace(_StatusWorkspace):
    """Ticket + granule scratch of asd_verify_accept, zeroed once (asd_workspace_init).

    One workspace serves any number of stream-ordered calls with B' <= B, K' <= K; calls that may
    overlap on different streams need one workspace each."""

    def __init__(self, B_: int, K: int, V: int, dtype: torch.dtype = torch.bfloat16,
                 device: Optional[torch.device] = None):
        self.B, self.K, self.V = B_, K, V
        self.dtype = dtype
        self.bytes = int(_lib().asd_verify_accept_workspace_bytes(B_, K, V, _DTYPE_CODE[dtype]))
        self.buf = torch.empty(self.bytes, dtype=torch.uint8, device=device or torch.device("cuda"))
        self.reset()

    def fits(self, B_: int, K: int) -> bool:
        need = int(_lib().asd_verify_accept_workspace_bytes(B_, K, self.V, _DTYPE_CODE[self.dtype]))
        return need <= self.bytes


@dataclass
class VerifyResult:
    lp_target: torch.Tensor   # [B,K] f32   log p_target(tok)
    accept: torch.Tensor      # [B,K] u8
    n_acc: torch.Tensor       # [B]   i32   accepted-prefix length
    accept_bits: torch.Tensor  # [B]  i64 (bit k = accept[b,k])


@dataclass
class NucleusVerifyResult(VerifyResult):
    t_nucleus_logit: torch.Tensor = None   # [B,K] f32  x* of each target row (raw score units; -inf: no truncation)
    n_finite: torch.Tensor = None          # [B]   i32  leading positions with a finite lp_target (the stop rule's n_valid)


def _verify_out(Bv: int, K: int, dev, cls=VerifyResult):
    """Fresh outputs of a verify call: the four tensors of VerifyResult, the six of NucleusVerifyResult."""
    t = [torch.empty((Bv, K), dtype=torch.float32, device=dev), torch.empty((Bv, K), dtype=torch.uint8, device=dev),
         torch.empty((Bv,), dtype=torch.int32, device=dev), torch.empty((Bv,), dtype=torch.int64, device=dev)]
    if cls is NucleusVerifyResult:
        t += [torch.empty((Bv, K), dtype=torch.float32, device=dev), torch.empty((Bv,), dtype=torch.int32, device=dev)]
    return cls(*t)


def _logits_2d(logits: torch.Tensor, Bv: int, K: int) -> Tuple[int, int, int]:
    if logits.dtype not in _DTYPE_CODE:
        raise ValueError(f"logits dtype {logits.dtype} unsupported (f32 / bf16 / f16)")
    if not logits.is_cuda:
        raise ValueError("logits must be a CUDA (HIP) tensor; this package has no CPU path")
    if logits.dim() == 3:
        if logits.shape[0] != Bv or logits.shape[1] != K:
            raise ValueError("logits must be [B,K,V]")
        # the stride of a size-1 dimension is arbitrary (a [1, 64, V] slice of [1, 70, V] keeps stride(0) = 70 V)
        if logits.stride(2) != 1 or (Bv > 1 and logits.stride(0) != K * logits.stride(1)):
            raise ValueError("logits rows must be unit-stride in V and evenly spaced over (b,k)")
        ld = logits.stride(1) if K > 1 else (logits.stride(0) if Bv > 1 else logits.shape[2])
        return logits.shape[2], ld, logits.data_ptr()
    if logits.dim() == 2:
        if logits.shape[0] != Bv * K or logits.stride(1) != 1:
            raise ValueError("2-D logits must be [B*K, V] with unit stride in V")
        return logits.shape[1], logits.stride(0), logits.data_ptr()
    raise ValueError("logits must be [B,K,V] or [B*K,V]")


def _verify_args(logits, tok, lp_draft, u, out, cls=VerifyResult):
    """What every verify call starts with: (out -- fresh unless given --, the nine leading arguments logits .. V of the C entry
    points, the four output pointers lp_target .. accept_bits)."""
    Bv, K = tok.shape
    V, ld, ptr = _logits_2d(logits, Bv, K)
    if out is None:
        out = _verify_out(Bv, K, logits.device, cls)
    lead = (ptr, _DTYPE_CODE[logits.dtype], ld, _dev(tok, "tok", torch.int32), _dev(lp_draft, "lp_draft", torch.float32),
            _dev(u, "u", torch.float32), Bv, K, V)
    outs = (_dev(out.lp_target, "lp_target", torch.float32), _dev(out.accept, "accept", torch.uint8),
            _dev(out.n_acc, "n_acc", torch.int32), _dev(out.accept_bits, "accept_bits", torch.int64))
    return out, lead, outs


def verify_accept(logits: torch.Tensor, tok: torch.Tensor, lp_draft: torch.Tensor, u: torch.Tensor,
                  workspace: VerifyWorkspace, out: Optional[VerifyResult] = None, *, inv_temperature: float = 1.0,
                  splits: int = 0, threads: int = 0, unroll: int = 0, nontemporal: int = -1) -> VerifyResult:
    """A5/A6 in one launch (include/asd_hip.h: asd_verify_accept_ex).  tok/lp_draft/u: [B,K].
    inv_temperature scales the logits inside the kernel (the test runs on softmax(logits / T))."""
    out, lead, outs = _verify_args(logits, tok, lp_draft, u, out)
    opt = B.verify_options(inv_temperature, splits, threads, unroll, nontemporal)
    rc = _lib().asd_verify_accept_ex(*lead, *outs, workspace.buf.data_ptr(), workspace.bytes, C.addressof(opt), _stream())
    B.check("asd_verify_accept_ex", rc)
    return out


def _verify_truncated(entry: str, logits, tok, lp_draft, u, workspace, inv_temperature, truncation: tuple, out):
    """The body of verify_accept_top_p / verify_accept_top_k: `entry` is the C entry point, `truncation` its arguments between
    inv_temperature and the outputs."""
    out, lead, outs = _verify_args(logits, tok, lp_draft, u, out, NucleusVerifyResult)
    ws_ptr, ws_bytes = (None, 0) if workspace is None else (workspace.buf.data_ptr(), workspace.bytes)
    rc = getattr(_lib(), entry)(
        *lead, float(inv_temperature), *truncation, *outs,
        _dev(out.t_nucleus_logit, "t_nucleus_logit", torch.float32), _dev(out.n_finite, "n_finite", torch.int32),
        ws_ptr, ws_bytes, _stream())
    B.check(entry, rc)
    return out


def verify_accept_top_p(logits: torch.Tensor, tok: torch.Tensor, lp_draft: torch.Tensor, u: torch.Tensor,
                        workspace: Optional[VerifyWorkspace], *, inv_temperature: float = 1.0, top_p: float = 1.0,
                        out: Optional[NucleusVerifyResult] = None) -> NucleusVerifyResult:
    """The verify step against the TARGET's nucleus (include/asd_hip.h: asd_verify_accept_top_p): lp_target = log p^N(tok)
    under softmax(logits / T) restricted to the top-p set of asd_draft_sample's select, -inf outside it.  top_p outside (0, 1)
    is asd_verify_accept_ex (the same bits; needs `workspace`); otherwise no workspace is used."""
    return _verify_truncated("asd_verify_accept_top_p", logits, tok, lp_draft, u, workspace, inv_temperature, (float(top_p),), out)


def verify_accept_top_k(logits: torch.Tensor, tok: torch.Tensor, lp_draft: torch.Tensor, u: torch.Tensor,
                        workspace: Optional[VerifyWorkspace], *, inv_temperature: float = 1.0, top_k: int = 0,
                        top_p: float = 1.0, out: Optional[NucleusVerifyResult] = None) -> NucleusVerifyResult:
    """The verify step against the target's Temperature -> TopK -> TopP set (include/asd_hip.h: asd_verify_accept_top_k):
    lp_target = log q(tok) over { x >= thr }, thr = max(x_k, x*_K) (t_nucleus_logit), -inf outside it.  HF
    generate(do_sample=True, ...) applies top_k = 50 unless told otherwise.  top_k <= 0 or >= V is verify_accept_top_p (the
    same bits; `workspace` only matters when top_p is off too)."""
    return _verify_truncated("asd_verify_accept_top_k", logits, tok, lp_draft, u, workspace, inv_temperature,
                             (int(top_k), float(top_p)), out)


def verify_accept_min_p(logits: torch.Tensor, tok: torch.Tensor, lp_draft: torch.Tensor, u: torch.Tensor,
                        workspace: Optional[VerifyWorkspace], *, inv_temperature: float = 1.0, top_k: int = 0,
                        top_p: float = 1.0, min_p: float = 0.0,
                        out: Optional[NucleusVerifyResult] = None) -> NucleusVerifyResult:
    """The verify step against the target's Temperature -> TopK -> TopP -> MinP set (include/asd_hip.h:
    asd_verify_accept_min_p): thr = max(thr_kp, x_max + T ln(min_p)) (t_nucleus_logit).  min_p <= 0 is verify_accept_top_k (the
    same bits); min_p > 1 or NaN is an argument error."""
    return _verify_truncated("asd_verify_accept_min_p", logits, tok, lp_draft, u, workspace, inv_temperature,
                             (int(top_k), float(top_p), float(min_p)), out)


# ------------------------------------------------------------------------------- per-sequence sampling parameters
class SamplingRows:
    """The packed per-sequence sampling table of the *_rows entry points (include/asd_hip.h: asd_sampling_rows_pack) on the
    device: one row of 32 bytes per sequence with what a scalar launch with that sequence's (inv_temperature, top_k, top_p,
    min_p) would use.  Packed on the host by the library, uploaded once; `inv_t` is the f32 [B] device copy of the
    temperatures (asd_top_logprobs_rows).  The table depends on V and the logits dtype (top_k >= V is off; the select's radix
    levels).  top_k / top_p / min_p: None = off for every sequence, else one value per sequence."""

    def __init__(self, inv_temperature, top_k=None, top_p=None, min_p=None, *, V: int, dtype: torch.dtype = torch.bfloat16,
                 device: Optional[torch.device] = None):
        if dtype not in _DTYPE_CODE:
            raise ValueError(f"logits dtype {dtype} unsupported (f32 / bf16 / f16)")
        inv = np.ascontiguousarray(inv_temperature, dtype=np.float32).reshape(-1)
        n = inv.shape[0]

        def arr(v, dt, name):
            if v is None:
                return None
            a = np.ascontiguousarray(v, dtype=dt).reshape(-1)
            if a.shape[0] != n:
                raise ValueError(f"{name} must hold one value per sequence ({n})")
            return a
        tk, tp, mp = arr(top_k, np.int32, "top_k"), arr(top_p, np.float32, "top_p"), arr(min_p, np.float32, "min_p")
        self.B, self.V, self.dtype = n, int(V), dtype
        self.host = np.zeros(int(_lib().asd_sampling_rows_bytes(n)), np.uint8)
        vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        B.check("asd_sampling_rows_pack", _lib().asd_sampling_rows_pack(vp(inv), vp(tk), vp(tp), vp(mp), n, int(V),
                                                                        _DTYPE_CODE[dtype], vp(self.host)))
        dev = device or torch.device("cuda")
        self.buf = torch.from_numpy(self.host).to(dev)
        self.inv_t = torch.from_numpy(inv).to(dev)

    def ptr(self, Bv: int, V: int, dtype) -> int:
        """The device table for a call on Bv sequences of [.., V] `dtype` logits."""
        if Bv != self.B or V != self.V or dtype != self.dtype:
            raise ValueError(f"the sampling table was packed for B={self.B}, V={self.V}, {self.dtype}")
        return self.buf.data_ptr()


def verify_accept_rows(logits: torch.Tensor, tok: torch.Tensor, lp_draft: torch.Tensor, u: torch.Tensor, rows: SamplingRows,
                       out: Optional[NucleusVerifyResult] = None) -> NucleusVerifyResult:
    """The verify step with every sequence's own temperature / top-k / top-p / min-p (include/asd_hip.h:
    asd_verify_accept_rows): sequence b returns the bits verify_accept_min_p returns for it with its values; a sequence that
    truncates nothing is scored by the same select (t_nucleus_logit = -inf).  No workspace."""
    out, lead, outs = _verify_args(logits, tok, lp_draft, u, out, NucleusVerifyResult)
    rc = _lib().asd_verify_accept_rows(*lead, rows.ptr(lead[6], lead[8], logits.dtype), *outs,
                                       _dev(out.t_nucleus_logit, "t_nucleus_logit", torch.float32),
                                       _dev(out.n_finite, "n_finite", torch.int32), None, 0, _stream())
    B.check("asd_verify_accept_rows", rc)
    return out


def verify_accept_stats(logits: torch.Tensor, tok: torch.Tensor, lp_draft: torch.Tensor, u: torch.Tensor,
                        workspace: VerifyWorkspace, out: Optional[VerifyResult] = None, *, inv_temperature: float = 1.0,
                        want_entropy: bool = True) -> Tuple[VerifyResult, torch.Tensor, Optional[torch.Tensor]]:
    """asd_verify_accept_stats: the verify pass + per position max log-prob [B,K] and (optionally) the entropy of the
    target softmax [B,K] -- the device-side inputs of the doc-only FeatureExtractor (RESEARCH_PROTOCOL.md:378-400)."""
    out, lead, outs = _verify_args(logits, tok, lp_draft, u, out)
    max_lp = torch.empty(tuple(tok.shape), dtype=torch.float32, device=logits.device)
    ent = torch.empty_like(max_lp) if want_entropy else None
    rc = _lib().asd_verify_accept_stats(
        *lead, *outs, max_lp.data_ptr(), None if ent is None else ent.data_ptr(), workspace.buf.data_ptr(),
        workspace.bytes, float(inv_temperature), _stream())
    B.check("asd_verify_accept_stats", rc)
    return out, max_lp, ent


def lse_partial(logits_shard: torch.Tensor, tok: torch.Tensor, v_offset: int, workspace: VerifyWorkspace,
                out: Optional[torch.Tensor] = None, inv_temperature: float = 1.0) -> torch.Tensor:
    """Per-shard (m2, s, g) triples, [B,K,3] f32, with sum_v exp(x) = s * 2^m2 (log2 domain)."""
    Bv, K = tok.shape
    V, ld, ptr = _logits_2d(logits_shard, Bv, K)
    if out is None:
        out = torch.empty((Bv, K, 3), dtype=torch.float32, device=logits_shard.device)
    rc = _lib().asd_lse_partial(ptr, _DTYPE_CODE[logits_shard.dtype], ld, _dev(tok, "tok", torch.int32), Bv, K, V,
                                int(v_offset), float(inv_temperature), _dev(out, "msg", torch.float32),
                                workspace.buf.data_ptr(), workspace.bytes, _stream())
    B.check("asd_lse_partial", rc)
    return out


def accept_from_partials(msg_all: torch.Tensor, lp_draft: torch.Tensor, u: torch.Tensor,
                         out: Optional[VerifyResult] = None, inv_temperature: float = 1.0) -> VerifyResult:
    """msg_all: [n_shards,B,K,3] (all-gathered asd_lse_partial outputs, shard order fixed)."""
    n_shards, Bv, K, three = msg_all.shape
    assert three == 3
    dev = msg_all.device
    if out is None:
        out = _verify_out(Bv, K, dev)
    rc = _lib().asd_accept_from_partials(_dev(msg_all, "msg_all", torch.float32), n_shards,
                                         _dev(lp_draft, "lp_draft", torch.float32), _dev(u, "u", torch.float32), Bv, K,
                                         float(inv_temperature), out.lp_target.data_ptr(), out.accept.data_ptr(), out.n_acc.data_ptr(),
                                         out.accept_bits.data_ptr(), _stream())
    B.check("asd_accept_from_partials", rc)
    return out


class LmHeadVerifier:
    """N2: lm_head projection fused with the verify pass (asd_lm_head_verify).  Holds the partials
    workspace for one (B, K, V); `weight` is the [V, D] bf16 or f16 lm_head matrix (nn.Linear layout); the hidden
    states must have the same element type."""

    def __init__(self, weight: torch.Tensor, B_: int, K: int, packed: bool = False, packed_image: Optional[torch.Tensor] = None):
        """Sized for batches of up to B_ sequences of exactly K positions (calls with fewer sequences reuse the workspace).
        packed=True: keep a tile-major copy of the matrix (asd_lm_head_pack_weights; +V*D*2 bytes, e.g. +2.5 GB for the
        152064 x 8192 head) and stream that: every 64-deep reduction step of a column block is one contiguous 32 KiB run.
        packed_image: an image another verifier of the SAME matrix already built (shared, read-only).
        Results are bit-identical either way.  The image is a snapshot: repack after changing the weights."""
        if weight.dim() != 2 or weight.dtype not in (torch.bfloat16, torch.float16) or not weight.is_cuda:
            raise ValueError("weight must be a [V, D] bf16 or f16 CUDA tensor")
        self._dt = _DTYPE_CODE[weight.dtype]
        if weight.stride(1) != 1:
            raise ValueError("weight rows must be contiguous")
        self.weight = weight
        self.B, self.K = int(B_), int(K)
        self.V, self.D = weight.shape
        self._w_ptr, self._ld_w = weight.data_ptr(), weight.stride(0)
        self.packed = None
        if packed_image is not None:
            self.packed = packed_image
            self._w_ptr, self._ld_w = packed_image.data_ptr(), 0
        elif packed:
            nbytes = int(_lib().asd_lm_head_packed_bytes(self.V, self.D))
            if nbytes == 0:
                raise ValueError("D must be a multiple of 64 to pack the lm_head")
            self.packed = torch.empty(nbytes, dtype=torch.uint8, device=weight.device)
            B.check("asd_lm_head_pack_weights", _lib().asd_lm_head_pack_weights(
                weight.data_ptr(), weight.stride(0), self._dt, self.V, self.D, self.packed.data_ptr(), nbytes, _stream()))
            self._w_ptr, self._ld_w = self.packed.data_ptr(), 0
        n = int(_lib().asd_lm_head_verify_workspace_bytes(self.B, self.K, self.V))
        self.workspace = torch.empty(max(n, 256), dtype=torch.uint8, device=weight.device)

    def _hidden_2d(self, hidden: torch.Tensor, Bv: int, K: int) -> Tuple[torch.Tensor, int]:
        """(hidden as [B*K, D], its row stride as the C entry points take it)"""
        h2 = hidden.reshape(Bv * K, hidden.shape[-1]) if hidden.dim() == 3 else hidden
        if h2.dtype != self.weight.dtype or h2.shape != (Bv * K, self.D) or h2.stride(1) != 1:
            raise ValueError("hidden must be [B*K, D] of the weight's element type with contiguous rows")
        return h2, (h2.stride(0) if Bv * K > 1 else self.D)

    def __call__(self, hidden: torch.Tensor, tok: torch.Tensor, lp_draft: Optional[torch.Tensor] = None,
                 u: Optional[torch.Tensor] = None, out: Optional[VerifyResult] = None, inv_temperature: float = 1.0,
                 greedy: bool = False, argmax_out: Optional[torch.Tensor] = None) -> VerifyResult:
        """hidden [B, K, D] (or [B*K, D]) bf16: the final-norm output the lm_head would consume.
        greedy=True: accept[b,k] = (tok[b,k] == argmax logits[b,k]) (lp_draft / u unused);
        argmax_out: optional [B, K] int32 tensor that receives the row arg-max either way."""
        Bv, K = tok.shape
        if Bv > self.B or K != self.K:
            raise ValueError(f"verifier was sized for B<={self.B}, K={self.K}, got {Bv}, {K}")
        if not greedy and (lp_draft is None or u is None):
            raise ValueError("lp_draft and u are required unless greedy=True")
        h2, ld_h = self._hidden_2d(hidden, Bv, K)
        if out is None:
            out = _verify_out(Bv, K, h2.device)
        rc = _lib().asd_lm_head_verify_ex(h2.data_ptr(), ld_h, self._w_ptr,
                                          self._ld_w, self._dt, self.D, _dev(tok, "tok", torch.int32),
                                          _opt(lp_draft, "lp_draft", torch.float32), _opt(u, "u", torch.float32), Bv, K,
                                          self.V, float(inv_temperature), 1 if greedy else 0, out.lp_target.data_ptr(),
                                          out.accept.data_ptr(), out.n_acc.data_ptr(), out.accept_bits.data_ptr(),
                                          _opt(argmax_out, "argmax_out", torch.int32), self.workspace.data_ptr(),
                                          self.workspace.numel(), _stream())
        B.check("asd_lm_head_verify_ex", rc)
        return out


    def partial(self, hidden: torch.Tensor, tok: torch.Tensor, v_offset: int, inv_temperature: float = 1.0,
                msg: Optional[torch.Tensor] = None) -> torch.Tensor:
        """`self.weight` is this rank's vocabulary shard starting at global id `v_offset`: returns the
        [B, K, 3] (m2, s, g) message of asd_lse_partial without forming the shard's logits (asd_lm_head_partial)."""
        Bv, K = tok.shape
        if Bv > self.B or K != self.K:
            raise ValueError(f"verifier was sized for B<={self.B}, K={self.K}, got {Bv}, {K}")
        h2, ld_h = self._hidden_2d(hidden, Bv, K)
        if msg is None:
            msg = torch.empty((Bv, K, 3), dtype=torch.float32, device=h2.device)
        rc = _lib().asd_lm_head_partial(h2.data_ptr(), ld_h, self._w_ptr,
                                        self._ld_w, self._dt, self.D, _dev(tok, "tok", torch.int32), Bv, K,
                                        self.V, int(v_offset), float(inv_temperature), _dev(msg, "msg", torch.float32),
                                        self.workspace.data_ptr(), self.workspace.numel(), _stream())
        B.check("asd_lm_head_partial", rc)
        return msg


class LinearWorkspace:
    """Slab buffer of asd_linear's reduction slices; grows to the largest (M, N, D) it has served.  One per stream:
    consecutive calls on a stream may share it."""

    def __init__(self, device, on_grow=None):
        """on_grow: called BEFORE the buffer is replaced by a larger one -- whoever captured hipGraphs that hold the old
        buffer's address (SyntheticLM.enable_graphs) must drop them."""
        self.device = torch.device(device)
        self.buf: Optional[torch.Tensor] = None
        self.on_grow = on_grow

    def ensure(self, M: int, N: int, D: int) -> Tuple[int, int]:
        need = int(_lib().asd_linear_workspace_bytes(M, N, D))
        if self.buf is None or self.buf.numel() < need:
            if self.buf is not None and self.on_grow is not None:
                self.on_grow()
            self.buf = torch.empty(max(need, 1 << 20), dtype=torch.uint8, device=self.device)
        return self.buf.data_ptr(), self.buf.numel()


def linear(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, *, workspace: LinearWorkspace,
           out: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None) -> torch.Tensor:
    """X3: y = x @ weight.T (+ bias) (+ residual) through asd_linear_ex.  x [..., D], weight [N, D] (nn.Linear layout), all bf16
    or all f16 CUDA tensors; returns [..., N] of the same type.  residual [M, N] may be `out` itself (in-place accumulate)."""
    if weight.dim() != 2 or weight.dtype not in (torch.bfloat16, torch.float16) or not weight.is_cuda or weight.stride(1) != 1:
        raise ValueError("weight must be a [N, D] bf16 or f16 CUDA tensor with contiguous rows")
    if x.dtype != weight.dtype or not x.is_cuda or x.shape[-1] != weight.shape[1]:
        raise ValueError("x must be a CUDA tensor of the weight's element type with D trailing elements")
    N, D = weight.shape
    x2 = x.reshape(-1, D)
    if x2.stride(1) != 1:
        x2 = x2.contiguous()
    M = x2.shape[0]
    if out is None:
        out = torch.empty((M, N), dtype=x.dtype, device=x.device)
    elif out.shape != (M, N) or out.dtype != x.dtype or out.stride(1) != 1:
        raise ValueError("out must be a [M, N] tensor of the operands' type with contiguous rows")
    if bias is not None and (bias.dtype != x.dtype or bias.numel() != N or not bias.is_contiguous()):
        raise ValueError("bias must be a contiguous [N] tensor of the operands' type")
    if residual is not None and (residual.shape != (M, N) or residual.dtype != x.dtype or residual.stride(1) != 1):
        raise ValueError("residual must be a [M, N] tensor of the operands' type with contiguous rows")
    ws_ptr, ws_bytes = workspace.ensure(M, N, D)
    rc = _lib().asd_linear_ex(x2.data_ptr(), x2.stride(0), weight.data_ptr(), weight.stride(0),
                              None if bias is None else bias.data_ptr(), None if residual is None else residual.data_ptr(),
                              0 if residual is None else residual.stride(0), _DTYPE_CODE[x.dtype], M, N, D, out.data_ptr(),
                              out.stride(0), ws_ptr, ws_bytes, _stream())
    B.check("asd_linear_ex", rc)
    return out.view(*x.shape[:-1], N)


def _commit_front(tok, n_acc, drawn, seq_len, out_tokens, n_commit, max_len, lp=None, ends=None):
    """What the four commit_step* wrappers share: the shape checks, then the device pointers in the order of the C argument
    lists -> (Bv, K, cap, head, tail).  `head` stands in front of B, K and the entry point's own arguments, `tail` behind them.
    lp = (lp_tok, lp_drawn, out_lp) where the entry point commits log-probs, ends = (finished, n_finished) where it ends rows."""
    if lp is None:
        Bv, K = tok.shape
    else:
        lp_tok, lp_drawn, out_lp = lp
        Bv = drawn.shape[0]
        K = 0 if tok is None else tok.shape[1]
        if tok is not None and (tok.shape[0] != Bv or lp_tok is None or lp_tok.shape != tok.shape):
            raise ValueError("tok and lp_tok must both be [B, K]")
    if out_tokens.dim() != 2 or out_tokens.shape[0] != Bv or out_tokens.stride(1) != 1:
        raise ValueError("out_tokens must be [B, T] int32 with contiguous rows")
    if lp is not None and (out_lp.shape != out_tokens.shape or out_lp.stride() != out_tokens.stride()):
        raise ValueError("out_lp must have the shape and strides of out_tokens")
    if ends is not None:
        finished, n_finished = ends
        if finished.shape != (Bv,):
            raise ValueError("finished must be [B] int32")
        if n_finished is not None and n_finished.numel() != 1:
            raise ValueError("n_finished must hold one int32")
    cap = out_tokens.shape[1] if max_len is None else int(max_len)
    i32, f32 = torch.int32, torch.float32
    if lp is None:
        head = (_dev(tok, "tok", i32), _dev(n_acc, "n_acc", i32), _dev(drawn, "drawn", i32))
        tail = (_dev(seq_len, "seq_len", i32), _dev(out_tokens, "out_tokens", i32))
    else:
        head = (_opt(tok, "tok", i32), _opt(lp_tok, "lp_tok", f32), _dev(n_acc, "n_acc", i32), _dev(drawn, "drawn", i32),
                _dev(lp_drawn, "lp_drawn", f32))
        tail = (_dev(seq_len, "seq_len", i32), _dev(out_tokens, "out_tokens", i32), _dev(out_lp, "out_lp", f32))
    tail += (out_tokens.stride(0), _opt(n_commit, "n_commit", i32))
    if ends is not None:
        tail += (_dev(finished, "finished", i32), _opt(n_finished, "n_finished", i32))
    return Bv, K, cap, head, tail


def commit_step(tok: torch.Tensor, n_acc: torch.Tensor, drawn: torch.Tensor, seq_len: torch.Tensor,
                out_tokens: torch.Tensor, n_commit: Optional[torch.Tensor] = None, max_len: Optional[int] = None) -> None:
    """N3: append every sequence's accepted prefix + drawn token to its row of `out_tokens` and advance
    `seq_len` in place (asd_commit_step).  tok [B,K] i32, n_acc / drawn / seq_len [B] i32, out_tokens [B, T] i32."""
    Bv, K, cap, head, tail = _commit_front(tok, n_acc, drawn, seq_len, out_tokens, n_commit, max_len)
    B.check("asd_commit_step", _lib().asd_commit_step(*head, Bv, K, *tail, cap, _stream()))


def commit_step_lp(tok: Optional[torch.Tensor], lp_tok: Optional[torch.Tensor], n_acc: torch.Tensor, drawn: torch.Tensor,
                   lp_drawn: torch.Tensor, seq_len: torch.Tensor, out_tokens: torch.Tensor, out_lp: torch.Tensor,
                   n_commit: Optional[torch.Tensor] = None, max_len: Optional[int] = None) -> None:
    """commit_step that also appends the committed tokens' log-probs to `out_lp` (asd_commit_step_lp): lp_tok [B,K] f32 beside
    tok, lp_drawn [B] f32 beside drawn, out_lp [B, T] f32 with the row stride of out_tokens.  tok = lp_tok = None is K = 0:
    every sequence appends its drawn token (plain sampled decoding)."""
    Bv, K, cap, head, tail = _commit_front(tok, n_acc, drawn, seq_len, out_tokens, n_commit, max_len, lp=(lp_tok, lp_drawn, out_lp))
    B.check("asd_commit_step_lp", _lib().asd_commit_step_lp(*head, Bv, K, *tail, cap, _stream()))


def commit_step_stop(tok: Optional[torch.Tensor], lp_tok: Optional[torch.Tensor], n_acc: torch.Tensor, drawn: torch.Tensor,
                     lp_drawn: torch.Tensor, seq_len: torch.Tensor, out_tokens: torch.Tensor, out_lp: torch.Tensor,
                     finished: torch.Tensor, stop_ids: Optional[torch.Tensor] = None, n_finished: Optional[torch.Tensor] = None,
                     n_commit: Optional[torch.Tensor] = None, max_len: Optional[int] = None) -> None:
    """commit_step_lp that ends a sequence at a stop token (asd_commit_step_stop): the append is cut behind the first committed
    token that is in `stop_ids` (device int32 [S], S <= 8; None: no stop set) and that token is kept.  finished [B] i32 in/out:
    0 running, 1 stopped, 2 reached max_len; a row that enters non-zero is left alone (n_commit 0).  n_finished [1] i32 in/out:
    rows that finished so far -- the one value a host loop reads."""
    Bv, K, cap, head, tail = _commit_front(tok, n_acc, drawn, seq_len, out_tokens, n_commit, max_len, lp=(lp_tok, lp_drawn, out_lp),
                                           ends=(finished, n_finished))
    if stop_ids is not None and stop_ids.dim() != 1:
        raise ValueError("stop_ids must be [S] int32")
    n_stop = 0 if stop_ids is None else stop_ids.shape[0]
    rc = _lib().asd_commit_step_stop(*head, Bv, K, _opt(stop_ids, "stop_ids", torch.int32) if n_stop else None, n_stop, *tail,
                                     cap, _stream())
    B.check("asd_commit_step_stop", rc)


def pack_stop_sequences(rows, device, shared: bool = False):
    """The stop-sequence tables of commit_step_finish from host lists, checked BEFORE anything is uploaded.
    shared=False: `rows` holds one list of sequences per batch row (each sequence 1..8 token ids, at most 16 per row, a row's
    list may be empty) -> (seq_tok i32 [n, 8], seq_n i32 [n], row_first i32 [B+1]) on `device`.  shared=True: `rows` is ONE such
    list, owned by every row -> (seq_tok, seq_n, None)."""
    lists = [list(rows)] if shared else [list(r) for r in rows]
    flat, first = [], [0]
    for r, seqs in enumerate(lists):
        if len(seqs) > B.MAX_STOP_SEQS:
            raise ValueError(f"row {r} owns {len(seqs)} stop sequences, at most {B.MAX_STOP_SEQS}")
        for s in seqs:
            s = [int(t) for t in s]
            if not 1 <= len(s) <= B.MAX_STOP_SEQ_LEN:
                raise ValueError(f"a stop sequence holds 1..{B.MAX_STOP_SEQ_LEN} token ids, got {len(s)}")
            if any(not -2 ** 31 <= t < 2 ** 31 for t in s):
                raise ValueError("stop sequence token ids must fit int32")
            flat.append(s)
        first.append(len(flat))
    tok = torch.zeros((len(flat), B.MAX_STOP_SEQ_LEN), dtype=torch.int32)
    for i, s in enumerate(flat):
        tok[i, :len(s)] = torch.tensor(s, dtype=torch.int32)
    n = torch.tensor([len(s) for s in flat], dtype=torch.int32)
    return tok.to(device), n.to(device), None if shared else torch.tensor(first, dtype=torch.int32).to(device)


def commit_step_finish(tok: Optional[torch.Tensor], lp_tok: Optional[torch.Tensor], n_acc: torch.Tensor, drawn: torch.Tensor,
                       lp_drawn: torch.Tensor, seq_len: torch.Tensor, out_tokens: torch.Tensor, out_lp: torch.Tensor,
                       finished: torch.Tensor, start: int, seq_tok: Optional[torch.Tensor] = None,
                       seq_n: Optional[torch.Tensor] = None, row_first: Optional[torch.Tensor] = None,
                       row_max_len: Optional[torch.Tensor] = None, n_finished: Optional[torch.Tensor] = None,
                       matched: Optional[torch.Tensor] = None, n_commit: Optional[torch.Tensor] = None,
                       max_len: Optional[int] = None) -> None:
    """commit_step_stop with multi-token stop sequences, per-row lists and per-row limits (asd_commit_step_finish): the append
    is cut behind the first committed token at which a sequence the row owns ENDS (the match may begin in earlier steps' tokens,
    never in front of position `start`, the prompt length) or at min(max_len, row_max_len[b]).  seq_tok i32 [n, 8] / seq_n i32
    [n] / row_first i32 [B+1] or None (every row owns all n <= 16): the tables of pack_stop_sequences, which checks that no row
    owns more than 16 on the host lists.  row_max_len i32 [B] or None.  finished / n_finished: as commit_step_stop.  matched
    i32 [B] in/out or None: the index, within the row's list, of the sequence that ended it."""
    Bv, K, cap, head, tail = _commit_front(tok, n_acc, drawn, seq_len, out_tokens, n_commit, max_len, lp=(lp_tok, lp_drawn, out_lp),
                                           ends=(finished, n_finished))
    if (seq_tok is None) != (seq_n is None):
        raise ValueError("seq_tok and seq_n come together")
    n_seq = 0 if seq_tok is None else seq_tok.shape[0]
    if seq_tok is not None and (seq_tok.dim() != 2 or seq_tok.shape[1] != B.MAX_STOP_SEQ_LEN or seq_n.shape != (n_seq,)):
        raise ValueError(f"seq_tok must be [n, {B.MAX_STOP_SEQ_LEN}] int32 and seq_n [n] int32")
    if row_first is not None and row_first.shape != (Bv + 1,):
        raise ValueError("row_first must be [B + 1] int32")
    if row_first is None and n_seq > B.MAX_STOP_SEQS:
        raise ValueError(f"at most {B.MAX_STOP_SEQS} stop sequences per row")
    if row_max_len is not None and row_max_len.shape != (Bv,):
        raise ValueError("row_max_len must be [B] int32")
    if matched is not None and matched.shape != (Bv,):
        raise ValueError("matched must be [B] int32")
    if int(start) < 0:
        raise ValueError("start must be >= 0")
    rc = _lib().asd_commit_step_finish(*head, Bv, K, _opt(seq_tok, "seq_tok", torch.int32) if n_seq else None,
                                       _opt(seq_n, "seq_n", torch.int32) if n_seq else None, n_seq,
                                       _opt(row_first, "row_first", torch.int32), _opt(row_max_len, "row_max_len", torch.int32),
                                       int(start), *tail, _opt(matched, "matched", torch.int32), cap, _stream())
    B.check("asd_commit_step_finish", rc)


# ------------------------------------------------------------------------------- predictor side
def logprob_stats(lp: torch.Tensor, n_valid: Optional[torch.Tensor] = None) -> torch.Tensor:
    """A7: [B,K] f32 log-probs -> [B,5] f64 (mean, std, min, q25, median), numpy semantics."""
    Bv, K = lp.shape
    out = torch.empty((Bv, 5), dtype=torch.float64, device=lp.device)
    rc = _lib().asd_logprob_stats(_dev(lp, "lp", torch.float32), lp.stride(0) if Bv else K,
                                  _opt(n_valid, "n_valid", torch.int32), Bv, K, out.data_ptr(), _stream())
    B.check("asd_logprob_stats", rc)
    return out


def pack_mlp_weights(w1, b1, w2, b2, device=None) -> torch.Tensor:
    """state_dict tensors (net.0.weight [H,D], net.0.bias [H], net.3.weight [1,H], net.3.bias [1])
    -> packed device buffer of asd_mlp_predict."""
    w1 = np.ascontiguousarray(torch.as_tensor(w1).detach().cpu().numpy(), dtype=np.float32)
    H, D = w1.shape
    b1 = np.ascontiguousarray(torch.as_tensor(b1).detach().cpu().numpy(), dtype=np.float32).reshape(H)
    w2 = np.ascontiguousarray(torch.as_tensor(w2).detach().cpu().numpy(), dtype=np.float32).reshape(H)
    b2 = np.ascontiguousarray(torch.as_tensor(b2).detach().cpu().numpy(), dtype=np.float32).reshape(1)
    n = int(_lib().asd_mlp_packed_floats(D, H))
    packed = np.empty(n, np.float32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    B.check("asd_mlp_pack_weights", _lib().asd_mlp_pack_weights(vp(w1), vp(b1), vp(w2), vp(b2), D, H, vp(packed)))
    t = torch.from_numpy(packed)
    return t.to(device or torch.device("cuda"))


def mlp_predict(x: torch.Tensor, packed_w: torch.Tensor, in_dim: int, hidden: int) -> torch.Tensor:
    """A8 (eval mode): x [B,in_dim] f32 -> score [B] f32."""
    Bv = x.shape[0]
    if not x.is_cuda or x.dtype != torch.float32 or x.dim() != 2 or (Bv and x.stride(1) != 1):
        raise ValueError("x must be a [B, in_dim] float32 CUDA tensor with unit stride along in_dim (rows may be strided)")
    out = torch.empty((Bv,), dtype=torch.float32, device=x.device)
    rc = _lib().asd_mlp_predict(x.data_ptr(), x.stride(0) if Bv else in_dim,
                                _dev(packed_w, "packed_w", torch.float32), Bv, in_dim, hidden, out.data_ptr(), _stream())
    B.check("asd_mlp_predict", rc)
    return out


def threshold_stop(score: torch.Tensor, theta: torch.Tensor) -> torch.Tensor:
    """A11: first stage s with score >= theta[s] (or the last)."""
    out = torch.empty((score.shape[0],), dtype=torch.int32, device=score.device)
    rc = _lib().asd_threshold_stop(_dev(score, "score", torch.float32), _dev(theta, "theta", torch.float64),
                                   score.shape[0], theta.shape[0], out.data_ptr(), _stream())
    B.check("asd_threshold_stop", rc)
    return out


def bayes_adjust(p: torch.Tensor, n_obs: int, alpha: float = 1.0, beta: float = 1.0) -> torch.Tensor:
    """A2 over a flat f64 tensor."""
    out = torch.empty_like(p)
    rc = _lib().asd_bayes_adjust(_dev(p, "p", torch.float64), int(n_obs), float(alpha), float(beta), p.numel(),
                                 out.data_ptr(), _stream())
    B.check("asd_bayes_adjust", rc)
    return out


def optimal_stopping(p: torch.Tensor, Cc: torch.Tensor, lam: float, risk_adjustment: bool = False,
                     alpha: float = 1.0, beta: float = 1.0, want_J: bool = True):
    """A1 batched: p [B,L] f64, C [L] f64 -> (k_star [B] i32, J [B,L+1] f64 or None)."""
    Bv, L = p.shape
    if Cc.numel() != L:
        raise ValueError("p and C must have the same length")  # dp_solver.py:34-35
    k = torch.empty((Bv,), dtype=torch.int32, device=p.device)
    J = torch.empty((Bv, L + 1), dtype=torch.float64, device=p.device) if want_J else None
    rc = _lib().asd_optimal_stopping(_dev(p, "p", torch.float64), _dev(Cc, "C", torch.float64), float(lam), Bv, L,
                                     int(bool(risk_adjustment)), float(alpha), float(beta), k.data_ptr(),
                                     None if J is None else J.data_ptr(), _stream())
    B.check("asd_optimal_stopping", rc)
    return k, J


def lambda_sweep(p: torch.Tensor, Cc: torch.Tensor, lam: torch.Tensor, risk_adjustment: bool = False, alpha: float = 1.0,
                 beta: float = 1.0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """N4: p [B,L] f64, Cc [L] f64, lam [G] f64 -> (k_star [G,B] i32, cost [G,B] f64, p_ok [G,B] f64)."""
    Bv, L = p.shape
    G = lam.shape[0]
    k = torch.empty((G, Bv), dtype=torch.int32, device=p.device)
    cost = torch.empty((G, Bv), dtype=torch.float64, device=p.device)
    ok = torch.empty((G, Bv), dtype=torch.float64, device=p.device)
    rc = _lib().asd_lambda_sweep(_dev(p, "p", torch.float64), _dev(Cc, "C", torch.float64), _dev(lam, "lam", torch.float64),
                                 Bv, L, G, 1 if risk_adjustment else 0, float(alpha), float(beta), k.data_ptr(),
                                 cost.data_ptr(), ok.data_ptr(), _stream())
    B.check("asd_lambda_sweep", rc)
    return k, cost, ok


def expected_cost(p: torch.Tensor, Cc: torch.Tensor, lam: float, k: torch.Tensor) -> torch.Tensor:
    """A3 batched."""
    Bv, L = p.shape
    out = torch.empty((Bv,), dtype=torch.float64, device=p.device)
    rc = _lib().asd_expected_cost(_dev(p, "p", torch.float64), _dev(Cc, "C", torch.float64), float(lam),
                                  _dev(k, "k", torch.int32), Bv, L, out.data_ptr(), _stream())
    B.check("asd_expected_cost", rc)
    return out


def derive_thresholds(q, c, lam: float) -> Tuple[np.ndarray, np.ndarray]:
    """A10 (host entry point of the library; O(n) f64, once per set_lambda)."""
    q = np.ascontiguousarray(q, dtype=np.float64).reshape(-1)
    c = np.ascontiguousarray(c, dtype=np.float64).reshape(-1)
    if q.size != c.size:
        raise ValueError("quality_bounds and cost_ratios must have the same length")
    theta = np.empty(q.size, np.float64)
    V = np.empty(q.size + 1, np.float64)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    B.check("asd_derive_thresholds", _lib().asd_derive_thresholds(vp(q), vp(c), q.size, float(lam), vp(theta), vp(V)))
    return theta, V


@dataclass
class StopResult:
    score: torch.Tensor       # [B] f32   predictor output
    k_star: Optional[torch.Tensor]    # [B] i32   DP rule
    stop: Optional[torch.Tensor]      # [B] u8    k_star == stage_idx
    thr_stop: Optional[torch.Tensor]  # [B] u8    score >= theta[stage_idx] (or last stage)
    stats: Optional[torch.Tensor]     # [B,5] f64


def _stop_out(Bv: int, dev, dp: bool, thr: bool, stats: bool) -> StopResult:
    """Fresh outputs of the predictor / stop epilogue; only the score is always computed."""
    u8 = lambda: torch.empty((Bv,), dtype=torch.uint8, device=dev)
    return StopResult(torch.empty((Bv,), dtype=torch.float32, device=dev),
                      torch.empty((Bv,), dtype=torch.int32, device=dev) if dp else None, u8() if dp else None,
                      u8() if thr else None, torch.empty((Bv, 5), dtype=torch.float64, device=dev) if stats else None)


def _stop_ptrs(res: StopResult):
    return [None if t is None else t.data_ptr() for t in (res.score, res.k_star, res.stop, res.thr_stop, res.stats)]


def predictor_stop(feat: torch.Tensor, packed_w: torch.Tensor, in_dim: int, hidden: int, *, stage_idx: int, L: int,
                   lp: Optional[torch.Tensor] = None, n_valid: Optional[torch.Tensor] = None, stats_col: int = -1,
                   risk_adjustment: bool = True, n_obs: int = 100, alpha: float = 1.0, beta: float = 1.0,
                   p_hist: Optional[torch.Tensor] = None, Cc: Optional[torch.Tensor] = None, lam: float = 1.0,
                   prefix_rule: bool = False, theta: Optional[torch.Tensor] = None,
                   want_stats: bool = False) -> StopResult:
    """Fused post-verify epilogue (asd_predictor_stop): stats -> features -> MLP -> Bayes -> DP / theta."""
    Bv = feat.shape[0]
    dev = feat.device
    res = _stop_out(Bv, dev, p_hist is not None and Cc is not None, theta is not None, want_stats)
    K = 0 if lp is None else lp.shape[1]
    rc = _lib().asd_predictor_stop(
        _opt(lp, "lp", torch.float32), (lp.stride(0) if lp is not None and Bv else K), _opt(n_valid, "n_valid", torch.int32),
        K, _dev(feat, "feat", torch.float32), feat.stride(0) if Bv else in_dim, stats_col,
        _dev(packed_w, "packed_w", torch.float32), in_dim, hidden, int(bool(risk_adjustment)), int(n_obs), float(alpha),
        float(beta), _opt(p_hist, "p_hist", torch.float64), _opt(Cc, "C", torch.float64), float(lam), L, stage_idx,
        int(bool(prefix_rule)), _opt(theta, "theta", torch.float64), Bv, *_stop_ptrs(res), _stream())
    B.check("asd_predictor_stop", rc)
    return res


def verify_accept_fused(logits: torch.Tensor, tok: torch.Tensor, lp_draft: torch.Tensor, u: torch.Tensor,
                        workspace: VerifyWorkspace, feat: torch.Tensor, packed_w: torch.Tensor, in_dim: int, hidden: int, *,
                        stage_idx: int, L: int, stats_col: int = 5, risk_adjustment: bool = True, n_obs: int = 100,
                        alpha: float = 1.0, beta: float = 1.0, p_hist: Optional[torch.Tensor] = None,
                        Cc: Optional[torch.Tensor] = None, lam: float = 1.0, prefix_rule: bool = False,
                        theta: Optional[torch.Tensor] = None, want_stats: bool = False,
                        out: Optional[VerifyResult] = None, inv_temperature: float = 1.0) -> Tuple[VerifyResult, StopResult]:
    """N1, second form: verify + accept + predictor/stop epilogue in ONE call (one launch for the reference's
    64->32->1 predictor at any batch size, two for other predictor shapes; asd_verify_accept_fused_ex in include/asd_hip.h)."""
    out, lead, outs = _verify_args(logits, tok, lp_draft, u, out)
    Bv = tok.shape[0]
    res = _stop_out(Bv, logits.device, p_hist is not None and Cc is not None, theta is not None, want_stats)
    opt = B.verify_options(inv_temperature)
    rc = _lib().asd_verify_accept_fused_ex(
        *lead, *outs, workspace.buf.data_ptr(), workspace.bytes,
        _dev(feat, "feat", torch.float32), feat.stride(0) if Bv else in_dim, stats_col,
        _dev(packed_w, "packed_w", torch.float32), in_dim, hidden, int(bool(risk_adjustment)), int(n_obs), float(alpha),
        float(beta), _opt(p_hist, "p_hist", torch.float64), _opt(Cc, "C", torch.float64), float(lam), L, stage_idx,
        int(bool(prefix_rule)), _opt(theta, "theta", torch.float64), *_stop_ptrs(res), C.addressof(opt), _stream())
    B.check("asd_verify_accept_fused_ex", rc)
    return out, res


def _rows(t: torch.Tensor, name: str) -> Tuple[int, int]:
    """(data_ptr, row stride in elements) of a [rows, V] or [B, K, V] logits tensor with unit stride in V."""
    if not t.is_cuda or t.dtype not in _DTYPE_CODE or t.stride(-1) != 1:
        raise ValueError(f"{name} must be a CUDA f32/bf16/f16 tensor with unit stride along the vocabulary")
    # (one sequence: its stride is never used, and torch leaves a size-1 dimension's stride as it was -- a slice [:, :K] of a
    # [1, K + 1, V] tensor is already "contiguous" and keeps stride(0) = (K + 1) V)
    if t.dim() == 3 and t.shape[0] > 1 and t.stride(0) != t.shape[1] * t.stride(1):
        raise ValueError(f"{name}: rows must be evenly spaced over (b, k)")
    return t.data_ptr(), t.stride(-2)


def _sampling_args(inv_temperature, scalars: tuple, Bv: int, V: int, dtype) -> tuple:
    """The sampling parameters of a draw as its C entry point takes them: inv_temperature and the scalars behind it, or the
    pointer of a SamplingRows table in their place."""
    if isinstance(inv_temperature, SamplingRows):
        return (inv_temperature.ptr(Bv, V, dtype),)
    return (float(inv_temperature), *scalars)


def _logit_strides(view: torch.Tensor, K1: int, rows: str = "K1") -> Tuple[int, int]:
    """(ld_seq, ld_row) in elements of a [B, K1, V] logits view with unit stride along V; `rows` is how the caller's error
    text spells K1."""
    Bv, V = view.shape[0], view.shape[2]
    # the stride of a size-1 dimension is arbitrary: give the kernel one that satisfies its checks
    ld_row = view.stride(1) if K1 > 1 else V
    ld_seq = view.stride(0) if Bv > 1 else K1 * ld_row
    if ld_row < V or ld_seq < K1 * ld_row:
        raise ValueError(f"logits rows overlap: the row stride must be >= V and the sequence stride >= {rows} row strides")
    return ld_seq, ld_row


class ResidualSampler(_StatusWorkspace):
    """asd_residual_sample with its workspace: the token each sequence commits after its accepted prefix."""

    def __init__(self, B_: int, V: int, dtype: torch.dtype = torch.bfloat16, device: Optional[torch.device] = None):
        self.B, self.V, self.dtype = B_, V, dtype
        # scratch of the multi-launch form + the mailboxes of the group form (B <= 64): zeroed ONCE, handed back empty by every call
        # (+ the bonus rows' nucleus thresholds of asd_residual_sample_top_p, behind the part asd_residual_sample_ex uses)
        self.bytes = int(_lib().asd_residual_sample_top_p_workspace_bytes(B_, V, _DTYPE_CODE[dtype]))
        self.buf = torch.empty(self.bytes, dtype=torch.uint8, device=device or torch.device("cuda"))
        self.reset()

    def _sample(self, entry: str, t_logits, d_logits, n_acc, r, bonus_logits, inv_temperature, out, scalars=(), lp_out=None,
                **thresholds):
        """The body of __call__ / top_p / top_k / lp / lp_rows: `entry` is the C entry point; `scalars`, then the optional [B,K]
        `thresholds` (in the entry point's order), are its arguments between inv_temperature and the token; `lp_out` ([B] f32)
        follows the token where the entry point has it.  A SamplingRows as inv_temperature: its table pointer takes the place
        of inv_temperature and the scalars."""
        Bv, K, V = t_logits.shape
        if d_logits.shape != t_logits.shape or d_logits.dtype != t_logits.dtype:
            raise ValueError("t_logits and d_logits must have the same shape and dtype")
        tp, ldt = _rows(t_logits, "t_logits")
        dp, ldd = _rows(d_logits, "d_logits")
        bp, ldb = (None, V) if bonus_logits is None else _rows(bonus_logits, "bonus_logits")
        if out is None:
            out = torch.empty((Bv,), dtype=torch.int32, device=t_logits.device)
        for name, t in thresholds.items():
            if t is not None and tuple(t.shape) != (Bv, K):
                raise ValueError(f"{name} must be [B, K]")
        rc = getattr(_lib(), entry)(tp, ldt, dp, ldd, bp, ldb, _DTYPE_CODE[t_logits.dtype], _dev(n_acc, "n_acc", torch.int32),
                                    _dev(r, "r", torch.float32), Bv, K, V,
                                    *_sampling_args(inv_temperature, scalars, Bv, V, t_logits.dtype),
                                    *[_opt(t, name, torch.float32) for name, t in thresholds.items()], out.data_ptr(),
                                    *(() if lp_out is None else (_dev(lp_out, "lp", torch.float32),)),
                                    self.buf.data_ptr(), self.bytes, _stream())
        B.check(entry, rc)
        return out

    def __call__(self, t_logits: torch.Tensor, d_logits: torch.Tensor, n_acc: torch.Tensor, r: torch.Tensor,
                 bonus_logits: Optional[torch.Tensor] = None, inv_temperature: float = 1.0,
                 out: Optional[torch.Tensor] = None, d_threshold: Optional[torch.Tensor] = None) -> torch.Tensor:
        """t_logits / d_logits: [B,K,V]; bonus_logits: [B,V] or None; n_acc: [B] i32; r: [B] f32 -> token [B] i32.
        d_threshold: [B,K] f32 nucleus thresholds of the draft rows (DraftSampler's `thr`) when the drafts were
        drawn with top-p (asd_residual_sample_ex); None = untruncated drafts."""
        return self._sample("asd_residual_sample_ex", t_logits, d_logits, n_acc, r, bonus_logits, inv_temperature, out,
                            d_threshold=d_threshold)

    def top_p(self, t_logits: torch.Tensor, d_logits: torch.Tensor, n_acc: torch.Tensor, r: torch.Tensor,
              bonus_logits: Optional[torch.Tensor] = None, inv_temperature: float = 1.0, *, top_p: float,
              t_threshold: Optional[torch.Tensor], d_threshold: Optional[torch.Tensor] = None,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The committed token against the TARGET's nucleus (asd_residual_sample_top_p): t_threshold [B,K] = the verify's
        t_nucleus_logit; the bonus rows' thresholds are found by the sampler.  top_p outside (0, 1) = __call__ (same bits)."""
        return self._sample("asd_residual_sample_top_p", t_logits, d_logits, n_acc, r, bonus_logits, inv_temperature, out,
                            (float(top_p),), t_threshold=t_threshold, d_threshold=d_threshold)

    def top_k(self, t_logits: torch.Tensor, d_logits: torch.Tensor, n_acc: torch.Tensor, r: torch.Tensor,
              bonus_logits: Optional[torch.Tensor] = None, inv_temperature: float = 1.0, *, top_k: int, top_p: float = 1.0,
              t_threshold: Optional[torch.Tensor], d_threshold: Optional[torch.Tensor] = None,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The committed token against the target's top-k + top-p set (asd_residual_sample_top_k): t_threshold [B,K] = the
        thresholds of verify_accept_top_k; the bonus rows' are found by the sampler with the same select.  top_k <= 0 or
        >= V is top_p(...) (the same bits)."""
        return self._sample("asd_residual_sample_top_k", t_logits, d_logits, n_acc, r, bonus_logits, inv_temperature, out,
                            (int(top_k), float(top_p)), t_threshold=t_threshold, d_threshold=d_threshold)

    def lp(self, t_logits: torch.Tensor, d_logits: torch.Tensor, n_acc: torch.Tensor, r: torch.Tensor,
           bonus_logits: Optional[torch.Tensor] = None, inv_temperature: float = 1.0, *, top_k: int = 0, top_p: float = 1.0,
           t_threshold: Optional[torch.Tensor] = None, d_threshold: Optional[torch.Tensor] = None,
           out: Optional[torch.Tensor] = None, lp_out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """The committed token AND its target log-prob (asd_residual_sample_lp) -> (token [B] i32, lp [B] f32): the token of
        __call__ / top_p / top_k on the same arguments (the same bits), lp = log p_t^N(token) under the target row the draw
        used (NaN where token == -1)."""
        if lp_out is None:
            lp_out = torch.empty((t_logits.shape[0],), dtype=torch.float32, device=t_logits.device)
        tok = self._sample("asd_residual_sample_lp", t_logits, d_logits, n_acc, r, bonus_logits, inv_temperature, out,
                           (int(top_k), float(top_p)), lp_out, t_threshold=t_threshold, d_threshold=d_threshold)
        return tok, lp_out

    def lp_min_p(self, t_logits: torch.Tensor, d_logits: torch.Tensor, n_acc: torch.Tensor, r: torch.Tensor,
                 bonus_logits: Optional[torch.Tensor] = None, inv_temperature: float = 1.0, *, top_k: int = 0, top_p: float = 1.0,
                 min_p: float = 0.0, t_threshold: Optional[torch.Tensor] = None, d_threshold: Optional[torch.Tensor] = None,
                 out: Optional[torch.Tensor] = None, lp_out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """lp(...) against the target's top-k + top-p + min-p set (asd_residual_sample_lp_min_p): t_threshold [B,K] = the
        thresholds of verify_accept_min_p; the bonus rows' are found by the sampler with the same select.  min_p <= 0 is
        lp(...) (the same bits)."""
        if lp_out is None:
            lp_out = torch.empty((t_logits.shape[0],), dtype=torch.float32, device=t_logits.device)
        tok = self._sample("asd_residual_sample_lp_min_p", t_logits, d_logits, n_acc, r, bonus_logits, inv_temperature, out,
                           (int(top_k), float(top_p), float(min_p)), lp_out, t_threshold=t_threshold, d_threshold=d_threshold)
        return tok, lp_out


    def lp_rows(self, t_logits: torch.Tensor, d_logits: torch.Tensor, n_acc: torch.Tensor, r: torch.Tensor,
                bonus_logits: Optional[torch.Tensor] = None, *, rows: "SamplingRows", t_threshold: torch.Tensor,
                d_threshold: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                lp_out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """lp_min_p(...) with every sequence's own parameters (asd_residual_sample_lp_rows): t_threshold [B,K] = the thresholds
        of verify_accept_rows; the bonus rows' are found by the sampler with the sequence's select."""
        if lp_out is None:
            lp_out = torch.empty((t_logits.shape[0],), dtype=torch.float32, device=t_logits.device)
        tok = self._sample("asd_residual_sample_lp_rows", t_logits, d_logits, n_acc, r, bonus_logits, rows, out, (), lp_out,
                           t_threshold=t_threshold, d_threshold=d_threshold)
        return tok, lp_out


@dataclass
class DraftDraw:
    tok: torch.Tensor   # [B] i32  the proposed token
    lp: torch.Tensor    # [B] f32  log q(tok) under the (nucleus-renormalised) draft distribution
    thr: torch.Tensor   # [B] f32  nucleus threshold logit (-inf: no truncation)


class DraftSampler(_StatusWorkspace):
    """X1: asd_draft_sample with its workspace -- one call proposes the next token of every sequence from the
    draft tier's next-token logits [B, V]: temperature and top-p folded in, inverse-CDF draw from caller-supplied
    uniforms, log q(tok) for the verify step, nucleus threshold for the exact residual."""

    def __init__(self, B_: int, V: int, dtype: torch.dtype = torch.bfloat16, device: Optional[torch.device] = None):
        self.B, self.V, self.dtype = B_, V, dtype
        # mailboxes of the workgroups a row is spread over (B <= 128): zeroed ONCE, handed back empty by every call
        self.bytes = int(_lib().asd_draft_sample_workspace_bytes(B_, V, _DTYPE_CODE[dtype]))
        self.buf = torch.empty(self.bytes, dtype=torch.uint8, device=device or torch.device("cuda"))
        self.reset()

    def _draw(self, entry: str, logits, r, inv_temperature, truncation: tuple, out) -> DraftDraw:
        """The body of __call__ / top_k / min_p / rows: `entry` is the C entry point, `truncation` its arguments between
        inv_temperature and the outputs.  A SamplingRows as inv_temperature: its table pointer takes the place of both."""
        if logits.dim() != 2 or logits.dtype != self.dtype or not logits.is_cuda or logits.stride(1) != 1:
            raise ValueError(f"logits must be a [B, V] {self.dtype} CUDA tensor with unit stride along V")
        Bv, V = logits.shape
        if Bv > self.B or V != self.V:
            raise ValueError(f"sampler was sized for B<={self.B}, V={self.V}")
        dev = logits.device
        if out is None:
            out = DraftDraw(torch.empty((Bv,), dtype=torch.int32, device=dev),
                            torch.empty((Bv,), dtype=torch.float32, device=dev),
                            torch.empty((Bv,), dtype=torch.float32, device=dev))
        rc = getattr(_lib(), entry)(logits.data_ptr(), logits.stride(0) if Bv > 1 else V, _DTYPE_CODE[logits.dtype],
                                    _dev(r, "r", torch.float32), Bv, V,
                                    *_sampling_args(inv_temperature, truncation, Bv, V, logits.dtype),
                                    _dev(out.tok, "tok", torch.int32), _dev(out.lp, "lp", torch.float32),
                                    _dev(out.thr, "thr", torch.float32), self.buf.data_ptr(), self.bytes, _stream())
        B.check(entry, rc)
        return out

    def __call__(self, logits: torch.Tensor, r: torch.Tensor, inv_temperature: float = 1.0, top_p: float = 1.0,
                 out: Optional[DraftDraw] = None) -> DraftDraw:
        return self._draw("asd_draft_sample", logits, r, inv_temperature, (float(top_p),), out)

    def top_k(self, logits: torch.Tensor, r: torch.Tensor, inv_temperature: float = 1.0, *, top_k: int, top_p: float = 1.0,
              out: Optional[DraftDraw] = None) -> DraftDraw:
        """The proposal under HF's Temperature -> TopK -> TopP chain (asd_draft_sample_top_k): thr = max(x_k, x*_K), the
        threshold of the top-p select taken over the top-k set.  HF generate(do_sample=True, ...) applies top_k = 50 unless
        told otherwise.  top_k <= 0 or >= V is __call__ (the same bits); otherwise one workgroup per row, the workspace unused."""
        return self._draw("asd_draft_sample_top_k", logits, r, inv_temperature, (int(top_k), float(top_p)), out)

    def min_p(self, logits: torch.Tensor, r: torch.Tensor, inv_temperature: float = 1.0, *, min_p: float, top_k: int = 0,
              top_p: float = 1.0, out: Optional[DraftDraw] = None) -> DraftDraw:
        """The proposal under Temperature -> TopK -> TopP -> MinP (asd_draft_sample_min_p; HF's MinPLogitsWarper, vLLM's
        min_p): thr = max(thr_kp, x_max + T ln(min_p)).  min_p <= 0 is top_k(...) (the same bits); otherwise one workgroup
        per row, the workspace unused."""
        return self._draw("asd_draft_sample_min_p", logits, r, inv_temperature, (int(top_k), float(top_p), float(min_p)), out)


    def rows(self, logits: torch.Tensor, r: torch.Tensor, rows: "SamplingRows", out: Optional[DraftDraw] = None) -> DraftDraw:
        """The proposal with every sequence's own temperature / top-k / top-p / min-p (asd_draft_sample_rows): one workgroup
        per row at every batch size, the workspace unused; sequence b returns the bits min_p(...) returns for it."""
        return self._draw("asd_draft_sample_rows", logits, r, rows, (), out)


# ------------------------------------------------------------------------------- greedy decoding (temperature 0)
@dataclass
class GreedyResult:
    lp_target: torch.Tensor   # [B,K]   f32  log p_target(tok) (-inf: tok outside the vocabulary)
    accept: torch.Tensor      # [B,K]   u8   tok == argmax of its row
    n_acc: torch.Tensor       # [B]     i32  accepted-prefix length
    drawn: torch.Tensor       # [B]     i32  argmax[b, n_acc[b]]: the token committed behind the prefix (-1: no finite logit)
    lp_drawn: torch.Tensor    # [B]     f32  its log-prob
    argmax: torch.Tensor      # [B,K+1] i32  the lowest id among each row's maxima
    lp_argmax: torch.Tensor   # [B,K+1] f32


class GreedyVerifier:
    """asd_verify_greedy with its workspace and outputs: arg-max, accepted prefix and commit token of every sequence from the
    target's [B, K+1, V] logits in ONE launch, read in place (any sequence / row stride, unit stride along V); K = 0 takes
    [B, V] -- the plain greedy step.  The workspace is zeroed by every call itself (no asd_workspace_init, no status word).
    `out` holds the outputs of a full-size call; a call writes there with `out=verifier.out`, into fresh tensors otherwise
    (the stage loop keeps the K draft steps' tokens side by side)."""

    def __init__(self, B_: int, K: int, V: int, dtype: torch.dtype = torch.bfloat16, device: Optional[torch.device] = None):
        self.B, self.K, self.V, self.dtype = B_, K, V, dtype
        self.device = device or torch.device("cuda")
        self.bytes = int(_lib().asd_verify_greedy_workspace_bytes(B_, K, V, _DTYPE_CODE[dtype]))
        self.buf = torch.empty(self.bytes, dtype=torch.uint8, device=self.device)
        self.out = self.new_out(B_)

    def new_out(self, Bv: int) -> GreedyResult:
        K, dev = self.K, self.device
        return GreedyResult(torch.empty((Bv, K), dtype=torch.float32, device=dev), torch.empty((Bv, K), dtype=torch.uint8, device=dev),
                            torch.empty((Bv,), dtype=torch.int32, device=dev), torch.empty((Bv,), dtype=torch.int32, device=dev),
                            torch.empty((Bv,), dtype=torch.float32, device=dev),
                            torch.empty((Bv, K + 1), dtype=torch.int32, device=dev),
                            torch.empty((Bv, K + 1), dtype=torch.float32, device=dev))

    def __call__(self, logits: torch.Tensor, tok: Optional[torch.Tensor] = None, inv_temperature: float = 1.0, splits: int = 0,
                 out: Optional[GreedyResult] = None) -> GreedyResult:
        K, V = self.K, self.V
        if not isinstance(logits, torch.Tensor) or not logits.is_cuda or logits.dtype != self.dtype:
            raise ValueError(f"logits must be a {self.dtype} CUDA (HIP) tensor; this package has no CPU path")
        if logits.dim() == 2 and K == 0:
            logits = logits[:, None]
        if logits.dim() != 3 or logits.shape[1] != K + 1 or logits.shape[2] != V or logits.stride(2) != 1:
            raise ValueError(f"logits must be [B, {K + 1}, {V}]" + (f" or [B, {V}]" if K == 0 else "") + " with unit stride along V")
        Bv = logits.shape[0]
        if Bv > self.B:
            raise ValueError(f"verifier was sized for B <= {self.B}")
        ld_seq, ld_row = _logit_strides(logits, K + 1, "(K + 1)")
        if K > 0:
            if tok is None or tuple(tok.shape) != (Bv, K):
                raise ValueError("tok must be [B, K]")
            tok_p = _dev(tok, "tok", torch.int32)
        else:
            tok_p = None
        if out is None:
            out = self.new_out(Bv)
        rc = _lib().asd_verify_greedy(logits.data_ptr(), _DTYPE_CODE[logits.dtype], ld_seq, ld_row, tok_p, Bv, K, V,
                                      float(inv_temperature), int(splits), _dev(out.argmax, "argmax", torch.int32),
                                      _dev(out.lp_argmax, "lp_argmax", torch.float32), _dev(out.lp_target, "lp_target", torch.float32),
                                      _dev(out.accept, "accept", torch.uint8), _dev(out.n_acc, "n_acc", torch.int32),
                                      _dev(out.drawn, "drawn", torch.int32), _dev(out.lp_drawn, "lp_drawn", torch.float32),
                                      self.buf.data_ptr(), self.bytes, _stream())
        B.check("asd_verify_greedy", rc)
        return out


# ------------------------------------------------------------------------------- top-N log-probs (SamplingParams(logprobs=N))
MAX_TOP_LOGPROBS = B.MAX_TOP_LOGPROBS


class TopLogprobs:
    """asd_top_logprobs with its workspace and outputs: the `n` most likely tokens of every row of [B, K1, V] logits and their
    log-probs over the whole vocabulary, read in place (any sequence / row stride, unit stride along V); K1 = 1 also takes
    [B, V].  Order: value descending, then id ascending; slots that cannot be filled hold (-1, -inf).  The workspace is zeroed
    by every call itself.  `out` = (top_id i32 [B,K1,n], top_lp f32 [B,K1,n]) holds the outputs of a full-size call; a call
    writes there with `out=obj.out`, into fresh tensors otherwise."""

    def __init__(self, B_: int, K1: int, V: int, dtype: torch.dtype = torch.bfloat16, n: int = 5,
                 device: Optional[torch.device] = None):
        if not 1 <= int(n) <= MAX_TOP_LOGPROBS:
            raise ValueError(f"n must be in [1, {MAX_TOP_LOGPROBS}]")
        self.B, self.K1, self.V, self.dtype, self.n = B_, K1, V, dtype, int(n)
        self.device = device or torch.device("cuda")
        self.bytes = int(_lib().asd_top_logprobs_workspace_bytes(B_, K1, self.n))
        self.buf = torch.empty(self.bytes, dtype=torch.uint8, device=self.device)
        self.out = self.new_out(B_)

    def new_out(self, Bv: int) -> Tuple[torch.Tensor, torch.Tensor]:
        return (torch.empty((Bv, self.K1, self.n), dtype=torch.int32, device=self.device),
                torch.empty((Bv, self.K1, self.n), dtype=torch.float32, device=self.device))

    def __call__(self, logits: torch.Tensor, inv_temperature=1.0, splits: int = 0,
                 out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """inv_temperature: a number, or a float32 [B] device tensor with one value per sequence (asd_top_logprobs_rows)."""
        K1, V = self.K1, self.V
        if not isinstance(logits, torch.Tensor) or not logits.is_cuda or logits.dtype != self.dtype:
            raise ValueError(f"logits must be a {self.dtype} CUDA (HIP) tensor; this package has no CPU path")
        if logits.dim() == 2 and K1 == 1:
            logits = logits[:, None]
        if logits.dim() != 3 or logits.shape[1] != K1 or logits.shape[2] != V or logits.stride(2) != 1:
            raise ValueError(f"logits must be [B, {K1}, {V}]" + (f" or [B, {V}]" if K1 == 1 else "") + " with unit stride along V")
        Bv = logits.shape[0]
        if Bv > self.B:
            raise ValueError(f"sized for B <= {self.B}")
        ld_seq, ld_row = _logit_strides(logits, K1)
        if out is None:
            out = self.new_out(Bv)
        top_id, top_lp = out
        if tuple(top_id.shape) != (Bv, K1, self.n) or tuple(top_lp.shape) != (Bv, K1, self.n):
            raise ValueError("out must be (int32 [B, K1, n], float32 [B, K1, n])")
        if isinstance(inv_temperature, torch.Tensor):
            if tuple(inv_temperature.shape) != (Bv,):
                raise ValueError("a per-sequence inv_temperature must be float32 [B]")
            entry, scale = "asd_top_logprobs_rows", _dev(inv_temperature, "inv_temperature", torch.float32)
        else:
            entry, scale = "asd_top_logprobs", float(inv_temperature)
        rc = getattr(_lib(), entry)(logits.data_ptr(), _DTYPE_CODE[logits.dtype], ld_seq, ld_row, Bv, K1, V,
                                    scale, self.n, int(splits), _dev(top_id, "top_id", torch.int32),
                                    _dev(top_lp, "top_lp", torch.float32), self.buf.data_ptr(), self.bytes, _stream())
        B.check(entry, rc)
        return out


class PromptLogprobs:
    """asd_prompt_logprobs with its workspace: per row of [B, T, V] logits the log-prob and the rank of the token `target[b, t]`
    and, with n >= 1, the row's top-n table (asd_top_logprobs' bits).  `logits` and `target` are read in place: strided views
    with unit last stride, nothing is copied.  Rows with t < first[b] are skipped (lp 0, rank 0, ids -1, table -inf).  The
    workspace is sized for the split count the launch uses at (B, T, V, dtype, splits), not for ASD_MAX_SPLITS."""

    def __init__(self, B_: int, T: int, V: int, dtype: torch.dtype = torch.bfloat16, n: int = 0, splits: int = 0,
                 device: Optional[torch.device] = None):
        if isinstance(n, bool) or not 0 <= int(n) <= MAX_TOP_LOGPROBS:
            raise ValueError(f"n must be in [0, {MAX_TOP_LOGPROBS}]")
        if dtype not in _DTYPE_CODE:
            raise ValueError(f"unsupported logits dtype {dtype}")
        self.B, self.T, self.V, self.dtype, self.n, self.splits = B_, T, V, dtype, int(n), int(splits)
        self.device = device or torch.device("cuda")
        with torch.cuda.device(self.device):       # splits == 0: the heuristic counts the CUs of the device that launches
            self.bytes = int(_lib().asd_prompt_logprobs_workspace_bytes(B_, T, V, _DTYPE_CODE[dtype], self.splits))
        self.buf = torch.empty(self.bytes, dtype=torch.uint8, device=self.device)

    def __call__(self, logits: torch.Tensor, target: torch.Tensor, first: Optional[torch.Tensor] = None,
                 inv_temperature: float = 1.0):
        """-> (lp f32 [B,T], rank i32 [B,T], top_id i32 [B,T,n] | None, top_lp f32 [B,T,n] | None), fresh tensors."""
        T, V, n = self.T, self.V, self.n
        if not isinstance(logits, torch.Tensor) or not logits.is_cuda or logits.dtype != self.dtype:
            raise ValueError(f"logits must be a {self.dtype} CUDA (HIP) tensor; this package has no CPU path")
        if logits.dim() != 3 or logits.shape[1] != T or logits.shape[2] != V or logits.stride(2) != 1:
            raise ValueError(f"logits must be [B, {T}, {V}] with unit stride along V")
        Bv = logits.shape[0]
        if Bv != self.B:                           # the heuristic's split count, and with it the workspace, depends on B
            raise ValueError(f"sized for B == {self.B}")
        if not isinstance(target, torch.Tensor) or not target.is_cuda or target.dtype != torch.int32:
            raise ValueError("target must be an int32 CUDA (HIP) tensor")
        if tuple(target.shape) != (Bv, T) or (T > 1 and target.stride(1) != 1):
            raise ValueError(f"target must be [B, {T}] with unit stride along T")
        ld_target = target.stride(0) if Bv > 1 else T
        if ld_target < T:
            raise ValueError("target rows overlap: the row stride must be >= T")
        if first is not None and tuple(first.shape) != (Bv,):
            raise ValueError("first must be int32 [B]")
        ld_seq, ld_row = _logit_strides(logits, T, rows="T")
        lp = torch.empty((Bv, T), dtype=torch.float32, device=self.device)
        rank = torch.empty((Bv, T), dtype=torch.int32, device=self.device)
        top_id = torch.empty((Bv, T, n), dtype=torch.int32, device=self.device) if n else None
        top_lp = torch.empty((Bv, T, n), dtype=torch.float32, device=self.device) if n else None
        rc = _lib().asd_prompt_logprobs(logits.data_ptr(), _DTYPE_CODE[logits.dtype], ld_seq, ld_row, Bv, T, V,
                                        target.data_ptr(), ld_target, _opt(first, "first", torch.int32), float(inv_temperature),
                                        n, self.splits, lp.data_ptr(), rank.data_ptr(),
                                        None if top_id is None else top_id.data_ptr(),
                                        None if top_lp is None else top_lp.data_ptr(), self.buf.data_ptr(), self.bytes, _stream())
        B.check("asd_prompt_logprobs", rc)
        return lp, rank, top_id, top_lp


def prompt_logprobs(logits: torch.Tensor, target: torch.Tensor, first: Optional[torch.Tensor], n: int,
                    inv_temperature: float = 1.0, splits: int = 0):
    """One asd_prompt_logprobs call with a workspace of its own -> (lp, rank, top_id | None, top_lp | None); see PromptLogprobs."""
    if not isinstance(logits, torch.Tensor) or logits.dim() != 3:
        raise ValueError("logits must be a [B, T, V] tensor")
    Bv, T, V = logits.shape
    return PromptLogprobs(Bv, T, V, logits.dtype, n, splits, logits.device)(logits, target, first, inv_temperature)


class TokenStats:
    """asd_token_stats with its workspace: per row of a step's [B, K1, V] logits that may be committed, the rank of the committed
    token, the arg-max and its log-prob, the entropy and, with n >= 1, the row's top-n table (asd_top_logprobs' bits), in one
    streaming pass.  Row j of sequence b is live while j <= a = clamp(n_acc[b], 0, K1 - 1) and scores tok[b, j] (j < a) or
    drawn[b] (j == a); later rows are not streamed and hold the neutral outputs (rank 0, id -1, 0.0, 0.0, table (-1, -inf)).
    `logits` and `tok` are read in place: strided views with unit last stride, nothing is copied; K1 = 1 also takes [B, V] and
    tok = None.  The workspace is sized for the split count the launch uses at (B, K1, V, dtype, splits)."""

    def __init__(self, B_: int, K1: int, V: int, dtype: torch.dtype = torch.bfloat16, n: int = 0, splits: int = 0,
                 device: Optional[torch.device] = None):
        if isinstance(n, bool) or not 0 <= int(n) <= MAX_TOP_LOGPROBS:
            raise ValueError(f"n must be in [0, {MAX_TOP_LOGPROBS}]")
        if dtype not in _DTYPE_CODE:
            raise ValueError(f"unsupported logits dtype {dtype}")
        self.B, self.K1, self.V, self.dtype, self.n, self.splits = B_, K1, V, dtype, int(n), int(splits)
        self.device = device or torch.device("cuda")
        with torch.cuda.device(self.device):       # splits == 0: the heuristic counts the CUs of the device that launches
            self.bytes = int(_lib().asd_token_stats_workspace_bytes(B_, K1, V, _DTYPE_CODE[dtype], self.splits))
        self.buf = torch.empty(self.bytes, dtype=torch.uint8, device=self.device)

    def __call__(self, logits: torch.Tensor, tok: Optional[torch.Tensor], n_acc: torch.Tensor, drawn: torch.Tensor,
                 inv_temperature=1.0):
        """inv_temperature: a number, or a float32 [B] device tensor with one value per sequence.
        -> (stat_id i32 [B,K1,2] (rank, arg-max id), stat_val f32 [B,K1,2] (entropy, max log-prob), top_id i32 [B,K1,n] | None,
        top_lp f32 [B,K1,n] | None), fresh tensors."""
        K1, V, n = self.K1, self.V, self.n
        if not isinstance(logits, torch.Tensor) or not logits.is_cuda or logits.dtype != self.dtype:
            raise ValueError(f"logits must be a {self.dtype} CUDA (HIP) tensor; this package has no CPU path")
        if logits.dim() == 2 and K1 == 1:
            logits = logits[:, None]
        if logits.dim() != 3 or logits.shape[1] != K1 or logits.shape[2] != V or logits.stride(2) != 1:
            raise ValueError(f"logits must be [B, {K1}, {V}]" + (f" or [B, {V}]" if K1 == 1 else "") + " with unit stride along V")
        Bv = logits.shape[0]
        if Bv != self.B:                           # the heuristic's split count, and with it the workspace, depends on B
            raise ValueError(f"sized for B == {self.B}")
        ld_seq, ld_row = _logit_strides(logits, K1)
        tok_p, ld_tok = None, 0
        if K1 > 1:
            if not isinstance(tok, torch.Tensor) or not tok.is_cuda or tok.dtype != torch.int32:
                raise ValueError("tok must be an int32 CUDA (HIP) tensor")
            if tuple(tok.shape) != (Bv, K1 - 1) or (K1 > 2 and tok.stride(1) != 1):
                raise ValueError(f"tok must be [B, {K1 - 1}] with unit stride along its rows")
            ld_tok = tok.stride(0) if Bv > 1 else K1 - 1
            if ld_tok < K1 - 1:
                raise ValueError("tok rows overlap: the row stride must be >= K1 - 1")
            tok_p = tok.data_ptr()
        elif tok is not None:
            raise ValueError("tok must be None when K1 == 1")
        if tuple(n_acc.shape) != (Bv,) or tuple(drawn.shape) != (Bv,):
            raise ValueError("n_acc and drawn must be int32 [B]")
        if isinstance(inv_temperature, torch.Tensor):
            if tuple(inv_temperature.shape) != (Bv,):
                raise ValueError("a per-sequence inv_temperature must be float32 [B]")
            scalar, rows = 1.0, _dev(inv_temperature, "inv_temperature", torch.float32)
        else:
            scalar, rows = float(inv_temperature), None
        stat_id = torch.empty((Bv, K1, 2), dtype=torch.int32, device=self.device)
        stat_val = torch.empty((Bv, K1, 2), dtype=torch.float32, device=self.device)
        top_id = torch.empty((Bv, K1, n), dtype=torch.int32, device=self.device) if n else None
        top_lp = torch.empty((Bv, K1, n), dtype=torch.float32, device=self.device) if n else None
        rc = _lib().asd_token_stats(logits.data_ptr(), _DTYPE_CODE[logits.dtype], ld_seq, ld_row, Bv, K1, V, tok_p, ld_tok,
                                    _dev(n_acc, "n_acc", torch.int32), _dev(drawn, "drawn", torch.int32), scalar, rows,
                                    n, self.splits, stat_id.data_ptr(), stat_val.data_ptr(),
                                    None if top_id is None else top_id.data_ptr(),
                                    None if top_lp is None else top_lp.data_ptr(), self.buf.data_ptr(), self.bytes, _stream())
        B.check("asd_token_stats", rc)
        return stat_id, stat_val, top_id, top_lp


def token_stats(logits: torch.Tensor, tok: Optional[torch.Tensor], n_acc: torch.Tensor, drawn: torch.Tensor, n: int = 0,
                inv_temperature=1.0, splits: int = 0):
    """One asd_token_stats call with a workspace of its own -> (stat_id, stat_val, top_id | None, top_lp | None); see TokenStats."""
    if not isinstance(logits, torch.Tensor) or logits.dim() not in (2, 3):
        raise ValueError("logits must be a [B, K1, V] (or [B, V]) tensor")
    Bv, V = logits.shape[0], logits.shape[-1]
    K1 = logits.shape[1] if logits.dim() == 3 else 1
    return TokenStats(Bv, K1, V, logits.dtype, n, splits, logits.device)(logits, tok, n_acc, drawn, inv_temperature)


def commit_top_logprobs(top_id: torch.Tensor, top_lp: torch.Tensor, seq_len: torch.Tensor, n_commit: torch.Tensor,
                        out_id: torch.Tensor, out_lp: torch.Tensor, max_len: Optional[int] = None) -> None:
    """The top-N rows of a step follow its commit (asd_commit_top_logprobs): out[b, seq_len[b] - n_commit[b] + j] = top[b, j]
    for j < n_commit[b], with seq_len / n_commit as asd_commit_step_lp / asd_commit_step_stop left them.  top_id i32 / top_lp
    f32 [B, K1, N]; out_id i32 / out_lp f32 [B, max_len, N], contiguous; bits are copied."""
    if top_id.dim() != 3 or top_lp.shape != top_id.shape:
        raise ValueError("top_id and top_lp must both be [B, K1, N]")
    Bv, K1, N = top_id.shape
    cap = out_id.shape[1] if max_len is None else int(max_len)
    if tuple(out_id.shape) != (Bv, cap, N) or out_lp.shape != out_id.shape:
        raise ValueError("out_id and out_lp must both be [B, max_len, N]")
    if seq_len.shape != (Bv,) or n_commit.shape != (Bv,):
        raise ValueError("seq_len and n_commit must be [B] int32")
    rc = _lib().asd_commit_top_logprobs(_dev(top_id, "top_id", torch.int32), _dev(top_lp, "top_lp", torch.float32),
                                        _dev(seq_len, "seq_len", torch.int32), _dev(n_commit, "n_commit", torch.int32), Bv, K1, N,
                                        _dev(out_id, "out_id", torch.int32), _dev(out_lp, "out_lp", torch.float32), cap, _stream())
    B.check("asd_commit_top_logprobs", rc)


# ------------------------------------------------------------------------------- per-request seeds (SamplingParams(seed=...))
def step_uniforms(seeds: torch.Tensor, step: int, stage: int, r_draft: Optional[torch.Tensor] = None,
                  u: Optional[torch.Tensor] = None, r_commit: Optional[torch.Tensor] = None) -> None:
    """Every uniform of a decoding step in one launch (asd_step_uniforms): Philox4x32-10 with key seeds[b] (int64 [B], read as
    uint64) and counter (step, k, stage, 0).  r_draft f32 [K_draft, B]: the proposal uniform of slot k; u f32 [B, K_accept]: the
    accept uniform of slot k; r_commit f32 [B]: the commit uniform.  An output left None is not written; at least one is
    given.  Values lie in [0, 1) and depend on (seeds[b], step, stage, k) alone."""
    if seeds.dim() != 1:
        raise ValueError("seeds must be int64 [B]")
    Bv = seeds.shape[0]
    if not 0 <= int(step) < 2 ** 32 or not 0 <= int(stage) < 2 ** 32:
        raise ValueError("step and stage must lie in [0, 2^32)")
    if r_draft is not None and (r_draft.dim() != 2 or r_draft.shape[1] != Bv):
        raise ValueError("r_draft must be float32 [K_draft, B]")
    if u is not None and (u.dim() != 2 or u.shape[0] != Bv):
        raise ValueError("u must be float32 [B, K_accept]")
    if r_commit is not None and tuple(r_commit.shape) != (Bv,):
        raise ValueError("r_commit must be float32 [B]")
    rc = _lib().asd_step_uniforms(_dev(seeds, "seeds", torch.int64), int(step), int(stage), Bv,
                                  0 if r_draft is None else r_draft.shape[0], 0 if u is None else u.shape[1],
                                  _opt(r_draft, "r_draft", torch.float32), _opt(u, "u", torch.float32),
                                  _opt(r_commit, "r_commit", torch.float32), _stream())
    B.check("asd_step_uniforms", rc)


# ------------------------------------------------------------------------------- logit edits (logit_bias, banned ids, min_tokens)
MAX_LOGIT_EDITS = B.MAX_LOGIT_EDITS
EDIT_FOREVER = 2 ** 31 - 1                   # `until` of a permanent ban


@dataclass
class LogitEdits:
    """The entry arrays of asd_logit_edit_rows on the device (pack_logit_edits): edit_id i32 [n], edit_bias f32 [n],
    edit_until i32 [n]; row_first i32 [B+1], or None when every row owns the entries [0, n) (n_shared = n)."""
    edit_id: torch.Tensor
    edit_bias: torch.Tensor
    edit_until: torch.Tensor
    row_first: Optional[torch.Tensor]
    n: int                                   # entries uploaded
    B: int                                   # rows the lists were packed for


def check_logit_edit_rows(rows):
    """The host side of pack_logit_edits: `rows` = one list of (id, bias, until) per batch row -> (flat entries, row_first list
    or None when all rows hold equal lists).  Inside a row the ids must be distinct
    (the kernel's packing contract), at most MAX_LOGIT_EDITS of them; a bias is finite; 0 <= until <= INT32_MAX."""
    lists = [[(int(i), float(b), int(u)) for i, b, u in r] for r in rows]
    for r, entries in enumerate(lists):
        if len(entries) > MAX_LOGIT_EDITS:
            raise ValueError(f"row {r} owns {len(entries)} logit edits, at most {MAX_LOGIT_EDITS}")
        if len({e[0] for e in entries}) != len(entries):
            raise ValueError(f"the logit edits of row {r} name a token id twice")
        for i, b, u in entries:
            if not -2 ** 31 <= i < 2 ** 31 or not 0 <= u <= EDIT_FOREVER:
                raise ValueError("logit edit ids must fit int32 and `until` must lie in [0, 2^31)")
            if b != b or b in (float("inf"), float("-inf")):
                raise ValueError("a logit bias must be finite")
    if lists and all(r == lists[0] for r in lists):
        return lists[0], None
    first = [0]
    for entries in lists:
        first.append(first[-1] + len(entries))
    return [e for entries in lists for e in entries], first


def pack_logit_edits(rows, device) -> LogitEdits:
    """The entry arrays of logit_edit_rows from host lists, checked BEFORE anything is uploaded: `rows` holds one list of
    (id, bias, until) per batch row (a row's list may be empty).  When all rows hold equal lists one copy is uploaded and
    row_first is None (the way pack_stop_sequences treats a shared list)."""
    rows = list(rows)
    flat, first = check_logit_edit_rows(rows)
    return LogitEdits(torch.tensor([e[0] for e in flat], dtype=torch.int32).to(device),
                      torch.tensor([e[1] for e in flat], dtype=torch.float32).to(device),
                      torch.tensor([e[2] for e in flat], dtype=torch.int32).to(device),
                      None if first is None else torch.tensor(first, dtype=torch.int32).to(device), len(flat), len(rows))


def logit_edit_rows(logits: torch.Tensor, edits: LogitEdits, seq_len: torch.Tensor, start: int, offset: int = 0) -> torch.Tensor:
    """Edit `logits` in place (asd_logit_edit_rows) and return it: [B, V] or [B, K1, V], bf16 / f16 / f32, any sequence / row
    stride with unit stride along V.  For every entry (id, bias, until) of row b and every position j, with
    g = seq_len[b] - start + offset + j: logits[b, j, id] = -inf while g < until, else += bias (one rounding; bias 0 stores
    nothing).  seq_len i32 [B]: the step's lengths BEFORE its commit; start: the prompt length."""
    if not isinstance(logits, torch.Tensor) or not logits.is_cuda or logits.dtype not in _DTYPE_CODE:
        raise ValueError("logits must be a bf16 / f16 / f32 CUDA (HIP) tensor; this package has no CPU path")
    view = logits[:, None] if logits.dim() == 2 else logits
    if view.dim() != 3 or (view.shape[2] > 1 and view.stride(2) != 1):
        raise ValueError("logits must be [B, V] or [B, K1, V] with unit stride along V")
    Bv, K1, V = view.shape
    if edits.B != Bv or tuple(seq_len.shape) != (Bv,):
        raise ValueError(f"the edits were packed for {edits.B} rows and seq_len must be int32 [B]; logits have {Bv} rows")
    ld_seq, ld_row = _logit_strides(view, K1)
    rc = _lib().asd_logit_edit_rows(view.data_ptr(), _DTYPE_CODE[view.dtype], ld_seq, ld_row, Bv, K1, V,
                                    _dev(edits.edit_id, "edit_id", torch.int32), _dev(edits.edit_bias, "edit_bias", torch.float32),
                                    _dev(edits.edit_until, "edit_until", torch.int32), _opt(edits.row_first, "row_first", torch.int32),
                                    edits.n, _dev(seq_len, "seq_len", torch.int32), int(start), int(offset), _stream())
    B.check("asd_logit_edit_rows", rc)
    return logits


# ------------------------------------------------------------------------------- token masks (allowed_token_ids)
@dataclass
class TokenMasks:
    """The mask arrays of asd_logit_mask_rows on the device (pack_token_masks): bits i32 [R, W], W = (V + 31) // 32, bit
    v & 31 of word v >> 5 set = token v is kept; mask_row i32 [B] (-1: the row has no list and is not touched), or None when
    every row uses mask 0."""
    bits: torch.Tensor
    mask_row: Optional[torch.Tensor]
    R: int                                   # distinct masks uploaded
    B: int                                   # rows the masks were packed for
    V: int


def check_token_mask_rows(rows, V: int):
    """The host side of pack_token_masks: `rows` = one sorted tuple of allowed ids, or None, per batch row -> (bits: numpy
    uint32 [R, W], mask_row: list of B ints with -1 for None, or None when every row uses mask 0).  Equal lists share one
    mask, so R <= B."""
    V = int(V)
    if V < 1:
        raise ValueError("V must be >= 1")
    W = (V + 31) // 32
    index, masks, mask_row = {}, [], []
    for r, ids in enumerate(rows):
        if ids is None:
            mask_row.append(-1)
            continue
        key = tuple(int(t) for t in ids)
        if key not in index:
            a = np.asarray(key, dtype=np.int64)
            if a.size and (a.min() < 0 or a.max() >= V):
                raise ValueError(f"the allowed token ids of row {r} must lie in [0, {V})")
            words = np.zeros(W, dtype=np.uint32)
            np.bitwise_or.at(words, a >> 5, np.uint32(1) << (a & 31).astype(np.uint32))
            index[key] = len(masks)
            masks.append(words)
        mask_row.append(index[key])
    bits = np.stack(masks) if masks else np.zeros((0, W), dtype=np.uint32)
    return bits, (None if mask_row and all(m == 0 for m in mask_row) else mask_row)


def pack_token_masks(rows, V: int, device) -> TokenMasks:
    """The bitmasks of logit_mask_rows from host lists: `rows` holds one sorted tuple of allowed token ids per batch row, or
    None for a row without a list.  The bits are built with numpy on the host and uploaded once; equal lists share one mask."""
    rows = list(rows)
    bits, mask_row = check_token_mask_rows(rows, V)
    return TokenMasks(torch.from_numpy(bits.view(np.int32)).to(device),
                      None if mask_row is None else torch.tensor(mask_row, dtype=torch.int32).to(device),
                      int(bits.shape[0]), len(rows), int(V))


def logit_mask_rows(logits: torch.Tensor, masks: TokenMasks) -> torch.Tensor:
    """Mask `logits` in place (asd_logit_mask_rows) and return it: [B, V] or [B, K1, V], bf16 / f16 / f32, any sequence / row
    stride with unit stride along V.  Element v of every position of row b becomes -inf where bit v of the row's mask is
    clear; a row without a list (mask_row -1) and everything else in the allocation keep their bits."""
    if not isinstance(logits, torch.Tensor) or not logits.is_cuda or logits.dtype not in _DTYPE_CODE:
        raise ValueError("logits must be a bf16 / f16 / f32 CUDA (HIP) tensor; this package has no CPU path")
    view = logits[:, None] if logits.dim() == 2 else logits
    if view.dim() != 3 or (view.shape[2] > 1 and view.stride(2) != 1):
        raise ValueError("logits must be [B, V] or [B, K1, V] with unit stride along V")
    Bv, K1, V = view.shape
    if masks.B != Bv or masks.V != V:
        raise ValueError(f"the masks were packed for {masks.B} rows of {masks.V} tokens; logits have {Bv} rows of {V}")
    if tuple(masks.bits.shape) != (masks.R, (V + 31) // 32):
        raise ValueError("mask bits must be int32 [R, (V + 31) // 32]")
    ld_seq, ld_row = _logit_strides(view, K1)
    rc = _lib().asd_logit_mask_rows(view.data_ptr(), _DTYPE_CODE[view.dtype], ld_seq, ld_row, Bv, K1, V,
                                    _dev(masks.bits, "mask bits", torch.int32), masks.R,
                                    _opt(masks.mask_row, "mask_row", torch.int32), _stream())
    B.check("asd_logit_mask_rows", rc)
    return logits


# ------------------------------------------------------------------------------- stateful penalties (repetition / presence / frequency)
@dataclass
class Penalties:
    """The state of asd_penalty_rows / asd_penalty_commit on the device (pack_penalties): seen i32 [B, W], W = (V + 31) // 32,
    bit v & 31 of word v >> 5 set = token v occurs in the row's prompt or among its committed generated tokens; counts i32
    [B, V], the occurrences among the committed generated tokens; params f32 [B, 3] = (rep, pres, freq)."""
    seen: torch.Tensor
    counts: torch.Tensor
    params: torch.Tensor
    B: int                                   # rows the state was packed for
    V: int


def check_penalty_rows(rep, pres, freq, prompt_ids, V: int):
    """The host side of pack_penalties -> (seen bits: numpy uint32 [B, W] with the bits of every row's prompt ids set, params:
    numpy float32 [B, 3]).  `prompt_ids`: one sequence of token ids in [0, V) per row -- the real prompt, without padding."""
    V = int(V)
    if V < 1:
        raise ValueError("V must be >= 1")
    rows = [np.asarray(list(r), dtype=np.int64).reshape(-1) for r in prompt_ids]
    if not len(rep) == len(pres) == len(freq) == len(rows):
        raise ValueError("rep, pres, freq and prompt_ids must hold one entry per row")
    params = np.stack([np.asarray(v, dtype=np.float32).reshape(-1) for v in (rep, pres, freq)], 1) if rows else \
        np.zeros((0, 3), dtype=np.float32)
    if not np.isfinite(params).all() or (params[:, 0] <= 0).any():
        raise ValueError("penalties must be finite and the repetition penalty > 0")
    bits = np.zeros((len(rows), (V + 31) // 32), dtype=np.uint32)
    for r, a in enumerate(rows):
        if a.size and (a.min() < 0 or a.max() >= V):
            raise ValueError(f"the prompt ids of row {r} must lie in [0, {V})")
        np.bitwise_or.at(bits[r], a >> 5, np.uint32(1) << (a & 31).astype(np.uint32))
    return bits, np.ascontiguousarray(params)


def pack_penalties(rep, pres, freq, prompt_ids, V: int, device) -> Penalties:
    """The state of penalty_rows / penalty_commit at the start of a generation: every row's (rep, pres, freq), the seen bits of
    its prompt (built with numpy on the host, uploaded once) and counts of zero."""
    bits, params = check_penalty_rows(rep, pres, freq, prompt_ids, V)
    return Penalties(torch.from_numpy(bits.view(np.int32)).to(device), torch.zeros((bits.shape[0], int(V)), dtype=torch.int32, device=device),
                     torch.from_numpy(params).to(device), int(bits.shape[0]), int(V))


def penalty_rows(logits: torch.Tensor, pen: Penalties, step_tok: Optional[torch.Tensor] = None, n_prev: int = 0) -> torch.Tensor:
    """Penalise `logits` in place (asd_penalty_rows) and return it: [B, V] or [B, K1, V], bf16 / f16 / f32, any sequence / row
    stride with unit stride along V.  step_tok i32 [B, n_tok] (unit stride along the proposals) or None: position j of row b
    sees step_tok[b, :n_prev + j] on top of the row's state."""
    if not isinstance(logits, torch.Tensor) or not logits.is_cuda or logits.dtype not in _DTYPE_CODE:
        raise ValueError("logits must be a bf16 / f16 / f32 CUDA (HIP) tensor; this package has no CPU path")
    view = logits[:, None] if logits.dim() == 2 else logits
    if view.dim() != 3 or (view.shape[2] > 1 and view.stride(2) != 1):
        raise ValueError("logits must be [B, V] or [B, K1, V] with unit stride along V")
    Bv, K1, V = view.shape
    if pen.B != Bv or pen.V != V:
        raise ValueError(f"the penalties were packed for {pen.B} rows of {pen.V} tokens; logits have {Bv} rows of {V}")
    if tuple(pen.seen.shape) != (Bv, (V + 31) // 32) or tuple(pen.counts.shape) != (Bv, V) or tuple(pen.params.shape) != (Bv, 3):
        raise ValueError("the state must be seen i32 [B, (V + 31) // 32], counts i32 [B, V] and params f32 [B, 3]")
    ld_tok = n_tok = 0
    if step_tok is None:
        if n_prev != 0:
            raise ValueError("n_prev must be 0 without step_tok")
    else:
        if not step_tok.is_cuda or step_tok.dtype != torch.int32 or step_tok.dim() != 2 or step_tok.shape[0] != Bv or \
                (step_tok.shape[1] > 1 and step_tok.stride(1) != 1):
            raise ValueError("step_tok must be a CUDA int32 [B, n_tok] tensor with unit stride along the proposals")
        n_tok = step_tok.shape[1]
        ld_tok = step_tok.stride(0) if Bv > 1 else n_tok
        if not 0 <= int(n_prev) or int(n_prev) + K1 - 1 > n_tok or ld_tok < n_tok:
            raise ValueError(f"position {K1 - 1} would see {int(n_prev) + K1 - 1} proposals; step_tok holds {n_tok}")
    ld_seq, ld_row = _logit_strides(view, K1)
    rc = _lib().asd_penalty_rows(view.data_ptr(), _DTYPE_CODE[view.dtype], ld_seq, ld_row, Bv, K1, V,
                                 _dev(pen.seen, "seen", torch.int32), _dev(pen.counts, "counts", torch.int32),
                                 _dev(pen.params, "params", torch.float32), None if step_tok is None else step_tok.data_ptr(),
                                 ld_tok, n_tok, int(n_prev), _stream())
    B.check("asd_penalty_rows", rc)
    return logits


def penalty_commit(tokens: torch.Tensor, seq_len: torch.Tensor, n_commit: torch.Tensor, pen: Penalties,
                   max_len: Optional[int] = None) -> None:
    """The step's committed tokens enter the state (asd_penalty_commit), behind the step's commit: for the n_commit[b] tokens
    at tokens[b, seq_len[b] - n_commit[b] : seq_len[b]], counts grows by each token's multiplicity and its seen bit is set.
    tokens i32 [B, >= max_len] contiguous; seq_len / n_commit i32 [B] as the commit left them."""
    if tokens.dim() != 2:
        raise ValueError("tokens must be int32 [B, max_len]")
    Bv = tokens.shape[0]
    cap = tokens.shape[1] if max_len is None else int(max_len)
    if pen.B != Bv or tokens.shape[1] < cap or tuple(seq_len.shape) != (Bv,) or tuple(n_commit.shape) != (Bv,):
        raise ValueError(f"the penalties were packed for {pen.B} rows; tokens must be [B, >= max_len], seq_len and n_commit [B]")
    rc = _lib().asd_penalty_commit(_dev(tokens, "tokens", torch.int32), tokens.shape[1], _dev(seq_len, "seq_len", torch.int32),
                                   _dev(n_commit, "n_commit", torch.int32), Bv, pen.V, cap, _dev(pen.seen, "seen", torch.int32),
                                   _dev(pen.counts, "counts", torch.int32), _stream())
    B.check("asd_penalty_commit", rc)


# ------------------------------------------------------------------------------- bad words (multi-token bans)
@dataclass
class BadWords:
    """The word tables of asd_bad_words_rows on the device (pack_bad_words): word_tok i32 [n, MAX_BAD_WORD_LEN], word_n i32 [n];
    row_first i32 [B+1], or None when every row owns the words [0, n) (n_shared = n)."""
    word_tok: torch.Tensor
    word_n: torch.Tensor
    row_first: Optional[torch.Tensor]
    n: int                                   # words uploaded
    B: int                                   # rows the lists were packed for


def check_bad_word_rows(rows):
    """The host side of pack_bad_words: `rows` = one list of words per batch row, a word 1..MAX_BAD_WORD_LEN token ids, at most
    MAX_BAD_WORDS per row -> (flat words, row_first list or None when all rows hold equal lists)."""
    lists = [[tuple(int(t) for t in w) for w in r] for r in rows]
    for r, words in enumerate(lists):
        if len(words) > B.MAX_BAD_WORDS:
            raise ValueError(f"row {r} owns {len(words)} bad words, at most {B.MAX_BAD_WORDS}")
        for w in words:
            if not 1 <= len(w) <= B.MAX_BAD_WORD_LEN:
                raise ValueError(f"a bad word holds 1..{B.MAX_BAD_WORD_LEN} token ids, got {len(w)}")
            if any(not -2 ** 31 <= t < 2 ** 31 for t in w):
                raise ValueError("bad word token ids must fit int32")
    if lists and all(r == lists[0] for r in lists):
        return lists[0], None
    first = [0]
    for words in lists:
        first.append(first[-1] + len(words))
    return [w for words in lists for w in words], first


def pack_bad_words(rows, device) -> BadWords:
    """The word tables of bad_words_rows from host lists, checked BEFORE anything is uploaded: `rows` holds one list of words per
    batch row (a row's list may be empty).  When all rows hold equal lists one copy is uploaded and row_first is None (the
    way pack_logit_edits treats a shared list)."""
    rows = list(rows)
    flat, first = check_bad_word_rows(rows)
    tok = np.zeros((len(flat), B.MAX_BAD_WORD_LEN), dtype=np.int32)
    for i, w in enumerate(flat):
        tok[i, :len(w)] = w
    return BadWords(torch.from_numpy(tok).to(device), torch.tensor([len(w) for w in flat], dtype=torch.int32).to(device),
                    None if first is None else torch.tensor(first, dtype=torch.int32).to(device), len(flat), len(rows))


def bad_words_rows(logits: torch.Tensor, words: BadWords, tokens: torch.Tensor, seq_len: torch.Tensor, start: int, max_len: int,
                   step_tok: Optional[torch.Tensor] = None, n_prev: int = 0) -> torch.Tensor:
    """Ban in place (asd_bad_words_rows) and return `logits`: [B, V] or [B, K1, V], bf16 / f16 / f32, any sequence / row stride
    with unit stride along V.  The last id of a word of row b becomes -inf at position j when the word's other ids are the end
    of the row's history tokens[b, start:seq_len[b]] ++ step_tok[b, :n_prev + j].  tokens i32 [B, >= max_len] contiguous;
    seq_len i32 [B]: the step's lengths BEFORE its commit; start: the prompt length; step_tok i32 [B, n_tok] (unit stride along
    the proposals) or None."""
    if not isinstance(logits, torch.Tensor) or not logits.is_cuda or logits.dtype not in _DTYPE_CODE:
        raise ValueError("logits must be a bf16 / f16 / f32 CUDA (HIP) tensor; this package has no CPU path")
    view = logits[:, None] if logits.dim() == 2 else logits
    if view.dim() != 3 or (view.shape[2] > 1 and view.stride(2) != 1):
        raise ValueError("logits must be [B, V] or [B, K1, V] with unit stride along V")
    Bv, K1, V = view.shape
    if words.B != Bv or tuple(seq_len.shape) != (Bv,):
        raise ValueError(f"the bad words were packed for {words.B} rows and seq_len must be int32 [B]; logits have {Bv} rows")
    if tokens.dim() != 2 or tokens.shape[0] != Bv or not 0 <= int(start) <= int(max_len) <= tokens.shape[1]:
        raise ValueError(f"tokens must be int32 [B, >= max_len] and 0 <= start <= max_len, got {tuple(tokens.shape)}, {start}, {max_len}")
    ld_tok = n_tok = 0
    if step_tok is None:
        if n_prev != 0:
            raise ValueError("n_prev must be 0 without step_tok")
    else:
        if not step_tok.is_cuda or step_tok.dtype != torch.int32 or step_tok.dim() != 2 or step_tok.shape[0] != Bv or \
                (step_tok.shape[1] > 1 and step_tok.stride(1) != 1):
            raise ValueError("step_tok must be a CUDA int32 [B, n_tok] tensor with unit stride along the proposals")
        n_tok = step_tok.shape[1]
        ld_tok = step_tok.stride(0) if Bv > 1 else n_tok
        if not 0 <= int(n_prev) or int(n_prev) + K1 - 1 > n_tok or ld_tok < n_tok:
            raise ValueError(f"position {K1 - 1} would see {int(n_prev) + K1 - 1} proposals; step_tok holds {n_tok}")
    ld_seq, ld_row = _logit_strides(view, K1)
    rc = _lib().asd_bad_words_rows(view.data_ptr(), _DTYPE_CODE[view.dtype], ld_seq, ld_row, Bv, K1, V,
                                   _dev(words.word_tok, "word_tok", torch.int32), _dev(words.word_n, "word_n", torch.int32),
                                   _opt(words.row_first, "row_first", torch.int32), words.n,
                                   _dev(tokens, "tokens", torch.int32), tokens.shape[1], _dev(seq_len, "seq_len", torch.int32),
                                   int(start), int(max_len), None if step_tok is None else step_tok.data_ptr(), ld_tok, n_tok,
                                   int(n_prev), _stream())
    B.check("asd_bad_words_rows", rc)
    return logits


# ------------------------------------------------------------------------------- guided decoding (token automata)
@dataclass
class TokenFsm:
    """The tables of asd_fsm_mask_rows / asd_fsm_advance / asd_fsm_commit on the device (pack_fsm): state_first i32 [S + 1],
    edge_tok / edge_next i32 [max(E, 1)], state_other i32 [S], state_bits i32 [S, W] with W = (V + 31) // 32 (the allow-list's
    bit layout), and the state columns pos_state i32 [B, ld_state]: column 0 the state behind a row's committed tokens (-1:
    the row has no automaton), column i the state behind the proposals 0 .. i - 1 of the running step."""
    state_first: torch.Tensor
    edge_tok: torch.Tensor
    edge_next: torch.Tensor
    state_other: torch.Tensor
    state_bits: torch.Tensor
    pos_state: torch.Tensor
    S: int
    E: int
    B: int                                   # rows the state was packed for
    V: int
    ld_state: int


def check_fsm_tables(state_first, edge_tok, edge_next, state_other, starts, V: int):
    """The host side of pack_fsm: the CSR tables as include/asd_hip.h states them, checked, -> (the four tables as int32
    arrays, state_bits: numpy uint32 [S, W] built FROM them -- bit v set = token v has a transition that is not -1 -- and the
    rows' start states)."""
    V = int(V)
    if V < 1:
        raise ValueError("V must be >= 1")
    first, tok, nxt, other = (np.ascontiguousarray(a, dtype=np.int32).reshape(-1) for a in (state_first, edge_tok, edge_next, state_other))
    S, E = other.size, tok.size
    if first.size != S + 1 or nxt.size != E or (S and (first[0] != 0 or first[-1] != E)) or (np.diff(first) < 0).any():
        raise ValueError("state_first must be S + 1 ascending CSR offsets from 0 to E, edge_tok and edge_next [E], state_other [S]")
    if E and (tok.min() < 0 or tok.max() >= V):
        raise ValueError(f"edge token ids must lie in [0, {V})")
    if (E and (nxt.min() < -1 or nxt.max() >= S)) or (S and (other.min() < -1 or other.max() >= S)):
        raise ValueError("next states must lie in [-1, S)")
    starts = [int(s) for s in starts]
    if any(not -1 <= s < S for s in starts):
        raise ValueError("a row's start state must lie in [0, S), or be -1 for a row without an automaton")
    W = (V + 31) // 32
    bits = np.zeros((S, W), dtype=np.uint32)
    keep = np.zeros(W * 32, dtype=bool)                      # one state's allowed set, padded to whole words (the padding stays clear)
    for s in range(S):
        ids, to = tok[first[s]:first[s + 1]], nxt[first[s]:first[s + 1]]
        if ids.size > 1 and (np.diff(ids) <= 0).any():
            raise ValueError(f"the edge token ids of state {s} must be ascending and distinct")
        keep[:V] = other[s] >= 0
        keep[ids] = to >= 0
        bits[s] = np.packbits(keep, bitorder="little").view("<u4")       # bit v & 31 of word v >> 5: one vectorised step
    return first, tok, nxt, other, bits, starts


def pack_fsm(fsm, ld_state: int, device) -> TokenFsm:
    """The device side of one call's automata: `fsm` carries state_first / edge_tok / edge_next / state_other (numpy), the rows'
    `starts` and `V` (serving/guided.py::compile_rows).  state_bits is built here from the other tables; everything is uploaded
    once, and pos_state [B, ld_state] starts with every column at the row's start state (-1 for a row without an automaton)."""
    first, tok, nxt, other, bits, starts = check_fsm_tables(fsm.state_first, fsm.edge_tok, fsm.edge_next, fsm.state_other, fsm.starts, fsm.V)
    ld_state = int(ld_state)
    if ld_state < 1:
        raise ValueError("ld_state must be >= 1")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)             # noqa: E731
    pad = lambda a: a if a.size else np.zeros(1, np.int32)                          # noqa: E731  (E == 0: never read)
    pos = np.repeat(np.asarray(starts, dtype=np.int32).reshape(-1, 1), ld_state, axis=1)
    return TokenFsm(up(first), up(pad(tok)), up(pad(nxt)), up(other), up(bits.view(np.int32)), up(pos), int(other.size), int(tok.size),
                    len(starts), int(fsm.V), ld_state)


def _fsm_tables(f: TokenFsm):
    return (_dev(f.state_first, "state_first", torch.int32), _dev(f.edge_tok, "edge_tok", torch.int32),
            _dev(f.edge_next, "edge_next", torch.int32), _dev(f.state_other, "state_other", torch.int32), f.S, f.E, f.V)


def _fsm_state(f: TokenFsm) -> int:
    if tuple(f.pos_state.shape) != (f.B, f.ld_state) or not f.pos_state.is_contiguous():
        raise ValueError("pos_state must be a contiguous int32 [B, ld_state] tensor")
    return _dev(f.pos_state, "pos_state", torch.int32)


def fsm_mask_rows(logits: torch.Tensor, fsm: TokenFsm, first: int = 0) -> torch.Tensor:
    """Mask `logits` in place (asd_fsm_mask_rows) and return it: [B, V] or [B, K1, V], bf16 / f16 / f32, any sequence / row
    stride with unit stride along V.  Position j of row b is masked with the bits of state pos_state[b, first + j]; a row
    without an automaton (-1) and everything else in the allocation keep their bits."""
    if not isinstance(logits, torch.Tensor) or not logits.is_cuda or logits.dtype not in _DTYPE_CODE:
        raise ValueError("logits must be a bf16 / f16 / f32 CUDA (HIP) tensor; this package has no CPU path")
    view = logits[:, None] if logits.dim() == 2 else logits
    if view.dim() != 3 or (view.shape[2] > 1 and view.stride(2) != 1):
        raise ValueError("logits must be [B, V] or [B, K1, V] with unit stride along V")
    Bv, K1, V = view.shape
    if fsm.B != Bv or fsm.V != V:
        raise ValueError(f"the automata were packed for {fsm.B} rows of {fsm.V} tokens; logits have {Bv} rows of {V}")
    if tuple(fsm.state_bits.shape) != (fsm.S, (V + 31) // 32):
        raise ValueError("state_bits must be int32 [S, (V + 31) // 32]")
    if not 0 <= int(first) or int(first) + K1 > fsm.ld_state:
        raise ValueError(f"positions {int(first)} .. {int(first) + K1 - 1} need that many state columns; pos_state holds {fsm.ld_state}")
    ld_seq, ld_row = _logit_strides(view, K1)
    rc = _lib().asd_fsm_mask_rows(view.data_ptr(), _DTYPE_CODE[view.dtype], ld_seq, ld_row, Bv, K1, V,
                                  _dev(fsm.state_bits, "state_bits", torch.int32), fsm.S, _fsm_state(fsm), fsm.ld_state, int(first),
                                  _stream())
    B.check("asd_fsm_mask_rows", rc)
    return logits


def fsm_advance(fsm: TokenFsm, step_tok: torch.Tensor, k: int) -> None:
    """pos_state[b, k + 1] = delta(pos_state[b, k], step_tok[b, k]) (asd_fsm_advance): behind proposal k of a step.  step_tok
    i32 [B, n_tok] with unit stride along the proposals."""
    if not step_tok.is_cuda or step_tok.dtype != torch.int32 or step_tok.dim() != 2 or step_tok.shape[0] != fsm.B or \
            (step_tok.shape[1] > 1 and step_tok.stride(1) != 1):
        raise ValueError("step_tok must be a CUDA int32 [B, n_tok] tensor with unit stride along the proposals")
    n_tok = step_tok.shape[1]
    ld_tok = step_tok.stride(0) if fsm.B > 1 else n_tok
    if not 0 <= int(k) < n_tok or int(k) + 1 >= fsm.ld_state or ld_tok < n_tok:
        raise ValueError(f"proposal {int(k)} needs step_tok column {int(k)} of {n_tok} and state column {int(k) + 1} of {fsm.ld_state}")
    rc = _lib().asd_fsm_advance(*_fsm_tables(fsm), _fsm_state(fsm), fsm.ld_state, fsm.B, int(k), step_tok.data_ptr(), ld_tok, n_tok,
                                _stream())
    B.check("asd_fsm_advance", rc)


def fsm_commit(fsm: TokenFsm, tokens: torch.Tensor, seq_len: torch.Tensor, n_commit: torch.Tensor, max_len: Optional[int] = None) -> None:
    """Behind the step's commit (asd_fsm_commit): for a row with c = n_commit[b] > 0, pos_state[b, 0] =
    delta(pos_state[b, c - 1], tokens[b, seq_len[b] - 1]); a finished row (c == 0) keeps its state.  tokens i32 [B, >= max_len]
    contiguous; seq_len / n_commit i32 [B] as the commit left them."""
    if tokens.dim() != 2:
        raise ValueError("tokens must be int32 [B, max_len]")
    cap = tokens.shape[1] if max_len is None else int(max_len)
    if fsm.B != tokens.shape[0] or not 1 <= cap <= tokens.shape[1] or tuple(seq_len.shape) != (fsm.B,) or tuple(n_commit.shape) != (fsm.B,):
        raise ValueError(f"the automata were packed for {fsm.B} rows; tokens must be [B, >= max_len >= 1], seq_len and n_commit [B]")
    rc = _lib().asd_fsm_commit(*_fsm_tables(fsm), _fsm_state(fsm), fsm.ld_state, fsm.B, _dev(tokens, "tokens", torch.int32),
                               tokens.shape[1], _dev(seq_len, "seq_len", torch.int32), _dev(n_commit, "n_commit", torch.int32), cap,
                               _stream())
    B.check("asd_fsm_commit", rc)


# ------------------------------------------------------------------------------- no repeated n-gram (no_repeat_ngram_size)
@dataclass
class NoRepeatNgram:
    """The per-row arguments of asd_no_repeat_ngram_rows on the device (pack_no_repeat_ngram): ngram_n i32 [B] (0: the row is
    off), or None when every row has n_shared; row_start i32 [B], the index of every row's first real prompt id behind the
    left-padding, or None when no row has a prompt id (row_start = P everywhere)."""
    ngram_n: Optional[torch.Tensor]
    row_start: Optional[torch.Tensor]
    n_shared: int                            # every row's n when ngram_n is None
    P: int                                   # the padded prompt length the rows were packed for (`start` of the calls)
    B: int                                   # rows the arguments were packed for


def check_no_repeat_ngram_rows(ns, prompt_lens, P: int):
    """The host side of pack_no_repeat_ngram: every row's n in [0, MAX_NGRAM] and its count of real prompt ids in [0, P] ->
    (ngram_n list, row_start list) with row_start[b] = P - prompt_lens[b]."""
    ns, lens = list(ns), list(prompt_lens)
    if len(ns) != len(lens):
        raise ValueError(f"{len(ns)} n-gram sizes for {len(lens)} prompt lengths")
    if isinstance(P, bool) or not isinstance(P, (int, np.integer)) or not 0 <= int(P) < 2 ** 31:
        raise ValueError(f"P must be an integer in [0, 2^31), got {P!r}")
    for b, (n, m) in enumerate(zip(ns, lens)):
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 0 <= int(n) <= B.MAX_NGRAM:
            raise ValueError(f"row {b}: the n-gram size must be an integer in [0, {B.MAX_NGRAM}], got {n!r}")
        if isinstance(m, bool) or not isinstance(m, (int, np.integer)) or not 0 <= int(m) <= int(P):
            raise ValueError(f"row {b}: the prompt length must be an integer in [0, {int(P)}], got {m!r}")
    return [int(n) for n in ns], [int(P) - int(m) for m in lens]


def pack_no_repeat_ngram(ns, prompt_lens, P: int, device) -> NoRepeatNgram:
    """The per-row arguments of no_repeat_ngram_rows from host lists, checked BEFORE anything is uploaded: `ns` holds every
    row's n (0: off), `prompt_lens` its number of real prompt ids, which end at index P of the row's token buffer."""
    n_list, first = check_no_repeat_ngram_rows(ns, prompt_lens, P)
    shared = bool(n_list) and all(n == n_list[0] for n in n_list)          # one n for every row: no table (a shared list's way)
    return NoRepeatNgram(None if shared else torch.tensor(n_list, dtype=torch.int32).to(device),
                         None if all(f == int(P) for f in first) else torch.tensor(first, dtype=torch.int32).to(device),
                         n_list[0] if shared else 0, int(P), len(n_list))


def no_repeat_ngram_rows(logits: torch.Tensor, ngram: NoRepeatNgram, tokens: torch.Tensor, seq_len: torch.Tensor, max_len: int,
                         step_tok: Optional[torch.Tensor] = None, n_prev: int = 0) -> torch.Tensor:
    """Ban in place (asd_no_repeat_ngram_rows) and return `logits`: [B, V] or [B, K1, V], bf16 / f16 / f32, any sequence / row
    stride with unit stride along V.  With n = ngram.ngram_n[b] (or ngram.n_shared) and H = tokens[b, row_start[b]:seq_len[b]] ++
    step_tok[b, :n_prev + j], every token that followed an earlier occurrence of H's last n - 1 tokens becomes -inf at
    position j.  tokens i32 [B, >= max_len] contiguous; seq_len i32 [B]: the step's lengths BEFORE its commit; step_tok
    i32 [B, n_tok] (unit stride along the proposals) or None."""
    if not isinstance(logits, torch.Tensor) or not logits.is_cuda or logits.dtype not in _DTYPE_CODE:
        raise ValueError("logits must be a bf16 / f16 / f32 CUDA (HIP) tensor; this package has no CPU path")
    view = logits[:, None] if logits.dim() == 2 else logits
    if view.dim() != 3 or (view.shape[2] > 1 and view.stride(2) != 1):
        raise ValueError("logits must be [B, V] or [B, K1, V] with unit stride along V")
    Bv, K1, V = view.shape
    start = ngram.P
    if ngram.B != Bv or tuple(seq_len.shape) != (Bv,):
        raise ValueError(f"the n-gram sizes were packed for {ngram.B} rows and seq_len must be int32 [B]; logits have {Bv} rows")
    if tokens.dim() != 2 or tokens.shape[0] != Bv or not 0 <= start <= int(max_len) <= tokens.shape[1]:
        raise ValueError(f"tokens must be int32 [B, >= max_len] and 0 <= start <= max_len, got {tuple(tokens.shape)}, {start}, {max_len}")
    ld_tok = n_tok = 0
    if step_tok is None:
        if n_prev != 0:
            raise ValueError("n_prev must be 0 without step_tok")
    else:
        if not step_tok.is_cuda or step_tok.dtype != torch.int32 or step_tok.dim() != 2 or step_tok.shape[0] != Bv or \
                (step_tok.shape[1] > 1 and step_tok.stride(1) != 1):
            raise ValueError("step_tok must be a CUDA int32 [B, n_tok] tensor with unit stride along the proposals")
        n_tok = step_tok.shape[1]
        ld_tok = step_tok.stride(0) if Bv > 1 else n_tok
        if not 0 <= int(n_prev) or int(n_prev) + K1 - 1 > n_tok or ld_tok < n_tok:
            raise ValueError(f"position {K1 - 1} would see {int(n_prev) + K1 - 1} proposals; step_tok holds {n_tok}")
    ld_seq, ld_row = _logit_strides(view, K1)
    rc = _lib().asd_no_repeat_ngram_rows(view.data_ptr(), _DTYPE_CODE[view.dtype], ld_seq, ld_row, Bv, K1, V,
                                         _opt(ngram.ngram_n, "ngram_n", torch.int32), int(ngram.n_shared),
                                         _opt(ngram.row_start, "row_start", torch.int32),
                                         _dev(tokens, "tokens", torch.int32), tokens.shape[1], _dev(seq_len, "seq_len", torch.int32),
                                         start, int(max_len), None if step_tok is None else step_tok.data_ptr(), ld_tok, n_tok,
                                         int(n_prev), _stream())
    B.check("asd_no_repeat_ngram_rows", rc)
    return logits


# ------------------------------------------------------------------------------- entropy cuts (typical_p / epsilon_cutoff / eta_cutoff)
CUT_OFF, CUT_TYPICAL, CUT_EPSILON, CUT_ETA = 0, 1, 2, 3
_CUT_REC = np.dtype([("inv_t", np.float32), ("mode", np.int32), ("value", np.float32)])


@dataclass
class EntropyCut:
    """The table of asd_entropy_cut_rows on the device (pack_entropy_cut): B records {inv_t f32, mode i32, value f32} of 12
    bytes, as a uint8 [B, 12] tensor; `modes`: the host's copy of the rows' modes."""
    table: torch.Tensor
    modes: Tuple[int, ...]
    B: int


def check_entropy_cut_rows(inv_t, modes, values) -> np.ndarray:
    """The host side of pack_entropy_cut: every row's 1 / temperature (a positive finite number), mode (0 off, 1 typical,
    2 epsilon, 3 eta) and value (inside (0, 1) where the row is on) -> the records, a numpy structured array."""
    inv_t, modes, values = list(inv_t), list(modes), list(values)
    if not len(inv_t) == len(modes) == len(values):
        raise ValueError(f"{len(inv_t)} temperatures, {len(modes)} modes and {len(values)} values must describe the same rows")
    rec = np.zeros(len(modes), dtype=_CUT_REC)
    for b, (t, m, v) in enumerate(zip(inv_t, modes, values)):
        if isinstance(m, bool) or not isinstance(m, (int, np.integer)) or int(m) not in (CUT_OFF, CUT_TYPICAL, CUT_EPSILON, CUT_ETA):
            raise ValueError(f"row {b}: the mode must be 0 (off), 1 (typical), 2 (epsilon) or 3 (eta), got {m!r}")
        t32 = np.float32(t)
        if isinstance(t, bool) or not (t32 > 0.0 and t32 < np.float32(3.0e38)):
            raise ValueError(f"row {b}: 1 / temperature must be a positive finite number, got {t!r}")
        v32 = np.float32(v)
        if int(m) != CUT_OFF and (isinstance(v, bool) or not 0.0 < float(v32) < 1.0):
            raise ValueError(f"row {b}: the value of a row that is on must lie inside (0, 1), got {v!r}")
        rec[b] = (t32, int(m), v32 if int(m) != CUT_OFF else np.float32(0.0))
    return rec


def pack_entropy_cut(inv_t, modes, values, device) -> EntropyCut:
    """The table of entropy_cut_rows from host lists, checked BEFORE anything is uploaded."""
    rec = check_entropy_cut_rows(inv_t, modes, values)
    table = torch.from_numpy(rec.view(np.uint8).reshape(len(rec), _CUT_REC.itemsize).copy()).to(device)
    return EntropyCut(table, tuple(int(m) for m in rec["mode"]), len(rec))


def entropy_cut_rows(logits: torch.Tensor, cut: EntropyCut) -> torch.Tensor:
    """Cut in place (asd_entropy_cut_rows) and return `logits`: [B, V] or [B, K1, V], bf16 / f16 / f32, any sequence / row
    stride with unit stride along V.  Row (b, j) under record b: with p = softmax(x * inv_t) and its entropy H, typical-p keeps
    the smallest set of tokens closest to H in -ln p whose mass reaches the value (ties kept), epsilon cuts p < value, eta cuts
    p < min(value, sqrt(value) exp(-H)); both keep every token that ties the maximum.  A cut token becomes -inf."""
    if not isinstance(logits, torch.Tensor) or not logits.is_cuda or logits.dtype not in _DTYPE_CODE:
        raise ValueError("logits must be a bf16 / f16 / f32 CUDA (HIP) tensor; this package has no CPU path")
    view = logits[:, None] if logits.dim() == 2 else logits
    if view.dim() != 3 or (view.shape[2] > 1 and view.stride(2) != 1):
        raise ValueError("logits must be [B, V] or [B, K1, V] with unit stride along V")
    Bv, K1, V = view.shape
    if cut.B != Bv:
        raise ValueError(f"the cuts were packed for {cut.B} rows; logits have {Bv}")
    ld_seq, ld_row = _logit_strides(view, K1)
    rc = _lib().asd_entropy_cut_rows(view.data_ptr(), _DTYPE_CODE[view.dtype], Bv, K1, V, ld_seq, ld_row,
                                     _dev(cut.table, "table", torch.uint8), _stream())
    B.check("asd_entropy_cut_rows", rc)
    return logits
