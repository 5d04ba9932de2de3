"""asd_watermark_rows and asd_watermark_score on the GPU against tests/watermark_ref.py, BIT-EQUAL: the rows over the whole
allocation (a guard band in front, the tensor with its row padding, a guard band behind), the counts as integers; the raw ABI's
status codes; and the stage scenario of tests/watermark_ref.py through the kernels and the real samplers.  B = 3: row 0 has
context width 1 and gamma 0.25, row 1 is off and must stay untouched, row 2 has another key, width 3, gamma 0.5 and a delta
that clamps; its one prompt id makes positions 0 and 1 of an empty step shorter than its context."""
import numpy as np
import pytest
import torch

from tests.stage_scenario import NAMES, stage_configs
from tests.watermark_ref import ref_watermark_rows, ref_watermark_score, scenario_every_token_green

pytestmark = pytest.mark.gpu

GUARD, START, B = 128, 4, 3
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
# (V, the base's offset in elements, K1, n_prev, with step_tok, row 0's context width, row 2's damage).  Offset 0 with ld_row a
# multiple of 8 is the one-call path, offset 1 with an odd ld_row the two-call path with a shift per row; 2061 elements are 257
# units, one more than a workgroup's 256 lanes: two workgroups per row
CASES = [(5, 0, 1, 0, False, 1, None), (5, 1, 3, 2, True, 2, "h=0"), (5, 0, 3, 0, True, 3, "h=4"), (1003, 0, 3, 0, True, 1, "delta=nan"),
         (1003, 1, 3, 2, True, 2, None), (2061, 0, 1, 0, False, 2, None), (2061, 1, 3, 0, True, 3, None), (152064, 0, 1, 0, False, 1, None)]


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16).numpy().tobytes()


def _packed(K_, recs, prompt_lens, start):
    """The device records WITHOUT the host's checks (a damaged record must reach the kernel): (key, delta, thr, h) per row."""
    rec = np.zeros(len(recs), dtype=K_._WATERMARK_REC)
    for b, (key, delta, thr, h) in enumerate(recs):
        rec[b] = (0, 0, 0.0, 0) if key is None else (key & 0xFFFFFFFF, key >> 32, np.float32(delta), thr | h << 16)
    table = torch.from_numpy(rec.view(np.uint8).reshape(len(recs), 16).copy()).cuda()
    return K_.Watermark(table, torch.tensor([start - m for m in prompt_lens], dtype=torch.int32).cuda(), start, len(recs),
                        tuple(r[2] for r in recs))


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16", "f32"])
@pytest.mark.parametrize("case", CASES, ids=str)
def test_rows_are_bit_equal_to_the_reference(case, dtype):
    from asd_amd import kernels as K_
    V, off, K1, n_prev, with_tok, h0, damage = case
    ld_row = V + 11 if off else (V + 15) // 8 * 8
    h2, d2 = {"h=0": (0, 3.0e38), "h=4": (4, 3.0e38), "delta=nan": (3, float("nan"))}.get(damage, (3, 3.0e38))
    recs = [(0x0123456789ABCDEF, 2.0 if dtype != torch.float16 else 60.0, 16384, h0), (None, 0.0, 0, 0), (2 ** 64 - 1, d2, 32768, h2)]
    prompt_lens, gen = [2, 3, 1], [7, 300000, 5]                                 # committed tokens behind the prompt, the same in every row
    tokens = np.zeros((B, START + len(gen) + 2), dtype=np.int32)
    tokens[:, 1:START] = [11, 12, 13]
    seq_len = [START + len(gen), START + len(gen), START]                        # row 2: its one prompt id is all its history
    tokens[:, START:START + len(gen)] = gen
    step = np.array([[60, 61, 62, 63]] * B, dtype=np.int32)
    n = B * K1 * ld_row
    buf = (torch.randn(n + 2 * GUARD + 1, generator=torch.Generator().manual_seed(V + K1)) * 4.0).to(dtype)
    view = lambda t: t[GUARD + off:GUARD + off + n].view(B, K1, ld_row)[:, :, :V]   # noqa: E731
    big = torch.finfo(dtype).max
    view(buf)[:, :, 1], view(buf)[:, :, 3] = big, float("nan")                   # (the view writes through) the largest finite value; one NaN
    if V > 64:
        view(buf)[:, :, 60], view(buf)[:, :, 61], view(buf)[:, :, 50] = 0.75 * big, -big, float("inf")
        view(buf)[:, :, 20:41], view(buf)[:, :, V - 9:] = float("-inf"), float("-inf")
    want = buf.clone()
    ref_watermark_rows(view(want), recs, tokens, seq_len, [START - m for m in prompt_lens], START, tokens.shape[1],
                       step if with_tok else None, n_prev)
    dev = buf.cuda()
    K_.watermark_rows(view(dev), _packed(K_, recs, prompt_lens, START), torch.from_numpy(tokens).cuda(),
                      torch.tensor(seq_len, dtype=torch.int32).cuda(), tokens.shape[1], torch.from_numpy(step).cuda() if with_tok else None, n_prev)
    torch.cuda.synchronize()
    assert _bits(dev) == _bits(want)
    if V > 64:                                                                   # never vacuous: row 0 is biased, row 2 where it may be
        assert _bits(view(want)[0]) != _bits(view(buf)[0])
        assert (_bits(view(want)[2]) != _bits(view(buf)[2])) == (damage is None and K1 == 3)


def test_score_is_equal_to_the_reference():
    from asd_amd import kernels as K_
    rng = np.random.default_rng(5)
    tokens = rng.integers(0, 152064, size=(5, 300), dtype=np.int32)
    recs = [(7, 1.0, 16384, 1), (8, 1.0, 32768, 2), (None, 0.0, 0, 0), (2 ** 63 + 9, 1.0, 60000, 3), (10, 1.0, 1000, 5)]
    row_start, row_from, seq_len = [0, 10, 0, 296, 0], [0, 3, 0, 297, 0], [300, 77, 50, 300, 50]     # from at / in front of / behind row_start
    packed = _packed(K_, recs, [300 - r for r in row_start], 300)
    got = K_.watermark_score(torch.from_numpy(tokens).cuda(), packed, torch.tensor(row_from, dtype=torch.int32).cuda(),
                             torch.tensor(seq_len, dtype=torch.int32).cuda(), 300).cpu().numpy()
    want = ref_watermark_score(tokens, recs, row_start, row_from, seq_len, 300)
    assert want[:, 0].tolist() == [299, 65, 0, 1, 0] and 0 < want[0, 1] < 299
    assert got.tolist() == want.tolist()


INVALID, UNSUPPORTED, ALIGNMENT = -1, -2, -5


@pytest.mark.parametrize("kw,status", [
    (dict(B=-1), INVALID), (dict(n_prev=-1, B=0), INVALID), (dict(B=0, logits=None), 0), (dict(dtype=7, logits=None), UNSUPPORTED),
    (dict(n_tok=65, ld_tok=65), UNSUPPORTED), (dict(max_len=2 ** 31 - 2, ld_tokens=2 ** 31), UNSUPPORTED), (dict(recs=None), INVALID),
    (dict(ld_row=256), INVALID), (dict(ld_seq=513), INVALID), (dict(ld_tokens=7), INVALID), (dict(start=9), INVALID), (dict(tok=None), INVALID),
    (dict(n_prev=4), INVALID), (dict(ld_row=255, logits=2), INVALID), (dict(logits=2), ALIGNMENT), (dict(recs=2), ALIGNMENT),
    (dict(seq_len=2), ALIGNMENT), (dict(), 0)], ids=str)
def test_argument_checks_return_their_status(kw, status):
    from asd_amd import _binding, kernels as K_
    lib, V = _binding.load_library(), 257
    x = torch.randn((B, 2, V), device="cuda")
    keep = x.clone()
    packed = K_.pack_watermark([1, None, 1], [1.0] * 3, [0.5] * 3, [1] * 3, [0] * 3, 4, "cuda")
    tokens = torch.ones((B, 8), dtype=torch.int32, device="cuda")
    seq = torch.full((B,), 6, dtype=torch.int32, device="cuda")
    tok = torch.full((B, 4), 7, dtype=torch.int32, device="cuda")
    good = dict(logits=x.data_ptr(), dtype=0, ld_seq=2 * V, ld_row=V, B=B, K1=2, V=V, recs=packed.table.data_ptr(), row_start=None,
                tokens=tokens.data_ptr(), ld_tokens=8, seq_len=seq.data_ptr(), start=4, max_len=8, tok=tok.data_ptr(), ld_tok=4,
                n_tok=4, n_prev=3, stream=None)
    for name, v in kw.items():                                                   # (an int for a pointer: that many bytes off)
        good[name] = good[name] + v if name in ("logits", "recs", "seq_len") and v is not None else v
    assert lib.asd_watermark_rows(*good.values()) == status
    score = dict(tokens=tokens.data_ptr(), ld_tokens=8, row_start=None, row_from=seq.data_ptr(), seq_len=seq.data_ptr(), B=B, max_len=8,
                 recs=packed.table.data_ptr(), out=torch.zeros((B, 2), dtype=torch.int32, device="cuda").data_ptr(), stream=None)
    if kw.keys() <= {"B", "recs", "ld_tokens", "seq_len"} and "logits" not in kw:
        score.update({k: good[k] for k in kw})
        assert lib.asd_watermark_score(*score.values()) == status
    torch.cuda.synchronize()
    if kw:
        assert torch.equal(x, keep)                                              # nothing was launched
    else:
        assert torch.equal(x[1], keep[1]) and not torch.equal(x[0], keep[0]) and bool(((x == keep) | (x == keep + 1.0)).all())


@pytest.mark.parametrize("greedy", [False, True], ids=["sampled", "greedy"])
@pytest.mark.parametrize("name", NAMES[:2])                                      # stage 0, and a verifying stage
def test_scenario(name, greedy):
    from asd_amd.serving.stages import StageManager
    manager = StageManager(stage_configs(vocab=64, dtype=torch.float32))
    scenario_every_token_green(manager.get_stage(name), greedy)
    manager.ops.check_status()
