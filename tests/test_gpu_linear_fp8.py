"""X3, weight-only FP8 (csrc/linear_fp8.hip): the quantiser bit for bit against torch's CPU arithmetic, and asd_linear_fp8
against an f64 product of the SAME codes and scales -- exact operands, f32 MFMA accumulation, one f32 multiply by the row
scale (2^-24 relative, far inside the slack) and one output rounding: the bound tests/test_gpu_linear.py derives,
|y - ref| <= 2^-8 |ref| + 2e-4 (bf16) / 2^-11 |ref| + 2e-4 (f16)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

E4M3 = torch.float8_e4m3fn


def _K():
    from asd_amd import kernels
    return kernels


def _unpermute(image, N, D):
    """image -> (codes [N, D] uint8, scale [N] f32): the layout include/asd_hip.h states,
    [N/256][D/64][8 waves][2 quarters][2 halves][32 rows][16 bytes], then the scales."""
    codes = image[: N * D].view(N // 256, D // 64, 8, 2, 2, 32, 16).permute(0, 2, 5, 1, 4, 3, 6).reshape(N, D)
    return codes.contiguous(), image[N * D:].view(torch.float32).clone()


def _weights(N, D, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(N, D, generator=g) / D ** 0.5
    ties = torch.tensor([17.0, 19.0, 21.0, 23.0, 2.0 ** -10, 3 * 2.0 ** -10, 0.00341796875, 272.0, 432.0])   # midpoints of E4M3 neighbours
    w[0] = 0.0                                                          # all zero: scale 1
    w[1] = 0.75 * (torch.randint(0, 2, (D,), generator=g) * 2 - 1)      # only +-amax: every code +-448
    w[2] = torch.randn(D, generator=g) * 2.0e-5                         # |w| / scale < 2^-6 with amax 1: E4M3 subnormals
    w[2, 5] = 1.0
    w[3] = ties[torch.arange(D) % len(ties)] * (torch.randint(0, 2, (D,), generator=g) * 2 - 1)
    w[3, 7] = 448.0                                                     # scale exactly 1: the ties reach the rounding as they are
    return w.to(dtype)


def test_cpu_cast_is_rne_and_reaches_448():
    got = torch.tensor([17.0, 19.0, 2.0 ** -10, 3 * 2.0 ** -10, 448.00003, -448.00003]).to(E4M3).float()
    assert got.tolist() == [16.0, 20.0, 0.0, 2.0 ** -8, 448.0, -448.0]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("N,D", [(256, 64), (512, 192)])
def test_quantiser_is_bit_exact(N, D, dtype):
    w = _weights(N, D, dtype, seed=N + D)
    codes, scale = _unpermute(_K().quantize_fp8(w.cuda()), N, D)
    wf = w.float()
    amax = wf.abs().amax(dim=1)
    want_scale = torch.where(amax > 0, amax / 448.0, torch.ones_like(amax))
    want = (wf / want_scale[:, None]).to(E4M3).view(torch.uint8)
    assert torch.equal(scale.cpu(), want_scale)
    assert torch.equal(codes.cpu(), want)
    assert not bool(((want & 0x7f) == 0x7f).any())                    # no NaN code


def _check(y, ref, dtype):
    rel = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11
    err = (y.double() - ref).abs()
    bound = rel * ref.abs() + 2e-4
    assert bool((err <= bound).all()), f"max excess {(err - bound).max().item():.3e}"


CASES = [
    # M, N, D, bias and aliasing residual, strided x and out
    (1, 256, 64, False, False), (8, 512, 192, False, True), (32, 3584, 3584, False, False), (33, 256, 128, True, False),
    (64, 4608, 3584, True, False), (65, 512, 256, False, False), (288, 1024, 512, False, False),
]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("M,N,D,extras,strided", CASES)
def test_product_matches_f64_on_the_same_codes(M, N, D, extras, strided, dtype):
    K = _K()
    g = torch.Generator(device="cuda").manual_seed(M * 7 + N)
    w = (torch.randn(N, D, generator=g, device="cuda") / D ** 0.5).to(dtype)
    x = torch.randn(M, D + (64 if strided else 0), generator=g, device="cuda").to(dtype)[:, :D]
    image = K.quantize_fp8(w)
    codes, scale = _unpermute(image, N, D)
    ref = (x.double() @ codes.cpu().view(E4M3).float().cuda().double().T) * scale.double()
    bias = res = None
    if extras:
        bias = torch.randn(N, generator=g, device="cuda").to(dtype)
        res = torch.randn(M, N, generator=g, device="cuda").to(dtype)
        ref = ref + bias.double() + res.double()
    ws = K.LinearWorkspace("cuda")
    outs = []
    for _ in range(2):
        big = torch.full((M, N + (24 if strided else 0)), 7.0, device="cuda", dtype=dtype)
        out = big[:, :N]
        if extras:
            out.copy_(res)                                               # y aliases the residual
        K.linear_fp8(x, image, N, bias, workspace=ws, out=out, residual=out if extras else None)
        assert bool((big[:, N:] == 7.0).all())                           # nothing written past N
        outs.append(out)
    _check(outs[0], ref, dtype)
    assert torch.equal(outs[0], outs[1])                                 # slices are added in slice order: the same bits
    if (M, N, D) == (32, 3584, 3584):
        assert K._lib().asd_linear_fp8_workspace_bytes(M, N, D) > 4 * M * N    # 14 column blocks: the plan is sliced


@pytest.mark.parametrize("N,D,short_image,short_ws,want", [
    (300, 64, 0, 0, -2), (256, 100, 0, 0, -2), (256, 64, 1, 0, -1), (3584, 3584, 0, 1, -3)])
def test_argument_checks_launch_nothing(N, D, short_image, short_ws, want):
    from asd_amd._binding import DTYPE_BF16 as BF16
    lib = _K()._lib()
    M = 32
    x = torch.zeros(M, D, device="cuda", dtype=torch.bfloat16)
    y = torch.full((M, N), 7.0, device="cuda", dtype=torch.bfloat16)
    nbytes = int(lib.asd_fp8_image_bytes(N, D))
    assert (nbytes == 0) == (want == -2)
    image = torch.zeros(max(nbytes, N * D + 4 * N), device="cuda", dtype=torch.uint8)
    ws = torch.zeros(max(int(lib.asd_linear_fp8_workspace_bytes(M, N, D)), 256), device="cuda", dtype=torch.uint8)
    rc = lib.asd_linear_fp8(x.data_ptr(), D, image.data_ptr(), image.numel() - short_image, None, None, 0, BF16, M, N, D, y.data_ptr(), N,
                            ws.data_ptr(), 16 if short_ws else ws.numel(), None)
    assert rc == want and bool((y == 7.0).all())
    if want == -2:
        w = torch.zeros(N, D, device="cuda", dtype=torch.bfloat16)
        assert lib.asd_fp8_quantize_weights(w.data_ptr(), D, BF16, N, D, image.data_ptr(), image.numel(), None) == -2
