"""-m gpu: operator tests of the float32 product kernels of csrc/k_f32.hip against float64 references.

  rs_gemm_f32, three-term form (rs_set_option "gemm_f32_x3": the "fp32x3" precision, avsr products="x3")
      |out - R3| <= 2e-5 where R3 is the kernel's split (tests/f32x3_split.py) summed in float64, |out - fp64| <= 2e-5 +
      2^-16 |A|.|W|^T, and at most 1/16 of the single-bf16 product's error; on inputs built so that every partial sum is exact,
      out == R3 bit for bit
  rs_gemm_f32, exact form: the SwooshL / SwooshR / GELU epilogues, row pitches wider than K / N, argument errors
  rs_debug_conv3x3_f32 (rs_launch_conv3x3_f32: the 3 x 3 patches gathered by the GEMM loader, the N64 and 1 x 1 forms, the
      folded BatchNorm + residual + PReLU epilogue), exact and three-term, against F.conv2d in float64
  rs_debug_gemm_f32_skinny (the decoder-step GEMM for M <= 128): every row-tile instantiation, K runs that leave waves empty
  both product kernels past 65535 row tiles (grid.y)

Every output buffer is prefilled with a sentinel: rows past M and columns past N inside the row pitch must keep it.
"""
import contextlib
import ctypes

import pytest
import torch
import torch.nn.functional as F

from reazonspeech_amd.runtime import capi
from reazonspeech_amd.runtime.config import TINY
from oracle.zipformer import swoosh_l, swoosh_r
from f32x3_split import ONE_PLUS, bf16_matmul, conv3x3_nchw, exact_operand, r3_conv, r3_matmul, split_bf16

pytestmark = pytest.mark.gpu

TOL = 2e-5              # the exact kernel's accumulation budget on O(1) outputs
SENT = 7.0


@pytest.fixture(scope="module")
def ctx(gpu_device):
    c = capi.Context(TINY, 0)
    vp, ci = ctypes.c_void_p, ctypes.c_int
    c.lib.rs_debug_conv3x3_f32.argtypes = [vp, vp, ci, ci, ci, ci, ci, ci, ci, vp, ci, vp, vp, vp, vp, vp, ci, vp]
    c.lib.rs_debug_conv3x3_f32.restype = ci
    c.lib.rs_debug_gemm_f32_skinny.argtypes = [vp, vp, ci, vp, ci, vp, ci, ci, ci, ci, ci, vp, vp, vp]
    c.lib.rs_debug_gemm_f32_skinny.restype = ci
    yield c
    c.close()


@contextlib.contextmanager
def x3(ctx, on=True):
    """the three-term products for the calls inside (off again afterwards, whatever happens)"""
    try:
        ctx.set_option("gemm_f32_x3", int(on))
        yield
    finally:
        ctx.set_option("gemm_f32_x3", 0)


def mode(ctx, use_x3):
    return x3(ctx) if use_x3 else contextlib.nullcontext()


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def conv3x3(ctx, x, n_img, H, W, C, OH, OW, stride, w, Cout, scale, shift, residual, prelu, out, one_by_one=0):
    ctx.check(ctx.lib.rs_debug_conv3x3_f32(ctx._h, _p(x), n_img, H, W, C, OH, OW, stride, _p(w), Cout, _p(scale), _p(shift),
                                           _p(residual), _p(prelu), _p(out), one_by_one, None))


def skinny(ctx, A, W, out, flags=0, bias=None, residual=None):
    M, K = A.shape
    N = W.shape[0]
    ctx.check(ctx.lib.rs_debug_gemm_f32_skinny(ctx._h, _p(A), A.stride(0), _p(W), W.stride(0), _p(out), out.stride(0), M, N, K,
                                               flags, _p(bias), _p(residual), None))


def sync():
    torch.cuda.synchronize()


def padded_out(M, N, pitch, device, fill=SENT):
    """an [M][N] view with row pitch `pitch` into a buffer of M + 3 rows, all of it prefilled"""
    full = torch.full((M + 3, pitch), fill, dtype=torch.float32, device=device)
    return full, full[:M, :N]


def assert_outside_untouched(full, M, N):
    full = full.cpu()
    assert torch.all(full[M:] == SENT), "rows past M were written"
    assert torch.all(full[:M, N:] == SENT), "columns past N (inside the row pitch) were written"


def randn(g, *shape, scale=1.0):
    return torch.randn(shape, generator=g) * scale


# ------------------------------------------------------------------------------------------------ three-term rs_gemm_f32
X3_SHAPES = [(128, 128, 32), (130, 72, 192), (1, 640, 256), (517, 3072, 256), (4416, 1024, 4096), (300, 256, 2560)]
X3_SHAPES += [(m, n, k) for m in (1, 127, 129, 300) for n in (4, 68, 132) for k in (32, 96, 4096)]


@pytest.mark.parametrize("M,N,K", X3_SHAPES)
def test_gemm_f32_x3_shapes(ctx, gpu_device, M, N, K):
    g = torch.Generator().manual_seed(M * 7 + N * 3 + K + 1)
    A = randn(g, M, K)
    W = randn(g, N, K, scale=K ** -0.5)
    full, out = padded_out(M, N, N, gpu_device)
    with x3(ctx):
        ctx.gemm_f32(A.to(gpu_device), W.to(gpu_device), out)
    sync()
    got = out.cpu().double()
    ref = A.double() @ W.double().t()
    r3 = r3_matmul(A, W)
    bound = TOL + 2.0 ** -16 * (A.double().abs() @ W.double().abs().t())
    assert (got - r3).abs().max().item() <= TOL
    assert torch.all((got - ref).abs() <= bound)
    err, err_bf16 = (got - ref).abs().max().item(), (bf16_matmul(A, W) - ref).abs().max().item()
    assert err <= err_bf16 / 16, (err, err_bf16)
    assert_outside_untouched(full, M, N)


@pytest.mark.parametrize("w_side", [True, False])
def test_gemm_f32_x3_exact_by_construction(ctx, gpu_device, w_side):
    """ONE_PLUS * I (hi = 1, lo = 2^-10) against values whose split is known and whose three-term sums are exact in float32:
    out == R3 bit for bit.  A missing, doubled or swapped term or plane, a lo not rounded to nearest even, or a transposed
    accumulator write changes bits; the exact kernel would give (1 + 2^-10) x rounded, which is not R3 either."""
    g = torch.Generator().manual_seed(21 + w_side)
    K = 160                                           # five K stages; 32 rows / columns of a second tile
    if w_side:
        M, N = K, 196
        A = ONE_PLUS * torch.eye(M, K)
        W, _, _ = exact_operand((N, K), g)
    else:
        M, N = 300, K
        A, _, _ = exact_operand((M, K), g)
        W = ONE_PLUS * torch.eye(N, K)
    full, out = padded_out(M, N, N, gpu_device)
    with x3(ctx):
        ctx.gemm_f32(A.to(gpu_device), W.to(gpu_device), out)
    sync()
    r3 = r3_matmul(A, W)
    assert torch.equal(r3.float().double(), r3), "the construction must be exact in float32"
    assert torch.equal(out.cpu(), r3.float())
    assert_outside_untouched(full, M, N)


def test_gemm_f32_x3_layout_asymmetric(ctx, gpu_device):
    """test_gemm_f32_layout_asymmetric under X3: A = I (lo = 0) leaves fl(lo_w + hi_w) = R3, and a transposed or permuted
    accumulator write shows; W has 24 significant bits, so the lo plane carries bits and drops some"""
    M = N = K = 256
    W = torch.arange(N)[:, None] * 0.5 + torch.arange(K)[None, :] * (2.0 ** -9 + 2.0 ** -17)
    out = torch.zeros((M, N), dtype=torch.float32, device=gpu_device)
    with x3(ctx):
        ctx.gemm_f32(torch.eye(M, K).to(gpu_device), W.to(gpu_device), out)
    sync()
    hi, lo = split_bf16(W)
    assert not torch.equal(hi + lo, W)                # the lo plane matters here
    assert torch.equal(out.cpu(), (hi + lo).t().contiguous())


ACTS = {capi.GEMM_RELU: torch.relu, capi.GEMM_SILU: F.silu, capi.GEMM_GELU: F.gelu,
        capi.GEMM_SWOOSHL: swoosh_l, capi.GEMM_SWOOSHR: swoosh_r}


@pytest.mark.parametrize("act", list(ACTS), ids=["relu", "silu", "gelu", "swooshl", "swooshr"])
def test_gemm_f32_x3_bias_activation(ctx, gpu_device, act):
    g = torch.Generator().manual_seed(act)
    M, N, K = 261, 200, 384
    A = randn(g, M, K)
    W = randn(g, N, K, scale=K ** -0.5)
    bias = randn(g, N, scale=2.0)
    full, out = padded_out(M, N, N + 8, gpu_device)
    with x3(ctx):
        ctx.gemm_f32(A.to(gpu_device), W.to(gpu_device), out, flags=capi.GEMM_BIAS | act, bias=bias.to(gpu_device))
    sync()
    ref = ACTS[act](r3_matmul(A, W) + bias.double())
    assert (out.cpu().double() - ref).abs().max().item() <= TOL
    assert_outside_untouched(full, M, N)


def test_gemm_f32_x3_residual_and_rowmask(ctx, gpu_device):
    g = torch.Generator().manual_seed(8)
    B, T, Fq, K, N = 3, 11, 5, 128, 192
    M = B * T * Fq
    A = randn(g, M, K)
    W = randn(g, N, K, scale=K ** -0.5)
    bias = randn(g, N)
    res = randn(g, M, N)
    dA, dW, db = A.to(gpu_device), W.to(gpu_device), bias.to(gpu_device)
    base = r3_matmul(A, W) + bias.double()
    stream = res.clone().to(gpu_device)               # the residual IS the output (the encoder's float32 stream)
    with x3(ctx):
        ctx.gemm_f32(dA, dW, stream, flags=capi.GEMM_BIAS | capi.GEMM_RESIDUAL, bias=db, alpha=0.5, residual=stream)
    sync()
    assert (stream.cpu().double() - (res.double() + 0.5 * base)).abs().max().item() <= TOL
    lens = torch.tensor([11, 4, 0], dtype=torch.int32)
    out = torch.ones((M, N), dtype=torch.float32, device=gpu_device)
    with x3(ctx):
        ctx.gemm_f32(dA, dW, out, flags=capi.GEMM_BIAS | capi.GEMM_GELU | capi.GEMM_ROWMASK, bias=db,
                     mask_lens=lens.to(gpu_device), mask_rows=Fq, mask_steps=T)
    sync()
    mask = (torch.arange(T)[None, :] < lens[:, None]).double()[:, :, None, None].expand(B, T, Fq, N).reshape(M, N)
    got = out.cpu()
    assert (got.double() - F.gelu(base) * mask).abs().max().item() <= TOL
    assert torch.all(got[mask == 0] == 0)


def test_gemm_f32_x3_invariance_and_isolation(ctx, gpu_device):
    """a row's bits do not depend on M or on its place in a tile; switching X3 off restores the exact kernel bit for bit"""
    g = torch.Generator().manual_seed(9)
    M, N, K = 400, 136, 256
    A = randn(g, M, K).to(gpu_device)
    W = randn(g, N, K, scale=K ** -0.5).to(gpu_device)
    bias = randn(g, N).to(gpu_device)
    full = torch.zeros((M, N), dtype=torch.float32, device=gpu_device)
    with x3(ctx):
        ctx.gemm_f32(A, W, full, flags=capi.GEMM_BIAS | capi.GEMM_SILU, bias=bias)
        for r0, r1 in ((130, 137), (0, 1), (255, 300), (383, 400)):
            part = torch.zeros((r1 - r0, N), dtype=torch.float32, device=gpu_device)
            ctx.gemm_f32(A[r0:r1].contiguous(), W, part, flags=capi.GEMM_BIAS | capi.GEMM_SILU, bias=bias)
            sync()
            assert torch.equal(part.cpu(), full[r0:r1].cpu()), (r0, r1)
    after = torch.zeros_like(full)
    ctx.gemm_f32(A, W, after, flags=capi.GEMM_BIAS | capi.GEMM_SILU, bias=bias)
    fresh = capi.Context(TINY, 0)
    try:
        never = torch.zeros_like(full)
        fresh.gemm_f32(A, W, never, flags=capi.GEMM_BIAS | capi.GEMM_SILU, bias=bias)
        sync()
    finally:
        fresh.close()
    assert torch.equal(after.cpu(), never.cpu())
    assert not torch.equal(after.cpu(), full.cpu()), "the option changed nothing: X3 not selected"


# ------------------------------------------------------------------------------------------------ exact rs_gemm_f32, the missing cases
@pytest.mark.parametrize("act", [capi.GEMM_SWOOSHL, capi.GEMM_SWOOSHR, capi.GEMM_GELU], ids=["swooshl", "swooshr", "gelu"])
def test_gemm_f32_exact_swoosh_gelu(ctx, gpu_device, act):
    """including pre-activations above 24, where softplus_exact takes its x > 20 branch for both Swoosh forms"""
    g = torch.Generator().manual_seed(30 + act)
    M, N, K = 300, 196, 320
    A = randn(g, M, K)
    W = randn(g, N, K, scale=K ** -0.5)
    bias = torch.where(torch.arange(N) % 3 == 0, 30.0, torch.where(torch.arange(N) % 3 == 1, -30.0, 0.0)) + randn(g, N)
    full, out = padded_out(M, N, N, gpu_device)
    ctx.gemm_f32(A.to(gpu_device), W.to(gpu_device), out, flags=capi.GEMM_BIAS | act, bias=bias.to(gpu_device))
    sync()
    pre = A.double() @ W.double().t() + bias.double()
    assert (pre > 24).sum() > 1000 and (pre < -24).sum() > 1000
    ref = ACTS[act](pre)
    assert (out.cpu().double() - ref).abs().max().item() <= TOL
    assert_outside_untouched(full, M, N)


@pytest.mark.parametrize("use_x3", [False, True], ids=["exact", "x3"])
def test_gemm_f32_strided_pitches(ctx, gpu_device, use_x3):
    """lda, ldw, ldc wider than K / N (multiples of 4): row views into wider matrices"""
    g = torch.Generator().manual_seed(40)
    M, N, K = 259, 132, 224
    Abig = randn(g, M, K + 36)
    Wbig = randn(g, N + 5, K + 12, scale=K ** -0.5)
    A, W = Abig[:, 4:4 + K], Wbig[:N, :K]
    bias = randn(g, N)
    res = randn(g, M, N)
    full, out = padded_out(M, N, N + 20, gpu_device)
    out.copy_(res.to(gpu_device))
    dA, dW = Abig.to(gpu_device)[:, 4:4 + K], Wbig.to(gpu_device)[:N, :K]
    assert dA.stride(0) == K + 36 and dW.stride(0) == K + 12 and out.stride(0) == N + 20
    with mode(ctx, use_x3):
        ctx.gemm_f32(dA, dW, out, flags=capi.GEMM_BIAS | capi.GEMM_RESIDUAL, bias=bias.to(gpu_device), alpha=1.5, residual=out)
    sync()
    prod = r3_matmul(A, W) if use_x3 else A.double() @ W.double().t()
    ref = res.double() + 1.5 * (prod + bias.double())
    assert (out.cpu().double() - ref).abs().max().item() <= TOL
    assert_outside_untouched(full, M, N)


def test_gemm_f32_argument_errors(ctx, gpu_device):
    dev = gpu_device
    out = torch.zeros((64, 64), dtype=torch.float32, device=dev)
    with pytest.raises(capi.RsError):                 # K % 32
        ctx.gemm_f32(torch.zeros((64, 48), device=dev), torch.zeros((64, 48), device=dev), out)
    with pytest.raises(capi.RsError):                 # N % 4
        ctx.gemm_f32(torch.zeros((64, 64), device=dev), torch.zeros((6, 64), device=dev), torch.zeros((64, 8), device=dev)[:, :6])
    for flags in (capi.GEMM_GLU, 1024):               # not an epilogue of the float32 kernel
        with pytest.raises(capi.RsError):
            ctx.gemm_f32(torch.zeros((64, 64), device=dev), torch.zeros((64, 64), device=dev), out, flags=flags)
    with pytest.raises(capi.RsError):                 # a flag without its operand
        ctx.gemm_f32(torch.zeros((64, 64), device=dev), torch.zeros((64, 64), device=dev), out, flags=capi.GEMM_BIAS)
    sync()


# ------------------------------------------------------------------------------------------------ gathered 3 x 3 convolution
def conv_epilogue(y, scale, shift, residual, prelu):
    v = y * scale.double() + shift.double()
    if residual is not None:
        v = v + residual.double()
    if prelu is not None:
        v = torch.where(v >= 0, v, prelu.double() * v)
    return v


# (C, Cout, H, W, stride, n_img, epilogue, one_by_one): Cout <= 64 the N64 form, above it the 128-column one; 1 x 1 maps are all
# padding but the centre; n_img 3 and 37 put image boundaries inside 128-row tiles
CONV_CASES = [
    (32, 64, 22, 22, 1, 3, "res+prelu", 0), (32, 64, 22, 22, 2, 37, "prelu", 0), (64, 36, 7, 7, 1, 37, "relu", 0),
    (64, 36, 7, 7, 2, 3, "none", 0), (128, 68, 3, 5, 1, 37, "res+relu", 0), (128, 128, 3, 5, 2, 3, "prelu", 0),
    (32, 256, 1, 1, 1, 37, "res+prelu", 0), (64, 256, 1, 1, 2, 3, "none", 0), (64, 128, 22, 22, 2, 3, "res", 0),
    (128, 256, 7, 7, 1, 3, "prelu", 0), (32, 68, 22, 22, 1, 1, "none", 0), (32, 36, 3, 5, 2, 1, "res+prelu", 0),
    (128, 64, 5, 3, 2, 37, "res+relu", 0),
    (64, 64, 7, 7, 1, 3, "none", 1), (128, 256, 22, 22, 1, 1, "res+prelu", 1), (32, 36, 3, 5, 1, 37, "relu", 1),
    (32, 68, 7, 7, 1, 37, "res", 1),
]


@pytest.mark.parametrize("use_x3", [False, True], ids=["exact", "x3"])
@pytest.mark.parametrize("C,Cout,H,W,stride,n_img,epi,one_by_one", CONV_CASES)
def test_conv3x3_f32(ctx, gpu_device, C, Cout, H, W, stride, n_img, epi, one_by_one, use_x3):
    g = torch.Generator().manual_seed(C + Cout * 3 + H * 7 + W * 11 + stride * 13 + n_img * 17 + one_by_one)
    OH, OW = ((H - 1) // stride + 1, (W - 1) // stride + 1) if not one_by_one else (H, W)
    rows, K = n_img * OH * OW, C if one_by_one else 9 * C
    x = randn(g, n_img, H, W, C)
    w = randn(g, Cout, K, scale=K ** -0.5)
    scale = 0.5 + torch.rand(Cout, generator=g)
    shift = 0.1 * randn(g, Cout)
    residual = randn(g, rows, Cout) if "res" in epi else None
    prelu = {"prelu": 0.25 * randn(g, Cout), "relu": torch.zeros(Cout)}.get(epi.split("+")[-1])
    full = torch.full((rows + 3, Cout), SENT, dtype=torch.float32, device=gpu_device)
    dev = {k: None if v is None else v.to(gpu_device) for k, v in dict(x=x, w=w, s=scale, b=shift, r=residual, p=prelu).items()}
    with mode(ctx, use_x3):
        conv3x3(ctx, dev["x"], n_img, H, W, C, OH, OW, stride, dev["w"], Cout, dev["s"], dev["b"], dev["r"], dev["p"], full,
                one_by_one)
    sync()
    got = full[:rows].cpu().double()
    assert torch.all(full[rows:].cpu() == SENT), "rows past the output were written"
    if one_by_one:
        xm = x.reshape(rows, C)
        y = xm.double() @ w.double().t()
        y3 = r3_matmul(xm, w)
        yabs = xm.double().abs() @ w.double().abs().t()
    else:
        y = conv3x3_nchw(x.double(), w.double(), stride, C, Cout)
        y3 = r3_conv(x, w, stride, C, Cout)
        yabs = conv3x3_nchw(x.double().abs(), w.double().abs(), stride, C, Cout)
    ref = conv_epilogue(y, scale, shift, residual, prelu)
    if not use_x3:
        assert (got - ref).abs().max().item() <= TOL
        return
    ref3 = conv_epilogue(y3, scale, shift, residual, prelu)
    assert (got - ref3).abs().max().item() <= TOL
    assert torch.all((got - ref).abs() <= TOL + 2.0 ** -16 * yabs * scale.double())


def test_conv3x3_f32_argument_errors(ctx, gpu_device):
    dev = gpu_device
    x = torch.zeros((1, 4, 4, 64), device=dev)
    w = torch.zeros((64, 9 * 64), device=dev)
    s = torch.ones(64, device=dev)
    out = torch.zeros((16, 64), device=dev)
    with pytest.raises(capi.RsError):                 # C % 32
        conv3x3(ctx, x, 1, 4, 4, 48, 4, 4, 1, w, 64, s, s, None, None, out)
    with pytest.raises(capi.RsError):                 # Cout % 4
        conv3x3(ctx, x, 1, 4, 4, 64, 4, 4, 1, w, 62, s, s, None, None, out)
    with pytest.raises(capi.RsError):                 # no folded BatchNorm
        conv3x3(ctx, x, 1, 4, 4, 64, 4, 4, 1, w, 64, None, s, None, None, out)
    sync()


# ------------------------------------------------------------------------------------------------ skinny GEMM (decoder steps)
# M: every row-tile instantiation (1 .. 6 tiles, 7 and 8 tiles in the default branch); K: 16-blocks per wave run 1 (K 16, 48: waves
# left empty), 2 (144: one trip past the run), 9 (1040: the last wave's run is short) and 24 (3072); N % 16 != 0: clamped weight rows
@pytest.mark.parametrize("N", [4, 20, 772])
@pytest.mark.parametrize("K", [16, 48, 144, 1040, 3072])
@pytest.mark.parametrize("M", [1, 15, 16, 17, 48, 63, 97, 112, 128])
def test_gemm_f32_skinny_shapes(ctx, gpu_device, M, N, K):
    g = torch.Generator().manual_seed(M * 131 + N * 7 + K)
    A = randn(g, M, K)
    W = randn(g, N, K, scale=K ** -0.5)
    full, out = padded_out(M, N, N, gpu_device)
    skinny(ctx, A.to(gpu_device), W.to(gpu_device), out)
    sync()
    assert (out.cpu().double() - A.double() @ W.double().t()).abs().max().item() <= TOL
    assert_outside_untouched(full, M, N)


@pytest.mark.parametrize("M", [1, 33, 128])
@pytest.mark.parametrize("act", [0, capi.GEMM_RELU, capi.GEMM_SILU, capi.GEMM_GELU], ids=["none", "relu", "silu", "gelu"])
def test_gemm_f32_skinny_epilogues_strided(ctx, gpu_device, M, act):
    """bias + activation (+ residual aliasing the output), operands and output as row views with wider pitches"""
    g = torch.Generator().manual_seed(M + act)
    N, K = 196, 784
    Abig = randn(g, M, K + 20)
    Wbig = randn(g, N, K + 8, scale=K ** -0.5)
    bias = randn(g, N)
    res = randn(g, M, N)
    full, out = padded_out(M, N, N + 12, gpu_device)
    dA, dW, db = Abig.to(gpu_device)[:, :K], Wbig.to(gpu_device)[:, 8:], bias.to(gpu_device)
    pre = Abig[:, :K].double() @ Wbig[:, 8:].double().t() + bias.double()
    f = ACTS.get(act, lambda v: v)
    skinny(ctx, dA, dW, out, flags=capi.GEMM_BIAS | act, bias=db)
    sync()
    assert (out.cpu().double() - f(pre)).abs().max().item() <= TOL
    out.copy_(res.to(gpu_device))
    skinny(ctx, dA, dW, out, flags=capi.GEMM_BIAS | act | capi.GEMM_RESIDUAL, bias=db, residual=out)
    sync()
    assert (out.cpu().double() - (f(pre) + res.double())).abs().max().item() <= TOL
    assert_outside_untouched(full, M, N)


def test_gemm_f32_skinny_ignores_x3_and_rejects_bad_shapes(ctx, gpu_device):
    """the skinny kernel has no three-term form: the avsr decoder multiplies exactly whatever gemm_f32_x3 says (a change to
    that must be deliberate)"""
    g = torch.Generator().manual_seed(50)
    M, N, K = 97, 772, 1040
    A = randn(g, M, K).to(gpu_device)
    W = randn(g, N, K, scale=K ** -0.5).to(gpu_device)
    off = torch.zeros((M, N), dtype=torch.float32, device=gpu_device)
    on = torch.zeros_like(off)
    skinny(ctx, A, W, off)
    with x3(ctx):
        skinny(ctx, A, W, on)
    sync()
    assert torch.equal(on.cpu(), off.cpu())
    dev = gpu_device
    for m, n, k in ((129, 64, 64), (16, 64, 8), (16, 6, 64)):      # (row pitch of the output 64: only M, K or N is wrong)
        with pytest.raises(capi.RsError):
            skinny(ctx, torch.zeros((m, k), device=dev), torch.zeros((n, k), device=dev), torch.zeros((m, 64), device=dev)[:, :n])
    with pytest.raises(capi.RsError):                 # GLU is not a skinny epilogue
        skinny(ctx, A, W, off, flags=capi.GEMM_GLU)
    sync()


# ------------------------------------------------------------------------------------------------ past 65535 row tiles
# The avsr encoder takes up to 65535 frames per call and its first trunk stage has 484 rows per frame, so a launch can have more
# than 65535 tiles of 128 rows in grid.y.  About 3.2 GB of device memory per test, released before the next one.
BIG_TILES = 65536 + 8


def _sample_rows(g, M):
    return torch.cat([torch.randint(0, M, (64,), generator=g), torch.arange(M - 128, M)])    # + the last tile


@pytest.mark.parametrize("use_x3", [False, True], ids=["exact", "x3"])
def test_gemm_f32_rows_past_65535_tiles(ctx, gpu_device, use_x3):
    M, N, K = BIG_TILES * 128 - 77, 64, 32
    g = torch.Generator().manual_seed(60)
    W = randn(g, N, K, scale=K ** -0.5)
    dg = torch.Generator(device=gpu_device).manual_seed(61)
    try:
        A = torch.randn((M, K), generator=dg, device=gpu_device)
        out = torch.full((M + 3, N), SENT, dtype=torch.float32, device=gpu_device)
        with mode(ctx, use_x3):
            ctx.gemm_f32(A, W.to(gpu_device), out[:M])
        sync()
        assert not bool((out[:M] == SENT).all(dim=1).any()), "rows left unwritten"
        assert bool((out[M:] == SENT).all()), "rows past M were written"
        rows = _sample_rows(g, M).to(gpu_device)
        a, got = A[rows].cpu(), out[rows].cpu().double()
    finally:
        A = out = None
        torch.cuda.empty_cache()
    ref = r3_matmul(a, W) if use_x3 else a.double() @ W.double().t()
    assert (got - ref).abs().max().item() <= TOL


@pytest.mark.parametrize("use_x3", [False, True], ids=["exact", "x3"])
def test_conv3x3_f32_rows_past_65535_tiles(ctx, gpu_device, use_x3):
    C, Cout, H = 32, 64, 22
    n_img = (BIG_TILES * 128) // (H * H) + 1
    rows = n_img * H * H
    assert (rows + 127) // 128 > BIG_TILES
    g = torch.Generator().manual_seed(70)
    w = randn(g, Cout, 9 * C, scale=(9 * C) ** -0.5)
    scale, shift, prelu = 0.5 + torch.rand(Cout, generator=g), 0.1 * randn(g, Cout), 0.25 * randn(g, Cout)
    imgs = torch.cat([torch.randint(0, n_img, (6,), generator=g), torch.tensor([0, n_img - 1])])   # the last image holds the last tile
    dg = torch.Generator(device=gpu_device).manual_seed(71)
    try:
        x = torch.randn((n_img, H, H, C), generator=dg, device=gpu_device)
        out = torch.full((rows + 3, Cout), SENT, dtype=torch.float32, device=gpu_device)
        with mode(ctx, use_x3):
            conv3x3(ctx, x, n_img, H, H, C, H, H, 1, w.to(gpu_device), Cout, scale.to(gpu_device), shift.to(gpu_device), None,
                    prelu.to(gpu_device), out)
        sync()
        assert not bool((out[:rows] == SENT).all(dim=1).any()), "rows left unwritten"
        assert bool((out[rows:] == SENT).all()), "rows past the output were written"
        xs = x[imgs.to(gpu_device)].cpu()
        got = out[:rows].view(n_img, H * H, Cout)[imgs.to(gpu_device)].cpu().double().reshape(-1, Cout)
    finally:
        x = out = None
        torch.cuda.empty_cache()
    y = r3_conv(xs, w, 1, C, Cout) if use_x3 else conv3x3_nchw(xs.double(), w.double(), 1, C, Cout)
    ref = conv_epilogue(y, scale, shift, None, prelu)
    assert (got - ref).abs().max().item() <= TOL
