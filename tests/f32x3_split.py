"""CPU restatement of the three-term float32 product of csrc/k_f32.hip (gemm_f32_kernel<.., X3 = true>), for the operator tests.

The kernel splits every float32 operand x into hi = bf16(x) and lo = bf16(x - hi), both rounded to nearest even (pack_bf16x4,
v_cvt_pk_bf16_f32), and accumulates three bf16 matrix-core terms in float32:  a . w ~= hi_a hi_w + hi_a lo_w + lo_a hi_w.
`r3_matmul` / `r3_conv` are that sum in float64; `exact_operand` builds float32 inputs whose split is known in advance and whose
three-term products are exact in float32 arithmetic, so a kernel result can be compared with them bit for bit.
"""
import torch
import torch.nn.functional as F

# A = ONE_PLUS * I splits into hi = 1, lo = 2^-10 (both bf16, RNE or not)
ONE_PLUS = 1.0 + 2.0 ** -10


def split_bf16(x):
    """(hi, lo) of a float32 tensor as float32 tensors holding bf16 values: hi = bf16(x), lo = bf16(x - hi), round to nearest even"""
    x = x.float()
    hi = x.to(torch.bfloat16).float()
    lo = (x - hi).to(torch.bfloat16).float()          # x - hi is exact in float32
    return hi, lo


def r3_matmul(A, W):
    """A [M][K] . W [N][K]^T as the kernel's three terms, summed in float64"""
    ha, la = (t.double() for t in split_bf16(A))
    hw, lw = (t.double() for t in split_bf16(W))
    return ha @ hw.t() + ha @ lw.t() + la @ hw.t()


def bf16_matmul(A, W):
    """the single-term product hi_a . hi_w in float64: what one bf16 matrix-core term alone would give"""
    return split_bf16(A)[0].double() @ split_bf16(W)[0].double().t()


def conv3x3_nchw(x, w, stride, C, Cout):
    """x channels-last [n][H][W][C], w [Cout][(kh, kw, c)] (any dtype) -> F.conv2d with padding 1 as rows [(n, oh, ow)][Cout]"""
    y = F.conv2d(x.permute(0, 3, 1, 2), w.reshape(Cout, 3, 3, C).permute(0, 3, 1, 2), stride=stride, padding=1)
    return y.permute(0, 2, 3, 1).reshape(-1, Cout)


def r3_conv(x, w, stride, C, Cout):
    """the 3 x 3 convolution with every product as the kernel's three terms, in float64 (zero padding splits into zeros)"""
    hx, lx = (t.double() for t in split_bf16(x))
    hw, lw = (t.double() for t in split_bf16(w))
    return conv3x3_nchw(hx, hw, stride, C, Cout) + conv3x3_nchw(hx, lw, stride, C, Cout) + conv3x3_nchw(lx, hw, stride, C, Cout)


def exact_operand(shape, generator):
    """float32 values x = h + l + t with a split known in advance: hi = h, lo = l.
      h  bf16, |h| in [(1 + 2^-7) 2^e, 1.5 2^e), e in [-2, 1]
      l  bf16, |l| in [2^(e-j), 2^(e-j+1)), j in [9, 13]: below half an ulp of h, so bf16(h + l + t) = h
      t  0 or +-2^(e-23) (the last bit of x): below an eighth of an ulp of l, so RNE gives bf16(l + t) = l, while rounding toward
         zero gives the bf16 value next to l whenever t points toward zero
    Against ONE_PLUS * I every partial sum of the three terms stays within 22 bits below 2^e: exact in float32.
    Returns (x, h, l) as float32 tensors."""
    def ints(lo, hi):
        return torch.randint(lo, hi, shape, generator=generator).double()

    def sign():
        return torch.where(torch.rand(shape, generator=generator) < 0.5, -1.0, 1.0).double()

    e = ints(-2, 2)
    sh = sign()
    h = sh * (1.0 + ints(1, 64) / 128.0) * torch.exp2(e)
    j = ints(9, 14)
    l = sign() * (1.0 + ints(0, 128) / 128.0) * torch.exp2(e - j)
    t = ints(-1, 2) * torch.exp2(e - 23)
    x = h + l + t
    assert torch.equal(x.float().double(), x), "x must be exact in float32"
    return x.float(), h.float(), l.float()
