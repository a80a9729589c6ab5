"""float64 references of the conv-module middle and the LayerNorms of csrc/k_layernorm.hip, plain torch on the CPU, and the two
tolerances the operator tests hold the kernels to.  tests/test_convmod_ref_host.py shows that the references agree with torch's own
float32 operators, that a float32 emulation of the kernels' arithmetic stays inside the tolerances and that deliberately wrong
variants do not; tests/test_gpu_convmod_ops.py compares the device with them.

Conventions are the kernels': x [B][T][2d] or [B][T][d] (values already rounded to bf16), w [k][d] tap-major, bias [d], lens [B].
"""
import torch
import torch.nn.functional as F

from oracle.zipformer import swoosh_r
from reazonspeech_amd.runtime.weights import glu_interleave_index

HALVES, BLOCK32, APPLIED = 0, 1, 2        # rs_asr.h RS_GLU_*
SILU, SWOOSH_R = 0, 1                     # the `act` argument of dwconv_act


def glu_dwconv(x, w, b, lens, k, layout, act=SILU):
    """GLU -> frame mask -> depthwise conv over time ("same" zero padding) + bias -> activation, float64, [B][T][d].
    layout 0: columns [0, d) are values, [d, 2d) gates; 1: blocks of 32 values / 32 gates (undone with glu_interleave_index);
    2: the GLU is already applied, x is [B][T][d].  Frames t >= min(len, T) are zeroed BEFORE the convolution and every output
    frame 0 .. T-1 is returned: the kernels write the convolution of the masked input at and past `len` too."""
    x = x.double()
    B, T = x.shape[:2]
    d = w.shape[1]
    assert w.shape[0] == k and k % 2 == 1
    if layout == APPLIED:
        assert x.shape[2] == d
        u = x
    else:
        assert x.shape[2] == 2 * d
        if layout == BLOCK32:
            x = x[..., torch.argsort(glu_interleave_index(d))]
        u = x[..., :d] * torch.sigmoid(x[..., d:])
    lens = torch.as_tensor(lens, dtype=torch.int64).clamp(max=T)
    u = u * (torch.arange(T)[None, :] < lens[:, None])[:, :, None]
    z = F.conv1d(u.transpose(1, 2), w.double().t()[:, None, :], b.double(), padding=(k - 1) // 2, groups=d).transpose(1, 2)
    if act == SILU:
        return F.silu(z)
    assert act == SWOOSH_R
    return swoosh_r(z)


def layernorm_stats(x, eps):
    """(mean, rstd) per row, float64, biased variance"""
    x = x.double()
    mean = x.mean(dim=-1, keepdim=True)
    var = ((x - mean) ** 2).mean(dim=-1, keepdim=True)
    return mean, 1.0 / torch.sqrt(var + eps)


def layernorm(x, g, b, eps):
    mean, rstd = layernorm_stats(x, eps)
    return (x.double() - mean) * rstd * g.double() + b.double()


def layernorm_pair(x, g1, b1, g2, b2, eps):
    """y = LN(x; g1, b1), z = LN(y; g2, b2) and the first norm's (mean, rstd), all float64 (y is not rounded in between)"""
    mean, rstd = layernorm_stats(x, eps)
    y = (x.double() - mean) * rstd * g1.double() + b1.double()
    return y, layernorm(y, g2, b2, eps), (mean[..., 0], rstd[..., 0])


def conv_tol(ref):
    """bf16 output of a float32 chain of <= 31 products: one bf16 ulp of the single output rounding (2^-7 relative; the rounding
    itself is at most half of that) plus an absolute allowance for the float32 accumulation and the fast exp / rcp of sigmoid_f"""
    return 1e-4 + 2.0 ** -7 * ref.abs()


def ln_tol(x, eps, ref=None):
    """float32 output of the two-pass LayerNorm, per row ([M][1]): 2e-5 for the arithmetic on O(1) values plus the float32 rounding
    of the mean that survives in x - mean, scaled by rstd.  With `ref` (the bf16 output): one bf16 ulp of |ref| more."""
    x = x.double()
    mean = x.mean(dim=-1, keepdim=True)
    var = ((x - mean) ** 2).mean(dim=-1, keepdim=True)
    tol = 2e-5 + 16 * 2.0 ** -24 * mean.abs() / torch.sqrt(var + eps)
    if ref is not None:
        tol = tol + 2.0 ** -7 * ref.abs()
    return tol


def worst_ratio(got, ref, tol):
    """max |got - ref| / tol over all elements (tol > 0 everywhere); inf when an element is NaN, so that `<= 1` never passes one"""
    r = (got.double() - ref).abs() / tol
    return float("inf") if bool(torch.isnan(r).any()) else float(r.max())
