"""CPU: the float64 references and the tolerances of tests/convmod_ref.py are right, and they discriminate.

  * the references agree with torch's own float32 F.conv1d / F.layer_norm within the tolerances;
  * a float32 emulation of the kernels' arithmetic (csrc/k_layernorm.hip: GLU in float32, a bias-first ascending-tap fmaf chain,
    two-pass statistics, one bf16 rounding of the output) stays INSIDE the tolerance;
  * the same emulation with one deliberate fault (a dropped tap, a mask off by one, a shifted halo, a value / gate swap, one-pass
    variance, rstd without eps) lands OUTSIDE it.
"""
import pytest
import torch
import torch.nn.functional as F

import convmod_ref as cr
from reazonspeech_amd.runtime.weights import glu_interleave_index

EPS = 1e-5


def rb(t):
    return t.to(torch.bfloat16).to(torch.float32)


def fmaf(a, b, c):
    """float32 fused multiply-add: the product of two float32 is exact in float64, so this is one float64 rounding of the sum before
    the float32 one (a double rounding that differs from a true fma only on a tie the float64 sum created)"""
    return (a.double() * b.double() + c.double()).float()


def sigmoid32(x):
    return 1.0 / (1.0 + torch.exp(-x))


def conv_case(k, layout, seed, B=3, T=70, d=64):
    g = torch.Generator().manual_seed(seed)
    x = rb(torch.randn((B, T, d if layout == cr.APPLIED else 2 * d), generator=g))     # garbage in the padded frames too
    w = torch.randn((k, d), generator=g) / 3
    b = 0.1 * torch.randn((d,), generator=g)
    lens = torch.tensor([T, 33, 1][:B], dtype=torch.int64)
    return x, w, b, lens


def emulate_conv(x, w, b, lens, k, layout, act=cr.SILU, tile=32, fault=None):
    """the kernels' arithmetic in float32: an output frame of a `tile`-frame tile reads input frame t + j - half for tap j; frames
    outside [0, min(len, T)) are zero.  `fault` turns one thing wrong."""
    B, T = x.shape[:2]
    d = w.shape[1]
    half = (k - 1) // 2
    if layout == cr.APPLIED:
        u = x.clone()
    else:
        idx = torch.arange(2 * d)
        if layout == cr.BLOCK32:
            idx = torch.argsort(glu_interleave_index(d))
            if fault == "swap_block":             # the values and gates of channels 32 .. 63 change places
                idx = idx.clone()
                idx[32:64], idx[d + 32:d + 64] = idx[d + 32:d + 64].clone(), idx[32:64].clone()
        xh = x[..., idx]
        u = xh[..., :d] * sigmoid32(xh[..., d:])
    t = torch.arange(T)[:, None]
    f = t + torch.arange(k)[None, :] - half                              # [T][k] input frame of (output frame, tap)
    if fault == "halo_shift":                                            # the halo rows of every tile come from one frame later
        t0 = (t // tile) * tile
        f = torch.where((f < t0) | (f >= t0 + tile), f + 1, f)
    n = lens.clamp(max=T)[:, None, None]
    ok = (f >= 0)[None] & (f < T)[None] & ((f[None] <= n) if fault == "mask_le" else (f[None] < n))     # [B][T][k]
    win = u[:, f.clamp(0, T - 1)] * ok[..., None]                        # [B][T][k][d]
    acc = b.expand(B, T, d).clone()
    for j in range(k - 1 if fault == "drop_last_tap" else k):
        acc = fmaf(win[:, :, j], w[j], acc)
    y = acc * sigmoid32(acc) if act == cr.SILU else cr.swoosh_r(acc)
    return rb(y)


def ln_rows(d, seed):
    """rows of (mean, std) = (1.5, 3), (+100, 0.1), (-100, 0.1), a constant row and an all-zero row"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((5, d), generator=g)
    x[0] = x[0] * 3 + 1.5
    x[1] = x[1] * 0.1 + 100
    x[2] = x[2] * 0.1 - 100
    x[3] = 3.7
    x[4] = 0
    gamma = 1 + 0.1 * torch.randn((d,), generator=g)
    beta = 0.1 * torch.randn((d,), generator=g)
    return x, gamma, beta


def wave_sum(v):
    """the kernels' row sum in their order, float32: lane l of 64 adds (a + b) + (c + d) of its float4 number i * 64 + l for
    i = 0 .. d / 256 - 1, then the xor butterfly over the lanes (every lane ends with the same value)"""
    q = v.view(v.shape[0], -1, 64, 4)
    s = torch.zeros((v.shape[0], 64))
    for i in range(q.shape[1]):
        s = s + ((q[:, i, :, 0] + q[:, i, :, 1]) + (q[:, i, :, 2] + q[:, i, :, 3]))
    for off in (32, 16, 8, 4, 2, 1):
        s = s + s[:, torch.arange(64) ^ off]
    return s[:, :1]


def emulate_ln(x, gamma, beta, fault=None):
    d = x.shape[1]
    mean = wave_sum(x) * (1.0 / d)
    if fault == "one_pass":
        var = wave_sum(x * x) * (1.0 / d) - mean * mean
    else:
        var = wave_sum((x - mean) ** 2) * (1.0 / d)
    rstd = 1.0 / torch.sqrt(var if fault == "no_eps" else var + EPS)
    return fmaf((x - mean) * rstd, gamma, beta)


# ---- the references against torch's float32 operators ------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 3, 7, 9, 15, 31])
@pytest.mark.parametrize("layout", [cr.HALVES, cr.BLOCK32, cr.APPLIED])
def test_conv_reference_agrees_with_torch_float32(k, layout):
    x, w, b, lens = conv_case(k, layout, 100 * layout + k)
    d = w.shape[1]
    xh = x[..., torch.argsort(glu_interleave_index(d))] if layout == cr.BLOCK32 else x
    u = xh if layout == cr.APPLIED else xh[..., :d] * torch.sigmoid(xh[..., d:])
    u = u * (torch.arange(x.shape[1])[None, :] < lens[:, None])[:, :, None]
    z = F.conv1d(u.transpose(1, 2), w.t()[:, None, :].contiguous(), b, padding=(k - 1) // 2, groups=d).transpose(1, 2)
    for act, fn in ((cr.SILU, F.silu), (cr.SWOOSH_R, cr.swoosh_r)):
        ref = cr.glu_dwconv(x, w, b, lens, k, layout, act)
        assert ref.dtype == torch.float64 and ref.shape == z.shape
        assert cr.worst_ratio(fn(z), ref, cr.conv_tol(ref)) <= 1.0


def test_conv_reference_masks_before_the_convolution_and_returns_every_frame():
    """a len of 0 gives act(bias) everywhere; a len past T is T; the frame at `len` still sees the frames before it"""
    k, d, T = 9, 32, 12
    g = torch.Generator().manual_seed(1)
    x = rb(torch.randn((3, T, d), generator=g))
    w = torch.randn((k, d), generator=g)
    b = torch.randn((d,), generator=g)
    ref = cr.glu_dwconv(x, w, b, [0, T + 5, 6], k, cr.APPLIED)
    assert torch.equal(ref[0], F.silu(b.double()).expand(T, d))
    assert (ref[1] - cr.glu_dwconv(x[1:2], w, b, [T], k, cr.APPLIED)[0]).abs().max() <= 1e-12
    z6 = b.double() + sum(x[2, 6 + j - 4].double() * w[j].double() for j in range(0, 4))       # taps 4 .. 8 read frames 6 .. 10: masked
    assert (ref[2, 6] - F.silu(z6)).abs().max() <= 1e-12
    assert torch.equal(ref[2, 6 + 5:], F.silu(b.double()).expand(T - 11, d))                    # past len + half: bias only


@pytest.mark.parametrize("d", [256, 512, 1024, 2048])
def test_layernorm_reference_agrees_with_torch_float32(d):
    x, gamma, beta = ln_rows(d, d)
    ref = cr.layernorm(x, gamma, beta, EPS)
    assert cr.worst_ratio(F.layer_norm(x, (d,), gamma, beta, EPS), ref, cr.ln_tol(x, EPS)) <= 1.0
    g2, b2 = gamma.flip(0), beta.flip(0)
    y, z, (mean, rstd) = cr.layernorm_pair(x, gamma, beta, g2, b2, EPS)
    assert torch.equal(y, ref) and torch.equal(z, cr.layernorm(y, g2, b2, EPS))
    assert mean.shape == rstd.shape == (5,)
    assert torch.equal(mean, x.double().mean(dim=1)) and abs(float(rstd[4]) - EPS ** -0.5) <= 1e-9


# ---- the kernels' float32 arithmetic stays inside the tolerance ------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 3, 7, 9, 15, 31])
def test_float32_emulation_of_the_conv_kernels_is_inside_conv_tol(k):
    worst = 0.0
    for layout in (cr.HALVES, cr.BLOCK32, cr.APPLIED):
        x, w, b, lens = conv_case(k, layout, 7 * k + layout)
        for act in (cr.SILU, cr.SWOOSH_R):
            ref = cr.glu_dwconv(x, w, b, lens, k, layout, act)
            worst = max(worst, cr.worst_ratio(emulate_conv(x, w, b, lens, k, layout, act), ref, cr.conv_tol(ref)))
    print(f"conv k={k}: worst err / conv_tol of the float32 emulation = {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("d", [256, 512, 768, 1024, 1280, 1536, 1792, 2048])
def test_float32_emulation_of_layernorm_is_inside_ln_tol(d):
    x, gamma, beta = ln_rows(d, d + 1)
    ref = cr.layernorm(x, gamma, beta, EPS)
    y = emulate_ln(x, gamma, beta)
    r32 = cr.worst_ratio(y, ref, cr.ln_tol(x, EPS))
    r16 = cr.worst_ratio(rb(y), ref, cr.ln_tol(x, EPS, ref))
    print(f"layernorm d={d}: worst err / ln_tol of the float32 emulation = {r32:.3f} (f32 out), {r16:.3f} (bf16 out)")
    assert r32 <= 1.0 and r16 <= 1.0
    assert cr.worst_ratio(y[3:4], beta.double().expand(1, d), cr.ln_tol(x[3:4], EPS)) <= 1.0      # the constant row is beta
    assert torch.equal(y[4], beta)                                                                 # the zero row exactly


# ---- one fault each: outside the tolerance ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [3, 9, 31])
@pytest.mark.parametrize("fault,layout", [("drop_last_tap", cr.APPLIED), ("drop_last_tap", cr.HALVES), ("mask_le", cr.APPLIED),
                                          ("mask_le", cr.BLOCK32), ("halo_shift", cr.APPLIED), ("halo_shift", cr.HALVES),
                                          ("swap_block", cr.BLOCK32)])
def test_a_wrong_conv_is_outside_conv_tol(k, fault, layout):
    x, w, b, lens = conv_case(k, layout, 11 * k + layout)
    ref = cr.glu_dwconv(x, w, b, lens, k, layout)
    assert cr.worst_ratio(emulate_conv(x, w, b, lens, k, layout), ref, cr.conv_tol(ref)) <= 1.0
    r = cr.worst_ratio(emulate_conv(x, w, b, lens, k, layout, fault=fault), ref, cr.conv_tol(ref))
    print(f"k={k} layout={layout} {fault}: err / conv_tol = {r:.1f}")
    assert r > 10.0


def test_a_mask_off_by_one_shows_only_in_the_rows_next_to_len():
    """why every row 0 .. T-1 is compared, not only the rows below len: with `t <= len` the rows up to len - half - 1 are right"""
    k, layout = 9, cr.APPLIED
    x, w, b, lens = conv_case(k, layout, 5)
    ref = cr.glu_dwconv(x, w, b, lens, k, layout)
    bad = emulate_conv(x, w, b, lens, k, layout, fault="mask_le")
    n, half = int(lens[1]), 4
    tol = cr.conv_tol(ref)
    assert cr.worst_ratio(bad[1, :n - half], ref[1, :n - half], tol[1, :n - half]) <= 1.0
    assert cr.worst_ratio(bad[1, n - half:n], ref[1, n - half:n], tol[1, n - half:n]) > 10.0
    assert cr.worst_ratio(bad[1, n:], ref[1, n:], tol[1, n:]) > 10.0


@pytest.mark.parametrize("d", [256, 1024, 2048])
def test_a_wrong_layernorm_is_outside_ln_tol(d):
    x, gamma, beta = ln_rows(d, d + 2)
    ref = cr.layernorm(x, gamma, beta, EPS)
    tol = cr.ln_tol(x, EPS)
    one = emulate_ln(x, gamma, beta, fault="one_pass")
    # mean +-100, std 0.1: E[x^2] ~ 1e4 has a float32 step of 1e-3 against a variance of 1e-2, so how wrong a row comes out depends on
    # where its E[x^2] lands on that grid: each row is outside the tolerance, the worse of the two far outside
    rs = [cr.worst_ratio(one[row:row + 1], ref[row:row + 1], tol[row:row + 1]) for row in (1, 2)]
    print(f"d={d} one-pass variance, rows of mean +100 / -100: err / ln_tol = {rs[0]:.1f} / {rs[1]:.1f}")
    assert min(rs) > 1.0 and max(rs) > 10.0
    noeps = emulate_ln(x, gamma, beta, fault="no_eps")
    assert cr.worst_ratio(noeps[3:4], ref[3:4], tol[3:4]) > 10.0            # the constant row: 0 * inf, or a huge rstd
