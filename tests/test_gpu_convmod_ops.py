"""-m gpu: every form of the conv-module kernels and of the two LayerNorms of csrc/k_layernorm.hip, one operator at a time through
the C ABI, against the float64 references of tests/convmod_ref.py (tests/test_convmod_ref_host.py shows on the CPU that those
references and tolerances are right and that they reject a dropped tap, a mask off by one, a shifted halo, a value / gate swap,
one-pass variance and a missing eps).

  kernel form                               reached by
  glu_dwconv_silu_fast_kernel<9,6,0 / 1>    k = 9, layouts 0 / 1                       test_k9_*
  dwconv_silu_dma_kernel<9,6>               k = 9, layout 2                            test_k9_*
  glu_dwconv_silu_fast_kernel<9,6,2>        k = 9, layout 2, RS_GLU_GENERIC=2          test_k9_*
  glu_dwconv_silu_kernel                    k not 9 (layouts 0, 1; layout 2 at k = 1, 3, 5), or RS_GLU_GENERIC=1   test_generic_*
  dwconv_act_kernel<7/15/31, SiLU/SwooshR>  rs_debug_dwconv_act; SiLU also layout 2    test_dwconv_act_*
  layernorm_kernel<1..8>                    rs_layernorm, d = 256 .. 2048              test_layernorm_*
  layernorm2_kernel<NV>                     rs_debug_layernorm2                        test_layernorm2_*

Every conv output buffer has 8 rows more than B * T, filled with a sentinel that must survive, and every row 0 .. B*T-1 is compared
(the rows at and past an utterance's length hold the convolution of the masked input: a halo that leaked padded frames shows there).
Each batch has the lengths T, 0, 1 and one next to a tile seam.  The forms of one operator run the same bias-first ascending-tap
fmaf chain on the same float32 inputs, so they are held to value equality with each other, which tolerates only the sign of a zero.
"""
import ctypes

import pytest
import torch

import convmod_ref as cr
from knobs import knob
from reazonspeech_amd.runtime import capi
from reazonspeech_amd.runtime.capi import _ptr
from reazonspeech_amd.runtime.config import TINY
from reazonspeech_amd.runtime.weights import glu_interleave_index

pytestmark = pytest.mark.gpu
SENTINEL = 7.0
PAD = 8
EPS = 1e-5
WORST = {}                                  # kernel form -> worst observed err / tol


@pytest.fixture(scope="module")
def ctx(gpu_device):
    c = capi.Context(TINY, 0)
    vp, ci = ctypes.c_void_p, ctypes.c_int
    c.lib.rs_debug_dwconv_act.argtypes = [vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, vp, vp]
    c.lib.rs_debug_dwconv_act.restype = ci
    c.lib.rs_debug_layernorm2.argtypes = [vp, vp, vp, vp, vp, vp, ci, ci, ctypes.c_float, vp, vp, vp, vp]
    c.lib.rs_debug_layernorm2.restype = ci
    yield c
    c.close()
    print("\nworst err / tol per kernel form:")
    for form in sorted(WORST):
        print(f"  {form:<44s} {WORST[form]:.3f}")


def rb(t):
    return t.to(torch.bfloat16).to(torch.float32)


def sync():
    torch.cuda.synchronize()


def note(form, got, ref, tol):
    """err / tol of one comparison, kept per kernel form for the summary; the caller asserts <= 1"""
    r = cr.worst_ratio(got, ref, tol)
    WORST[form] = max(WORST.get(form, 0.0), r)
    return r


def same_values(a, b):
    return bool((a.float() == b.float()).all())


def edge_lens(T, tile, half, salt=0):
    """T, 0, 1 and a length inside the halo of the last tile seam below T (seam - half .. seam + half, at most T); where T has no
    seam, a length past T instead (the kernels clamp it)"""
    seam = tile * max(1, (T - 1) // tile)
    edge = T + 2 if T < seam - half else min(seam - half + (T + salt) % (2 * half + 1), T)
    return [T, 0, 1, edge]


class ConvCase:
    """random bf16 inputs of one (T, d, k) in the three layouts (garbage in the padded frames too), uploaded once"""

    def __init__(self, dev, T, d, k, lens, seed):
        g = torch.Generator().manual_seed(seed)
        self.B, self.T, self.d, self.k, self.lens, self.dev = len(lens), T, d, k, lens, dev
        B = self.B
        self.w = torch.randn((k, d), generator=g) / 3
        self.b = 0.1 * torch.randn((d,), generator=g)
        halves = rb(torch.randn((B, T, 2 * d), generator=g))
        self.x = {cr.HALVES: halves, cr.BLOCK32: halves[..., glu_interleave_index(d)].contiguous(),
                  cr.APPLIED: rb(torch.randn((B, T, d), generator=g))}
        self.dx = {ly: x.to(torch.bfloat16).reshape(B * T, -1).to(dev) for ly, x in self.x.items()}
        self.dw, self.db = self.w.to(dev), self.b.to(dev)
        self.dlens = torch.tensor(lens, dtype=torch.int32).to(dev)
        self._ref = {}

    def ref(self, layout, act=cr.SILU):
        if (layout, act) not in self._ref:
            self._ref[layout, act] = cr.glu_dwconv(self.x[layout], self.w, self.b, self.lens, self.k, layout, act)
        return self._ref[layout, act]

    def out_buffer(self):
        return torch.full((self.B * self.T + PAD, self.d), SENTINEL, dtype=torch.bfloat16, device=self.dev)

    def finish(self, out):
        sync()
        assert (out[self.B * self.T:].float() == SENTINEL).all(), "rows past B * T were written"
        return out[:self.B * self.T].cpu().view(self.B, self.T, self.d)

    def glu(self, ctx, layout, generic=0):
        """the public operator at `layout` with RS_GLU_GENERIC = generic"""
        out = self.out_buffer()
        with knob(ctx.lib, "RS_GLU_GENERIC", generic):
            ctx.glu_dwconv(self.dx[layout], self.dw, self.db, self.dlens, self.B, self.T, self.d, self.k, out, layout=layout)
            return self.finish(out)

    def act(self, ctx, act):
        """rs_debug_dwconv_act on the gated input"""
        out = self.out_buffer()
        ctx.check(ctx.lib.rs_debug_dwconv_act(ctx._h, _ptr(self.dx[cr.APPLIED]), _ptr(self.dw), _ptr(self.db), _ptr(self.dlens),
                                              self.B, self.T, self.d, self.k, act, _ptr(out), None))
        return self.finish(out)


def check_conv(form, case, got, layout, act=cr.SILU):
    ref = case.ref(layout, act)
    r = note(form, got, ref, cr.conv_tol(ref))
    print(f"{form} T={case.T} d={case.d} k={case.k} lens={case.lens}: err / tol = {r:.3f}")
    assert r <= 1.0, (form, case.T, case.d, case.k, case.lens, r)


# ---- k = 9: the register-window kernels (48-frame tiles, halo 4) ----------------------------------------------------------------
K9_FORMS = [("fast<9,6,0>", cr.HALVES, 0), ("fast<9,6,1>", cr.BLOCK32, 0), ("dma<9,6>", cr.APPLIED, 0), ("fast<9,6,2>", cr.APPLIED, 2)]


@pytest.mark.parametrize("T,d", [(1, 512), (4, 512), (5, 512), (47, 512), (48, 512), (49, 512), (96, 512), (97, 512), (144, 512),
                                 (97, 1024)])
def test_k9_forms_at_tile_edges(ctx, gpu_device, T, d):
    """d = 512 / 1024: blockIdx.y > 0, c0 >= 256 in all three layouts; T on, one short of and one past a 48-frame seam, and T no
    longer than the halo"""
    case = ConvCase(gpu_device, T, d, 9, edge_lens(T, 48, 4), 1000 + T + d)
    for form, layout, generic in K9_FORMS:
        check_conv(form, case, case.glu(ctx, layout, generic), layout)


@pytest.mark.parametrize("T", [1, 5, 47, 48, 49, 97, 144])
def test_k9_forms_agree(ctx, gpu_device, T):
    """fast == generic (layouts 0, 1), block-of-32 == halves on the permuted input, DMA == fast<.., 2> == generic (layout 2)"""
    case = ConvCase(gpu_device, T, 512, 9, edge_lens(T, 48, 4, salt=3), 2000 + T)
    fast0, fast1 = case.glu(ctx, cr.HALVES), case.glu(ctx, cr.BLOCK32)
    gen0, gen1 = case.glu(ctx, cr.HALVES, 1), case.glu(ctx, cr.BLOCK32, 1)
    assert same_values(fast0, gen0), "fast<9,6,0> != generic, layout 0"
    assert same_values(fast1, gen1), "fast<9,6,1> != generic, layout 1"
    assert same_values(fast1, fast0), "block-of-32 != halves"
    dma, fast2, gen2 = case.glu(ctx, cr.APPLIED), case.glu(ctx, cr.APPLIED, 2), case.glu(ctx, cr.APPLIED, 1)
    assert same_values(dma, fast2), "dma<9,6> != fast<9,6,2>"
    assert same_values(dma, gen2), "dma<9,6> != generic, layout 2"


# ---- the generic kernel (32-frame tiles, any odd k <= 31) ------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 31, 32, 33, 70])
@pytest.mark.parametrize("k", [1, 3, 5, 7, 9, 15, 31])
def test_generic_kernel_at_tile_edges(ctx, gpu_device, k, T):
    """k = 1, 3, 5: the generic kernel is the only form, all three layouts.  k = 31 at layouts 0, 1 (default switches) is its
    largest launch, 62 rows x 256 channels x 4 B = 63 488 B of dynamic LDS.  k = 7, 9, 15, 31 at layout 2 and k = 9 at layouts 0, 1
    reach it under RS_GLU_GENERIC=1 (by default they take dwconv_act / the k = 9 kernels; k = 9 at layouts 0, 1 is run at the
    default switches on this T grid as well)."""
    case = ConvCase(gpu_device, T, 512, k, edge_lens(T, 32, (k - 1) // 2), 3000 + 40 * k + T)
    if k in (1, 3, 5):
        runs = [(cr.HALVES, 0), (cr.BLOCK32, 0), (cr.APPLIED, 0)]
    elif k == 9:
        runs = [(cr.HALVES, 1), (cr.BLOCK32, 1), (cr.APPLIED, 1)]
    elif k == 31:
        runs = [(cr.HALVES, 0), (cr.BLOCK32, 0), (cr.APPLIED, 1)]
    else:
        runs = [(cr.APPLIED, 1)]
    for layout, generic in runs:
        check_conv(f"generic layout {layout}", case, case.glu(ctx, layout, generic), layout)
    if k == 9:
        for layout in (cr.HALVES, cr.BLOCK32):
            check_conv(f"fast<9,6,{layout}>", case, case.glu(ctx, layout), layout)


# ---- dwconv_act (128 frames x 64 channels; the ESPnet and Zipformer conv modules) --------------------------------------------------
@pytest.mark.parametrize("T", [1, 3, 15, 16, 127, 128, 129, 143, 257])
@pytest.mark.parametrize("K", [7, 15, 31])
def test_dwconv_act_at_tile_edges(ctx, gpu_device, K, T):
    """SiLU and SwooshR at d = 64 (one channel block), 320 (not a multiple of 256) and 512; T below the half-width of every K, on and
    around the 128-frame seam.  SiLU at d = 512 through the public entry is the same launch: bit for bit."""
    for d in (64, 320, 512):
        case = ConvCase(gpu_device, T, d, K, edge_lens(T, 128, (K - 1) // 2, salt=d), 4000 + 300 * K + T + d)
        for act, name in ((cr.SILU, "SiLU"), (cr.SWOOSH_R, "SwooshR")):
            got = case.act(ctx, act)
            check_conv(f"dwconv_act<{K},{name}>", case, got, cr.APPLIED, act)
            if act == cr.SILU and d == 512:
                assert torch.equal(case.glu(ctx, cr.APPLIED), got), "rs_glu_dwconv_silu_layout(RS_GLU_APPLIED) != rs_debug_dwconv_act"


@pytest.mark.parametrize("K", [7, 15, 31])
def test_dwconv_act_agrees_with_the_generic_kernel(ctx, gpu_device, K):
    for T in (1, 33, 129, 257):
        case = ConvCase(gpu_device, T, 512, K, edge_lens(T, 128, (K - 1) // 2, salt=1), 5000 + 300 * K + T)
        assert same_values(case.act(ctx, cr.SILU), case.glu(ctx, cr.APPLIED, 1)), f"dwconv_act<{K},SiLU> != generic, T={T}"


def test_conv_rejections_leave_the_output_untouched(ctx, gpu_device):
    T = 20
    for d, k, layout in ((512, 8, cr.HALVES), (512, 33, cr.HALVES), (512, 0, cr.APPLIED), (320, 9, cr.HALVES), (320, 31, cr.APPLIED),
                         (512, 9, 3)):
        case = ConvCase(gpu_device, T, d, max(k, 1), [T, 0, 1], 6000 + d + k)
        out = case.out_buffer()
        with pytest.raises(capi.RsError):
            ctx.glu_dwconv(case.dx[min(layout, 2)], case.dw, case.db, case.dlens, case.B, T, d, k, out, layout=layout)
        sync()
        assert (out.float() == SENTINEL).all(), (d, k, layout)
    for k, act in ((9, cr.SILU), (31, 2), (31, -1)):
        case = ConvCase(gpu_device, T, 512, k, [T, 0, 1], 6100 + k)
        out = case.out_buffer()
        with pytest.raises(capi.RsError):
            ctx.check(ctx.lib.rs_debug_dwconv_act(ctx._h, _ptr(case.dx[cr.APPLIED]), _ptr(case.dw), _ptr(case.db), _ptr(case.dlens),
                                                  case.B, T, 512, k, act, _ptr(out), None))
        sync()
        assert (out.float() == SENTINEL).all(), (k, act)
    case = ConvCase(gpu_device, T, 96, 7, [T, 0, 1], 6200)                # dwconv_act: d % 64
    out = case.out_buffer()
    with pytest.raises(capi.RsError):
        case.act(ctx, cr.SILU)
    with pytest.raises(capi.RsError):                                     # a null pointer never reaches the launcher
        ctx.check(ctx.lib.rs_debug_dwconv_act(ctx._h, _ptr(case.dx[cr.APPLIED]), _ptr(case.dw), None, _ptr(case.dlens), case.B, T, 96,
                                              7, 0, _ptr(out), None))


# ---- LayerNorm --------------------------------------------------------------------------------------------------------------------
def ln_case(dev, M, d, seed):
    """M rows (+ PAD rows of garbage that must not be read into anything) cycling through N(1.5, 3), N(+100, 0.1), N(-100, 0.1), a
    constant row and an all-zero row; which kind row 0 is moves with d, so M = 1 meets every kind over the d grid"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((M + PAD, d), generator=g)
    kinds = [(r + d // 256) % 5 for r in range(M)]
    for r, kind in enumerate(kinds):
        x[r] = (x[r] * 3 + 1.5, x[r] * 0.1 + 100, x[r] * 0.1 - 100, torch.full((d,), 3.7), torch.zeros(d))[kind]
    gb = [1 + 0.1 * torch.randn((d,), generator=g), 0.1 * torch.randn((d,), generator=g),
          1 + 0.1 * torch.randn((d,), generator=g), 0.1 * torch.randn((d,), generator=g)]
    return x, kinds, gb, x.to(dev), [t.to(dev) for t in gb]


def ln_call(ctx, x, g, b, M, d, o16, o32):
    ctx.check(ctx.lib.rs_layernorm(ctx._h, _ptr(x), _ptr(g), _ptr(b), M, d, EPS, _ptr(o16), _ptr(o32), None))


def ln_buffers(dev, M, d):
    return (torch.full((M + PAD, d), SENTINEL, dtype=torch.bfloat16, device=dev),
            torch.full((M + PAD, d), SENTINEL, dtype=torch.float32, device=dev))


@pytest.mark.parametrize("d", [256, 512, 768, 1024, 1280, 1536, 1792, 2048])
def test_layernorm_every_width_and_row_edge(ctx, gpu_device, d):
    """all eight NV; M around the four rows of a workgroup; rows whose mean dwarfs their spread (what the two-pass statistics are
    for), a constant row (-> beta) and a zero row; f32-only, bf16-only, both outputs, in place"""
    for M in (1, 3, 4, 5, 77):
        x, kinds, (g1, b1, _, _), dx, (dg, db, _, _) = ln_case(gpu_device, M, d, 10 * d + M)
        ref = cr.layernorm(x[:M], g1, b1, EPS)
        o16, o32 = ln_buffers(gpu_device, M, d)
        ln_call(ctx, dx, dg, db, M, d, o16, o32)
        sync()
        assert (o32[M:] == SENTINEL).all() and (o16[M:].float() == SENTINEL).all(), "rows past M were written"
        r32 = note(f"layernorm<{d // 256}> f32", o32[:M].cpu(), ref, cr.ln_tol(x[:M], EPS))
        r16 = note(f"layernorm<{d // 256}> bf16", o16[:M].cpu().float(), ref, cr.ln_tol(x[:M], EPS, ref))
        print(f"layernorm d={d} M={M}: err / tol = {r32:.3f} (f32), {r16:.3f} (bf16)")
        assert r32 <= 1.0 and r16 <= 1.0, (d, M, r32, r16)
        for r, kind in enumerate(kinds):
            if kind >= 3:                   # constant and zero rows: beta
                assert cr.worst_ratio(o32[r:r + 1].cpu(), b1.double()[None], cr.ln_tol(x[r:r + 1], EPS)) <= 1.0, (d, M, r, kind)
        only16, only32 = ln_buffers(gpu_device, M, d)
        ln_call(ctx, dx, dg, db, M, d, None, only32)
        ln_call(ctx, dx, dg, db, M, d, only16, None)
        inplace = dx.clone()
        ln_call(ctx, inplace, dg, db, M, d, None, inplace)
        sync()
        assert torch.equal(only32, o32) and torch.equal(only16, o16)
        assert torch.equal(inplace[:M], o32[:M]) and torch.equal(inplace[M:], dx[M:])


def test_layernorm_rejections_and_empty_call(ctx, gpu_device):
    for d in (128, 2304):
        x, _, _, dx, (dg, db, _, _) = ln_case(gpu_device, 4, d, d)
        o16, o32 = ln_buffers(gpu_device, 4, d)
        with pytest.raises(capi.RsError):
            ln_call(ctx, dx, dg, db, 4, d, o16, o32)
        sync()
        assert (o32 == SENTINEL).all() and (o16.float() == SENTINEL).all()
    x, _, _, dx, (dg, db, dg2, db2) = ln_case(gpu_device, 4, 256, 1)
    o16, o32 = ln_buffers(gpu_device, 4, 256)
    ln_call(ctx, dx, dg, db, 0, 256, o16, o32)                    # M = 0: nothing to do, RS_OK
    ctx.check(ctx.lib.rs_debug_layernorm2(ctx._h, _ptr(dx), _ptr(dg), _ptr(db), _ptr(dg2), _ptr(db2), 0, 256, EPS, _ptr(o32), _ptr(o16),
                                          None, None))
    sync()
    assert (o32 == SENTINEL).all() and (o16.float() == SENTINEL).all()


def ln2_call(ctx, x, gb, M, d, o32, o16, stats):
    ctx.check(ctx.lib.rs_debug_layernorm2(ctx._h, _ptr(x), _ptr(gb[0]), _ptr(gb[1]), _ptr(gb[2]), _ptr(gb[3]), M, d, EPS, _ptr(o32),
                                          _ptr(o16), _ptr(stats), None))


@pytest.mark.parametrize("d", [256, 512, 1024, 2048])
def test_layernorm2_is_two_layernorms_and_their_statistics(ctx, gpu_device, d):
    """out_bf16 = rs_layernorm(out_f32; g2, b2) bit for bit; stats = the first norm's (mean, rstd); the stats-only call (the deferred
    output norm) gives the same bits and writes no f32 rows; neither f32 rows nor stats is refused.

    out_f32 against rs_layernorm(x; g1, b1) is NOT bit for bit, and is held to ln_tol against float64 like rs_layernorm itself
    instead.  The operation that differs is the sum of squared deviations, q += (a*a + b*b) + (c*c + d*d): it is written the same
    in both kernels, but under the default -ffp-contract=fast the compiler fuses a product into the neighbouring add
    (v_pk_mul_f32 + v_pk_fma_f32) in layernorm_kernel and in layernorm2_kernel's second norm, and leaves layernorm2_kernel's first
    norm as two v_pk_mul_f32 and plain adds.  The variance, hence rstd and the rows, differ in the last float32 bit on some rows
    (measured on an MI355X: up to a sixth of the elements of a case (whole rows), by at most 9.5e-7 = 0.035 of ln_tol; many cases are equal).  Both
    roundings are inside ln_tol of float64; the kernels are left as they are."""
    for M in (1, 3, 4, 5, 77):
        x, kinds, gb, dx, dgb = ln_case(gpu_device, M, d, 20 * d + M)
        _, y = ln_buffers(gpu_device, M, d)
        ln_call(ctx, dx, dgb[0], dgb[1], M, d, None, y)
        o16, o32 = ln_buffers(gpu_device, M, d)
        stats = torch.full((M + PAD, 2), SENTINEL, dtype=torch.float32, device=gpu_device)
        ln2_call(ctx, dx, dgb, M, d, o32, o16, stats)
        z, _ = ln_buffers(gpu_device, M, d)
        ln_call(ctx, o32, dgb[2], dgb[3], M, d, z, None)
        sync()
        y_ref = cr.layernorm(x[:M], gb[0], gb[1], EPS)
        r32 = note(f"layernorm2<{d // 256}> f32", o32[:M].cpu(), y_ref, cr.ln_tol(x[:M], EPS))
        pair = note(f"layernorm2<{d // 256}> f32 vs layernorm", o32[:M].cpu(), y[:M].cpu().double(), cr.ln_tol(x[:M], EPS))
        y32 = o32[:M].cpu()
        z_ref = cr.layernorm(y32, gb[2], gb[3], EPS)
        r16 = note(f"layernorm2<{d // 256}> bf16", o16[:M].cpu().float(), z_ref, cr.ln_tol(y32, EPS, z_ref))
        print(f"layernorm2 d={d} M={M}: err / tol = {r32:.3f} (f32), {r16:.3f} (bf16); f32 rows vs rs_layernorm: "
              f"{int((o32[:M] != y[:M]).sum())} of {M * d} elements differ, by at most {float((o32[:M] - y[:M]).abs().max()):.3g} = {pair:.4f} of ln_tol; "
              f"bf16 rows equal rs_layernorm(out_f32): {torch.equal(o16, z)}")
        assert r32 <= 1.0 and pair <= 1.0 and r16 <= 1.0, (d, M, r32, pair, r16)
        assert torch.equal(o16, z), (d, M, "out_bf16 != rs_layernorm(out_f32; g2, b2)")
        assert (o32[M:] == SENTINEL).all() and (stats[M:] == SENTINEL).all()
        _, _, (mean, rstd) = cr.layernorm_pair(x[:M], *gb, EPS)
        got = stats[:M].cpu().double()
        rm = float(((got[:, 0] - mean).abs() / (2.0 ** -22 * (mean.abs() + 1))).max())
        rr = float(((got[:, 1] - rstd).abs() / (2.0 ** -20 * rstd)).max())
        WORST[f"layernorm2<{d // 256}> stats mean"] = max(WORST.get(f"layernorm2<{d // 256}> stats mean", 0.0), rm)
        WORST[f"layernorm2<{d // 256}> stats rstd"] = max(WORST.get(f"layernorm2<{d // 256}> stats rstd", 0.0), rr)
        print(f"layernorm2 d={d} M={M}: stats err / tol = {rm:.3f} (mean), {rr:.3f} (rstd)")
        assert rm <= 1.0 and rr <= 1.0, (d, M, rm, rr)
        # the deferred form: statistics and the second norm only
        s16, untouched = ln_buffers(gpu_device, M, d)
        stats2 = torch.full_like(stats, SENTINEL)
        ln2_call(ctx, dx, dgb, M, d, None, s16, stats2)
        # the first norm's rows without its statistics
        n16, n32 = ln_buffers(gpu_device, M, d)
        ln2_call(ctx, dx, dgb, M, d, n32, n16, None)
        sync()
        assert torch.equal(s16, o16) and torch.equal(stats2, stats) and (untouched == SENTINEL).all()
        assert torch.equal(n16, o16) and torch.equal(n32, o32)
        assert torch.equal(dx.cpu(), x), "the input was written"
        r16, _ = ln_buffers(gpu_device, M, d)
        with pytest.raises(capi.RsError):
            ln2_call(ctx, dx, dgb, M, d, None, r16, None)
        sync()
        assert (r16.float() == SENTINEL).all()
