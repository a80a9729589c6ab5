"""-m gpu: the compile-time epilogue forms of the bf16 GEMM (k_gemm_bf16.hip: ACT / UNIT_ALPHA) against the run-time-flag
form of the same launch.

Every case runs twice on the same operands, with $RS_GEMM_EPI_GENERIC at 0 (the launcher may pick a compile-time form) and at 1
(every launch takes the form that tests the ReLU / SiLU bits and multiplies by alpha at run time), and the two outputs must agree
bit for bit — NaNs by position.  Shapes cross every seam of the launcher: a lone row, a partial 64-row tile, one row past a 192-
and a 256-row tile, a pair of tiles plus a single with a ragged last tile; a partial column tile; one K tile, the ring-carry
threshold and the encoder's depth; each tile height forced.  Rows 1 .. 6 of A are one-hot against a weight column of ones, so
the activation sees +-88, +-0, 1e-30 and a NaN row exactly (plus the bias where there is one).
"""
import ctypes

import pytest
import torch

from reazonspeech_amd.runtime import capi
from reazonspeech_amd.runtime.capi import _ptr
from reazonspeech_amd.runtime.config import TINY
from knobs import knob

pytestmark = pytest.mark.gpu

MS = (1, 63, 193, 257, 520)
NS = (256, 264, 512)
KS = (64, 128, 1024)
TILES = (64, 128, 192, 256)
TAILS = (88.0, -88.0, float("nan"), 0.0, -0.0, 1e-30)
PAD, SENTINEL = 8, 7.0
F32 = capi.GEMM_OUT_F32
RES = capi.GEMM_RESIDUAL | capi.GEMM_OUT_F32
# name, flags, alpha, kind of call
EPILOGUES = (
    ("bf16", 0, 1.0, "plain"),
    ("bf16_silu", capi.GEMM_SILU, 1.0, "plain"),
    ("bf16_relu", capi.GEMM_RELU, 1.0, "plain"),
    ("bf16_relu_rowmask", capi.GEMM_RELU | capi.GEMM_ROWMASK, 1.0, "mask"),
    ("glu", capi.GEMM_GLU, 1.0, "glu"),
    ("f32", F32, 1.0, "plain"),
    ("res_alpha1", RES, 1.0, "res"),
    ("res_alpha_half", RES, 0.5, "res"),
    ("res_row_stats", RES, 1.0, "resln"),
    ("res_bf16_copy", RES, 1.0, "res2"),
)


@pytest.fixture(scope="module")
def ctx(gpu_device):
    c = capi.Context(TINY, 0)
    vp, ci = ctypes.c_void_p, ctypes.c_int
    c.lib.rs_debug_gemm_bf16_res.argtypes = [vp, vp, ci, vp, ci, vp, ci, ci, ci, ci, ci, vp, ctypes.c_float, vp, vp, vp, vp, vp, ci, vp]
    c.lib.rs_debug_gemm_bf16_res.restype = ci
    c.lib.rs_debug_gemm_epi_form.argtypes = [ci, ci, ctypes.c_float, ci, ci]
    c.lib.rs_debug_gemm_epi_form.restype = ci
    yield c
    c.close()


class Operands:
    """seeded operands of one (M, N, K), made once and left unchanged"""

    def __init__(self, M, N, K, dev):
        g = torch.Generator().manual_seed(1000 * M + 10 * N + K)
        A = torch.randn((M, K), generator=g)
        W = torch.randn((N, K), generator=g) / K ** 0.5
        if M > len(TAILS):
            W[:, 0] = 1.0
            for i, v in enumerate(TAILS):
                A[1 + i] = 0.0
                A[1 + i, 0] = v
        self.M, self.N, self.K, self.dev = M, N, K, dev
        self.A, self.W = A.to(torch.bfloat16).to(dev), W.to(torch.bfloat16).to(dev)
        self.bias = torch.randn((N,), generator=g).to(dev)
        self.res = torch.randn((M, N), generator=g).to(dev)
        mean, rstd = torch.randn((M,), generator=g), torch.rand((M,), generator=g) + 0.5
        self.stats = torch.stack([mean, rstd], dim=1).contiguous().to(dev)
        self.ln_g, self.ln_b = torch.randn((N,), generator=g).to(dev), torch.randn((N,), generator=g).to(dev)
        # two utterances of `steps` rows each; the second keeps none
        self.steps = (M + 1) // 2
        self.lens = torch.tensor([max(1, self.steps - 2), 0], dtype=torch.int32).to(dev)

    def run(self, ctx, flags, alpha, kind, with_bias):
        """one launch -> (out, bf16 copy or None), both with PAD sentinel rows behind row M"""
        M, N = self.M, self.N
        f32 = bool(flags & F32)
        out = torch.full((M + PAD, N // 2 if kind == "glu" else N), SENTINEL, dtype=torch.float32 if f32 else torch.bfloat16, device=self.dev)
        copy = torch.full((M + PAD, N), SENTINEL, dtype=torch.bfloat16, device=self.dev) if kind == "res2" else None
        bias = self.bias if with_bias else None
        if with_bias:
            flags |= capi.GEMM_BIAS
        res = self.res if flags & capi.GEMM_RESIDUAL else None
        if kind in ("resln", "res2"):
            ln = kind == "resln"
            ctx.check(ctx.lib.rs_debug_gemm_bf16_res(ctx._h, _ptr(self.A), self.K, _ptr(self.W), self.K, _ptr(out), N, M, N, self.K, flags, _ptr(bias),
                                                     alpha, _ptr(res), _ptr(self.stats if ln else None), _ptr(self.ln_g if ln else None),
                                                     _ptr(self.ln_b if ln else None), _ptr(copy), N if copy is not None else 0, None))
        elif kind == "mask":
            ctx.gemm(self.A, self.W, out[:M], flags=flags, bias=bias, alpha=alpha, mask_lens=self.lens, mask_rows=1, mask_steps=self.steps)
        else:
            ctx.gemm(self.A, self.W, out[:M], flags=flags, bias=bias, alpha=alpha, residual=res)
        return out, copy


def same_bits(a, b):
    """device bool: NaNs at the same positions, every other element bit for bit"""
    ia, ib = (a.view(torch.int32), b.view(torch.int32)) if a.dtype == torch.float32 else (a.view(torch.int16), b.view(torch.int16))
    na, nb = torch.isnan(a), torch.isnan(b)
    return (na == nb).all() & ((ia == ib) | na).all()


def cases(N):
    for name, flags, alpha, kind in EPILOGUES:
        if kind == "glu" and N % 64:
            continue                                              # the launcher refuses GLU unless N % 64 == 0
        for with_bias in (False, True):
            yield name + ("+bias" if with_bias else ""), flags, alpha, kind, with_bias
    yield "bf16_relu_and_silu+bias", capi.GEMM_RELU | capi.GEMM_SILU, 1.0, "plain", True


@pytest.mark.parametrize("tile", TILES)
def test_compile_time_forms_match_run_time_form(ctx, gpu_device, tile):
    bad = []
    with knob(ctx.lib, "RS_GEMM_TILE", tile):
        for M in MS:
            for N in NS:
                for K in KS:
                    ops = Operands(M, N, K, gpu_device)
                    verdicts = []
                    for name, flags, alpha, kind, with_bias in cases(N):
                        outs = []
                        for generic in (0, 1):
                            with knob(ctx.lib, "RS_GEMM_EPI_GENERIC", generic):
                                outs.append(ops.run(ctx, flags, alpha, kind, with_bias))
                        ok = same_bits(outs[0][0], outs[1][0])
                        if outs[0][1] is not None:
                            ok = ok & same_bits(outs[0][1], outs[1][1])
                        ok = ok & (outs[0][0][M:].float() == SENTINEL).all()      # nothing behind row M
                        verdicts.append((name, ok))
                    flat = torch.stack([v for _, v in verdicts]).cpu()           # one synchronisation per shape
                    bad += [(M, N, K, name) for (name, _), v in zip(verdicts, flat) if not v]
    assert not bad, f"tile {tile}: {len(bad)} cases differ from the run-time form, first {bad[:8]}"


def test_tail_inputs_reach_the_activation(ctx, gpu_device):
    """the one-hot rows do what the module docstring says: without a bias the SiLU launch sees +-88, a NaN row, +-0 and 1e-30"""
    ops = Operands(63, 256, 64, gpu_device)
    out, _ = ops.run(ctx, capi.GEMM_SILU, 1.0, "plain", False)
    got = out[1:7, :4].float().cpu()
    assert (got[0] == 88.0).all() and (got[1].abs() < 1e-30).all() and torch.isnan(got[2]).all() and (got[3:5] == 0.0).all()
    assert ((got[5] > 0.0) & (got[5] < 1e-30)).all()              # silu(x) = x / 2 for tiny x
    assert not torch.isnan(out[:1].float()).any() and not torch.isnan(out[7:63].float()).any()


def test_launcher_takes_the_compile_time_forms(ctx):
    """the cases above compare two different kernels where a compile-time form exists: SiLU and plain bf16 at 256 rows, GLU and
    ReLU + row mask at 192"""
    form = ctx.lib.rs_debug_gemm_epi_form
    assert form(256, capi.GEMM_BIAS | capi.GEMM_SILU, 1.0, 0, 0) == 3 + 8 and form(256, capi.GEMM_BIAS, 1.0, 0, 0) == 1 + 8
    assert form(192, capi.GEMM_BIAS | capi.GEMM_GLU, 1.0, 0, 0) == 1 + 8 and form(192, capi.GEMM_RELU | capi.GEMM_ROWMASK, 1.0, 0, 0) == 2 + 8
    with knob(ctx.lib, "RS_GEMM_EPI_GENERIC", 1):
        assert form(256, capi.GEMM_BIAS | capi.GEMM_SILU, 1.0, 0, 0) == 0 and form(192, capi.GEMM_BIAS | capi.GEMM_GLU, 1.0, 0, 0) == 0
