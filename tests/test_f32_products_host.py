"""CPU: the float32 product test hooks are exported, and the split emulation the GPU operator tests compare against
(tests/f32x3_split.py) is what it claims to be."""
import ctypes
import os
import re

import numpy as np
import torch

from reazonspeech_amd import build as rs_build
from reazonspeech_amd.runtime import capi
from f32x3_split import ONE_PLUS, exact_operand, r3_matmul, split_bf16

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOOKS = ("rs_debug_conv3x3_f32", "rs_debug_gemm_f32_skinny")


def test_debug_hooks_are_exported_but_not_part_of_the_abi():
    lib = ctypes.CDLL(rs_build.build())
    for s in HOOKS:
        assert hasattr(lib, s), f"{s} not exported"
        assert s not in capi.EXPORTS
    header = open(os.path.join(ROOT, "include", "rs_asr.h")).read()
    assert not any(re.search(rf"\b{s}\b", header) for s in HOOKS)


def rne_bf16_bits(x):
    """bf16 rounding to nearest even on the float32 bit pattern (finite inputs): the reference for torch's .to(bfloat16)"""
    u = np.asarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(np.float32)


def test_split_rounds_to_nearest_even_and_reproduces_x():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(200000, generator=g) * torch.exp2(torch.randint(-30, 30, (200000,), generator=g).float())
    # ties of both roundings: 1 + 2^-8 (even: down), 1 + 3 * 2^-8 (odd: up); x - hi a tie again for lo
    ties = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 1 + 2.0 ** -9 + 2.0 ** -17 + 2.0 ** -23, 3.0 + 2.0 ** -7])
    x = torch.cat([x, ties])
    hi, lo = split_bf16(x)
    assert torch.equal(hi, torch.from_numpy(rne_bf16_bits(x.numpy())))
    assert torch.equal(lo, torch.from_numpy(rne_bf16_bits((x - hi).numpy())))
    assert torch.equal(hi.to(torch.bfloat16).float(), hi) and torch.equal(lo.to(torch.bfloat16).float(), lo)
    assert torch.all((hi.double() + lo.double() - x.double()).abs() <= 2.0 ** -16 * x.double().abs())
    assert torch.all((x.double() - hi.double()).abs() <= 2.0 ** -8 * x.double().abs())


def test_r3_drops_only_the_lo_lo_term():
    g = torch.Generator().manual_seed(4)
    A, W = torch.randn((17, 64), generator=g), torch.randn((9, 64), generator=g)
    (ha, la), (hw, lw) = split_bf16(A), split_bf16(W)
    full = (ha.double() + la.double()) @ (hw.double() + lw.double()).t()
    assert torch.allclose(r3_matmul(A, W) + la.double() @ lw.double().t(), full, rtol=0, atol=1e-13)


def _chain_f32(*terms):
    """terms added one after the other in float32, the order of the kernel's three MFMAs"""
    acc = np.float32(0)
    for t in terms:
        acc = np.float32(acc + np.float32(t))
    return acc


def test_exact_operands_are_exact_in_float32():
    g = torch.Generator().manual_seed(5)
    x, h, l = exact_operand((4096,), g)
    hi, lo = split_bf16(x)
    assert torch.equal(hi, h) and torch.equal(lo, l), "the split must recover the construction"
    one_hi, one_lo = split_bf16(torch.tensor([ONE_PLUS]))
    assert one_hi.item() == 1.0 and one_lo.item() == 2.0 ** -10
    xs, hs, ls = x.numpy().astype(np.float64), h.numpy().astype(np.float64), l.numpy().astype(np.float64)
    r3 = hs + ls + 2.0 ** -10 * hs                                # = r3 of (ONE_PLUS * I) against x, either way round
    for i in range(len(xs)):
        # W = x against A = ONE_PLUS I: wl.ah, wh.al, wh.ah;  A = x against W = ONE_PLUS I: wl.ah, wh.al, wh.ah with the roles swapped
        assert float(_chain_f32(ls[i], 2.0 ** -10 * hs[i], hs[i])) == r3[i]
        assert float(_chain_f32(2.0 ** -10 * hs[i], ls[i], hs[i])) == r3[i]
    # the inputs tell the three-term product from the exact one and catch a lo rounded toward zero
    exact = (x.double() * ONE_PLUS).float().double()
    assert (torch.from_numpy(r3) != exact).float().mean() > 0.9
    lo_trunc = ((x - hi).view(torch.int32) & ~0xFFFF).view(torch.float32)
    assert (lo_trunc != lo).float().mean() > 0.2
