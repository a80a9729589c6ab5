"""CPU: the float64 reference and the bf16 tolerance of tests/attention_ref.py are right, and they discriminate.

  * the reference equals oracle/model.py's attention_core (the `fp32` recipe on float64 inputs: the gather form of the rel-shift)
    for full, windowed, global-token and one-sided windows, and a literal triple loop at T <= 9;
  * zero-filled instead of poisoned padding does not change it, and a length above T is the length T;
  * a float32 emulation of the device recipe (csrc/k_attention.hip: float32 scores, an online softmax over 32-key blocks,
    probabilities rounded to bf16 for the P.V product while the normaliser sums the unrounded ones, one bf16 rounding of the
    context) stays INSIDE the tolerance on every bf16 case tests/test_gpu_attention_edges.py runs;
  * the same emulation with one deliberate fault lands OUTSIDE it on the case meant to catch that fault.
"""
import math

import pytest
import torch

import attention_ref as ar
from oracle import model as om
from reazonspeech_amd.runtime.config import TINY

NEG = -1.0e30


def oracle_core(case, window, recipe="fp32"):
    cfg = TINY.with_(n_heads=case.H, att_left=window[0], att_right=window[1], n_global=window[2])
    lens = torch.tensor(ar.clamp_lens(case.lens, case.T), dtype=torch.int64)
    return om.attention_core(cfg, case.q.double(), case.k.double(), case.v.double(), case.pos.double(), case.bias_u.double(),
                             case.bias_v.double(), lens, recipe)


@pytest.mark.parametrize("window", [ar.FULL, (5, 3, 0), (0, 0, 0), (20, 10, 1), (20, 10, 33), (-1, 4, 0), (4, -1, 0), (128, 128, 1)])
@pytest.mark.parametrize("dh,T", [(128, 70), (64, 45)])
def test_reference_equals_the_oracle(dh, T, window):
    case = ar.make(dh, T, window, [T, 0, 1, 33, T + 5])
    ctx, A = ar.relpos_attention(*case.args(), *window, round_q="f32")
    want = oracle_core(case, window)
    assert (ctx - want).abs().max() <= 1e-12
    assert (A >= ctx.abs() - 1e-12).all()


def triple_loop(case, window):
    """ctx by the definition, one scalar at a time"""
    left, right, n_global = window
    B, T, H, dh = case.q.shape
    out = torch.zeros((B, T, H * dh), dtype=torch.float64)
    q, k, v, pos = (t.double() for t in (case.q, case.k, case.v, case.pos))
    u, w = case.bias_u.double(), case.bias_v.double()
    for b in range(B):
        n = min(case.lens[b], T)
        for h in range(H):
            for i in range(n):
                s = {}
                for j in range(n):
                    see = True
                    if left >= 0 or right >= 0:
                        see = (left < 0 or i - j <= left) and (right < 0 or j - i <= right)
                        see = see or (n_global > 0 and (i < n_global or j < n_global))
                    if see:
                        s[j] = sum(float((q[b, i, h, e] + u[h, e]) * k[b, j, h, e] + (q[b, i, h, e] + w[h, e]) * pos[j - i + T - 1, h, e])
                                   for e in range(dh)) / math.sqrt(dh)
                m = max(s.values())
                den = sum(math.exp(x - m) for x in s.values())
                for j, x in s.items():
                    out[b, i, h * dh:(h + 1) * dh] += math.exp(x - m) / den * v[b, j, h]
    return out


@pytest.mark.parametrize("window", [ar.FULL, (2, 1, 0), (0, 0, 0), (1, 2, 2), (-1, 1, 0), (1, -1, 0)])
def test_reference_equals_a_triple_loop(window):
    case = ar.Case(9, 2, 8, [9, 0, 1, 5, 12], seed=9)
    ctx, _ = ar.relpos_attention(*case.args(), *window, round_q="f32")
    assert (ctx - triple_loop(case, window)).abs().max() <= 1e-12


@pytest.mark.parametrize("window", [ar.FULL, (5, 3, 0), (20, 10, 2)])
def test_padding_content_and_overlong_lengths_do_not_reach_the_reference(window):
    lens = [70, 0, 1, 33, 75]
    poisoned, zeroed = ar.make(128, 70, window, lens), ar.make(128, 70, window, lens, poison=False)
    assert not torch.equal(poisoned.k, zeroed.k) and torch.equal(poisoned.k[0], zeroed.k[0])
    for round_q in ("bf16", "f32"):
        a, b = ar.relpos_attention(*poisoned.args(), *window, round_q=round_q), ar.relpos_attention(*zeroed.args(), *window, round_q=round_q)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        clamped = ar.relpos_attention(*poisoned.args()[:-1], [70, 0, 1, 33, 70], *window, round_q=round_q)
        assert torch.equal(clamped[0], a[0])
        for b_, n in enumerate(ar.clamp_lens(lens, 70)):
            assert (a[0][b_, n:] == 0).all() and (a[1][b_, n:] == 0).all()


# ---- the device recipe in float32, and what it looks like with one thing wrong ---------------------------------------------------
def emulate(case, window, chunk, fault=None):
    """bf16 context [B][T][H*dh] by the staged kernel's recipe.  chunk: key blocks per staged chunk (5 at head_dim 128, 6 / 4 at 64).
    fault: None or one of mask_le, left+1, right+1, global+1, left-1, pos+1, pos-1, swap_uv, drop_last_block, drop_chunk2."""
    left, right, n_global = window
    if fault == "left+1" and left >= 0:
        left += 1
    if fault == "left-1" and left >= 0:
        left -= 1
    if fault == "right+1" and right >= 0:
        right += 1
    if fault == "global+1":
        n_global += 1
    B, T, H, dh = case.q.shape
    bu, bv = (case.bias_v, case.bias_u) if fault == "swap_uv" else (case.bias_u, case.bias_v)
    qu, qv = ar.rb(case.q + bu), ar.rb(case.q + bv)
    shift = {"pos+1": 1, "pos-1": -1}.get(fault, 0)
    ac = torch.einsum("bihe,bjhe->bhij", qu, case.k)
    bd = torch.empty_like(ac)
    for i in range(T):
        rows = (torch.arange(T) - i + T - 1 + shift).clamp(0, 2 * T - 2)
        bd[:, :, i, :] = torch.einsum("bhe,jhe->bhj", qv[:, i], case.pos[rows])
    s = (ac + bd) * torch.tensor(dh ** -0.5, dtype=torch.float32)
    n = torch.tensor(ar.clamp_lens(case.lens, T))
    ok = ar.visible(T, [T] * B, left, right, n_global)                   # the window alone
    i, j = torch.arange(T)[None, :, None], torch.arange(T)[None, None, :]
    nb = n[:, None, None]
    ok = ok & (i < nb) & ((j <= nb) if fault == "mask_le" else (j < nb))
    ok = ok[:, None]
    m_run = torch.full((B, H, T), NEG)
    l_run = torch.zeros((B, H, T))
    o = torch.zeros((B, H, T, dh))
    vt = case.v.permute(0, 2, 1, 3)                                       # [B][H][T][dh]
    for blk in range((T + 31) // 32):
        if fault == "drop_chunk2" and chunk <= blk < 2 * chunk:
            continue
        j0, j1 = 32 * blk, min(32 * blk + 32, T)
        okb = ok[..., j0:j1]
        if fault == "drop_last_block":
            okb = okb & (blk != (n - 1).clamp(min=0) // 32)[:, None, None, None]
        sc = torch.where(okb, s[..., j0:j1], torch.tensor(NEG))
        m_new = torch.maximum(m_run, sc.max(dim=-1).values)
        alpha = torch.exp(m_run - m_new)
        e = torch.where(sc > 0.5 * NEG, torch.exp(sc - m_new[..., None]), torch.zeros(()))
        l_run = l_run * alpha + e.sum(dim=-1)
        o = o * alpha[..., None] + torch.einsum("bhij,bhje->bhie", ar.rb(e), vt[:, :, j0:j1])
        m_run = m_new
    inv = torch.where(l_run > 0, 1.0 / torch.where(l_run > 0, l_run, torch.ones(())), torch.zeros(()))
    return ar.rb(o * inv[..., None]).permute(0, 2, 1, 3).reshape(B, T, H * dh)


def ratio(case, window, got):
    ref, A = ar.relpos_attention(*case.args(), *window, round_q="bf16")
    tol = ar.tol_bf16(ref, A, ar.score_delta(*case.args(), *window))
    for b, n in enumerate(ar.clamp_lens(case.lens, case.T)):
        assert (got[b, n:] == 0).all()
    v = lambda x: ar.valid_rows(x, case.lens)
    return ar.worst_ratio(v(got), v(ref), v(tol))


def test_the_clean_recipe_is_inside_the_tolerance_on_every_gpu_case():
    worst, where = 0.0, None
    for dh, T, window, lens in ar.all_bf16_cases():
        case = ar.make(dh, T, window, lens)
        r = ratio(case, window, emulate(case, window, 5 if dh == 128 else 6))
        if r > worst:
            worst, where = r, (dh, T, window, lens)
        assert r <= 1.0, (dh, T, window, lens, r)
    print(f"\nCPU emulation of the bf16 recipe, {len(ar.all_bf16_cases())} cases: worst err / tol = {worst:.3f} at {where}")


WIN_LENS = ar.edge_lens(161, 32)
MUTANTS = [("mask_le", 161, ar.FULL), ("mask_le", 161, (5, 3, 0)), ("left+1", 161, (5, 3, 0)), ("left+1", 161, (31, 0, 0)),
           ("right+1", 161, (5, 3, 0)), ("right+1", 161, (0, 31, 0)), ("right+1", 161, (-1, 4, 0)), ("left+1", 161, (4, -1, 0)),
           ("global+1", 161, (20, 10, 1)), ("global+1", 161, (20, 10, 32)), ("left-1", 161, (5, 3, 0)), ("left-1", 353, (200, 17, 0)),
           ("pos+1", 161, ar.FULL), ("pos-1", 161, ar.FULL), ("pos+1", 353, (20, 10, 0)), ("swap_uv", 161, ar.FULL),
           ("drop_last_block", 161, ar.FULL), ("drop_last_block", 353, (20, 10, 2)), ("drop_chunk2", 161, ar.FULL),
           ("drop_chunk2", 353, (200, 17, 0))]


@pytest.mark.parametrize("fault,T,window", MUTANTS)
@pytest.mark.parametrize("dh", [128, 64])
def test_one_fault_is_outside_the_tolerance(dh, fault, T, window):
    if fault == "drop_chunk2" and dh == 64 and T == 161:
        T = 257                              # head_dim 64 stages 6 key blocks at once: the second chunk begins at key 192
    case = ar.make(dh, T, window, ar.edge_lens(T, 32))
    chunk = 5 if dh == 128 else 6
    clean = ratio(case, window, emulate(case, window, chunk))
    r = ratio_or_inf(case, window, emulate(case, window, chunk, fault))
    print(f"head_dim {dh} T={T} window={window} {fault}: err / tol = {r:.1f} (clean {clean:.3f})")
    assert clean <= 1.0 < r


def ratio_or_inf(case, window, got):
    """a fault may also break the zero rows; that counts as caught"""
    try:
        return ratio(case, window, got)
    except AssertionError:
        return float("inf")


def test_a_mutant_that_changes_nothing_shows_nothing():
    """att_left + 1 on a window that is unbounded to the left is the same window"""
    window = (-1, 4, 0)
    case = ar.make(128, 161, window, WIN_LENS)
    assert torch.equal(emulate(case, window, 5, "left+1"), emulate(case, window, 5))
