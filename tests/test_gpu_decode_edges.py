"""-m gpu: the greedy transducer loop (csrc/k_rnnt.hip rs_rnnt_greedy_impl) at every seam of its dispatch, on the fixtures of
tests/decode_edges_ref.py (tests/test_decode_edges_host.py shows on the CPU that each reaches its edge).  Every case drives
ctx.rnnt_greedy directly and requires token ids AND emission frames equal to oracle/rnnt_greedy.c (k2_greedy.c), bit for bit, and
the `screen` / `narrow` / `lookahead` flags of $RS_DECODE_TRACE it was written for, so that a silent fall-back cannot pass.

One AsrModel per configuration (module scope); a fixture's decoder tensors go onto a clone of its context.
"""
import re

import pytest
import torch

from reazonspeech_amd.runtime import capi
from reazonspeech_amd.runtime.model import AsrModel
from reazonspeech_amd.runtime.tokenizer import SyntheticTokenizer
from reazonspeech_amd.runtime.weights import screen_tensors, to_fragment_major
import decode_edges_ref as de
from knobs import knob

pytestmark = pytest.mark.gpu
TRACE = re.compile(r"\[decode trace\] B=(\d+) T'=(\d+): (\d+) steps \(screen (\d), narrow (\d), lookahead (\d)\)")


@pytest.fixture(scope="module")
def models(gpu_device):
    cache = {}

    def get(cfg, sd):
        if repr(cfg) not in cache:
            tok = SyntheticTokenizer(cfg.vocab_size) if getattr(cfg, "family", "nemo") == "nemo" else None
            cache[repr(cfg)] = AsrModel(cfg, sd, tok, device="cuda:0")
        return cache[repr(cfg)]

    yield get
    cache.clear()
    torch.cuda.empty_cache()


def decoder_tensors(sd):
    """the registered form of the decoder tensors a fixture edits (runtime/weights.py prepare_weights)"""
    f32 = lambda t: t.detach().to(torch.float32).contiguous()  # noqa: E731
    out = {"joint.pred.w": to_fragment_major(sd["joint.pred.weight"]), "joint.pred.b": f32(sd["joint.pred.bias"]),
           "joint.out.w": to_fragment_major(sd[de.JOUT + ".weight"]), "joint.out.b": f32(sd[de.JOUT + ".bias"])}
    out.update(screen_tensors(sd[de.JOUT + ".weight"], sd[de.JOUT + ".bias"]))
    return out


def greedy(models, case, capfd, *, screen=1, narrow=1, knobs=None, u_max=None, expect=None):
    """the device on a fixture -> [(ids, frames)]; asserts the trace flags (default: the screened joint, narrow tiles, look-ahead on)"""
    cfg, sd, f, lens, rec = case
    model = models(cfg, sd)
    dev = model.device
    ctx = model.ctx.clone()
    try:
        if getattr(cfg, "family", "nemo") == "nemo":
            for name, t in decoder_tensors(sd).items():
                ctx.set_tensor(name, t.to(dev).contiguous())
            ctx.finalize()
        ctx.set_option("decode_screen", screen)
        ctx.set_option("decode_narrow", narrow)
        B, Tp, _ = f.shape
        u_max = u_max or max(1, Tp * getattr(cfg, "max_symbols", 1))
        ids = torch.zeros((B, u_max), dtype=torch.int32, device=dev)
        frames = torch.zeros_like(ids)
        n_ids = torch.zeros((B,), dtype=torch.int32, device=dev)
        ws = torch.empty((ctx.workspace_bytes(B, 16000),), dtype=torch.uint8, device=dev)
        knobs = dict(knobs or {}, RS_DECODE_TRACE=1)
        capfd.readouterr()
        try:
            with_knobs(ctx.lib, list(knobs.items()), lambda: ctx.rnnt_greedy(f.to(dev), lens.to(dev), B, Tp, u_max, ids, frames, n_ids, ws,
                                                                              torch.cuda.current_stream().cuda_stream))
            torch.cuda.synchronize()
        finally:
            err = capfd.readouterr().err
        m = TRACE.search(err)
        assert m, f"no decode trace in {err!r}"
        want = dict(screen=screen, narrow=narrow, lookahead=0 if knobs.get("RS_DECODE_NO_LOOKAHEAD") else 1)
        want.update(expect or {})
        seen = dict(screen=int(m.group(4)), narrow=int(m.group(5)), lookahead=int(m.group(6)))
        assert (int(m.group(1)), int(m.group(2))) == (B, Tp) and seen == want, (seen, want)
        n = n_ids.cpu().numpy()
        return [(ids[b, :n[b]].cpu().tolist(), frames[b, :n[b]].cpu().tolist()) for b in range(B)]
    finally:
        ctx.close()


def with_knobs(lib, items, fn):
    if not items:
        return fn()
    with knob(lib, items[0][0], items[0][1]):
        return with_knobs(lib, items[1:], fn)


def same(got, ref):
    for b, (g, r) in enumerate(zip(got, ref)):
        assert g[0] == r[0], f"ids differ for utterance {b}"
        assert g[1] == r[1], f"frames differ for utterance {b}"
    assert len(got) == len(ref)


# ---- verify-kernel seams: <8> | <48> | wide<48> | <0> by the logit count ---------------------------------------------------------
@pytest.mark.parametrize("V", de.SEAM_V)
def test_ragged_rows_at_every_verify_seam(models, capfd, V):
    case = de.ragged_rows(V, 9, 32 if V > 4000 else de.TP_MAX)
    same(greedy(models, case, capfd), de.oracle(case))


# ---- candidate lists ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,knobs,kw", de.block_cases(), ids=[c[0] for c in de.block_cases()])
def test_tied_and_near_tied_blocks(models, capfd, name, knobs, kw):
    case = de.tied_block(**kw)
    ref = de.oracle(case)
    de.check_block(case, ref)
    same(greedy(models, case, capfd, knobs=knobs), ref)


@pytest.mark.parametrize("V", [512, 3072])
def test_all_columns_tied_fills_the_candidate_list(models, capfd, V):
    """V candidates per row: CAND_ROWS of rnnt_verify_kernel<8> (V = 512) and <48> (V = 3072), the LDS list filled to its last entry"""
    case = de.all_tied(V)
    ref = de.oracle(case)
    assert {t for r in ref for t in r[0]} == {0}
    same(greedy(models, case, capfd), ref)


@pytest.mark.parametrize("V", [512, 3001])
def test_all_columns_tied_wide_verify(models, capfd, V):
    case = de.all_tied(V) if V == 512 else de.tied_block(V=3001, start=0, N=3000, B=2, Tp=6)
    same(greedy(models, case, capfd, knobs={"RS_VERIFY_WIDE": 1}), de.oracle(case))


# ---- rows: the 4-row verify grid, the 32-row screen tile ------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 4, 5, 31, 32, 33, 65])
def test_ragged_rows_screened_path(models, capfd, B):
    case = de.ragged_rows(64, B)
    same(greedy(models, case, capfd), de.oracle(case))


@pytest.mark.parametrize("screen", [1, 0])
def test_all_empty_batch(models, capfd, screen):
    case = de.ragged_rows(64, 6, all_empty=True)
    assert greedy(models, case, capfd, screen=screen) == [([], [])] * 6


# ---- look-ahead (exact joint): depths 8 / 4 / 2 / 1 and the switches between them as rows finish ----------------------------------
@pytest.mark.parametrize("B", [16, 17, 32, 33, 64, 65, 128, 129])
def test_ragged_rows_reach_every_lookahead_depth(models, capfd, B):
    case = de.ragged_rows(64, B)
    same(greedy(models, case, capfd, screen=0), de.oracle(case))


@pytest.mark.parametrize("B,Tp,screen", [(5, 24, 0), (40, 24, 0), (100, 24, 0), (5, 3, 0), (5, 24, 1), (40, 24, 1), (100, 24, 1)])
@pytest.mark.parametrize("ms", [1, 2, 3])
def test_binding_cap(models, capfd, ms, B, Tp, screen):
    """max_symbols ends frames inside a look-ahead window (exact joint) and on the screened path; Tp = 3 is shorter than the window"""
    case = de.binding_cap(ms, B, Tp)
    same(greedy(models, case, capfd, screen=screen), de.oracle(case))


# ---- knobs ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("screen", [0, 1])
@pytest.mark.parametrize("no_xcd", [0, 1])
@pytest.mark.parametrize("B", [33, 65])
def test_joint_grid_padding_on_and_off(models, capfd, B, no_xcd, screen):
    """more than one 32-row tile: the only place joint_grid_x pads the grid to a multiple of 8 column tiles"""
    case = de.ragged_rows(3001, B, 20, seed=5)
    same(greedy(models, case, capfd, screen=screen, knobs={"RS_DECODE_NO_XCD": no_xcd}), de.oracle(case))


def test_no_lookahead_knob(models, capfd):
    case = de.ragged_rows(64, 17)
    same(greedy(models, case, capfd, screen=0, knobs={"RS_DECODE_NO_LOOKAHEAD": 1}), de.oracle(case))


@pytest.mark.parametrize("narrow", [0, 1])
def test_wide_lstm_tiles(models, capfd, narrow):
    case = de.ragged_rows(1001, 9)
    same(greedy(models, case, capfd, narrow=narrow), de.oracle(case))


# ---- other checks -----------------------------------------------------------------------------------------------------------------------
def test_j640_near_tie(models, capfd):
    """J = 640: 20 k-steps, the register cap of the screen kernel"""
    case = de.tied_block(V=3001, start=60, N=9, raised=68, wide=True, B=2, Tp=10)
    same(greedy(models, case, capfd), de.oracle(case))


def test_j768_runs_the_exact_joint(models, capfd):
    """J / 32 = 24 weight fragments do not fit the screen kernel: the exact joint runs, and says so"""
    case = de.ragged_rows(64, 9, 24, J=768)
    same(greedy(models, case, capfd, screen=1, expect=dict(screen=0)), de.oracle(case))


@pytest.mark.parametrize("screen", [0, 1])
def test_u_max_one_below_the_emission_count(models, capfd, screen):
    case = de.ragged_rows(64, 5)
    ref = de.oracle(case)
    most = max(len(r[0]) for r in ref)
    same(greedy(models, case, capfd, screen=screen, u_max=most), ref)
    with pytest.raises(capi.RsError) as e:
        greedy(models, case, capfd, screen=screen, u_max=most - 1)
    assert e.value.code == capi.RS_EOVERFLOW


@pytest.mark.parametrize("screen", [0, 1])
def test_k2_tied_block_with_unk(models, capfd, screen):
    case = de.k2_tied()            # (the stateless decoder has no LSTM: the narrow LSTM tiles do not apply and the trace says 0)
    same(greedy(models, case, capfd, screen=screen, expect=dict(narrow=0)), de.oracle(case))


@pytest.mark.parametrize("screen", [0, 1])
def test_espnet_tied_block(models, capfd, screen):
    case = de.espnet_tied()
    same(greedy(models, case, capfd, screen=screen), de.oracle(case))


# ---- small activation rows ------------------------------------------------------------------------------------------------------------
SMALL = [(n, b, w) for n, b in de.small_cases() for w in ((0, 1) if n.endswith("V1001") else (0,))]


@pytest.mark.parametrize("name,build,wide", SMALL, ids=[f"{s[0]}-wide{s[2]}" for s in SMALL])
def test_small_activation_rows(models, capfd, name, build, wide):
    """the candidate margin has to cover the final bias additions, its own subtraction and ||a||^2 underflowing (screen_margin,
    k_rnnt.hip): with thr = m - 2 eps the one-hot rows returned the higher of two tied columns and the 2^-80 rows the wrong one of
    two.  V = 1001: rnnt_verify_kernel<48>, and rnnt_verify_wide_kernel<12> with $RS_VERIFY_WIDE; V = 12288: rnnt_verify_wide_kernel<48>."""
    case = build()
    ref = de.oracle(case)
    assert {t for r in ref for t in r[0]} == {case[4]["winner"]}
    same(greedy(models, case, capfd, knobs={"RS_VERIFY_WIDE": wide}), ref)
