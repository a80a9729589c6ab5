"""CPU checks of tests/conformer_lengths_ref.py, the fixtures of tests/test_gpu_conformer_lengths.py: the sample counts give the stated T', no
utterance sits on a near-tie of the oracle's own greedy search (so the GPU module compares ids on EVERY case, with no exemption list), the
table of forms states what the dispatch code computes, and the shared comparison catches a mutated oracle on the shortest rung where the
mutation can show."""
import os

import pytest
import torch

import conformer_lengths_ref as cl
from oracle import model as om
from test_gpu_espnet_fp32 import TOL_F32 as TOL_ENC_ESPNET
from test_gpu_fp32_mode import TOL_ENC

TOL_FP32 = {"nemo": TOL_ENC, "espnet": TOL_ENC_ESPNET}


def test_sample_counts_give_the_stated_frames():
    for fam, tp in cl.utterances() + [("nemo", 0), ("espnet", 0)]:
        cfg = cl.CFGS[fam]
        n = cl.samples_for(cfg, tp)
        assert n % 64 == 0 and len(cl.wave(fam, tp)) == n
        assert cfg.enc_frames(cfg.mel_frames(n)) == tp < cfg.enc_frames(cfg.mel_frames(n + 64))
    assert cl.samples_for(cl.CFGS["nemo"], 0) == 128 and cl.samples_for(cl.CFGS["espnet"], 0) == 704
    for fam, pad in (("nemo", 16000), ("espnet", 24000)):          # the public path: the package's own padding leaves room for audio
        assert all(cl.samples_for(cl.CFGS[fam], tp) > pad for tp in cl.PUBLIC_TP[fam])
    assert set(cl.FORM_TP) | set(cl.FORM_BUF) <= {t for f, t in cl.utterances() if f == "espnet"}


@pytest.mark.parametrize("fam", ["nemo", "espnet", "nemo_w"])
def test_no_utterance_is_a_near_tie_and_long_ones_emit(fam):
    """the float64 walk along the float32 oracle's greedy path: smallest margin >= 1e-3 on every utterance; at least one token from T' = 8"""
    bad = []
    for f, tp in cl.utterances():
        if f != fam:
            continue
        ref = cl.oracle(fam, tp, "fp32")
        assert ref["enc_len"] == tp
        ids, frames = cl.greedy(fam, tp)
        m = cl.margin(fam, tp)
        if not m >= cl.NEAR_TIE or (tp >= 8 and not ids):
            bad.append((tp, cl.seed_for(fam, tp), m, len(ids)))
    assert not bad, f"{fam}: pick other seeds (T', seed, margin, tokens): {bad}"


def test_margin_walks_follow_the_path_and_reject_another():
    for fam, tp in (("nemo", 9), ("espnet", 9)):
        cfg, sd = cl.CFGS[fam], cl.weights(fam)
        ids, frames = cl.greedy(fam, tp)
        assert ids and cl.margin(fam, tp) > 0
        f = cl.oracle(fam, tp, "fp32")["joint"]
        wrong = [ids[0] + 1 if ids[0] + 1 < cfg.vocab_size else ids[0] - 1] + ids[1:]
        if cfg.espnet:
            assert cl._espnet_golden_tools().greedy_margins(cfg, sd, f.numpy(), tp, wrong, frames) == 0.0
        else:
            assert cl.nemo_greedy_margins(cfg, sd, f, tp, wrong, frames) == 0.0
            assert cl.nemo_greedy_margins(cfg, sd, f, tp, ids[:-1], frames[:-1]) == 0.0


# the lines of the dispatch code that `forms()` restates: when one of them changes, the table (and the ladder's rungs) must be looked at again
DISPATCH_SOURCE = {
    "k_attention.hip": ["static constexpr int KB_CHUNK = HD == 128 ? 5 : 6;", "const int qblocks = (T + 31) / 32;", "const int nw = qblocks < 6 ? qblocks : 6;",
                        "const int nw2 = qblocks < nwmax ? qblocks : (nwmax < 1 ? 1 : nwmax > 6 ? 6 : nwmax);",
                        "else if (nw2 == 1) go(relpos_attention_kernel<HD, false, false, 2>",
                        "if (window) hipLaunchKernelGGL((relpos_attention_kernel<HD, false, true>), grid, block, lds, s, p);"],
    "rs_knobs.h": ['X(ATTN64, "RS_ATTN64", INT, 4,', 'X(ATTN64_NW, "RS_ATTN64_NW", INT, 4,'],
    "k_f32.hip": ["const dim3 grid16((T + 63) / 64, dm.n_heads, B);", "if (T <= 256) RS_ATT_KEYS(4);", "else if (T <= 512) RS_ATT_KEYS(8);", "else RS_ATT_KEYS(0);"],
    "k_layernorm.hip": ["constexpr int TT = 32;   // output frames per workgroup", "constexpr int R = 6, TTF = 8 * R;",
                        "const dim3 grid((T + 127) / 128, d / 64, B), block(256);",
                        "if (layout == 2 && (k == 7 || k == 15 || k == 31) && glu_generic != 1) return rs_launch_dwconv_act(",
                        "else hipLaunchKernelGGL((dwconv_silu_dma_kernel<9, R>), grid, block, 0, s, x, w, b, lens, T, d, out);"],
}


def test_forms_table_at_the_seams_and_the_source_lines_it_restates():
    """`forms()` is a restatement of the dispatch arithmetic, not a reading of it: this pins its strings at the seams and pins the source
    lines the restatement was made from, so that a change of a chunk, tile or threshold in the dispatch code fails here"""
    csrc = os.path.join(os.path.dirname(cl.HERE), "reazonspeech_amd", "csrc")
    for name, lines in DISPATCH_SOURCE.items():
        text = open(os.path.join(csrc, name)).read()
        for line in lines:
            assert line in text, f"{name} no longer has `{line}`: check forms() and the ladder of tests/test_gpu_conformer_lengths.py"
    f = cl.forms
    assert f("nemo", 192)["attention bf16"] == "staged<128> 6 waves x 1 wg, 2 key chunk(s) of 5"
    assert f("nemo", 193)["attention bf16"] == "staged<128> 6 waves x 2 wg, 2 key chunk(s) of 5"
    assert f("nemo", 160)["attention bf16"].endswith("1 key chunk(s) of 5") and f("nemo", 161)["attention bf16"].endswith("2 key chunk(s) of 5")
    assert f("espnet", 32)["attention bf16"] == "staged<64,kbc 2> one wave" and f("espnet", 33)["attention bf16"].startswith("staged<64,kbc 4> 2 waves x 1 wg")
    assert f("espnet", 128)["attention bf16"] == "staged<64,kbc 4> 4 waves x 1 wg, 1 key chunk(s) of 4"
    assert f("espnet", 129)["attention bf16"] == "staged<64,kbc 4> 4 waves x 2 wg, 2 key chunk(s) of 4"
    assert [f("nemo_w", t)["attention fp32"] for t in (256, 257, 512, 513)] == ["keys<4>", "keys<8>", "keys<8>", "keys<0>"]
    assert f("nemo_w", 257)["attention bf16"].startswith("WINDOW<128>")
    assert f("nemo", 64)["attention fp32"] == "mfma<128> 1 x 64 queries" and f("nemo", 65)["attention fp32"] == "mfma<128> 2 x 64 queries"
    assert f("nemo", 48)["conv fused"] == "dwconv_silu_dma<9,6> 1 x 48" and f("nemo", 49)["conv unfused"] == "glu_fast<9,6,1> 2 x 48"
    assert f("espnet", 129)["conv fused"] == "dwconv_act<15,0> 2 x 128" and f("espnet", 33)["conv unfused"] == "glu_generic 2 x 32"


def mutated(fam, tp, recipe, mutation):
    """the oracle with a position index off by one (row n of the table holds relative position T' - n instead of T' - 1 - n) or with
    every length mask one frame short"""
    orig_pos, orig_mask = om.rel_pos_table, om._len_mask
    if mutation == "position":
        om.rel_pos_table = lambda cfg, T: orig_pos(cfg, T + 1)[:2 * T - 1]
    else:
        om._len_mask = lambda lengths, T: orig_mask(lengths - 1, T)
    try:
        return cl.forward(cl.CFGS[fam], cl.weights(fam), cl.wave(fam, tp), recipe)
    finally:
        om.rel_pos_table, om._len_mask = orig_pos, orig_mask


@pytest.mark.parametrize("fam", ["nemo", "espnet"])
def test_the_comparison_catches_a_mutated_oracle_on_the_shortest_rung(fam):
    """the comparison of the GPU module (`errors` + `violations` under ITS tolerances) fed the mutated oracle in the device's place"""
    def caught(tp, recipe, mutation):
        errs = cl.errors(mutated(fam, tp, recipe, mutation), cl.oracle(fam, tp, recipe))
        if recipe == "fp32":
            return bool(cl.violations(errs, TOL_FP32[fam]))
        return bool(cl.violations(errs, cl.TOL_BF16_MAX, cl.TOL_BF16_MEAN))
    # a length mask one frame short shows at T' = 1 (the one frame is masked out of the attention and the conv module), in both modes
    assert caught(1, "fp32", "mask") and caught(1, "bf16-fused-glu", "mask")
    # a position off by one cannot show at T' = 1 (the softmax over one key is 1 whatever its score) ...
    assert not caught(1, "fp32", "position")
    e1 = cl.errors(mutated(fam, 1, "fp32", "position"), cl.oracle(fam, 1, "fp32"))
    assert all(v[0] == 0.0 for v in e1.values())
    # ... the float32 comparison catches it at T' = 2; the bf16 tolerance (6e-2 / 6e-3 on O(1) values) is coarser: its mean catches it
    # from T' = 3 (nemo) / 9 (espnet), the next rungs of the ladder
    assert caught(2, "fp32", "position")
    assert caught(3 if fam == "nemo" else 9, "bf16-fused-glu", "position")


# caps of the sub_out yardstick, asserted for EVERY utterance so that no rung can widen its own bound unseen.  sub_out reaches 82 here:
# float32 1e-2 = 1.2e-4 of that (about 1000 float32 ulps at 64 .. 128; the worst rung's oracle is 8e-4 from float64, times the factor 8);
# bf16 max 0.5 = one bf16 ulp at 64 .. 128, mean 4e-2
YARD_CAP = {"fp32": 1e-2, "bf16_max": 0.5, "bf16_mean": 4e-2}


@pytest.mark.parametrize("fam", ["nemo", "espnet", "nemo_w"])
def test_sub_out_yardstick_is_reference_only_positive_and_capped_on_every_rung(fam):
    """the float64 oracle of the yardstick is the oracle's own front-end run in another type (at float32: the oracle's bits, on every
    rung), and the yardstick stays under YARD_CAP on every rung"""
    worst = {k: (0.0, None) for k in YARD_CAP}
    for f, tp in cl.utterances():
        if f != fam:
            continue
        ref = cl.oracle(fam, tp, "fp32")
        f32, n = cl.frontend_as(cl.CFGS[fam], cl.weights(fam), cl.wave(fam, tp), torch.float32)
        assert n == ref["n_frames"] and f32.dtype == torch.float32 and torch.equal(f32[0], ref["feats"][:n])
        y = cl.sub_out_yardstick(fam, tp)
        for k, cap in YARD_CAP.items():
            assert 0 < y[k] <= cap, (fam, tp, k, y[k], cap)
            worst[k] = max(worst[k], (y[k], tp))
    print(f"{fam}: largest sub_out yardsticks (value, T'): {worst}")
    tp = 33
    f32, _ = cl.frontend_as(cl.CFGS[fam], cl.weights(fam), cl.wave(fam, tp), torch.float32)
    f64, _ = cl.frontend_as(cl.CFGS[fam], cl.weights(fam), cl.wave(fam, tp), torch.float64)
    assert f64.dtype == torch.float64 and 0 < float((f64 - f32.double()).abs().max()) < 2e-3
    assert float(cl.oracle(fam, tp, "fp32")["sub_out"].abs().max()) > 8.0, "sub_out is not LayerNorm-ed: values of tens, hence a bound of its own"
