"""CPU tests of tests/avsr_forms_ref.py: the inputs it builds, the float64 oracle it uses as reference, and that d32 (the float32
oracle's distance from the float64 one) keeps the bound min(16 d32, TOL) of tests/test_gpu_avsr_forms.py from degenerating to TOL.
TOL_ENC / TOL_LOGITS are restated here, so that this file imports nothing of the GPU suite; the first test holds them to the
assignment in tests/test_gpu_avsr.py."""
import numpy as np
import pytest
import torch

import avsr_forms_ref as R
from reazonspeech_amd.runtime.avsr_synth import synthetic_clips

TOL_ENC, TOL_LOGITS = 5e-4, 2e-3
# d32 runs over EVERY tabled case (the oracle takes a second at most per case on a CPU); tiny_valu shares tiny's inputs and oracle
D32_LADDER = [(g, t) for g, t in R.LADDER_CASES if g != R.VALU]
D32_VIDEO = R.VIDEO_CASES


def test_the_tolerance_restated_here_is_the_gpu_suites():
    import ast
    import os
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_avsr.py"), encoding="utf-8").read()
    for node in ast.parse(src).body:
        if isinstance(node, ast.Assign) and isinstance(node.targets[0], ast.Tuple) and [e.id for e in node.targets[0].elts][:2] == ["TOL_ENC", "TOL_LOGITS"]:
            assert tuple(ast.literal_eval(node.value))[:2] == (TOL_ENC, TOL_LOGITS)
            return
    pytest.fail("tests/test_gpu_avsr.py no longer assigns TOL_ENC, TOL_LOGITS together")


def test_geometries_validate_and_select_the_tabled_forms():
    for name, cfg in R.GEOMS.items():
        cfg.validate()
    f = R.forms
    assert f("tiny", 1) == ("step<1>", "step<1>", "posconv mfma<2>") and f("tiny", 256)[:2] == ("keys<4>", "step<1>")
    assert f("tiny", 257)[:2] == ("keys<8>", "step<2>") and f("tiny", 512)[:2] == ("keys<8>", "step<2>") and f("tiny", 513)[:2] == ("general<1>", "general<1>")
    assert f(R.VALU, 64)[2] == "posconv valu(cg 32)"
    assert f("hd64", 2) == ("mfma<64>", "step<1>", "posconv mfma<1>") and f("hd64", 530)[:2] == ("mfma<64>", "general<1>")
    assert f("hd128", 300) == ("mfma<128>", "step<2>", "posconv mfma<4>") and f("hd128", 513)[1] == "general<2>"
    assert f("hd20", 300) == ("keys<8>", "step<2>", "posconv valu(cg 40)") and (R.GEOMS["hd20"].decoder_embed_dim // R.GEOMS["hd20"].decoder_attention_heads // 4) % 2 == 1
    assert {f("hd6", t)[:2] for t in R.LADDER} == {("general<1>", "general<1>")} and f("hd6", 9)[2] == "posconv valu(cg 24)"
    assert f("base2", 257) == ("mfma<64>", "step<2>", "posconv mfma<3>") and f("base2", 513)[1] == "general<4>"
    assert R.geometry("base2").conv_pos == 128 and R.geometry("hd64").conv_pos // 2 == 64
    # weights are seeded per tensor name: base2's state dict is the 161M dict's entries of its layers, without building that dict
    from reazonspeech_amd.runtime.avsr_weights import expected_shapes_avsr
    from reazonspeech_amd.runtime.avsr_config import AVSR_BASE
    full, part = expected_shapes_avsr(AVSR_BASE), R.weights("base2")
    assert set(part) < set(full) and all(tuple(v.shape) == full[k] for k, v in part.items())
    assert len(R.LADDER_CASES) == 6 * len(R.LADDER) + len(R.LADDER_BASE2)


def test_clips_lay_out_mask_and_audio():
    T, lens = 50, (50, 30, 3)
    audio, mask = R.clips(T, lens, seed=7, holes=((1, 0, 20), (2, 1, 2), (0, 40, 60)))
    full = synthetic_clips(3, T, 7, ragged=False, image_size=8)[0]
    assert audio.shape == (3, T, 104) and mask.shape == (3, T) and audio.dtype == np.float32 and mask.dtype == np.float32
    want = np.zeros((3, T), np.float32)
    want[1, 30:] = want[2, 3:] = want[1, :20] = want[2, 1:2] = want[0, 40:] = 1.0
    assert np.array_equal(mask, want)
    assert np.array_equal(audio[mask == 0], full[mask == 0]) and not audio[mask == 1].any() and np.abs(audio[mask == 0]).min(axis=-1).max() > 0
    assert R.ladder_lens(1) == (1, 1, 1) and R.ladder_lens(2) == (2, 2, 2) and R.ladder_lens(250) == (250, 150, 3) and R.ladder_lens(513) == (513, 308, 3)
    with pytest.raises(AssertionError):
        R.clips(8, (8, 8), seed=1, holes=((1, 0, 8),))                  # a fully masked clip is out of scope
    # section 2's masks
    for T in (40, 300):
        a, m = R.hole_clips(T, seed=3)
        assert not m[0].any() and m[1, :20].all() and not m[1, 20:].any() and m[2, 16:48].all() and not m[2, :16].any()
        assert (m[2, 48:260].sum() == 0 and m[2, 260:].all()) if T == 300 else m[2, 16:].all()
        assert not a[m == 1].any()
    # section 6's buffers
    alone, _ = R.clips(40, (40,), seed=60)
    a, m = R.embed_clip(alone, 300, seed=61)
    assert a.shape == (2, 300, 104) and np.array_equal(a[0, :40], alone[0]) and not a[0, 40:].any() and m[0, 40:].all() and not m[0, :40].any() and not m[1].any()
    # section 4's lengths and section 5's clips
    lens = R.ragged_lens(R.ROWS_CLIPS, R.ROWS_T, seed=44)
    assert len(lens) == 44 and max(lens) == 12 and min(lens) == 1 and len(set(lens)) > 6
    a, v, m = R.av_clips(5, (5, 3), seed=1, image_size=16)
    assert v.shape == (2, 5, 1, 16, 16) and m[1, 3:].all() and not a[1, 3:].any() and np.ptp(v[1, 3:]) == 0 and np.ptp(v[1, :3]) > 0
    ids = R.token_ids(R.GEOMS["tiny"], 3, 6, seed=5)
    assert ids.shape == (3, 6) and (ids[:, 0] == 0).all() and int(ids[:, 1:].min()) >= 3 and int(ids.max()) < 61


def test_the_float64_oracle_is_deterministic_and_float64():
    cfg = R.geometry("hd20")
    audio, mask = R.clips(65, R.ladder_lens(65), seed=65)
    ids = R.token_ids(cfg, 3, 6, seed=65)
    a = R.reference(cfg, R.weights("hd20"), R.weights64("hd20"), audio, None, mask, ids)
    b = R.reference(cfg, R.weights("hd20"), R.to64(R.weights("hd20")), audio, None, mask, ids)
    assert a["enc"].dtype == torch.float64 and a["logits"].dtype == torch.float64 and a["f32_enc"].dtype == torch.float32
    assert torch.equal(a["enc"], b["enc"]) and torch.equal(a["logits"], b["logits"]) and a["d32_enc"] == b["d32_enc"] and a["d32_logits"] == b["d32_logits"]
    assert a["enc"].shape == (3, 65, 160) and a["logits"].shape == (3, 6, 61)
    # the reference zeroes masked rows before the positional convolution and a masked key weighs nothing: audio BEHIND clip 1's mask
    # changes none of its valid frames
    audio2 = audio.copy()
    audio2[1, 50:] = 1.0
    c = R.reference(cfg, R.weights("hd20"), R.weights64("hd20"), audio2, None, mask, ids)
    assert torch.equal(a["enc"][1, :39], c["enc"][1, :39])


def _assert_d32(label, ref, keys):
    for k, tol in keys:
        d = ref["d32_" + k]
        assert 0.0 < d < tol / R.FACTOR, (label, k, d)


@pytest.mark.parametrize("name", ["tiny", "hd64", "hd128", "hd20", "hd6", "base2"])
def test_d32_keeps_the_ladder_bound_below_tol(name):
    worst = {"enc": 0.0, "logits": 0.0}
    for g, T in D32_LADDER:
        if g != name:
            continue
        cfg = R.geometry(g)
        audio, mask = R.clips(T, R.ladder_lens(T), seed=T)
        ref = R.reference(cfg, R.weights(g), R.weights64(g), audio, None, mask, R.token_ids(cfg, 3, R.DECODE_STEPS, seed=T))
        _assert_d32((g, T), ref, (("enc", TOL_ENC), ("logits", TOL_LOGITS)))
        worst = {k: max(v, ref["d32_" + k]) for k, v in worst.items()}
    print(f"avsr forms d32 {name}:", {k: f"{v:.2e}" for k, v in worst.items()})


def test_d32_keeps_the_other_sections_bounds_below_tol():
    for g, T in R.HOLE_CASES:
        cfg = R.geometry(g)
        audio, mask = R.hole_clips(T, seed=1000 + T)
        _assert_d32(("holes", g, T), R.reference(cfg, R.weights(g), R.weights64(g), audio, None, mask, R.token_ids(cfg, 3, R.DECODE_STEPS, seed=T)),
                    (("enc", TOL_ENC), ("logits", TOL_LOGITS)))
    kw = dict(max_target_positions=R.PREFIX_MAX_POSITIONS)
    for g in R.PREFIX_GEOMS:
        cfg = R.geometry(g, **kw)
        audio, mask = R.clips(R.PREFIX_T, R.PREFIX_LENS, seed=31)
        ref = R.reference(cfg, R.weights(g, **kw), R.weights64(g, **kw), audio, None, mask, R.token_ids(cfg, 2, R.PREFIX_POSITIONS, seed=32))
        for lo, hi in R.PREFIX_SLICES:
            d = float((ref["f32_logits"][:, lo:hi].double() - ref["logits"][:, lo:hi]).abs().max())
            assert 0.0 < d < TOL_LOGITS / R.FACTOR, (g, lo, hi, d)
    cfg = R.geometry("tiny")
    audio, mask = R.clips(R.ROWS_T, R.ragged_lens(R.ROWS_CLIPS, R.ROWS_T, seed=44), seed=45)
    _assert_d32("rows132", R.reference(cfg, R.weights("tiny"), R.weights64("tiny"), audio, None, mask, R.token_ids(cfg, R.ROWS_CLIPS, R.ROWS_STEPS, seed=46)),
                (("enc", TOL_ENC), ("logits", TOL_LOGITS)))
    for H, T in D32_VIDEO:
        kw = dict(image_size=H)
        audio, video, mask = R.av_clips(T, (T, min(T, 3)), seed=50 + H + T, image_size=H)
        _assert_d32(("video", H, T), R.reference(R.geometry("tiny", **kw), R.weights("tiny", **kw), R.weights64("tiny", **kw), audio, video, mask),
                    (("enc", TOL_ENC), ("video", TOL_ENC)))
    for g in R.ALONE_GEOMS:
        audio, mask = R.clips(R.ALONE_LEN, (R.ALONE_LEN,), seed=60)
        _assert_d32(("alone", g), R.reference(R.geometry(g), R.weights(g), R.weights64(g), audio, None, mask), (("enc", TOL_ENC),))


@pytest.mark.parametrize("name,T,clip,frame", [("tiny", 300, 2, 280), ("hd64", 300, 2, 280), ("hd20", 511, 1, 400), ("hd128", 530, 1, 529), ("hd6", 530, 1, 520)])
def test_one_wrongly_visible_frame_lies_far_outside_the_bound(name, T, clip, frame):
    """what the bound is for: ONE padded frame of a few hundred taken for a valid one (its row not zeroed, its key not masked) moves
    the float64 oracle's valid frames and logits of that clip by more than 100 times min(16 d32, TOL)"""
    cfg = R.geometry(name)
    audio, mask = R.hole_clips(T, seed=1000 + T) if T == 300 else R.clips(T, R.ladder_lens(T), seed=T)
    assert mask[clip, frame] == 1.0
    ids = R.token_ids(cfg, 3, R.DECODE_STEPS, seed=T)
    ref = R.reference(cfg, R.weights(name), R.weights64(name), audio, None, mask, ids)
    mask2 = mask.copy()
    mask2[clip, frame] = 0.0
    off = R.reference(cfg, R.weights(name), R.weights64(name), audio, None, mask2, ids)
    valid = torch.from_numpy(mask[clip] == 0)
    assert float((ref["enc"][clip][valid] - off["enc"][clip][valid]).abs().max()) > 100 * R.bound(ref["d32_enc"], TOL_ENC)
    assert float((ref["logits"][clip] - off["logits"][clip]).abs().max()) > 100 * R.bound(ref["d32_logits"], TOL_LOGITS)
