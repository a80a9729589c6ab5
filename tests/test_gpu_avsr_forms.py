"""-m gpu: the AV-HuBERT encoder-decoder at the lengths and widths that pick each kernel form of csrc/k_avsr.hip (toy geometries).

launch_attn chooses from the buffer length T (= the number of keys), the head width hd and the number of queries; the positional
convolution from its group width cg.  Geometries, reference (oracle/avsr.py in FLOAT64) and the bound are tests/avsr_forms_ref.py's:
every device output stays within min(16 d32, TOL) of the float64 oracle, d32 = max |float32 oracle - float64 oracle| of that case and
output, TOL = this family's TOL_ENC / TOL_LOGITS (tests/test_gpu_avsr.py).  Every case prints its errors next to d32.

1. LENGTH LADDER, audio only, 3 clips of lens (T, ceil(0.6 T), min(T, 3)); every frame of every clip (padded queries too: the
   reference computes them), then 6 teacher-forced steps of `decoding(beams=2)` with the same ids in both hypotheses of a clip
   (rows_per_kb = 2, cross-attention over T masked keys; the steps' self-attention is step<1>, general<1> at hd6), both rows
   against `decode_logits` on the float64 encoder output.  T -> (encoder attention | cross-attention of a step):
                    tiny (hd 32 | 64)       hd64 (64 | 64)        hd128 (128 | 128)      hd20 (20 | 20, odd tail)   hd6 (6 | 6)
     1              step<1> | step<1>       step<1> | step<1>     step<1> | step<1>      step<1> | step<1>          general<1> | general<1>
     2 .. 256       keys<4> | step<1>       mfma<64> | step<1>    mfma<128> | step<1>    keys<4> | step<1>          general<1> | general<1>
     257 .. 512     keys<8> | step<2>       mfma<64> | step<2>    mfma<128> | step<2>    keys<8> | step<2>          general<1> | general<1>
     513, 530       general<1> | general<1> mfma<64> | general<1> mfma<128> | general<2> general<1> | general<1>    general<1> | general<1>
   2, 15 .. 17, 63 .. 65, 127 .. 129, 255 .. 257, 511 .. 513 are the edges of the 16-key tiles, the 64-key chunks, the 64-query and
   64-frame workgroups and the thresholds; 250 is the benchmark's length, 300 and 530 lie inside a form.
   positional convolution: tiny mfma<2> (cg 32, K 16); tiny_valu the VALU form on the same weights (switch RS_AVSR_POSCONV_OLD = 1 through
   tests/knobs.py, back at its previous value afterwards); hd64 mfma<1> (cg 16) with K 128: the halo of 64 frames is longer than
   the short clips; hd128 mfma<4> (cg 64); hd20 / hd6 the VALU form at cg 40 / 24 (8-frame tiles); 64-frame tiles elsewhere.
   base2 (AVSR_BASE, 2 + 1 layers) at 17, 65, 250, 257, 513: mfma<64>, posconv mfma<3> with K 128, cross-attention at hd 192
   step<1> / step<1> / step<1> / step<2> / general<4>.
2. MASKS THAT ARE NOT TAIL PADDING, tiny / hd64 / hd128 / hd20 at T = 40 and 300: clip 0 full; clip 1 without frames [0, 20) — its
   first 16-key tile is fully masked, so the mfma kernel's `continue` runs and the first visible tile follows m_run = -inf; clip 2
   without [16, 48), two whole tiles in the middle, and cut at 260 when T = 300.  Encoder, then 6 decoder steps as in 1.
3. LONG PREFIXES AT THE NEW HEAD WIDTHS, hd128 / hd20 / hd6 / base2 with max_target_positions = 320: 2 clips at T = 17 (lens 17, 11),
   260 teacher-forced positions through `model(decoder_input_ids=)`: self-attention crosses from step<1> to step<2> at hd 128, 20 (the
   odd tail) and 192; hd6 takes general<1> throughout.  Slices [0, 64), [64, 256), [256, 260), each under its own d32.
4. MORE THAN 128 HYPOTHESIS ROWS, tiny, 44 ragged clips at T = 12, beams = 3: 132 rows send every decoder GEMM through the tiled
   kernel instead of the skinny one; 4 steps, from step 1 on a different non-trivial permutation of each clip's rows as
   src_rows, the same ids per clip; every row against the oracle.
5. VIDEO FRONT-END SIZES AND SHORT CLIPS, tiny.with_(image_size=H), audio and video, 2 clips of lens (T, min(T, 3)): H = 16, 24, 96 at
   T = 7; H = 16 at T = 1, 2, 3, 5 (the 5-frame Conv3d window longer than the clip).  The `video` tap of every clip against the
   oracle's `tap_video` (video_frontend; under its own d32) and the encoder output.  At H = 16 the trunk runs its 3 x 3
   convolutions on 4 x 4, 2 x 2 and 1 x 1 maps.
6. A CLIP ALONE AND IN LONGER BUFFERS, tiny and hd64: one 40-frame clip alone (T = 40: keys<4> / mfma<64>), then as clip 0 of buffers
   with T = 300 and 530 beside a full-length clip (keys<8> / general<1>; mfma<64> over 19 and 34 key tiles): its 40 valid frames
   stay within the ALONE case's bound of the alone run's float64 oracle (the oracle's valid frames do not depend on the buffer
   length); the worst pairwise device difference is printed.

The worst error per section, with its d32, is written to avsr_forms.json in the suite's report directory (beside
avsr_parity.json); DESIGN.md §6d keeps the figures beside the rule.
Out of scope: a clip whose mask covers every frame (the reference's softmax over an all-finfo.min row is uniform, the kernels
return zeros).
"""
import json
import os

import numpy as np
import pytest
import torch

from reazonspeech_amd.avsr import AVHubertForConditionalGeneration

import avsr_forms_ref as R
from knobs import knob, get_knob
from test_gpu_avsr import TOL_ENC, TOL_LOGITS
from test_gpu_k2_fp32 import REPORT as K2_REPORT

pytestmark = pytest.mark.gpu
REPORT = os.path.join(os.path.dirname(K2_REPORT), "avsr_forms.json")          # the suite's report directory, where avsr_parity.json goes too
WORST = {}


@pytest.fixture(scope="module")
def models(gpu_device):
    cache = {}

    def get(name, **kw):
        key = (R.geometry(name, **kw), )
        if key not in cache:
            cache[key] = AVHubertForConditionalGeneration(key[0], R.weights("tiny" if name == R.VALU else name, **kw), device=str(gpu_device), products="exact",
                                                          search="host")
        return cache[key]
    yield get
    cache.clear()
    torch.cuda.empty_cache()


def check(section, label, rows):
    """rows: (output, device error, d32, TOL).  Prints every figure, records the section's worst, then asserts min(16 d32, TOL)."""
    print(f"avsr forms {section} {label}: " + "; ".join(f"{k} err {e:.2e} d32 {d:.2e} bound {R.bound(d, tol):.2e}" for k, e, d, tol in rows))
    w = WORST.setdefault(section, {})
    for k, e, d, tol in rows:
        if e >= w.get(k, {"max_err": -1.0})["max_err"]:
            w[k] = {"max_err": e, "d32": d, "bound": R.bound(d, tol), "at": label}
    os.makedirs(os.path.dirname(REPORT), exist_ok=True)
    with open(REPORT, "w") as fp:
        json.dump(WORST, fp, indent=1, sort_keys=True)
    for k, e, d, tol in rows:
        assert d > 0.0 and R.FACTOR * d < tol, (section, label, k, "the reference's own d32 makes the bound degenerate", d)
        assert e <= R.bound(d, tol), (section, label, k, f"device error {e:.3e} > min(16 x d32 {d:.3e}, {tol})")


def err(got, want):
    assert tuple(got.shape) == tuple(want.shape), (got.shape, want.shape)
    got = got.detach().cpu().double()
    assert torch.isfinite(got).all()
    return float((got - want).abs().max())


def decode_steps(model, enc, mask, ids, beams=R.DECODE_BEAMS, steps=R.DECODE_STEPS, perms=None):
    """`steps` teacher-forced tokens through decoding(beams), every hypothesis of a clip fed the clip's ids -> [B][beams][steps][V]"""
    B = enc.shape[0]
    dec = model.dev.decoding(enc, mask, beams, R.DECODE_MAX_LEN)
    out = []
    for t in range(steps):
        src = None
        if perms is not None and t > 0:
            src = (np.arange(B)[:, None] * beams + np.asarray(perms[t % len(perms)])[None, :]).reshape(-1)
        out.append(dec.step(np.repeat(ids[:, t].numpy(), beams), t, src).clone())
    torch.cuda.synchronize()
    return torch.stack(out, dim=1).view(B, beams, steps, -1)


def encoder_and_steps(model, name, section, label, audio, mask):
    """the checks of sections 1 and 2: every encoder frame, then both hypothesis rows of 6 decoder steps"""
    cfg = R.geometry(name)
    ids = R.token_ids(cfg, audio.shape[0], R.DECODE_STEPS, seed=audio.shape[1])
    ref = R.reference(cfg, R.weights("tiny" if name == R.VALU else name), R.weights64("tiny" if name == R.VALU else name), audio, None, mask, ids)
    enc = model.avhubert(input_values=audio, padding_mask=mask).last_hidden_state
    lg = decode_steps(model, enc, mask, ids)
    rows = [("enc", err(enc, ref["enc"]), ref["d32_enc"], TOL_ENC)]
    rows += [(f"logits_row{r}", err(lg[:, r], ref["logits"]), ref["d32_logits"], TOL_LOGITS) for r in range(R.DECODE_BEAMS)]
    check(section, label, rows)
    assert float(enc.abs().max()) > 0.1 and float(lg.abs().max()) > 1.0


@pytest.mark.parametrize("name,T", R.LADDER_CASES)
def test_length_ladder(models, name, T):
    """section 1: 3 clips of lens (T, ceil(0.6 T), min(T, 3)), encoder and 6 decoder steps of two hypotheses per clip"""
    model = models(name)
    audio, mask = R.clips(T, R.ladder_lens(T), seed=T)
    label = f"{name} T={T} {R.forms(name, T)}"
    if name == R.VALU:
        lib = model.dev.ctx.lib
        before = get_knob(lib, "RS_AVSR_POSCONV_OLD")
        with knob(lib, "RS_AVSR_POSCONV_OLD", 1):
            assert get_knob(lib, "RS_AVSR_POSCONV_OLD") == 1
            encoder_and_steps(model, name, "ladder", label, audio, mask)
        assert get_knob(lib, "RS_AVSR_POSCONV_OLD") == before
    else:
        encoder_and_steps(model, name, "ladder", label, audio, mask)


@pytest.mark.parametrize("name,T", R.HOLE_CASES)
def test_masks_that_are_not_tail_padding(models, name, T):
    """section 2: a fully masked first tile (clip 1) and two fully masked tiles in the middle (clip 2)"""
    audio, mask = R.hole_clips(T, seed=1000 + T)
    assert mask[1, :20].all() and not mask[1, 20:].any() and mask[2, 16:48].all() and not mask[2, :16].any() and not mask[0].any()
    encoder_and_steps(models(name), name, "holes", f"{name} T={T} {R.forms(name, T)}", audio, mask)


@pytest.mark.parametrize("name", R.PREFIX_GEOMS)
def test_long_prefix_at_the_new_head_widths(models, name):
    """section 3: 260 teacher-forced positions; the self-attention of a step moves from step<1> to step<2> past 256 keys"""
    kw = dict(max_target_positions=R.PREFIX_MAX_POSITIONS)
    cfg = R.geometry(name, **kw)
    model = models(name, **kw)
    audio, mask = R.clips(R.PREFIX_T, R.PREFIX_LENS, seed=31)
    ids = R.token_ids(cfg, len(R.PREFIX_LENS), R.PREFIX_POSITIONS, seed=32)
    ref = R.reference(cfg, R.weights(name, **kw), R.weights64(name, **kw), audio, None, mask, ids)
    got = model(input_values=audio, padding_mask=mask, decoder_input_ids=ids).logits
    hd = cfg.decoder_embed_dim // cfg.decoder_attention_heads
    rows = []
    for lo, hi in R.PREFIX_SLICES:
        d32 = float((ref["f32_logits"][:, lo:hi].double() - ref["logits"][:, lo:hi]).abs().max())
        rows.append((f"logits[{lo}:{hi}] {R.attn_form(hd, 1, lo + 1)}..{R.attn_form(hd, 1, hi)}", err(got[:, lo:hi], ref["logits"][:, lo:hi]), d32, TOL_LOGITS))
    check("prefix", f"{name} hd={hd}", rows)


def test_more_than_128_hypothesis_rows(models):
    """section 4: 44 clips x 3 beams = 132 rows: the decoder's GEMMs leave the skinny kernel; rows re-parented inside each clip"""
    cfg, model = R.geometry("tiny"), models("tiny")
    lens = R.ragged_lens(R.ROWS_CLIPS, R.ROWS_T, seed=44)
    audio, mask = R.clips(R.ROWS_T, lens, seed=45)
    ids = R.token_ids(cfg, R.ROWS_CLIPS, R.ROWS_STEPS, seed=46)
    ref = R.reference(cfg, R.weights("tiny"), R.weights64("tiny"), audio, None, mask, ids)
    enc = model.avhubert(input_values=audio, padding_mask=mask).last_hidden_state
    assert R.ROWS_CLIPS * R.ROWS_BEAMS > 128
    lg = decode_steps(model, enc, mask, ids, beams=R.ROWS_BEAMS, steps=R.ROWS_STEPS, perms=((1, 2, 0), (2, 0, 1), (0, 2, 1)))
    rows = [("enc", err(enc, ref["enc"]), ref["d32_enc"], TOL_ENC)]
    rows += [(f"logits_row{r}", err(lg[:, r], ref["logits"]), ref["d32_logits"], TOL_LOGITS) for r in range(R.ROWS_BEAMS)]
    check("rows132", f"tiny {R.ROWS_CLIPS} clips x {R.ROWS_BEAMS} beams T={R.ROWS_T}", rows)


@pytest.mark.parametrize("H,T", R.VIDEO_CASES)
def test_video_front_end_sizes_and_short_clips(models, H, T):
    """section 5: image_size 16 / 24 / 96 and clips shorter than the Conv3d's 5-frame window"""
    kw = dict(image_size=H)
    cfg, model = R.geometry("tiny", **kw), models("tiny", **kw)
    audio, video, mask = R.av_clips(T, (T, min(T, 3)), seed=50 + H + T, image_size=H)
    ref = R.reference(cfg, R.weights("tiny", **kw), R.weights64("tiny", **kw), audio, video, mask)
    enc, taps = model.dev.encode(audio, video, mask, taps=[0])
    torch.cuda.synchronize()
    check("video", f"H={H} T={T}", [("video", err(taps["video"], ref["video"]), ref["d32_video"], TOL_ENC), ("enc", err(enc, ref["enc"]), ref["d32_enc"], TOL_ENC)])
    assert float(taps["video"].abs().max()) > 0.1


@pytest.mark.parametrize("name", R.ALONE_GEOMS)
def test_a_clip_alone_and_in_longer_buffers(models, name):
    """section 6: the same 40 frames through keys<4>, keys<8> and general<1> (tiny), mfma<64> over 3, 19 and 34 key tiles (hd64)"""
    cfg, model, n = R.geometry(name), models(name), R.ALONE_LEN
    audio, mask = R.clips(n, (n,), seed=60)
    ref = R.reference(cfg, R.weights(name), R.weights64(name), audio, None, mask)
    runs = {n: model.avhubert(input_values=audio, padding_mask=mask).last_hidden_state[0].cpu()}
    for T in R.ALONE_BUFFERS:
        a, m = R.embed_clip(audio, T, seed=61)
        assert np.array_equal(a[0, :n], audio[0]) and not a[0, n:].any() and m[0, n:].all() and not m[0, :n].any() and not m[1].any()
        runs[T] = model.avhubert(input_values=a, padding_mask=m).last_hidden_state[0, :n].cpu()
    pairwise = max(float((runs[x] - runs[y]).abs().max()) for x in runs for y in runs)
    print(f"avsr forms alone {name}: worst pairwise device difference over T = {sorted(runs)}: {pairwise:.2e}")
    hd = cfg.encoder_embed_dim // cfg.encoder_attention_heads
    check("alone", name, [(f"enc T={T} {R.attn_form(hd, T, T)}", err(x, ref["enc"][0]), ref["d32_enc"], TOL_ENC) for T, x in sorted(runs.items())])
