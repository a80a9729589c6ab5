"""Case tables and reference helpers of tests/test_gpu_avsr_forms.py (AV-HuBERT at the lengths and widths that pick each kernel
form of csrc/k_avsr.hip); importable without a GPU, held to its own statements by tests/test_avsr_forms_host.py.

REFERENCE: oracle/avsr.py (`encode`, `decode_logits`, `video_frontend`) in FLOAT64 — the state dict's floating tensors, the inputs
and the mask cast to double; the oracle runs unchanged that way.
TOLERANCE: per case the float32 oracle runs too and d32 = max |oracle_f32 - oracle_f64| is taken separately for the encoder output,
the logits (the float32 decoder on the float32 encoder output) and the video tap: a property of the reference alone.  The device
must stay within min(16 d32, TOL) of the float64 oracle, TOL = TOL_ENC / TOL_LOGITS of tests/test_gpu_avsr.py.  Why 16: the
device's exact-f32 MFMA chains differ from the CPU's float32 only in the order of their sums and sit at 1 - 2 d32 in the family's
logs; 16 leaves room for longer chains, and one key weighted wrongly by 1 / 512 moves an attention output by ~2e-3, far outside.
The factor is never scaled from what the device measures.

GEOMETRIES (`.with_()` on AVSR_TINY with 2 + 2 layers unless said otherwise; cg = the positional convolution's group width):
  tiny    as is: encoder hd 32, cg 32, K 16, decoder hd 64
  hd64    encoder_attention_heads 2 (hd 64), conv_pos_groups 8 (cg 16), conv_pos 128 (halo 64)
  hd128   widths 256, 2 / 2 heads (hd 128 / 128), conv_pos_groups 4 (cg 64)
  hd20    widths 160, ffn 160, 8 / 8 heads (hd 20: hd / 4 odd), conv_pos_groups 4 (cg 40)
  hd6     widths 96, ffn 96, 16 / 16 heads (hd 6: hd % 4 != 0), conv_pos_groups 4 (cg 24)
  base2   AVSR_BASE with 2 encoder layers and 1 decoder layer: hd 64 / 192, cg 48, K 128.  Weights are seeded per tensor name, so its
          state dict IS the 161M dict's entries of those layers; it is built once per process.
`attn_form` / `posconv_form` restate launch_attn's and the positional convolution's dispatch for the docstrings and the printed lines."""
import functools
import math

import numpy as np
import torch

from reazonspeech_amd.runtime.avsr_config import AVSR_TINY, AVSR_BASE
from reazonspeech_amd.runtime.avsr_synth import synthetic_clips, IMAGE_MEAN, IMAGE_STD
from reazonspeech_amd.runtime.avsr_weights import synthetic_state_dict_avsr
from oracle import avsr as oa

FACTOR = 16
WEIGHT_SEED = 3
GEOMS = {
    "tiny": AVSR_TINY,
    "hd64": AVSR_TINY.with_(encoder_attention_heads=2, conv_pos_groups=8, conv_pos=128),
    "hd128": AVSR_TINY.with_(encoder_embed_dim=256, decoder_embed_dim=256, encoder_attention_heads=2, decoder_attention_heads=2, conv_pos_groups=4),
    "hd20": AVSR_TINY.with_(encoder_embed_dim=160, decoder_embed_dim=160, encoder_ffn_embed_dim=160, decoder_ffn_embed_dim=160,
                            encoder_attention_heads=8, decoder_attention_heads=8, conv_pos_groups=4),
    "hd6": AVSR_TINY.with_(encoder_embed_dim=96, decoder_embed_dim=96, encoder_ffn_embed_dim=96, decoder_ffn_embed_dim=96,
                           encoder_attention_heads=16, decoder_attention_heads=16, conv_pos_groups=4),
    "base2": AVSR_BASE.with_(encoder_layers=2, decoder_layers=1),
}
VALU = "tiny_valu"                      # `tiny` under the switch RS_AVSR_POSCONV_OLD = 1: the same weights and oracle
LADDER = (1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 250, 255, 256, 257, 300, 511, 512, 513, 530)
LADDER_BASE2 = (17, 65, 250, 257, 513)
LADDER_CASES = ([(g, t) for g in ("tiny", VALU, "hd64", "hd128", "hd20", "hd6") for t in LADDER] + [("base2", t) for t in LADDER_BASE2])
HOLE_CASES = [(g, t) for g in ("tiny", "hd64", "hd128", "hd20") for t in (40, 300)]
PREFIX_GEOMS = ("hd128", "hd20", "hd6", "base2")
PREFIX_POSITIONS, PREFIX_T, PREFIX_LENS, PREFIX_SLICES = 260, 17, (17, 11), ((0, 64), (64, 256), (256, 260))
PREFIX_MAX_POSITIONS = 320
ROWS_CLIPS, ROWS_T, ROWS_BEAMS, ROWS_STEPS = 44, 12, 3, 4
VIDEO_CASES = [(16, 7), (24, 7), (96, 7), (16, 1), (16, 2), (16, 3), (16, 5)]          # (image_size, T); lens (T, min(T, 3))
ALONE_GEOMS, ALONE_LEN, ALONE_BUFFERS = ("tiny", "hd64"), 40, (300, 530)
DECODE_STEPS, DECODE_BEAMS, DECODE_MAX_LEN = 6, 2, 8


def geometry(name, **kw):
    cfg = GEOMS["tiny" if name == VALU else name]
    return cfg.with_(**kw) if kw else cfg


@functools.lru_cache(maxsize=None)
def weights(name, **kw):
    """the seeded state dict of a geometry, once per process (base2: the 161M dict's tensors of its layers, see the module docstring)"""
    return synthetic_state_dict_avsr(geometry(name, **kw), WEIGHT_SEED)


def to64(sd):
    return {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}


@functools.lru_cache(maxsize=None)
def weights64(name, **kw):
    return to64(weights(name, **kw))


def ladder_lens(T):
    return (T, math.ceil(0.6 * T), min(T, 3))


def clips(T, lens, seed, holes=()):
    """audio float32 [len(lens)][T][104] and padding mask float32 [len(lens)][T] (1 = padding): full-length synthetic audio, then
    frames >= lens[b] and the frames of every hole (clip, first, last) — first inclusive, last exclusive, cut at T — get zero audio
    and mask 1.  The lengths are explicit because random ones do not land on tile edges."""
    audio, _, mask, _ = synthetic_clips(len(lens), T, seed, ragged=False, image_size=8)          # the tiny image keeps the unused video cheap
    audio, mask = audio.copy(), mask.copy()
    for b, n in enumerate(lens):
        assert 1 <= n <= T, (b, n, T)
        audio[b, n:] = 0.0
        mask[b, n:] = 1.0
    for b, first, last in holes:
        audio[b, first:last] = 0.0
        mask[b, first:last] = 1.0
    assert (mask == 0).any(axis=1).all(), "a clip whose mask covers every frame is out of scope (the reference's softmax is uniform there)"
    return audio, mask


def av_clips(T, lens, seed, image_size):
    """audio, video float32 [B][T][1][H][H] and mask; padded frames carry what the extractor puts there (zero audio, a black image)"""
    audio, video, mask, _ = synthetic_clips(len(lens), T, seed, ragged=False, image_size=image_size)
    for b, n in enumerate(lens):
        audio[b, n:] = 0.0
        video[b, n:] = (0.0 - IMAGE_MEAN) / IMAGE_STD
        mask[b, n:] = 1.0
    return audio, video, mask


def hole_clips(T, seed):
    """section 2: clip 0 full; clip 1 without frames [0, 20) (its first 16-key tile fully masked); clip 2 without [16, 48) (two whole
    tiles in the middle) and, at T = 300, cut at 260"""
    lens = (T, T, 260 if T > 260 else T)
    return clips(T, lens, seed, holes=((1, 0, 20), (2, 16, 48)))


def embed_clip(audio_alone, T, seed):
    """section 6: a buffer of T frames whose clip 0 is `audio_alone` [1][n][104] (padded) and whose clip 1 is full-length"""
    n = audio_alone.shape[1]
    audio, mask = clips(T, (n, T), seed)
    audio[0, :n] = audio_alone[0]
    return audio, mask


def ragged_lens(n, T, seed):
    lens = np.random.default_rng(seed).integers(1, T + 1, size=n)
    lens[0], lens[1] = T, 1
    return tuple(int(x) for x in lens)


def token_ids(cfg, B, L, seed):
    ids = torch.randint(3, cfg.vocab_size, (B, L), generator=torch.Generator().manual_seed(seed))
    ids[:, 0] = cfg.bos_token_id
    return ids


def reference(cfg, sd, sd64, audio, video, mask, ids=None):
    """-> dict: enc / logits / video = the FLOAT64 oracle's outputs (logits on the float64 encoder output; video = every clip's
    `tap_video`), d32_enc / d32_logits / d32_video = max |float32 oracle - float64 oracle| of each, f32_* = the float32 oracle's"""
    t = lambda x, dt: None if x is None else torch.from_numpy(np.asarray(x)).to(dt)            # noqa: E731
    out = {}
    with torch.no_grad():
        run = {}
        for dt, w in ((torch.float64, sd64), (torch.float32, sd)):
            a, v, m = t(audio, dt), t(video, dt), t(mask, dt)
            r = {"enc": oa.encode(cfg, w, a, v, m)}
            assert r["enc"].dtype == dt
            if ids is not None:
                r["logits"] = oa.decode_logits(cfg, w, r["enc"], m, ids)
            if v is not None:
                r["video"] = oa.video_frontend(cfg, w, v)
            run[dt] = r
    for k, v64 in run[torch.float64].items():
        out[k], out["f32_" + k] = v64, run[torch.float32][k]
        out["d32_" + k] = float((run[torch.float32][k].double() - v64).abs().max())
    return out


def bound(d32, tol):
    return min(FACTOR * d32, tol)


def attn_form(hd, Tq, n_keys, causal=False):
    """launch_attn's choice (csrc/k_avsr.hip) for one attention call"""
    if Tq > 1 and not causal and hd in (64, 128):
        return f"mfma<{hd}>"
    if Tq == 1 and n_keys <= 512 and hd % 4 == 0:
        return "step<1>" if n_keys <= 256 else "step<2>"
    if not causal and n_keys <= 512 and hd % 4 == 0:
        return "keys<4>" if n_keys <= 256 else "keys<8>"
    return "general<%d>" % (1 if hd <= 64 else 2 if hd <= 128 else 4)


def posconv_form(cfg, old=False):
    cg = cfg.encoder_embed_dim // cfg.conv_pos_groups
    return f"posconv mfma<{cg // 16}>" if cg % 16 == 0 and cg <= 64 and not old else f"posconv valu(cg {cg})"


def forms(name, T):
    """(encoder attention, cross-attention of a decoding step, positional convolution) of a buffer of T frames"""
    cfg = geometry(name)
    return (attn_form(cfg.encoder_embed_dim // cfg.encoder_attention_heads, T, T), attn_form(cfg.decoder_embed_dim // cfg.decoder_attention_heads, 1, T),
            posconv_form(cfg, old=name == VALU))
