"""-m gpu: the Zipformer2 encoder at the utterance lengths that pick each kernel form (toy geometry, csrc/k_zipformer.hip).

The encoder chooses its kernels from the frame count of the BUFFER, per stack: Ts = ceil(T3 / ds) frames (T3 = the frames of the
50 Hz stack = cfg.embed_frames(n_feat), ds = 1 / 2 / 4 for the toy's three stacks) and Tp = Ts rounded up to a multiple of 32.
  attention weights (bf16 mode)   k2_attn_weights1_kernel<10 | 20 | 40> for Tp <= 160 / 320 / 640, the three-sweep
                                  k2_attn_weights_kernel above; 64-query blocks, 16-key tiles
  k2_vt_kernel / k2_pv_kernel     64-key tiles / 128-query blocks, 256-key chunks
  k2_cnx_dw_kernel                29-frame tiles (CNX_TT)
  dwconv_act_kernel<k, 1>         128-frame tiles with halos of (k - 1) / 2 = 3 / 7 / 15 frames
  k2_stack_in / k2_stack_out      groups of ds frames, the last one partly filled when T3 % ds != 0
  k2_output_kernel                pairs of frames, the last one half filled when T3 is odd
  float32 mode (k2f_* kernels)    one thread or wave per output, no forms: the same lengths check its masks and edges
Utterances are `runtime/synth.py` speech-like audio of exactly (2 T3 + 7) feature frames (seed = T3), no padding.

1 / 2. LENGTH LADDER, float32 and bf16 mode, each utterance alone in a buffer sized to it.  T3 -> stack 0's attention form:
     1 2 3 4 7 8 9        one-sweep<10>, Tp 32; stacks 1 / 2 hold ONE frame up to T3 = 2 / 4; every stack is shorter than its
                          depthwise half-width (7 / 3 / 7) up to T3 = 7; T3 % 4 = 1, 2, 3 leave stack 2's last group partly filled
     28 29 30             one-sweep<10>, Tp 32; the ConvNeXt tile edge (29)
     63 64 65             one-sweep<10>, Tp 64 / 64 / 96; the 64-query / 64-key edge
     127 128 129          one-sweep<10>, Tp 128 / 128 / 160; the 128-frame (depthwise, weights x values) edge
     159 160 161          one-sweep<10> / <10> / <20>, Tp 160 / 160 / 192: a form boundary
     255 256 257          one-sweep<20>, Tp 256 / 256 / 288; the 256-key chunk edge of k2_pv_kernel
     319 320 321          one-sweep<20> / <20> / <40>, Tp 320 / 320 / 352: a form boundary (stack 1 crosses 160 / 161 here)
     511 513              one-sweep<40>, Tp 512 / 544
     639 640 641 673      one-sweep<40> / <40> / THREE-SWEEP / THREE-SWEEP, Tp 640 / 640 / 672 / 704: a form boundary (stack 1 at 320 /
                          321, stack 2 at 160 / 161)
     1100                 three-sweep in stack 0 (Tp 1120), one-sweep<40> in stack 1 (Tp 576), one-sweep<20> in stack 2 (Tp 288)
   the ladder again at 3, 9, 29, 129, 641 with cnn_kernel = (31, 15, 7): dwconv_act_kernel<31, 1> shorter than its half-width
   (15), at a tile edge and in two tiles per stack.
   float32 mode: every tap within 2e-4 of the float32 oracle, ids and frames identical to `oz.greedy_search`; each utterance's
   smallest decision margin in the oracle (float64 walk, `greedy_margins`) is asserted >= 1e-3 (the project's near-tie), so
   there is no exemption list.  bf16 mode: taps within max 0.08 / mean 0.01 of the bf16-recipe oracle, ids and frames
   bit-exact against oracle/k2_greedy.c on the device's own projection.
3. ONE UTTERANCE THROUGH EVERY FORM, bits, both modes: T3 = 9, 65, 161, 321, 600 alone (one-sweep<10>, <10>, <20>, <40>, <40>),
   then as row 0 of buffers whose stack-0 Tp is 192 / 352 / 672 / 1120 (one-sweep<20> / <40> / three-sweep / three-sweep; stacks 1
   and 2 move through <10> .. <40> with them), then inside a ragged batch with a T3 = 1100 row (three-sweep): enc, joint_enc,
   ids and frames `torch.equal` to the alone run.  In bf16 mode this holds the three-sweep kernel to every one-sweep form bit
   for bit.
4. POSITION-TABLE CAPACITY, both modes: a model built with pos_cap = 64 against the default (1024) on T3 = 40, 300 (grows the
   tables to 512 rows of relative positions), 40 again: bits.
5. TOO-SHORT INPUT, both modes: a row of 8 feature frames (T3 = 0) inside a ragged batch returns no ids and leaves its neighbours'
   bits alone.  (Read beforehand: k2_lens_kernel clamps T3 to 0, every kernel of both modes masks by the row's own length and
   guards `len - 1`, the attention kernels write zeros for a block with no valid query, rnnt_init_kernel leaves a row with
   enc_len 0 off the alive list; a BUFFER of fewer than 9 frames is refused by rs_k2_encoder_forward with RS_EINVAL.)
6. THE PUBLIC PATH: `transcribe_batch` of three utterances == `transcribe` of each alone (tokens, timestamps, text), through the
   whole-second buffer buckets.  The package pads 0.9 s on both sides, so the shortest utterance it can hand over has T3 = 86:
   the three have T3 = 87, 330 and 700 (one-sweep<10>, one-sweep<40>, three-sweep when alone; all three-sweep together).

Every case prints its worst error per tap; the worst of a run lands in the parity report of tests/test_gpu_k2_fp32.py (keys
k2_lengths_fp32 / k2_lengths_bf16) and DESIGN.md keeps the figures beside the tolerances.
"""
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch

from reazonspeech_amd.runtime.k2_config import ZIPFORMER_TINY
from reazonspeech_amd.runtime.k2_weights import synthetic_state_dict_k2
from reazonspeech_amd.runtime.synth import synthetic_batch
from reazonspeech_amd.k2.asr.model import K2Model, synthetic_tokens
from reazonspeech_amd.k2.asr import interface
from oracle import zipformer as oz, greedy as og

from test_gpu_k2 import run, k2tr, PAD
from test_gpu_k2_fp32 import report, TOL_F32, TOL_FEAT, TOL_BF16

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
TOL_BF16_MEAN = 0.01
NEAR_TIE = 1e-3          # tests/golden/make_k2_golden.py NEAR_TIE
WEIGHT_SEED = 3
CFGS = {"tiny": ZIPFORMER_TINY, "k31": ZIPFORMER_TINY.with_(cnn_kernel=(31, 15, 7))}
LADDER = (1, 2, 3, 4, 7, 8, 9, 28, 29, 30, 63, 64, 65, 127, 128, 129, 159, 160, 161, 255, 256, 257, 319, 320, 321, 511, 513,
          639, 640, 641, 673, 1100)
LADDER_K31 = (3, 9, 29, 129, 641)
CASES = [("tiny", t) for t in LADDER] + [("k31", t) for t in LADDER_K31]
FORM_T3 = (9, 65, 161, 321, 600)
FORM_TP = (192, 352, 672, 1120)
WORST = {"fp32": {}, "bf16": {}}


@functools.lru_cache(maxsize=None)
def _golden_tools():
    spec = importlib.util.spec_from_file_location("make_k2_golden", os.path.join(HERE, "golden", "make_k2_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=None)
def weights(variant):
    return synthetic_state_dict_k2(CFGS[variant], WEIGHT_SEED)


def samples_for(cfg, t3):
    """samples of an utterance whose 50 Hz stack has exactly t3 frames: 2 t3 + 7 feature frames (t3 = 0: 8, one too few)"""
    n_feat = 2 * t3 + 7 if t3 > 0 else 8
    n = n_feat * cfg.frame_shift
    assert cfg.embed_frames(cfg.fbank_frames(n)) == t3
    return n


@functools.lru_cache(maxsize=None)
def wave(t3, seed=None):
    cfg = ZIPFORMER_TINY
    n = samples_for(cfg, t3)
    w = synthetic_batch(1, n / cfg.sample_rate, seed=t3 if seed is None else seed)[0][0][:n]
    assert w.shape[0] == n
    return w


@functools.lru_cache(maxsize=None)
def oracle(variant, t3, recipe):
    """the CPU oracle's forward pass of wave(t3), once per (geometry, length, recipe) -> (outputs, taps)"""
    taps = {}
    ref = oz.forward(CFGS[variant], weights(variant), wave(t3), recipe, taps)
    return ref, taps


def stack_forms(cfg, t3):
    """the attention-weights form each stack of a buffer of t3 frames selects in bf16 mode (csrc/k_zipformer.hip)"""
    out = []
    for ds in cfg.downsampling:
        tp = (-(-t3 // ds) + 31) // 32 * 32
        out.append((tp, "3sweep" if tp > 640 else "1sweep<%d>" % (10 if tp <= 160 else 20 if tp <= 320 else 40)))
    return out


@pytest.fixture(scope="module")
def models(gpu_device):
    cache = {}

    def get(variant, precision, **kw):
        key = (variant, precision, tuple(sorted(kw.items())))
        if key not in cache:
            cfg = CFGS[variant]
            cache[key] = K2Model(cfg, weights(variant), synthetic_tokens(cfg.vocab_size, WEIGHT_SEED), device="cuda:0", precision=precision, **kw)
        return cache[key]
    yield get
    cache.clear()
    torch.cuda.empty_cache()


def tap_pairs(cfg, t3, n, emb, stacks, enc, buf, ref, taps):
    pairs = [("embed", emb[0, :t3], taps["embed"])] + [(f"S{s}", stacks[s][0, :t3], taps[f"S{s}"]) for s in range(cfg.n_stacks)]
    return pairs + [("enc", enc[0, :n], ref["enc"]), ("joint", buf.joint_enc[0, :n].cpu(), ref["joint_enc"])]


def lengths_and_features(cfg, buf, got, ref, t3):
    nf, n = ref["feats"].shape[0], ref["enc"].shape[0]
    assert int(buf.n_frames[0]) == nf and cfg.embed_frames(nf) == t3
    assert got.enc_lens[0] == n == cfg.enc_frames(nf)
    d = float((buf.feats[0, :nf].cpu() - ref["feats"]).abs().max())
    assert d <= TOL_FEAT, d
    return n, d


def note(mode, variant, t3, stats):
    w = WORST[mode]
    for k, v in stats.items():
        if v > w.get(k, (0.0,))[0]:
            w[k] = (v, f"{variant}:{t3}")
    report("k2_lengths_" + mode, {k: {"max_err": v[0], "at": v[1]} for k, v in sorted(w.items())})


@pytest.mark.parametrize("variant,t3", CASES)
def test_ladder_fp32_mode_vs_fp32_oracle(models, variant, t3):
    """float32 mode: every tap within 2e-4, ids and frames identical; the oracle's decision margin is >= 1e-3 at every length"""
    cfg, sd = CFGS[variant], weights(variant)
    ref, taps = oracle(variant, t3, "fp32")
    want = oz.greedy_search(cfg, sd, ref["joint_enc"])
    margin = _golden_tools().greedy_margins(cfg, sd, ref["joint_enc"].numpy(), *want)
    assert margin >= NEAR_TIE, f"T3 = {t3}: the oracle's own margin {margin:.2e} is a near-tie: pick another seed"
    buf, emb, stacks, enc, got = run(models(variant, "fp32"), [wave(t3)])
    n, dfeat = lengths_and_features(cfg, buf, got, ref, t3)
    stats = {"feats": dfeat}
    for name, a, r in tap_pairs(cfg, t3, n, emb, stacks, enc, buf, ref, taps):
        assert a.shape == r.shape, (name, a.shape, r.shape)
        stats[name] = float((a - r).abs().max())
    print(f"k2 lengths fp32 {variant} T3={t3} {stack_forms(cfg, t3)} margin={margin:.2e} tokens={len(want[0])}:", {k: f"{v:.2e}" for k, v in stats.items()})
    note("fp32", variant, t3, stats)
    for name, v in stats.items():
        if name != "feats":
            assert v <= TOL_F32, (name, t3, v)
    assert (got.ids[0], got.frames[0]) == want


@pytest.mark.parametrize("variant,t3", CASES)
def test_ladder_bf16_mode_vs_bf16_recipe_oracle(models, variant, t3):
    """bf16 mode: taps within 0.08 / 0.01 of the bf16-recipe oracle, the search bit-exact on the device's own projection"""
    cfg, sd = CFGS[variant], weights(variant)
    ref, taps = oracle(variant, t3, "bf16")
    buf, emb, stacks, enc, got = run(models(variant, "bf16"), [wave(t3)])
    n, dfeat = lengths_and_features(cfg, buf, got, ref, t3)
    stats, means = {"feats": dfeat}, {}
    for name, a, r in tap_pairs(cfg, t3, n, emb, stacks, enc, buf, ref, taps):
        assert a.shape == r.shape, (name, a.shape, r.shape)
        e = (a - r).abs()
        stats[name], means[name] = float(e.max()), float(e.mean())
    print(f"k2 lengths bf16 {variant} T3={t3} {stack_forms(cfg, t3)}:", {k: f"{v:.2e}" for k, v in stats.items()}, "mean", {k: f"{v:.2e}" for k, v in means.items()})
    note("bf16", variant, t3, stats)
    for name in means:
        assert stats[name] <= TOL_BF16 and means[name] <= TOL_BF16_MEAN, (name, t3, stats[name], means[name])
    same = og.k2_greedy(cfg, sd, buf.joint_enc.cpu().numpy(), np.asarray(got.enc_lens, np.int32))
    assert got.ids == [r[0] for r in same] and got.frames == [r[1] for r in same]
    assert cfg.unk_id not in got.ids[0] and cfg.blank_id not in got.ids[0]


def outputs(buf, enc, got, b):
    n = got.enc_lens[b]
    return n, enc[b, :n].clone(), buf.joint_enc[b, :n].cpu(), got.ids[b], got.frames[b]


def same_bits(a, b):
    return a[0] == b[0] and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and a[3] == b[3] and a[4] == b[4]


ALONE = {}


def alone(models, precision, t3):
    """(enc_len, enc, joint_enc, ids, frames) of wave(t3) alone in a buffer sized to it, once per (mode, length)"""
    key = (precision, t3)
    if key not in ALONE:
        buf, _, _, enc, got = run(models("tiny", precision), [wave(t3)], taps=False)
        ALONE[key] = outputs(buf, enc.cpu(), got, 0)
        assert ALONE[key][0] == (t3 + 1) // 2
    return ALONE[key]


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
@pytest.mark.parametrize("t3", FORM_T3)
def test_one_utterance_through_every_form_bits(models, precision, t3):
    """row 0 of a buffer whose stack-0 Tp is 192 / 352 / 672 / 1120 == the utterance alone, bit for bit"""
    cfg = ZIPFORMER_TINY
    ref = alone(models, precision, t3)
    ran = []
    for tp in FORM_TP:
        if tp < t3:
            continue
        buf, _, _, enc, got = run(models("tiny", precision), [wave(t3)], taps=False, l_max=samples_for(cfg, tp))
        assert stack_forms(cfg, cfg.embed_frames(buf.t_max))[0][0] == tp
        assert same_bits(outputs(buf, enc.cpu(), got, 0), ref), (precision, t3, tp)
        ran.append(stack_forms(cfg, tp))
    assert ran
    print(f"k2 forms {precision} T3={t3}: alone {stack_forms(cfg, t3)} == in buffers {ran}")


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_ragged_batch_across_forms_bits(models, precision):
    """the five utterances next to a T3 = 1100 row (three-sweep in stack 0) == each alone, bit for bit"""
    cfg = ZIPFORMER_TINY
    t3s = FORM_T3 + (1100,)
    buf, _, _, enc, got = run(models("tiny", precision), [wave(t) for t in t3s], taps=False)
    assert stack_forms(cfg, cfg.embed_frames(buf.t_max))[0] == (1120, "3sweep")
    enc = enc.cpu()
    for b, t3 in enumerate(t3s):
        assert same_bits(outputs(buf, enc, got, b), alone(models, precision, t3)), (precision, t3)
    assert sum(len(x) for x in got.ids) > 10


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_position_table_capacity_and_growth_bits(models, precision):
    """pos_cap = 64 (every kernel indexes the tables as cap - len + r) and the tables grown by AsrModel.ensure_pos_cap == the
    default capacity, bit for bit, before and after the growth"""
    small = models("tiny", precision, pos_cap=64)
    full = models("tiny", precision)
    assert small.am.pos_cap == 64 and full.am.pos_cap >= 2 * 64
    cap0 = full.am.pos_cap
    for step, t3 in enumerate((40, 300, 40)):
        buf, _, _, enc, got = run(small, [wave(t3)], taps=False)
        if step == 0:
            assert small.am.pos_cap == 64, "T3 = 40 fits the small tables: they must not have grown yet"
        else:
            assert small.am.pos_cap >= 2 * 150 + 2 and small.am.pos_cap >= 2 * buf.tp_max + 2
        b2, _, _, e2, g2 = run(full, [wave(t3)], taps=False)
        assert same_bits(outputs(buf, enc.cpu(), got, 0), outputs(b2, e2.cpu(), g2, 0)), (precision, step, t3)
        assert got.enc_lens[0] == (t3 + 1) // 2
    assert small.am.pos_cap == 512 and full.am.pos_cap == cap0
    assert float(enc.abs().max()) > 0.1


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_too_short_row_inside_a_ragged_batch(models, precision):
    """8 feature frames are one too few for encoder_embed (T3 = 0): the row returns no ids, its neighbours keep their bits"""
    cfg = ZIPFORMER_TINY
    model = models("tiny", precision)
    t3s = (65, 0, 161, 30)
    waves = [wave(t) for t in t3s]
    l_max = max(len(w) for w in waves)
    buf, _, _, enc, got = run(model, waves, taps=False)
    assert int(buf.n_frames[1]) == 8 and got.enc_lens[1] == 0
    assert got.ids[1] == [] and got.frames[1] == []
    assert torch.all(enc[1] == 0) and torch.all(torch.isfinite(buf.joint_enc))
    keep = [0, 2, 3]
    b2, _, _, e2, g2 = run(model, [waves[b] for b in keep], taps=False, l_max=l_max)
    enc, e2 = enc.cpu(), e2.cpu()
    for k, b in enumerate(keep):
        assert got.enc_lens[b] == (t3s[b] + 1) // 2
        assert same_bits(outputs(buf, enc, got, b), outputs(b2, e2, g2, k)), (precision, b)
        assert same_bits(outputs(buf, enc, got, b), alone(models, precision, t3s[b])), (precision, b)
    assert sum(len(got.ids[b]) for b in keep) > 0


def test_transcribe_batch_equals_transcribe_across_forms(models):
    """the public path (whole-second buffer buckets): three utterances of T3 = 87 (the shortest the 0.9 s padding allows), 330
    and 700 after padding, together == each alone: tokens, timestamps, text"""
    cfg = ZIPFORMER_TINY
    model = models("tiny", "bf16")
    audios = []
    for t3 in (87, 330, 700):
        n = samples_for(cfg, t3) - 2 * PAD
        assert n > 0
        wav = synthetic_batch(1, n / cfg.sample_rate, seed=7000 + t3)[0][0][:n]
        assert cfg.embed_frames(cfg.fbank_frames(len(wav) + 2 * PAD)) == t3
        audios.append(interface.AudioData(wav, cfg.sample_rate))
    together = k2tr.transcribe_batch(model, audios)
    for a, res in zip(audios, together):
        one = k2tr.transcribe(model, a, interface.TranscribeConfig(verbose=False))
        assert [s.token for s in res.subwords] == [s.token for s in one.subwords]
        assert [s.seconds for s in res.subwords] == [s.seconds for s in one.subwords]
        assert res.text == one.text
    assert sum(len(r.subwords) for r in together) > 10
