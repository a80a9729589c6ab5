"""-m gpu: sherpa-onnx's modified_beam_search on the device (rs_rnnt_mbs, csrc/k_rnnt_mbs.hip) against its C checker
(tests/k2_mbs_checker.c, the device's float32 order restated on the oracle library's decoder / projection / joint routines):
ids, frames and the float32 score of every utterance BIT FOR BIT, given the device's own joiner.encoder_proj output.

  toy geometry (V = 97)          K = 1, 2, 4, 8; ragged batch with a zero-frame row; <unk>-biased joiner; blank_penalty 0 and 1.5;
                                 with and without length normalisation
  159M decoder geometry          V = 10 720 (ragged last column tile: 10 720 = 167 x 64 + 32), J = D = 512, B = 37, random projection
  K = 1                          == the greedy kernel's ids and frames
  batch invariance               an utterance alone == the same utterance inside a ragged batch, bits
  the public surface             K2Model(decoding_method="modified_beam_search"), transcribe_batch, pipelined == sequential
  errors                         RS_EINVAL on a context without the stateless decoder, bad max_active_paths / penalty, RS_EOVERFLOW
"""
import importlib

import numpy as np
import pytest
import torch

import k2_mbs_ref as R
from reazonspeech_amd.k2.asr import interface
from reazonspeech_amd.k2.asr.model import K2Model, synthetic_tokens
from reazonspeech_amd.runtime import capi
from reazonspeech_amd.runtime.config import TINY
from reazonspeech_amd.runtime.k2_config import ZIPFORMER_TINY
from reazonspeech_amd.runtime.k2_weights import synthetic_state_dict_k2
from reazonspeech_amd.runtime.model import AsrModel
from reazonspeech_amd.runtime.synth import synthetic_batch
from reazonspeech_amd.runtime.tokenizer import SyntheticTokenizer
from reazonspeech_amd.runtime.weights import synthetic_state_dict

k2tr = importlib.import_module("reazonspeech_amd.k2.asr.transcribe")

pytestmark = pytest.mark.gpu
PAD = int(0.9 * 16000)


def build(cfg, seed, sd=None, **kw):
    sd = sd if sd is not None else synthetic_state_dict_k2(cfg, seed)
    return K2Model(cfg, sd, synthetic_tokens(cfg.vocab_size, seed), device="cuda:0", **kw), sd


def ragged_waves(n, seconds, seed, min_seconds):
    audio, lens = synthetic_batch(n, seconds, seed=seed, ragged=True, min_seconds=min_seconds)
    return [np.pad(audio[b, :lens[b]], PAD) for b in range(n)]


def device_mbs(am, f, lens, K, blank_penalty=0.0, length_norm=True, out_cap=None):
    """rs_rnnt_mbs on a projection f [B][Tp][J] (any device) -> list of (ids, frames, score bits)"""
    dev = am.device
    B, Tp, _ = f.shape
    out_cap = out_cap or max(Tp, 1)
    f = f.to(dev).contiguous()
    lens = torch.as_tensor(np.asarray(lens), dtype=torch.int32).to(dev)
    ids = torch.zeros((B, out_cap), dtype=torch.int32, device=dev)
    frames = torch.zeros_like(ids)
    n_ids = torch.full((B,), -1, dtype=torch.int32, device=dev)
    scores = torch.full((B,), float("nan"), dtype=torch.float32, device=dev)
    ws = torch.empty((am.ctx.mbs_workspace_bytes(B, K, Tp, out_cap),), dtype=torch.uint8, device=dev)
    am.ctx.rnnt_mbs(f, lens, B, Tp, K, blank_penalty, length_norm, ids, frames, n_ids, scores, ws, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    n = n_ids.cpu().numpy()
    bits = scores.cpu().numpy().view(np.int32)
    return [(ids[b, :n[b]].cpu().tolist(), frames[b, :n[b]].cpu().tolist(), int(bits[b])) for b in range(B)]


def check(cfg, sd, am, f, lens, **kw):
    got = device_mbs(am, f, lens, **kw)
    want = R.mbs_checker(cfg, sd, f.cpu().numpy(), np.asarray(lens, np.int32), **kw)
    for b, (g, w) in enumerate(zip(got, want)):
        assert g[0] == w["ids"] and g[1] == w["frames"], (kw, b, g[:2], w["ids"], w["frames"])
        assert g[2] == w["score_bits"], (kw, b, g[2], w["score_bits"], w["score"])
    return got, want


def encoder_projection(model, waves):
    """the device's own joiner.encoder_proj output for `waves` (greedy run of the whole path) -> f on the device, lengths, greedy result"""
    am = model.am
    buf = am.stage(waves, buf=am.new_buffers(len(waves), max(len(w) for w in waves)))
    am.run_device(buf)
    torch.cuda.synchronize()
    got = am.collect(buf)
    return buf.joint_enc.clone(), list(got.enc_lens), got


@pytest.fixture(scope="module")
def tiny(gpu_device):
    return build(ZIPFORMER_TINY, 3)


@pytest.fixture(scope="module")
def tiny_projection(tiny):
    model, sd = tiny
    f, lens, greedy = encoder_projection(model, ragged_waves(7, 3.0, 5, 0.7))
    lens[2] = 0                                                           # a zero-frame row inside the batch
    return f, lens, greedy


@pytest.mark.parametrize("K", [1, 2, 4, 8])
@pytest.mark.parametrize("blank_penalty", [0.0, 1.5])
def test_device_equals_checker_toy_geometry(tiny, tiny_projection, K, blank_penalty):
    model, sd = tiny
    f, lens, _ = tiny_projection
    got, want = check(ZIPFORMER_TINY, sd, model.am, f, lens, K=K, blank_penalty=blank_penalty)
    assert got[2] == ([], [], 0)                                          # no frames: no tokens, log_prob 0
    assert sum(len(g[0]) for g in got) > 5
    if K >= 2 and blank_penalty == 0.0:
        assert sum(w["merges"] for w in want) > 0, "the merge path must be exercised"
    check(ZIPFORMER_TINY, sd, model.am, f, lens, K=K, blank_penalty=blank_penalty, length_norm=False)


def test_one_active_path_equals_the_greedy_kernel(tiny, tiny_projection):
    model, sd = tiny
    f, lens, greedy = tiny_projection
    got = device_mbs(model.am, f, lens, K=1)
    for b in range(len(lens)):
        if b != 2:
            assert got[b][0] == greedy.ids[b] and got[b][1] == greedy.frames[b], b
    assert sum(len(x) for x in greedy.ids) > 10


def test_unk_biased_joiner(gpu_device):
    """as test_unk_is_never_emitted_and_costs_no_context: with a joiner biased towards <unk> (+9) it is the best candidate of
    nearly every frame, extends nothing and never appears in a result.  Whether it also MERGES depends on the blank being among
    the K best of the same parent, which this bias alone does not arrange (the checker counts no merge at K = 2 here); the
    second joiner lifts the blank too (+6: blank and <unk> both e^6 above every label), so that (parent, blank) and
    (parent, <unk>) are both taken and merge in most frames — the checker counts 212 merges in 221 frames at K = 4 on the
    oracle's projection of these utterances."""
    cfg = ZIPFORMER_TINY
    waves = ragged_waves(3, 2.0, 11, 0.8)
    for blank_bias in (0.0, 6.0):
        sd = synthetic_state_dict_k2(cfg, 4)
        sd["joiner.output_linear.bias"][cfg.unk_id] += 9.0
        sd["joiner.output_linear.bias"][cfg.blank_id] += blank_bias
        model, _ = build(cfg, 4, sd=sd)
        f, lens, _ = encoder_projection(model, waves)
        for K in (2, 4):
            got, want = check(cfg, sd, model.am, f, lens, K=K)
            assert all(cfg.unk_id not in g[0] for g in got)
            print(f"<unk> +9, blank +{blank_bias:g}, K = {K}: merges {[w['merges'] for w in want]} in {lens} frames")
            if blank_bias > 0 and K == 4:
                assert sum(w["merges"] for w in want) > 0, "blank and <unk> of one parent must merge here"


def test_159m_decoder_geometry(gpu_device):
    """V = 10 720, J = D = 512 behind the toy encoder; a random projection straight into rs_rnnt_mbs as tests/test_gpu_fullsize.py
    does for the other searches: B = 37, ragged lengths, an empty and a full-length row"""
    cfg = ZIPFORMER_TINY.with_(vocab_size=10720, decoder_dim=512, joiner_dim=512).validate()
    model, sd = build(cfg, 0)
    g = torch.Generator().manual_seed(2)
    B, Tp = 37, 30
    f = torch.randn((B, Tp, cfg.joiner_dim), generator=g) * (0.8 + 0.4 * torch.rand((B, 1, 1), generator=g))
    lens = torch.randint(1, Tp + 1, (B,), generator=g, dtype=torch.int32).tolist()
    lens[3], lens[5] = 0, Tp
    got, want = check(cfg, sd, model.am, f, lens, K=4)
    print("159M decoder geometry: tokens", sum(len(g[0]) for g in got), "merges", sum(w["merges"] for w in want))
    assert sum(len(g[0]) for g in got) > 30
    check(cfg, sd, model.am, f[:5], lens[:5], K=8, blank_penalty=1.5)


def test_alone_equals_inside_a_ragged_batch(tiny):
    model, sd = tiny
    f, lens, _ = encoder_projection(model, ragged_waves(5, 3.0, 9, 0.5))
    together = device_mbs(model.am, f, lens, K=4)
    for b in (0, 3):
        alone = device_mbs(model.am, f[b:b + 1, :lens[b]], lens[b:b + 1], K=4)
        assert alone[0] == together[b], b


def test_through_k2model_and_transcribe_batch(tiny):
    cfg = ZIPFORMER_TINY
    _, sd = tiny
    model, _ = build(cfg, 3, sd=sd, decoding_method="modified_beam_search")
    assert (model.cfg.decoding, model.cfg.beam_size) == ("modified_beam_search", 4)
    audio, lens = synthetic_batch(4, 3.0, seed=21, ragged=True, min_seconds=1.0)
    audios = [interface.AudioData(audio[b, :lens[b]], 16000) for b in range(4)]
    res = k2tr.transcribe_batch(model, audios, interface.TranscribeConfig(verbose=False))
    one = k2tr.transcribe(model, audios[1], interface.TranscribeConfig(verbose=False))
    assert one.text == res[1].text and [s.seconds for s in one.subwords] == [s.seconds for s in res[1].subwords]
    # the same batch through the runtime: scores come back, and the result is the checker's on the device's projection
    waves = [np.pad(a.waveform, PAD) for a in audios]
    am = model.am
    buf = am.stage(waves, buf=am.new_buffers(len(waves), max(len(w) for w in waves)))
    am.run_device(buf)
    torch.cuda.synchronize()
    dec = am.collect(buf)
    assert dec.scores is not None and all(s <= 0.0 for s in dec.scores)
    want = R.mbs_checker(cfg, sd, buf.joint_enc.cpu().numpy(), np.asarray(dec.enc_lens, np.int32), K=4)
    assert dec.ids == [w["ids"] for w in want] and dec.frames == [w["frames"] for w in want]
    assert [np.float32(s) for s in dec.scores] == [np.float32(w["score"]) for w in want]
    assert ["".join(model.symbol(i) for i in ids) for ids in dec.ids] == [r.text for r in res]
    assert sum(len(x) for x in dec.ids) > 5


def test_pipelined_equals_sequential(tiny):
    cfg = ZIPFORMER_TINY
    _, sd = tiny
    model, _ = build(cfg, 3, sd=sd, decoding_method="modified_beam_search", max_active_paths=3)
    am = model.am
    bufs, want = [], []
    for k in range(2):
        waves = ragged_waves(6, 2.5, 40 + k, 0.5)
        ref = am.transcribe_waveforms(waves)
        want.append((ref.ids, ref.frames, ref.scores))
        bufs.append(am.stage(waves, buf=am.new_buffers(6, max(len(w) for w in waves))))
    got = {}

    def grab(buf):
        torch.cuda.current_stream().synchronize()
        got.setdefault(id(buf), []).append(am.collect(buf))

    am.run_pipelined(bufs, 5, after_decode=grab)
    for k in range(2):
        runs = got[id(bufs[k])]
        assert len(runs) == (3 if k == 0 else 2)
        for r in runs:
            assert (r.ids, r.frames, r.scores) == want[k]
    # a list longer than max_batch goes through the host pipeline
    waves = ragged_waves(9, 2.0, 50, 0.5)
    whole, parts = am.transcribe_waveforms(waves), am.transcribe_waveforms(waves, max_batch=4)
    assert (whole.ids, whole.frames, whole.scores) == (parts.ids, parts.frames, parts.scores)


def test_argument_errors(tiny, tiny_projection):
    model, sd = tiny
    f, lens, _ = tiny_projection
    for kw in (dict(K=0), dict(K=9)):
        with pytest.raises(RuntimeError):
            device_mbs(model.am, f, lens, **kw)                            # the workspace query rejects it first
    ctx, dev = model.am.ctx, model.am.device
    B, Tp, _ = f.shape
    i32 = lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)        # noqa: E731
    ws = torch.empty((ctx.mbs_workspace_bytes(B, 8, Tp, Tp),), dtype=torch.uint8, device=dev)
    args = lambda K, pen: (f, torch.as_tensor(lens, dtype=torch.int32).to(dev), B, Tp, K, pen, True, i32(B, Tp), i32(B, Tp), i32(B),   # noqa: E731
                           torch.zeros((B,), device=dev), ws, 0)
    for K, pen, word in ((9, 0.0, "max_active_paths"), (0, 0.0, "max_active_paths"), (4, -1.0, "blank_penalty")):
        with pytest.raises(capi.RsError, match=word) as e:
            ctx.rnnt_mbs(*args(K, pen))
        assert e.value.code == capi.RS_EINVAL
    with pytest.raises(capi.RsError) as e:                                 # a result that does not fit out_cap
        device_mbs(model.am, f, lens, K=4, out_cap=1)
    assert e.value.code == capi.RS_EOVERFLOW


def test_a_context_without_the_stateless_decoder_is_rejected(gpu_device):
    sd = synthetic_state_dict(TINY, 0)
    nemo = AsrModel(TINY, sd, SyntheticTokenizer(TINY.vocab_size), device="cuda:0")
    with pytest.raises(RuntimeError):
        nemo.ctx.mbs_workspace_bytes(2, 4, 10, 10)
    dev = nemo.device
    f = torch.zeros((2, 10, TINY.joint_hidden), device=dev)
    z = lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)          # noqa: E731
    with pytest.raises(capi.RsError, match="Zipformer") as e:
        nemo.ctx.rnnt_mbs(f, z(2) + 10, 2, 10, 4, 0.0, True, z(2, 10), z(2, 10), z(2), torch.zeros((2,), device=dev),
                          torch.empty((1 << 20,), dtype=torch.uint8, device=dev), 0)
    assert e.value.code == capi.RS_EINVAL
