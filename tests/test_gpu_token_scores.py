"""-m gpu: token log-probabilities on the device (rs_rnnt_token_scores, csrc/k_rnnt_scores.hip) against the C checker
(tests/token_scores_checker.c: the pass restated on the oracle library in the device's float32 order): logp BITS and top1, given
the device's own joint-encoder projection, ids and frames.

  greedy, per family            7 ragged utterances (weight recipes and wave seeds chosen with the CPU oracle); the lengths are
                                cut (a greedy result on a shorter utterance is the prefix of the longer one's) so that the batch holds: a zero-frame row, a row with frames but no token, a row
                                with one token, a token at frame 0, a token at frame enc_len - 1, a frame carrying two tokens (nemo:
                                the only family whose greedy search emits more than one token per frame) and a row whose count
                                reaches u_cap; top1 == ids
  beam results, per family      nemo ALSD 4 (frames are alignment steps: the flag), espnet beam 4, k2 modified beam search K = 4;
                                top1 may differ from ids
  real output widths            random projections, B = 5, Tp = 30: V + 1 = 3001 / J = 640 / two LSTM layers; k2 V = 10 720,
                                J = D = 512; the espnet 120M decoder geometry (V = 2600, H = 512, J = 640); the toy V = 97
  chunking                      the minimum workspace (32 rows per chunk: several chunks, a boundary inside an utterance) and a
                                generous one give identical bits
  batch invariance              an utterance alone == the same utterance inside the ragged batch, bits
  the public surface            per family: transcribe == the transcribe_batch row; 9 utterances at max_batch = 4 through the host
                                pipeline == one batch; scores on leaves ids / frames / text as they are; off = the plain type
  errors                        an avsr or unfinalised context and a short workspace: RS_EINVAL before any launch; a bad frame / id:
                                NaN in its slot and RS_EINVAL after the sync, the other slots keep their bits
"""
import importlib

import numpy as np
import pytest
import torch

import token_scores_ref as R
from reazonspeech_amd.espnet.asr import interface as ei
from reazonspeech_amd.espnet.asr.model import EspnetModel, synthetic_token_list
from reazonspeech_amd.k2.asr import interface as ki
from reazonspeech_amd.k2.asr.model import K2Model, synthetic_tokens
from reazonspeech_amd.nemo.asr import interface as ni
from reazonspeech_amd.runtime import capi
from reazonspeech_amd.runtime.avsr_config import AVSR_TINY
from reazonspeech_amd.runtime.config import ESPNET_TINY, TINY, WIDE2
from reazonspeech_amd.runtime.k2_config import ZIPFORMER_TINY
from reazonspeech_amd.runtime.k2_weights import synthetic_state_dict_k2
from reazonspeech_amd.runtime.model import AsrModel
from reazonspeech_amd.runtime.synth import synthetic_batch
from reazonspeech_amd.runtime.tokenizer import SyntheticTokenizer
from reazonspeech_amd.runtime.weights import synthetic_state_dict
from reazonspeech_amd.runtime.weights_espnet import synthetic_state_dict_espnet

ntr = importlib.import_module("reazonspeech_amd.nemo.asr.transcribe")
etr = importlib.import_module("reazonspeech_amd.espnet.asr.transcribe")
ktr = importlib.import_module("reazonspeech_amd.k2.asr.transcribe")

pytestmark = pytest.mark.gpu
FAMILIES = ("nemo", "espnet", "k2")
RECHOOSE = "re-choose the inputs (seed / lengths) of this fixture: the batch must hold "


def build(family, cfg=None, espnet_blank_bias=8.0, **kw):
    """-> (runtime model, state dict, configuration, the package's model object)"""
    if family == "nemo":
        cfg = cfg or TINY
        # (TINY: the recipe and the wave seed of `scene` were chosen with the CPU oracle — oracle/model.py in its bf16 recipe + the
        #  oracle's greedy search — so that the shaped batch holds every boundary case; the default recipe emits ten tokens per
        #  frame at the last frames of two utterances and nothing else)
        sd = synthetic_state_dict(cfg, 0, **({"blank_bias": 6.5} if cfg is WIDE2 else {"blank_bias": 3.5, "dec_gain": 4.0}))
        am = AsrModel(cfg, sd, SyntheticTokenizer(cfg.vocab_size), device="cuda:0", **kw)
        return am, sd, am.cfg, am
    if family == "espnet":                                  # (chosen with the CPU oracle like the nemo recipe; the beam search ends on it)
        cfg = cfg or ESPNET_TINY
        sd = synthetic_state_dict_espnet(cfg, 11, blank_bias=espnet_blank_bias, dec_gain=8.0)
        m = EspnetModel(cfg, sd, synthetic_token_list(cfg.vocab_size, 11), device="cuda:0", **kw)
        return m.am, sd, m.cfg, m
    cfg = cfg or ZIPFORMER_TINY
    sd = synthetic_state_dict_k2(cfg, 3)
    m = K2Model(cfg, sd, synthetic_tokens(cfg.vocab_size, 3), device="cuda:0", **kw)
    return m.am, sd, m.cfg, m


def ragged_waves(n, seconds, seed, min_seconds=0.5):
    audio, lens = synthetic_batch(n, seconds, seed=seed, ragged=True, min_seconds=min_seconds)
    return [audio[b, :lens[b]] for b in range(n)]


def dev_i32(am, a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32)).to(am.device)


def device_greedy(am, f, lens):
    """rs_rnnt_greedy on a projection f [B][Tp][J] (device) -> [(ids, frames)]"""
    B, Tp, _ = f.shape
    u_max = max(am.cfg.label_cap(Tp), 1)
    ids = torch.zeros((B, u_max), dtype=torch.int32, device=am.device)
    frames, n_ids = torch.zeros_like(ids), torch.zeros((B,), dtype=torch.int32, device=am.device)
    ws = torch.empty((am.ctx.workspace_bytes(B, 16),), dtype=torch.uint8, device=am.device)
    am.ctx.rnnt_greedy(f, dev_i32(am, lens), B, Tp, u_max, ids, frames, n_ids, ws, torch.cuda.current_stream().cuda_stream)
    n, ids, frames = n_ids.cpu().numpy(), ids.cpu().numpy(), frames.cpu().numpy()
    return [(ids[b, :n[b]].tolist(), frames[b, :n[b]].tolist()) for b in range(B)]


def device_scores(am, f, lens, ids, frames, n, steps=False, workspace="generous", want_code=None):
    """rs_rnnt_token_scores -> (logp float32 [B][u_cap], top1 int32 [B][u_cap]); slots the call must not touch hold 7.0 / -9"""
    B, Tp, _ = f.shape
    u_cap = ids.shape[1]
    logp = torch.full((B, u_cap), 7.0, dtype=torch.float32, device=am.device)
    top1 = torch.full((B, u_cap), -9, dtype=torch.int32, device=am.device)
    least = am.ctx.token_scores_workspace_bytes(B, u_cap)
    ws = torch.empty((least if workspace == "minimum" else least + (64 << 20),), dtype=torch.uint8, device=am.device)
    args = (f, dev_i32(am, lens), B, Tp, dev_i32(am, ids), dev_i32(am, frames), dev_i32(am, n), logp, top1, ws,
            torch.cuda.current_stream().cuda_stream)
    if want_code is None:
        am.ctx.rnnt_token_scores(*args, frames_are_steps=steps)
    else:
        with pytest.raises(capi.RsError) as e:
            am.ctx.rnnt_token_scores(*args, frames_are_steps=steps)
        assert e.value.code == want_code
    torch.cuda.synchronize()
    return logp.cpu().numpy(), top1.cpu().numpy()


def check(am, sd, f, lens, rows, steps=False, workspace="generous"):
    """device == checker: bits of every log-probability, top1; untouched slots.  rows = [(ids, frames)] -> (logp, top1, n)"""
    u_cap = max(max(len(r[0]) for r in rows), 1)
    ids, n = R.pack([r[0] for r in rows], u_cap)
    frames, _ = R.pack([r[1] for r in rows], u_cap)
    got_lp, got_t1 = device_scores(am, f, lens, ids, frames, n, steps, workspace)
    want_lp, want_t1 = R.scores_checker(am.cfg, sd, f.cpu().numpy(), np.asarray(lens, np.int32), ids, frames, n, steps)
    valid = np.arange(u_cap)[None, :] < n[:, None]
    assert (got_lp[~valid] == 7.0).all() and (got_t1[~valid] == -9).all(), "slots at u >= n_ids must be left untouched"
    assert not np.isnan(got_lp[valid]).any()
    diff = np.argwhere(valid & (got_lp.view(np.int32) != want_lp.view(np.int32)))
    assert len(diff) == 0, (diff[:5].tolist(), got_lp[valid & (got_lp.view(np.int32) != want_lp.view(np.int32))][:5], want_lp[tuple(diff[0])])
    assert (got_t1[valid] == want_t1[valid]).all()
    assert (got_lp[valid] <= 1e-6).all()
    return got_lp, got_t1, n


def shape_lengths(rows, enc_lens):
    """lengths of the greedy fixture: a greedy result on the first T frames of an utterance is the prefix (frames < T) of the
    result on all of them, so cutting a length places a boundary case where the batch does not hold it already; the richest row
    stays whole"""
    lens = [int(t) for t in enc_lens]
    count = lambda b: len(rows[b][0])                                           # noqa: E731
    free = sorted(range(len(rows)), key=lambda b: (count(b), b))                # poorest first
    free.pop()                                                                  # the richest row stays whole

    def take(pred):
        for b in free:
            if pred(b):
                free.remove(b)
                return b
        return None

    b = take(lambda b: count(b) == 0)                                           # a zero-frame row
    lens[free.pop(0) if b is None else b] = 0
    if take(lambda b: count(b) == 0 and lens[b] > 0) is None:                   # frames, no token: stop before the first token
        b = take(lambda b: count(b) >= 1 and rows[b][1][0] >= 1)
        if b is not None:
            lens[b] = rows[b][1][0]
    if take(lambda b: count(b) == 1) is None:                                   # one token: stop before the second
        b = take(lambda b: count(b) >= 2 and rows[b][1][1] > rows[b][1][0])
        if b is not None:
            lens[b] = rows[b][1][1]
    if not any(count(b) and lens[b] > 0 and rows[b][1][-1] == lens[b] - 1 for b in range(len(rows))):   # a token at the last frame
        b = take(lambda b: count(b) >= 1)
        if b is not None:
            lens[b] = rows[b][1][-1] + 1
    return lens


_scenes = {}


def scene(family):
    """per family, once: the model, the device's projection of 7 ragged utterances, the shaped lengths and the device's greedy
    result on them"""
    if family not in _scenes:
        am, sd, cfg, model = build(family)
        waves = ragged_waves(7, 3.0, {"nemo": 9, "espnet": 21, "k2": 5}[family])
        buf = am.stage(waves, buf=am.new_buffers(len(waves), max(len(w) for w in waves)))
        am.run_device(buf)
        torch.cuda.synchronize()
        whole = am.collect(buf)
        f = buf.joint_enc.clone()
        lens = shape_lengths(list(zip(whole.ids, whole.frames)), whole.enc_lens)
        rows = device_greedy(am, f, lens)
        print(f"{family}: frames {list(whole.enc_lens)} -> {lens}, tokens {[len(x) for x in whole.ids]} -> {[len(r[0]) for r in rows]}, "
              f"first frames {[r[1][0] if r[1] else None for r in rows]}")
        _scenes[family] = (am, sd, cfg, f, lens, rows)
    return _scenes[family]


@pytest.mark.parametrize("family", FAMILIES)
def test_greedy_device_equals_checker(gpu_device, family):
    am, sd, cfg, f, lens, rows = scene(family)
    counts = [len(r[0]) for r in rows]
    assert any(t == 0 for t in lens), RECHOOSE + "a zero-frame row"
    assert any(t > 0 and c == 0 for t, c in zip(lens, counts)), RECHOOSE + "a row with frames but no token"
    assert any(c == 1 for c in counts), RECHOOSE + "a row with one token"
    assert any(r[1] and r[1][0] == 0 for r in rows), RECHOOSE + "a token at frame 0"
    assert any(r[1] and r[1][-1] == t - 1 for r, t in zip(rows, lens)), RECHOOSE + "a token at frame enc_len - 1"
    if cfg.max_symbols > 1 and family == "nemo":
        assert any(len(set(r[1])) < len(r[1]) for r in rows), RECHOOSE + "a frame carrying two tokens"
    lp, t1, n = check(am, sd, f, lens, rows)                 # u_cap = the largest count: that row reaches u_cap
    assert n.max() == lp.shape[1] and n.sum() > 20
    for b, r in enumerate(rows):
        assert t1[b, :n[b]].tolist() == r[0], (family, b)    # a greedy token is its row's argmax


def device_beam_rows(family, am, cfg, f, lens):
    """the family's beam search through the C ABI -> ([(ids, frames or steps)], frames are steps)"""
    B, Tp, _ = f.shape
    dev, stream = am.device, torch.cuda.current_stream().cuda_stream
    z = lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)       # noqa: E731
    scores, n_ids, el = torch.zeros((B,), device=dev), z(B), dev_i32(am, lens)
    if family == "nemo":
        cap = Tp + int(1.0 * Tp)
        ids, fr = z(B, cap), z(B, cap)
        ws = torch.empty((am.ctx.alsd_workspace_bytes(B, 4, Tp, 1.0),), dtype=torch.uint8, device=dev)
        am.ctx.rnnt_alsd(f, el, B, Tp, 4, 1.0, True, False, ids, fr, n_ids, scores, ws, stream)
    elif family == "espnet":
        cap = 2 * Tp + 16
        ids, fr, pops = z(B, cap), z(B, cap), z(B)
        ws = torch.empty((am.ctx.beam_workspace_bytes(B, 4, Tp, 0),), dtype=torch.uint8, device=dev)
        am.ctx.rnnt_beam(f, el, B, Tp, 4, True, 0, ids, n_ids, scores, pops, ws, stream, frames=fr)
    else:
        cap = Tp
        ids, fr = z(B, cap), z(B, cap)
        ws = torch.empty((am.ctx.mbs_workspace_bytes(B, 4, Tp, cap),), dtype=torch.uint8, device=dev)
        am.ctx.rnnt_mbs(f, el, B, Tp, 4, 0.0, True, ids, fr, n_ids, scores, ws, stream)
    torch.cuda.synchronize()
    n, ids, fr = n_ids.cpu().numpy(), ids.cpu().numpy(), fr.cpu().numpy()
    return [(ids[b, :n[b]].tolist(), fr[b, :n[b]].tolist()) for b in range(B)], family == "nemo"


@pytest.mark.parametrize("family", FAMILIES)
def test_beam_results_device_equals_checker(gpu_device, family):
    am, sd, cfg, f, lens, greedy = scene(family)
    if family == "espnet":          # the recipe of tests/test_gpu_espnet_beam.py, on which the default search stays within its pops bound
        am, sd, cfg, _ = build(family, espnet_blank_bias=12.0)
        waves = ragged_waves(7, 3.0, 21)
        buf = am.stage(waves, buf=am.new_buffers(len(waves), max(len(w) for w in waves)))
        am.run_device(buf)
        torch.cuda.synchronize()
        f, lens = buf.joint_enc.clone(), [int(t) for t in buf.enc_lens.cpu()]
        lens[3] = 0
        greedy = None
    rows, steps = device_beam_rows(family, am, cfg, f, lens)
    assert sum(len(r[0]) for r in rows) > 10
    lp, t1, n = check(am, sd, f, lens, rows, steps=steps)
    differ = sum(int(t1[b, u] != r[0][u]) for b, r in enumerate(rows) for u in range(n[b]))
    print(f"{family}: beam tokens {n.tolist()}, {differ} tokens are not their row's argmax; same as greedy: {rows == greedy}")


@pytest.mark.parametrize("shape", ["nemo-3001", "k2-10720", "espnet-120m-decoder", "k2-toy-97"])
def test_real_output_widths(gpu_device, shape):
    if shape == "nemo-3001":
        am, sd, cfg, _ = build("nemo", WIDE2)
        assert (cfg.n_logits, cfg.joint_hidden, cfg.pred_layers) == (3001, 640, 2)
    elif shape == "k2-10720":
        am, sd, cfg, _ = build("k2", ZIPFORMER_TINY.with_(vocab_size=10720, decoder_dim=512, joiner_dim=512).validate())
    elif shape == "espnet-120m-decoder":
        am, sd, cfg, _ = build("espnet", ESPNET_TINY.with_(vocab_size=2600, pred_hidden=512, joint_hidden=640).validate())
    else:
        am, sd, cfg, _ = scene("k2")[:4]
        assert cfg.vocab_size == 97
    J = cfg.joiner_dim if R.is_k2(cfg) else cfg.joint_hidden
    V = cfg.vocab_size if R.is_k2(cfg) else cfg.n_logits
    g = torch.Generator().manual_seed(2)
    B, Tp = 5, 30
    f = (torch.randn((B, Tp, J), generator=g) * (0.8 + 0.4 * torch.rand((B, 1, 1), generator=g))).to(am.device).contiguous()
    lens = [Tp, 17, 0, 30, 9]
    rows = device_greedy(am, f, lens)
    print(f"{shape}: V = {V}, tokens {[len(r[0]) for r in rows]}")
    assert sum(len(r[0]) for r in rows) > 20, RECHOOSE + "tokens"
    lp, t1, n = check(am, sd, f, lens, rows)
    for b, r in enumerate(rows):
        assert t1[b, :n[b]].tolist() == r[0]
    if shape in ("nemo-3001", "k2-10720"):
        assert V % 64 != 0
        check(am, sd, f, lens, rows, workspace="minimum")


@pytest.mark.parametrize("family", FAMILIES)
def test_chunking_gives_the_same_bits(gpu_device, family):
    am, sd, cfg, f, lens, rows = scene(family)
    counts = [len(r[0]) for r in rows]
    total, starts = sum(counts), np.cumsum([0] + counts)
    # the minimum workspace scores 32 rows per chunk (include/rs_asr.h): chunk boundaries are the multiples of 32 below `total`
    assert total > 32, RECHOOSE + "more than 32 tokens (two chunks at the minimum workspace)"
    inside = [w for w in range(32, total, 32) if w not in set(starts.tolist())]
    assert inside, RECHOOSE + "a chunk boundary inside an utterance"
    J = cfg.joiner_dim if R.is_k2(cfg) else cfg.joint_hidden
    V = cfg.vocab_size if R.is_k2(cfg) else cfg.n_logits
    # ... and every further 32 rows cost less than 32 x 4 x (3 J + 64 ceil(V / 64) + 2 H + 64) bytes: the generous one holds them all
    assert (64 << 20) > (total + 31) // 32 * 32 * 4 * (3 * J + (V + 63) // 64 * 64 + 2 * (cfg.decoder_dim if R.is_k2(cfg) else cfg.pred_hidden) + 64), "generous = one chunk"
    a = check(am, sd, f, lens, rows, workspace="minimum")
    b = check(am, sd, f, lens, rows, workspace="generous")
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


@pytest.mark.parametrize("family", FAMILIES)
def test_alone_equals_inside_the_ragged_batch(gpu_device, family):
    am, sd, cfg, f, lens, rows = scene(family)
    together = check(am, sd, f, lens, rows)
    rich = sorted(range(len(rows)), key=lambda b: -len(rows[b][0]))[:2]
    for b in rich:
        assert rows[b][0]
        alone = check(am, sd, f[b:b + 1, :lens[b]].contiguous(), lens[b:b + 1], rows[b:b + 1])
        k = len(rows[b][0])
        assert alone[0][0, :k].tobytes() == together[0][b, :k].tobytes() and alone[1][0, :k].tolist() == together[1][b, :k].tolist()


def test_bad_entries_are_refused_without_touching_anything_else(gpu_device):
    am, sd, cfg, f, lens, rows = scene("nemo")
    u_cap = max(len(r[0]) for r in rows)
    ids, n = R.pack([r[0] for r in rows], u_cap)
    frames, _ = R.pack([r[1] for r in rows], u_cap)
    good = device_scores(am, f, lens, ids, frames, n)
    rich = sorted(range(len(rows)), key=lambda b: -len(rows[b][0]))[:3]
    bad_i, bad_f = ids.copy(), frames.copy()
    bad_f[rich[0], 1] = lens[rich[0]]                       # a frame at enc_len
    bad_f[rich[1], 0] = -1                                  # a negative frame
    bad_i[rich[2], 2] = cfg.n_logits                        # an id outside the vocabulary
    lp, t1 = device_scores(am, f, lens, bad_i, bad_f, n, want_code=capi.RS_EINVAL)
    bad = np.zeros_like(ids, bool)
    bad[rich[0], 1] = bad[rich[1], 0] = bad[rich[2], 2] = True
    want_lp, want_t1 = R.scores_checker(cfg, sd, f.cpu().numpy(), np.asarray(lens, np.int32), bad_i, bad_f, n, want_rc=-1)
    valid = np.arange(u_cap)[None, :] < n[:, None]
    assert np.isnan(lp[bad]).all() and (t1[bad] == -1).all()
    ok = valid & ~bad
    assert (lp.view(np.int32)[ok] == want_lp.view(np.int32)[ok]).all() and (t1[ok] == want_t1[ok]).all()
    others = [b for b in range(len(rows)) if b not in rich]
    assert lp[others].tobytes() == good[0][others].tobytes()
    n_bad = n.copy()
    n_bad[rich[0]] = u_cap + 1                              # a count beyond the row
    device_scores(am, f, lens, ids, frames, n_bad, want_code=capi.RS_EINVAL)


def test_argument_errors_come_before_any_launch(gpu_device):
    am, sd, cfg, f, lens, rows = scene("nemo")
    B, Tp, _ = f.shape
    dev = am.device
    z = lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)       # noqa: E731
    logp = torch.full((B, 8), 7.0, device=dev)
    least = am.ctx.token_scores_workspace_bytes(B, 8)
    ws = torch.empty((least,), dtype=torch.uint8, device=dev)
    args = lambda ctx, **kw: ctx.rnnt_token_scores(f, dev_i32(am, lens), B, Tp, z(B, 8), z(B, 8), z(B), logp, None, ws, 0, **kw)   # noqa: E731
    with pytest.raises(capi.RsError, match="workspace") as e:
        args(am.ctx, ws_bytes=least - 1)
    assert e.value.code == capi.RS_EINVAL
    for other in (capi.Context(AVSR_TINY, 0), capi.Context(TINY, 0)):   # an AV-HuBERT context; a context that was never finalized
        with pytest.raises(RuntimeError):
            other.token_scores_workspace_bytes(B, 8)
        with pytest.raises(capi.RsError) as e:
            args(other)
        assert e.value.code == capi.RS_EINVAL
        other.close()
    assert am.ctx.lib.rs_rnnt_token_scores(am.ctx._h, None, None, -1, Tp, None, None, None, 8, 0, None, None, None, 0, None) == capi.RS_EINVAL
    args(am.ctx)                                            # n_ids all zero: nothing to score, nothing written
    torch.cuda.synchronize()
    assert (logp == 7.0).all()


# ---- the public surface -------------------------------------------------------------------------------------------------------
def public(family):
    am, sd, cfg, model = build(family, token_scores=True)
    waves = ragged_waves(9, 2.0, 50)
    if family == "nemo":
        return am, model, ntr, ni, [ni.AudioData(w, 16000) for w in waves], waves
    if family == "espnet":
        return am, model, etr, ei, [ei.AudioData(w, 16000) for w in waves], waves
    return am, model, ktr, ki, [ki.AudioData(w, 16000) for w in waves], waves


@pytest.mark.parametrize("family", FAMILIES)
def test_public_path(gpu_device, family):
    am, model, tr, iface, audios, waves = public(family)
    cfg = iface.TranscribeConfig(verbose=False)
    assert model.token_scores is True
    res = tr.transcribe_batch(model, audios[:4], cfg)
    assert all(isinstance(r, iface.ScoredTranscribeResult) for r in res)
    for r in res:
        assert len(r.token_logprobs) == len(r.token_ids) and all(v <= 1e-6 for v in r.token_logprobs)
        assert (r.confidence is None) == (not r.token_ids) and (r.confidence is None or 0.0 < r.confidence <= 1.0 + 1e-6)
    assert sum(len(r.token_ids) for r in res) > 5
    one = tr.transcribe(model, audios[1], cfg)
    assert isinstance(one, iface.ScoredTranscribeResult)
    assert (one.text, one.token_ids, one.token_logprobs, one.confidence) == (res[1].text, res[1].token_ids, res[1].token_logprobs, res[1].confidence)
    if family == "nemo":
        assert all(len(r.subword_logprobs) == len(r.subwords) and len(r.segment_confidence) == len(r.segments) for r in res)
        raw = tr.transcribe_batch(model, audios[:2], iface.TranscribeConfig(verbose=False, raw_hypothesis=True))
        assert raw[1].hypothesis.token_confidence == [float(np.exp(v)) for v in raw[1].token_logprobs]
    if family == "k2":
        assert all(r.subword_logprobs == r.token_logprobs and len(r.subwords) == len(r.token_ids) for r in res)
    # 9 utterances at max_batch = 4 (the host pipeline, narrowed buffer views, two decode lanes) == one batch
    whole, parts = am.transcribe_waveforms(waves), am.transcribe_waveforms(waves, max_batch=4)
    assert whole.token_logprobs is not None and [len(x) for x in whole.token_logprobs] == [len(x) for x in whole.ids]
    assert (whole.ids, whole.frames, whole.token_logprobs) == (parts.ids, parts.frames, parts.token_logprobs)
    # scores off: the same ids, frames and text, and the plain types
    model.token_scores = False
    off, off_parts = am.transcribe_waveforms(waves), am.transcribe_waveforms(waves, max_batch=4)
    assert off.token_logprobs is None and off_parts.token_logprobs is None
    assert (off.ids, off.frames) == (whole.ids, whole.frames) == (off_parts.ids, off_parts.frames)
    plain = tr.transcribe_batch(model, audios[:4], cfg)
    assert all(type(r) is iface.TranscribeResult for r in plain) and type(tr.transcribe(model, audios[1], cfg)) is iface.TranscribeResult
    assert [r.text for r in plain] == [r.text for r in res]
    if family != "espnet":
        assert [r.subwords for r in plain] == [r.subwords for r in res]
    if family == "nemo":
        assert [r.segments for r in plain] == [r.segments for r in res]
    with pytest.raises(ValueError, match="token_scores"):
        model.token_scores = True
        am.transcribe_waveforms_sharded(waves)


def test_public_path_with_the_beam_searches(gpu_device):
    """the option with every decoding: nemo ALSD (alignment steps converted on the device), the k2 modified beam search"""
    from reazonspeech_amd.nemo.asr import load_model
    audio, alens = synthetic_batch(5, 2.0, seed=13)
    waves = [audio[b, :alens[b] - 1500 * b] for b in range(5)]
    model = load_model(device="cuda:0", config=TINY, decoding="alsd", beam_size=3, token_scores=True)
    res = ntr.transcribe_batch(model, [ni.AudioData(w, 16000) for w in waves], ni.TranscribeConfig(verbose=False, raw_hypothesis=True))
    buf = model.stage([np.ascontiguousarray(w, dtype=np.float32) for w in waves])
    model.run_device(buf)
    dec = model.collect(buf)
    sd = synthetic_state_dict(TINY, 0)
    u_cap = max(max(len(x) for x in dec.ids), 1)
    ids, n = R.pack(dec.ids, u_cap)
    frames, _ = R.pack(dec.frames, u_cap)               # `collect` returns frames, not steps
    want, _ = R.scores_checker(TINY, sd, buf.joint_enc.cpu().numpy(), np.asarray(dec.enc_lens, np.int32), ids, frames, n)
    for b, r in enumerate(res):
        assert r.token_ids == dec.ids[b] and r.hypothesis.score is not None
        assert np.asarray(r.token_logprobs, np.float32).tobytes() == want[b, :n[b]].tobytes() == np.asarray(dec.token_logprobs[b], np.float32).tobytes()
    assert n.sum() > 5
    am, sd, cfg, k2 = build("k2", decoding_method="modified_beam_search", max_active_paths=4, blank_penalty=1.0, token_scores=True)
    out = ktr.transcribe_batch(k2, [ki.AudioData(w, 16000) for w in waves], ki.TranscribeConfig(verbose=False))
    assert all(isinstance(r, ki.ScoredTranscribeResult) and len(r.token_logprobs) == len(r.subwords) for r in out)
    assert sum(len(r.token_ids) for r in out) > 5 and all(v <= 1e-6 for r in out for v in r.token_logprobs)
