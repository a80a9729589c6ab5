"""-m gpu: CTC segmentation on the device (rs_ctc_align, csrc/k_ctc_align.hip) and `segmentation="device"` of the espnet family.

The reference of every kernel case is this package's host aligner (`ctc_segmentation.ctc_segmentation`) on the SAME float32
posteriors, and the comparison has no tolerance: the forward table is float32 adds and maxima in the host's order and the
backtracking compares in double, so `frames * index_duration` must equal the host's `timings` to the last bit, and a row is
refused (status 1) exactly where the host raises its "Audio is shorter than text!" assertion.  End to end, `transcribe_batch` /
`transcribe` / `find_blank` with `model.segmentation = "device"` must return what `"host"` returns, field for field."""
import importlib

import numpy as np
import pytest
import torch

from reazonspeech_amd.runtime import capi
from reazonspeech_amd.runtime.config import ESPNET_TINY
from reazonspeech_amd.runtime.synth import synthetic_batch
from reazonspeech_amd.runtime.weights_espnet import synthetic_state_dict_espnet
from reazonspeech_amd.espnet.asr.model import EspnetModel, synthetic_token_list
from reazonspeech_amd.espnet.asr import ctc as ectc, ctc_segmentation as cs, interface

etr = importlib.import_module("reazonspeech_amd.espnet.asr.transcribe")
pytestmark = pytest.mark.gpu

ABC = ["<blank>", "a", "b", "ab", "c", "abc"]
BLOCK = 256                                    # threads of an align workgroup (csrc/k_ctc_align.hip: ALIGN_THREADS)


@pytest.fixture(scope="module")
def tiny(gpu_device):
    sd = synthetic_state_dict_espnet(ESPNET_TINY, 3)
    return EspnetModel(ESPNET_TINY, sd, synthetic_token_list(ESPNET_TINY.vocab_size, 3), device="cuda:0")


@pytest.fixture(scope="module")
def ctx(tiny):
    return tiny.am.ctx                         # the aligner reads no weights: any context serves


def posteriors(rng, T, V, sharp=3.0):
    z = rng.standard_normal((T, V)) * sharp
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return (e / e.sum(axis=1, keepdims=True)).astype(np.float32)


def host_align(post, gt, index_duration, char_list):
    """-> ("ok", timings) | ("short", None) | (exception name, None)"""
    params = cs.CtcSegmentationParameters(index_duration=index_duration, char_list=char_list)
    try:
        return "ok", cs.ctc_segmentation(params, post, gt)[0]
    except AssertionError:
        return "short", None
    except Exception as e:                     # noqa: BLE001 — the kind is what the caller checks
        return type(e).__name__, None


def device_align(ctx, posts, gt, gt_lens, pad=4, extra_rows=3):
    """posts: [float32 [T][V]] -> (frames int32 [B][c_max], status int32 [B]).  The posteriors sit in a buffer of pitch
    V + pad and tp_max = longest + extra_rows rows per utterance whose unused cells hold NaN: reading one would show."""
    B, V = len(posts), posts[0].shape[1]
    tp_max = max(p.shape[0] for p in posts) + extra_rows
    ld = V + pad
    host = np.full((B, tp_max, ld), np.nan, np.float32)
    for b, p in enumerate(posts):
        host[b, :p.shape[0], :V] = p
    probs = torch.from_numpy(host.reshape(B * tp_max, ld)).cuda()
    enc_lens = torch.tensor([p.shape[0] for p in posts], dtype=torch.int32, device="cuda")
    d_gt, d_len = torch.from_numpy(gt).cuda(), torch.from_numpy(gt_lens).cuda()
    frames = torch.full((B, gt.shape[1]), -7, dtype=torch.int32, device="cuda")
    status = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    ws = torch.empty((ctx.ctc_align_workspace_bytes(B, tp_max, gt.shape[1], gt.shape[2]),), dtype=torch.uint8, device="cuda")
    ctx.ctc_align(probs, enc_lens, B, tp_max, d_gt, d_len, 0, frames, status, ws, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return frames.cpu().numpy(), status.cpu().numpy()


def check_batch(ctx, char_list, texts, Ts, rng, V=None):
    """aligns the batch on the device and every row on the host; -> the host outcomes"""
    V = V or len(char_list)
    params = cs.CtcSegmentationParameters(char_list=char_list)
    gt, gt_lens, _ = cs.pack_ground_truth(params, texts)
    posts = [posteriors(rng, T, V) for T in Ts]
    frames, status = device_align(ctx, posts, gt, gt_lens)
    outcomes = []
    for b, post in enumerate(posts):
        dur = 16000.0 * (b + 3) / (post.shape[0] + 1)                       # an index duration that is no round number
        kind, timings = host_align(post, gt[b, :gt_lens[b]].astype(np.int64), dur, char_list)
        outcomes.append((kind, timings))
        assert kind in ("ok", "short"), (b, kind)
        assert (status[b] == 0) == (kind == "ok") and (status[b] == 1) == (kind == "short"), (b, kind, status[b])
        if kind == "ok":
            got = frames[b, :gt_lens[b]].astype(np.float64) * dur
            assert np.array_equal(got, timings), (b, Ts[b], int(gt_lens[b]), np.flatnonzero(got != timings)[:8])
        assert np.all(frames[b, gt_lens[b]:] == 0)
    return outcomes


def random_text(rng, body, n):
    return "".join(rng.choice(body, size=n)) if n else ""


@pytest.fixture(scope="module")
def tokens96():
    toks = synthetic_token_list(96, 3)[:-1]
    return toks, [t for t in toks if len(t) == 1 and t not in cs.CtcSegmentationParameters.excluded_characters]


def test_ragged_batch_matches_the_host_aligner(ctx, tokens96):
    toks, body = tokens96
    rng = np.random.default_rng(101)
    n_chars = [45, 0, 17, 62, 30, 5]
    Ts = [48, 9, 90, 70, 29, 41]                     # 45 + 3 symbols in 48 frames: exactly C == T; 30 + 3 in 29: too short
    out = check_batch(ctx, toks, [random_text(rng, body, n) for n in n_chars], Ts, rng, V=96)
    assert [k for k, _ in out] == ["ok", "ok", "ok", "ok", "short", "ok"]
    assert sum(int(np.count_nonzero(t)) for _, t in out if t is not None) >= 100


def test_multi_character_tokens_match_the_host_aligner(ctx):
    rng = np.random.default_rng(202)
    texts = [random_text(rng, list("abc"), int(rng.integers(1, 16))) for _ in range(40)]
    Ts = [len(t) + 3 + int(rng.integers(0, 30)) for t in texts]
    out = check_batch(ctx, ABC, texts, Ts, rng)
    multi = 0
    for kind, timings in out:
        assert kind == "ok"
        body = timings[2:-1]                                                 # the text's own symbols
        multi += bool(np.any((body[1:] == body[:-1]) & (body[1:] > 0)))      # two symbols switched at one frame: a longer token
    assert multi >= 1, "no case took a multi-character switch: the comparison would not cover s > 0"


@pytest.mark.parametrize("C", [2, 3, 63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 1, 4 * BLOCK + 1])
def test_symbol_counts_at_the_block_boundaries(ctx, tokens96, C):
    """C below, at and above the workgroup size and its multiples — 1, 2 and 4 symbols per thread in registers, and the
    strided form above 4 x 256 — each with T = C, T = C + 5 and T = C - 1 (refused), and the two-frame input"""
    toks, body = tokens96
    rng = np.random.default_rng(300 + C)
    n = C - 3 if C > 2 else 0
    texts = [random_text(rng, body, n)] * 3 + [""]
    if C == 3:                                                               # "#·" + one character + "·" is 4 symbols: build C == 3 by hand
        gt = np.full((4, 3, 7), -1, np.int32)
        gt[:, 1, 0], gt[:, 2, 0] = 0, toks.index(body[0])
        gt_lens = np.asarray([3, 3, 3, 2], np.int32)
        gt[3, 2] = -1
    else:
        gt, gt_lens, _ = cs.pack_ground_truth(cs.CtcSegmentationParameters(char_list=toks), texts)
        assert gt_lens.tolist() == [C, C, C, 2]
    Ts = [C, C + 5, C - 1, 2]
    posts = [posteriors(rng, T, 96) for T in Ts]
    frames, status = device_align(ctx, posts, gt, gt_lens)
    for b, post in enumerate(posts):
        dur = 160000.0 / (post.shape[0] + 1)
        kind, timings = host_align(post, gt[b, :gt_lens[b]].astype(np.int64), dur, toks)
        assert kind == ("short" if b == 2 else "ok")
        assert status[b] == (1 if b == 2 else 0), (C, b, status[b])
        if kind == "ok":
            assert np.array_equal(frames[b, :gt_lens[b]].astype(np.float64) * dur, timings), (C, b)
        assert np.all(frames[b, gt_lens[b]:] == 0)


def test_full_vocabulary_row(ctx):
    """one window of the 120M model's size: V = 2600, T = 311 (10 s), C = 153, S = 7"""
    toks = synthetic_token_list(2600, 0)[:-1]
    body = [t for t in toks if len(t) == 1 and t not in cs.CtcSegmentationParameters.excluded_characters]
    rng = np.random.default_rng(404)
    out = check_batch(ctx, toks, [random_text(rng, body, 150)], [311], rng, V=2600)
    assert out[0][0] == "ok" and np.count_nonzero(out[0][1]) >= 150


def test_row_between_an_empty_and_a_full_neighbour(ctx, tokens96):
    """rows of very different cost side by side: the middle row's neighbours have 2 symbols and c_max symbols"""
    toks, body = tokens96
    rng = np.random.default_rng(505)
    texts = [random_text(rng, body, n) for n in (10, 0, 40, 117, 3)]
    out = check_batch(ctx, toks, texts, [60, 60, 75, 130, 12], rng, V=96)
    assert all(k == "ok" for k, _ in out)


def test_seeded_small_inputs_raise_only_the_short_audio_assertion(tokens96):
    """the host aligner's other exit (IndexError: backtracking reached frame 0 early, status 2) does not occur on random input:
    the device's guard for it is by inspection, not by a provoked case"""
    rng = np.random.default_rng(606)
    kinds = set()
    for _ in range(60):
        n, T = int(rng.integers(0, 9)), int(rng.integers(2, 16))
        gt, gt_lens, _ = cs.pack_ground_truth(cs.CtcSegmentationParameters(char_list=ABC), [random_text(rng, list("abc"), n)])
        kinds.add(host_align(posteriors(rng, T, 6), gt[0].astype(np.int64), 1.0, ABC)[0])
    assert kinds == {"ok", "short"}


def test_bad_arguments_are_refused_before_anything_runs(ctx):
    B, tp_max, c_max = 2, 8, 5
    probs = torch.rand((B * tp_max, 8), device="cuda")
    enc_lens = torch.full((B,), 8, dtype=torch.int32, device="cuda")
    gt_lens = torch.full((B,), c_max, dtype=torch.int32, device="cuda")
    frames = torch.full((B, c_max), -7, dtype=torch.int32, device="cuda")
    status = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    ws = torch.empty((ctx.ctc_align_workspace_bytes(B, tp_max, c_max, 2),), dtype=torch.uint8, device="cuda")
    gt9 = torch.full((B, c_max, 9), -1, dtype=torch.int32, device="cuda")
    gt2 = torch.full((B, c_max, 2), -1, dtype=torch.int32, device="cuda")
    gt2[:, 1:, 0] = torch.arange(1, c_max, dtype=torch.int32, device="cuda")          # symbol c is token c
    with pytest.raises(capi.RsError):
        ctx.ctc_align(probs, enc_lens, B, tp_max, gt9, gt_lens, 0, frames, status, ws, stream)                       # S = 9
    with pytest.raises(capi.RsError):
        ctx.ctc_align(probs, enc_lens, B, tp_max, gt2, gt_lens, 0, frames, status, ws, stream, S=0)
    with pytest.raises(capi.RsError):
        ctx.ctc_align(probs, enc_lens, B, tp_max, gt2, gt_lens, 0, frames, status, ws, stream, ws_bytes=ws.numel() - 1)
    with pytest.raises(capi.RsError):
        ctx.ctc_align(probs, enc_lens, B, tp_max, gt2[:, :1], gt_lens, 0, frames[:, :1], status, ws, stream)         # c_max = 1
    with pytest.raises(capi.RsError):
        ctx.ctc_align_workspace_bytes(B, tp_max, c_max, 9)
    torch.cuda.synchronize()
    assert torch.all(frames == -7) and torch.all(status == -7)
    ctx.ctc_align(probs, enc_lens, B, tp_max, gt2, gt_lens, 0, frames, status, ws, stream)                           # and the good call runs
    torch.cuda.synchronize()
    assert torch.all(status == 0)


def test_ground_truth_without_tokens_is_the_hosts_index_error(ctx):
    """a ground truth no token matches cannot leave symbol C - 1: the host's backtracking starts at frame 0 and raises
    IndexError, the device reports status 2 (nothing is provoked on the device: the walk ends at its first step)"""
    rng = np.random.default_rng(707)
    gt = np.full((2, 5, 2), -1, np.int32)
    gt[1, 1:, 0] = np.arange(1, 5)
    posts = [posteriors(rng, 9, 8), posteriors(rng, 9, 8)]
    frames, status = device_align(ctx, posts, gt, np.asarray([5, 5], np.int32))
    kinds = [host_align(p, gt[b].astype(np.int64), 1.0, [str(i) for i in range(8)])[0] for b, p in enumerate(posts)]
    assert kinds == ["IndexError", "ok"] and status.tolist() == [2, 0]


# ---- end to end: segmentation = "device" against "host" on the same model ------------------------------------------

@pytest.fixture(scope="module")
def six(tiny):
    audio, lens = synthetic_batch(6, 3.0, seed=9, ragged=True, min_seconds=0.5)
    waves = [audio[b, :int(lens[b])] for b in range(6)]
    tiny.segmentation = "host"
    host = etr.transcribe_batch(tiny, [interface.AudioData(w, 16000) for w in waves])
    return waves, host


def test_transcribe_batch_device_equals_host(tiny, six):
    waves, host = six
    aligned = chars = 0
    for w, r in zip(waves, host):                    # the comparison is not vacuous: the host path aligns, it does not fall back
        try:
            t = ectc.get_timings(tiny, w, r.text)
            aligned, chars = aligned + 1, chars + len(t)
        except Exception:                            # noqa: BLE001 — what split_text catches
            pass
    assert aligned >= 4 and chars >= 100, (aligned, chars)
    tiny.segmentation = "device"
    try:
        dev = etr.transcribe_batch(tiny, [interface.AudioData(w, 16000) for w in waves])
    finally:
        tiny.segmentation = "host"
    assert len(dev) == len(host) == 6
    for d, h in zip(dev, host):
        assert d.text == h.text
        assert [(s.start_seconds, s.end_seconds, s.text) for s in d.segments] == [(s.start_seconds, s.end_seconds, s.text) for s in h.segments]
    assert dev == host
    assert sum(len(r.segments) for r in host) > 6    # more than the one whole-window segment of a fallback


def test_long_recording_device_equals_host(tiny):
    wav = synthetic_batch(1, 47.0, seed=77)[0][0]
    audio = interface.AudioData(wav, 16000)
    quiet = interface.TranscribeConfig(verbose=False)
    tiny.segmentation = "host"
    host = etr.transcribe(tiny, audio, quiet)
    cut_host = ectc.find_blank(tiny, wav[:20 * 16000])
    tiny.segmentation = "device"
    try:
        dev = etr.transcribe(tiny, audio, quiet)
        cut_dev = ectc.find_blank(tiny, wav[:20 * 16000])
        col = tiny.blank_posteriors(wav[:20 * 16000])
    finally:
        tiny.segmentation = "host"
    assert cut_dev == cut_host
    assert np.array_equal(col, tiny.ctc_posteriors(wav[:20 * 16000])[:, tiny.asr_model.blank_id])
    assert dev == host and len(host.segments) >= 3   # three windows at least: the cuts are part of the result


def test_align_batch_chunks_equal_one_batch(tiny, six):
    waves, host = six
    texts = [r.text for r in host]
    one = tiny.align_batch(waves, texts)
    chunked = tiny.align_batch(waves, texts, max_batch=4)
    assert len(one) == len(chunked) == 6
    for b, (a, c) in enumerate(zip(one, chunked)):
        assert (a is None) == (c is None)
        if a is not None:
            assert a.dtype == np.float64 and np.array_equal(a, c)
            assert np.array_equal(a, ectc.get_timings(tiny, waves[b], texts[b]))


def test_segmentation_attribute_is_checked(tiny):
    with pytest.raises(ValueError):
        tiny.segmentation = "bogus"
    assert tiny.segmentation == "host"
