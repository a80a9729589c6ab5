"""`load_model()` / `transcribe()` of `reazonspeech.espnet.asr` (pkg/espnet-asr/src/transcribe.py:12-82).

The control flow is the reference's: audio longer than WINDOW_SECONDS is cut at the midpoint of the longest non-speech
stretch the CTC head finds in the next 20 s (:59-67), each piece is recognised with (16000, 8000) samples of zero padding
(:69) and split into time-stamped segments by CTC segmentation (:72-77).  Underneath, `Speech2Text` is replaced by
`EspnetModel` (model.py): HIP front-end, Conv2dSubsampling, conformer blocks, CTC head and transducer greedy search."""
import sys

import numpy as np
import torch

from ...runtime import fusion
from ...runtime.resample import norm_batch
from .audio import norm_audio, SAMPLERATE
from .interface import AudioData, TranscribeConfig, TranscribeResult, Segment, make_result
from .ctc import split_text, find_blank, segments_from_timings

# Hyper parameters (transcribe.py:9-10)
WINDOW_SECONDS = 20
PADDING = (16000, 8000)


CHECKPOINT_ENV = "REAZONSPEECH_ESPNET_CHECKPOINT"


def load_model(device=None, checkpoint=None, config=None, seed=0, beam_size=None, max_pops=0, precision="bf16", synthetic=False,
               segmentation="host", resample="host", token_scores=False, nbest=None, ngram_lm_model=None, ngram_lm_alpha=0.0,
               ngram_lm_tokens="pieces", hotwords_file="", hotwords_score=1.5, rescore=None):
    """Load the ReazonSpeech ESPnet model onto a ROCm GPU (transcribe.py:12-32).

    Args:
      device (str): "cuda" / "cuda:N"; None picks "cuda" when available like the reference (:20-24).  There is no CPU path
        in this package: "cpu" raises.
      checkpoint (str): an ESPnet2 model directory or model-zoo `.zip` (training `config.yaml`, `*.pth`, `feats_stats.npz`);
        defaults to $REAZONSPEECH_ESPNET_CHECKPOINT.  Read without ESPnet (runtime/weights_espnet.py: read_espnet), strictly.
      config (ModelConfig): architecture (family "espnet") for synthetic weights; default: the 120M Conformer-Transducer shape.
      seed (int): seed of the synthetic weights.
      beam_size (int): transducer search width, as Speech2Text's `beam_size`: <= 1 greedy search, larger the default beam
        search.  None = 20 for a checkpoint (Speech2Text's default, which the reference keeps: :27-31) and 1 for synthetic
        weights (an untrained joint can make the default search extend one frame without end; see `max_pops`).
      max_pops (int): prediction-network evaluations the beam search may spend per frame (0 = 16 * beam_size); upstream has
        no bound.  A window that exceeds it is retried with four and sixteen times the bound, then decoded greedily with a
        warning (model.py: EspnetModel._search) — never truncated, and the windows already decoded are kept.
      precision (str): "bf16" = the throughput mode; "fp32" = the float32 parity mode (float32 weights, activations and
        arithmetic end to end — what ESPnet computes on the reference's path; include/rs_asr.h "precision_f32").
      segmentation (str): where the time stamps of the segments are computed.  "host" (default) = like the reference, one more
        encoder pass and one run of the CTC aligner in numpy per window; "device" = one batched encoder pass and one
        rs_ctc_align launch for all windows of a `transcribe_batch` call (`EspnetModel.align_batch`), and the blank finder
        copies back the blank column only; `transcribe_batch` then takes recordings of any length and finds their cut points
        on the device too (rs_ctc_find_blank).  The results are the same; stored as `model.segmentation`, may be changed later.
      resample (str): where input at another rate than 16 kHz, or with several channels, is normalised (`norm_audio`): "host"
        (default) = scipy / soxr per utterance as before; "device" = one HIP launch per (rate, channel count) group of a call
        (`AsrModel.resample_batch`, rs_resample; the host path's Kaiser filter).  Stored as `model.resample`.

      token_scores (bool): every result is a `ScoredTranscribeResult` (interface.py): token ids, the log-probability of each under
        the model's own distribution (computed on the device right after the search, rs_rnnt_token_scores) and
        confidence = exp(mean); the pieces of a long recording are concatenated in order.  Valid with every `precision` and
        `beam_size`.  Off (default): today's objects.  Stored as `model.token_scores`, may be changed later.

      nbest (int): upstream's `Speech2Text(nbest=N)`, 1..8 and at most `beam_size`: `model(speech)` returns the N best hypotheses of
        the default beam search as N tuples (text, tokens, ids, hyp) with `hyp.score` set — upstream's `sort_nbest(kept_hyps)[:nbest]`,
        ranked on the device (include/rs_asr.h rs_rnnt_beam_nbest) — and `model.recognize_batch(..., nbest=N)` the same per window.
        `transcribe` / `transcribe_batch` keep returning the best hypothesis.  None (default): one tuple, as ever.  A window that the
        greedy fall-back decodes (see `max_pops`), and every window of a greedy model asked for nbest = 1, returns a list of ONE
        whose `hyp.score` and `hyp.norm_score` are NaN — the greedy search keeps no score; test with `math.isnan` before sorting.  N above the
        beam, or N > 1 with the greedy search, raises ValueError.

      rescore (str): None (default), "likelihood" or "norm_likelihood", with `nbest >= 2`: every entry of the list is scored by
        log P(text | audio) over ALL alignments, on the device right after the search (include/rs_asr.h rs_rnnt_align_rows: one
        lattice per window, the entries' common prefixes computed once), and the list is re-ranked by it (or by it divided by
        max(tokens, 1)), descending, ties in the search's order: `hyp.log_likelihood`, `hyp.alignment_log_prob`,
        `hyp.norm_log_likelihood`, `hyp.search_rank` on the tuples of `model(speech)` / `recognize_batch`; `transcribe` and
        `transcribe_batch` (both segmentations; `recognize_batch` without `nbest=` and `recognize_batch_scored` too) follow the
        re-ranked best.  The list of one of a window the greedy fall-back decoded is scored too.  ValueError (before anything is
        loaded) for another value, the greedy search or nbest < 2.  Stored as `model.rescore`, may be set later.
        A batch whose lists are beyond one call's lattice bound is scored over several calls; only lists of more than 2047 labels per entry, or ONE utterance's lists beyond the bound, raise ValueError (window the audio).

      ngram_lm_model (str or NgramLm), ngram_lm_alpha (float), ngram_lm_tokens (str): shallow fusion of a backoff n-gram language
        model trained on the user's own text into the default beam search — [UPSTREAM] the `lm_weight * lm_scores` slot of
        default_beam_search, which the reference closes with lm_weight = 0 (include/rs_asr.h rs_rnnt_beam_lm).  An ARPA text file
        (`.gz` allowed; a KenLM binary is refused) or an `NgramLm`; its weight (0 = off; `model.ngram_lm_alpha` is settable); how a
        word of the file names a token: "pieces" (default) = the symbols of token_list, '<space>' included, "ids" = decimal ids.
        `<s>` is the start state; there is no end-of-sentence term.
      hotwords_file (str), hotwords_score (float): contextual biasing from a phrase list, one phrase per line with an optional
        ` :score` (runtime/k2_hotwords.py); a phrase is encoded per character against token_list (whitespace is '<space>' when the
        list has it, dropped otherwise; a phrase with a character outside the list is skipped with a warning).  `model(speech,
        hotwords=...)`, `recognize_batch`, `transcribe` and `transcribe_batch` take a call's own phrases.
        Both need `beam_size > 1`: with the greedy search they raise ValueError.  A bonus can make a frame take more pops than
        `max_pops` allows: the retry ladder is the one described there, and the greedy fall-back runs without either.

    The reference downloads `reazon-research/reazonspeech-espnet-v2` through espnet_model_zoo (:27-31), which an offline box
    cannot do: give `checkpoint=` / the environment variable.  Without a checkpoint this RAISES; seeded synthetic weights of
    the architecture (timings valid, transcripts meaningless) are loaded only on request — `config=`, `synthetic=True` or
    $REAZONSPEECH_AMD_SYNTHETIC=1 — and a warning says so."""
    from ...runtime.config import ESPNET_CONFORMER_120M
    from ...runtime.weights_espnet import synthetic_state_dict_espnet
    from .model import EspnetModel, synthetic_token_list, SEGMENTATION_MODES, check_nbest, check_fusion_keywords
    beam_known = beam_size if beam_size is not None else (1 if config is not None or synthetic else 20)
    from ...runtime import rescore as rescoring
    rescoring.check(rescore, check_nbest(nbest, beam_known), int(beam_known) > 1)       # argument errors first
    check_fusion_keywords(beam_known, ngram_lm_model, ngram_lm_alpha, ngram_lm_tokens, hotwords_file, hotwords_score)
    fusion = dict(ngram_lm_model=ngram_lm_model, ngram_lm_alpha=ngram_lm_alpha, ngram_lm_tokens=ngram_lm_tokens, hotwords_file=hotwords_file,
                  hotwords_score=hotwords_score)
    from ...runtime.resample import check_mode
    if segmentation not in SEGMENTATION_MODES:
        raise ValueError(f"segmentation must be one of {SEGMENTATION_MODES}, got {segmentation!r}")
    check_mode(resample)
    if device is None:
        device = "cuda" if torch.cuda.is_available() else "cpu"
    if str(device).startswith("cpu"):
        raise RuntimeError("reazonspeech_amd runs on MI355X (gfx950) only; no CPU path exists (use the reference package for CPU inference)")
    import os
    from ...runtime.weights_espnet import read_espnet
    checkpoint = checkpoint or (os.environ.get(CHECKPOINT_ENV) if config is None else None)
    if checkpoint:
        if not os.path.exists(checkpoint):
            raise FileNotFoundError(f"checkpoint {checkpoint!r} does not exist")
        cfg, sd, tokens = read_espnet(checkpoint)
        return EspnetModel(cfg, sd, tokens, device=device, beam_size=20 if beam_size is None else beam_size, max_pops=max_pops,
                           precision=precision, segmentation=segmentation, resample=resample, token_scores=token_scores, nbest=nbest,
                           rescore=rescore, **fusion)
    cfg = config or ESPNET_CONFORMER_120M
    if config is None:
        if not (synthetic or os.environ.get("REAZONSPEECH_AMD_SYNTHETIC", "0") not in ("", "0")):
            raise FileNotFoundError(f"no ESPnet2 checkpoint: give `checkpoint=` or ${CHECKPOINT_ENV} (a model directory / model-zoo .zip of "
                                    "reazon-research/reazonspeech-espnet-v2; the reference downloads it through espnet_model_zoo, :27-31).  Seeded "
                                    "synthetic weights are loaded only on request: config=..., synthetic=True or $REAZONSPEECH_AMD_SYNTHETIC=1.")
        print("[reazonspeech_amd] WARNING: SEEDED SYNTHETIC weights of the 120M Conformer-Transducer architecture were requested "
              "(`synthetic=True` / $REAZONSPEECH_AMD_SYNTHETIC): timings are valid, transcripts are meaningless.", file=sys.stderr, flush=True)
    return EspnetModel(cfg, synthetic_state_dict_espnet(cfg, seed), synthetic_token_list(cfg.vocab_size, seed), device=device,
                       beam_size=1 if beam_size is None else beam_size, max_pops=max_pops, precision=precision,
                       segmentation=segmentation, resample=resample, token_scores=token_scores, nbest=nbest, rescore=rescore, **fusion)


def _windows(model, waveform, window):
    """Cut `waveform` into the pieces the recogniser sees (transcribe.py:59-67,78): everything that is left when it fits one
    window, otherwise the head of the next `window` samples up to the middle of its longest silent stretch (`find_blank`).
    Lazy: the blank finder of a piece runs after the previous piece has been recognised, like the reference's loop.
    -> (offset, samples)"""
    offset = 0
    while offset < len(waveform):
        rest = waveform[offset:]
        if len(rest) > window:
            gap = find_blank(model, rest[:window])
            rest = rest[:int((gap.start + gap.end) / 2)]
        yield offset, rest
        offset += len(rest)


def plan_windows(lengths, window, find_cuts):
    """The pieces `_windows` cuts, for many recordings at once: -> [[(offset, n_samples), ...] per recording].

    Only the chain of cut points is sequential — the cut of a window fixes where the next window of the SAME recording begins
    and nothing else — so the recordings advance in lockstep: a round collects the next window `(recording, offset, window)`
    of every recording that has more than `window` samples left, asks `find_cuts(requests)` ONCE for their `Blank`s (one
    batched pass over as many windows as there are such recordings) and cuts each head at int((start + end) / 2).  A recording
    with at most `window` samples left contributes its rest as its last piece; one of length 0 contributes no piece.  Pure host
    code: what runs the blank finder is the caller's `find_cuts`."""
    pieces = [[] for _ in lengths]
    offsets = [0] * len(lengths)
    live = []
    for i, n in enumerate(lengths):
        if n > window:
            live.append(i)
        elif n > 0:
            pieces[i].append((0, n))
    while live:
        gaps = find_cuts([(i, offsets[i], window) for i in live])
        assert len(gaps) == len(live)
        still = []
        for i, gap in zip(live, gaps):
            head = min(int((gap.start + gap.end) / 2), window)      # `rest[:int((gap.start + gap.end) / 2)]` of `_windows`
            if head <= 0:
                raise RuntimeError(f"recording {i}: the cut at offset {offsets[i]} leaves an empty piece")
            pieces[i].append((offsets[i], head))
            offsets[i] += head
            rest = lengths[i] - offsets[i]
            if rest > window:
                still.append(i)
            elif rest > 0:
                pieces[i].append((offsets[i], rest))
        live = still
    return pieces


def _fused(hotwords, ngram_lm_alpha):
    """the keywords a recogniser call gets: only those that were given, so that a model without them is called as ever"""
    return {k: v for k, v in (("hotwords", hotwords), ("ngram_lm_alpha", ngram_lm_alpha)) if v is not None}


def per_recording(hotwords, n):
    """`hotwords=` of transcribe_batch -> one spec per recording: a string (phrases separated by `/`) or a HotwordGraph is every
    recording's; a list has one entry per recording (a string, a list of phrases, a HotwordGraph, or None = the model's own)"""
    if hotwords is None:
        return None
    if isinstance(hotwords, str) or not hasattr(hotwords, "__len__"):
        return [hotwords] * n
    fusion.check_entries(fusion.ESPNET, hotwords, n, "recording")
    return list(hotwords)


def transcribe(model, audio, config=None, hotwords=None, ngram_lm_alpha=None):
    """Interface function to transcribe audio data (transcribe.py:34-82).

    Args:
      model (EspnetModel): what `load_model()` returned
      audio (AudioData): Audio to transcribe
      config (TranscribeConfig): Additional settings
      hotwords: this recording's phrases (a string of phrases separated by `/`, a list of phrases, or a HotwordGraph) instead of
        the model's; they apply to every 20 s window cut from it
      ngram_lm_alpha (float): the weight of the model's n-gram LM in this call (None = `model.ngram_lm_alpha`, 0 = without the LM)

    Returns:
      TranscribeResult

    The windows are recognised and time-stamped one after the other, like the reference's loop.  With
    `segmentation="device"`, `transcribe_batch(model, [audio])` returns the same result with the windows of the recording
    recognised and aligned as one batch.
    """
    config = config or TranscribeConfig()
    audio = AudioData(norm_batch(model, [audio], norm_audio)[0], SAMPLERATE)
    rate = audio.samplerate
    total = len(audio.waveform)
    texts, segments = [], []
    scored = [] if getattr(model, "token_scores", False) else None
    if hotwords is not None and not isinstance(hotwords, str) and hasattr(model, "hotword_graph"):
        hotwords = model.hotword_graph(hotwords)           # a list is ONE recording's phrases: built once, shared by its windows
    fused = _fused(hotwords, ngram_lm_alpha)
    for offset, samples in _windows(model, audio.waveform, int(WINDOW_SECONDS * rate)):
        best = model(np.pad(samples, PADDING, mode="constant"), **fused)[0]           # nbest[0] = (text, tokens, ids, hypothesis)
        text = best[0]
        texts.append(text)
        if scored is not None:
            scored.append((best[3].yseq, best[3].token_logprobs))
        segments.extend(Segment(start_seconds=(offset + first) / rate, end_seconds=(offset + last) / rate, text=piece)
                        for first, last, piece in split_text(model, samples, text))
        if config.verbose:       # the reference draws a tqdm bar over the samples (transcribe.py:55-56,79-80)
            done = offset + len(samples)
            print(f"\rTranscribe: {done}/{total}", end="" if done < total else "\n", file=sys.stderr, flush=True)
    return make_result("".join(texts), segments, scored)


def transcribe_batch(model, audios, config=None, hotwords=None, ngram_lm_alpha=None):
    """Additive: many utterances recognised as one batch on the device.

    `hotwords`: one spec for every recording (a string) or a list with one entry per recording (`per_recording`); a recording's
    hotwords apply to every window cut from it, also on the pooled long-form path.  `ngram_lm_alpha`: the weight of the model's
    n-gram LM in this call (0 = without the LM).

    `model.segmentation == "host"`: SHORT utterances (each at most one 20 s window) are recognised as one batch and segmented
    one by one on the host; an utterance longer than a window goes through `transcribe` on its own.

    `model.segmentation == "device"`: recordings of ANY length.  The cut points of all long recordings are found in lockstep
    (`plan_windows`: one batched blank pass and one rs_ctc_find_blank launch per round, `EspnetModel.find_blank_batch`), then
    the pieces of all recordings — the whole of every short one included — form one pool that is recognised as batches
    (`recognize_batch`) and aligned as batches (`align_batch`).  The results equal `transcribe`'s, in the caller's order.  A
    caller with ONE long file passes `[audio]`: its windows are then recognised and aligned as a batch, not one at a time."""
    if config is None:
        config = TranscribeConfig(verbose=False)
    norm = [AudioData(w, SAMPLERATE) for w in norm_batch(model, audios, norm_audio)]
    window = int(WINDOW_SECONDS * 16000)
    hotwords = per_recording(hotwords, len(norm))
    if getattr(model, "segmentation", "host") == "device":
        return _transcribe_pooled(model, norm, window, hotwords, ngram_lm_alpha)
    short = [i for i, a in enumerate(norm) if len(a.waveform) <= window]
    out = [None] * len(norm)
    with_scores = getattr(model, "token_scores", False)
    fused = _fused(None if hotwords is None else [hotwords[i] for i in short], ngram_lm_alpha)
    if with_scores and short:
        texts, scored = model.recognize_batch_scored([norm[i].waveform for i in short], **fused)
    else:
        texts, scored = (model.recognize_batch([norm[i].waveform for i in short], **fused) if short else []), None
    pieces = [split_text(model, norm[i].waveform, asr) for i, asr in zip(short, texts)]
    for k, (i, asr, segments) in enumerate(zip(short, texts, pieces)):
        segs = [Segment(start / 16000, end / 16000, text) for start, end, text in segments]
        out[i] = make_result(asr, segs, [scored[k]] if scored is not None else None)
    for i, a in enumerate(norm):
        if out[i] is None:
            out[i] = transcribe(model, a, TranscribeConfig(verbose=False), **_fused(None if hotwords is None else hotwords[i], ngram_lm_alpha))
    return out


def _transcribe_pooled(model, norm, window, hotwords=None, ngram_lm_alpha=None):
    """`transcribe_batch` with the segmentation on the device: plan the pieces of every recording, then recognise and align
    the pool of all pieces, longest first so that a chunk of 256 holds pieces of similar length"""
    waves = [a.waveform for a in norm]
    plan = plan_windows([len(w) for w in waves], window,
                        lambda requests: model.find_blank_batch([waves[i][o:o + n] for i, o, n in requests]))
    pool = [(i, o, n) for i, pieces in enumerate(plan) for o, n in pieces]
    order = sorted(range(len(pool)), key=lambda k: (-pool[k][2], k))
    samples = [waves[pool[k][0]][pool[k][1]:pool[k][1] + pool[k][2]] for k in order]
    texts, timings = [None] * len(pool), [None] * len(pool)
    scored = [None] * len(pool) if getattr(model, "token_scores", False) else None
    # a piece is recognised with the hotwords of the recording it was cut from
    fused = _fused(None if hotwords is None else [hotwords[pool[k][0]] for k in order], ngram_lm_alpha)
    if pool:
        if scored is not None:
            recognised, piece_scores = model.recognize_batch_scored(samples, isolate_overflow=True, **fused)
            for k, sc in zip(order, piece_scores):
                scored[k] = sc
        else:
            recognised = model.recognize_batch(samples, isolate_overflow=True, **fused)
        for k, text in zip(order, recognised):
            texts[k] = text
        for k, t in zip(order, model.align_batch(samples, [texts[k] for k in order])):
            timings[k] = t
    out, k = [], 0
    for a, pieces in zip(norm, plan):
        rate = a.samplerate
        joined, segments = [], []
        first_piece = k
        for offset, n in pieces:
            joined.append(texts[k])
            segments.extend(Segment(start_seconds=(offset + first) / rate, end_seconds=(offset + last) / rate, text=piece)
                            for first, last, piece in segments_from_timings(timings[k], n, texts[k]))
            k += 1
        out.append(make_result("".join(joined), segments, scored[first_piece:k] if scored is not None else None))
    return out
