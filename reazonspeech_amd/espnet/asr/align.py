"""`align_text()` / `align_text_batch()` — additive: a KNOWN text placed on the audio and scored by the TRANSDUCER lattice
(include/rs_asr.h rs_rnnt_align, the standard topology ESPnet trains and searches).  `EspnetModel.align_batch` is the CTC
aligner of a recognised text and stays what it is.  The audio takes the way of one window of `transcribe` (`norm_audio`, PADDING
samples of silence around it); a long recording is windowed by the caller."""
import numpy as np

from ...runtime.resample import norm_batch
from .audio import norm_audio
from .interface import AlignedTranscribeResult, Segment, mean_confidence
from .transcribe import PADDING


def text_ids(model, text):
    """a string through the model's token list, one token per character (' ' is '<space>'); a character that is no token
    raises ValueError.  A sequence of token ids is taken as it is."""
    if not isinstance(text, str):
        return [int(i) for i in text]
    table = {s: i for i, s in reversed(list(enumerate(model.token_list)))}
    syms = ["<space>" if c == " " else c for c in text]
    bad = [c for c in syms if c not in table or table[c] == model.cfg.blank_id]
    if bad:
        raise ValueError(f"align_text: {bad[0]!r} is not in the token list (pass token ids to bring another tokenisation)")
    return [table[c] for c in syms]


def frame_seconds(cfg):
    """the encoder's stride in seconds"""
    return cfg.hop_length * cfg.sub_factor / cfg.sample_rate


def aligned_result(model, ids, frames, logprobs, log_likelihood, alignment_log_prob, feasible, duration):
    """tokens with frame x encoder stride seconds (minus the left padding, inside [0, duration]); one Segment per token, ending
    where the next begins"""
    tokens = [model.token_list[i] for i in ids]
    step, left = frame_seconds(model.cfg), PADDING[0] / model.cfg.sample_rate
    times = [float(min(max(step * t - left, 0.0), duration)) for t in frames] if feasible else []
    ends = times[1:] + [float(duration)]
    segments = [Segment(s, e, model.tokens2text([tok])) for s, e, tok in zip(times, ends, tokens)]
    lp = list(logprobs)
    return AlignedTranscribeResult(model.tokens2text(tokens), segments, token_ids=list(ids), token_logprobs=lp,
                                   confidence=mean_confidence(lp) if feasible else None, token_seconds=times,
                                   log_likelihood=float(log_likelihood), alignment_log_prob=float(alignment_log_prob),
                                   norm_log_likelihood=float(log_likelihood) / max(len(ids), 1), feasible=bool(feasible))


def align_text_batch(model, audios, texts, config=None):
    """Align a list of (AudioData, text) pairs in batched passes.  `texts[i]`: a string (one token per character) or a sequence
    of token ids.  A text without an alignment (no frames) returns `feasible=False`, it does not raise.

    Returns:
      list[AlignedTranscribeResult]
    """
    if len(audios) != len(texts):
        raise ValueError(f"align_text_batch: {len(audios)} audios but {len(texts)} texts")
    labels = [text_ids(model, t) for t in texts]
    norm = norm_batch(model, audios, norm_audio)
    waves = [np.pad(np.asarray(w, np.float32), PADDING, mode="constant") for w in norm]
    res = model.am.align_waveforms(waves, labels, one_per_frame=False)
    return [aligned_result(model, labels[i], res.frames[i], res.token_logprobs[i], res.log_likelihood[i], res.alignment_log_prob[i],
                           res.feasible[i], len(norm[i]) / model.cfg.sample_rate) for i in range(len(waves))]


def score_texts_batch(model, audios, texts_per_audio, config=None):
    """Score several candidate transcripts per audio on one lattice each (include/rs_asr.h rs_rnnt_align_rows): `texts_per_audio[i]` is
    a list of texts for `audios[i]`, each a string or a sequence of token ids, tokenised as `align_text` tokenises.  Every audio goes
    through the front-end and the encoder ONCE, and the texts of an audio share the lattice cells of their common prefixes.

    Returns:
      list[list[AlignedTranscribeResult]]: per audio, one result per text in the order given; each equals what `align_text` returns
      for that (audio, text) pair, field for field.
    """
    if len(audios) != len(texts_per_audio):
        raise ValueError(f"score_texts_batch: {len(audios)} audios but {len(texts_per_audio)} lists of texts")
    labels = [[text_ids(model, t) for t in texts] for texts in texts_per_audio]
    norm = norm_batch(model, audios, norm_audio)
    waves = [np.pad(np.asarray(w, np.float32), PADDING, mode="constant") for w in norm]
    res, _ = model.am.align_candidates(waves, labels, one_per_frame=False)
    return [[aligned_result(model, ids, r.frames[j], r.token_logprobs[j], r.log_likelihood[j], r.alignment_log_prob[j], r.feasible[j],
                            len(norm[i]) / model.cfg.sample_rate) for j, ids in enumerate(labels[i])] for i, r in enumerate(res)]


def score_texts(model, audio, texts, config=None):
    """`score_texts_batch` for one audio: its candidate transcripts scored by full likelihood, in the order given.

    Returns:
      list[AlignedTranscribeResult]
    """
    return score_texts_batch(model, [audio], [texts], config)[0]


def align_text(model, audio, text, config=None):
    """Place `text` on `audio` and score it: when each token was spoken (the best alignment), log P(text | audio) over all
    alignments, and the best alignment's own score.

    Args:
      model (EspnetModel): what `load_model()` returned
      audio (AudioData): the audio (one window: up to about 20 s)
      text: a string, or a sequence of token ids
      config (TranscribeConfig): additional settings

    Returns:
      AlignedTranscribeResult
    """
    return align_text_batch(model, [audio], [text], config)[0]
