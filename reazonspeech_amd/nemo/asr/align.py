"""`align_text()` / `align_text_batch()` — additive: a KNOWN text placed on the audio and scored by the transducer lattice
(include/rs_asr.h rs_rnnt_align), where the reference's corpus tools (pkg/_v1/src/align.py, pkg/espnet-oneseg) use a CTC head
this model does not have.  The audio takes the way of `transcribe` (`norm_audio`, the padding inside the front-end kernel), so
times mean what they mean there."""
import numpy as np

from .audio import norm_audio
from .decode import decode_hypothesis
from .interface import AlignedTranscribeResult, Hypothesis, TranscribeConfig
from ...runtime.resample import norm_batch


def text_ids(model, text):
    """a string through the model's tokenizer (`text_to_ids`: its first reading), or a sequence of token ids as it is"""
    if not isinstance(text, str):
        return [int(i) for i in text]
    if not text.strip():
        return []
    readings = model.tokenizer.text_to_ids(text)
    if not readings:
        raise ValueError(f"align_text: the vocabulary cannot spell {text!r} (pass token ids to bring another tokenisation)")
    return [int(i) for i in readings[0]]


def aligned_result(model, ids, frames, logprobs, log_likelihood, alignment_log_prob, feasible, raw_hypothesis=False):
    """`decode_hypothesis` over (ids, frames), as `transcribe` assembles a greedy result; an infeasible text keeps its text and ids
    and has no times"""
    hyp = Hypothesis.from_greedy(ids, frames if feasible else [0] * len(ids), model.cfg.blank_id)
    ret = decode_hypothesis(model, hyp, list(logprobs))
    out = AlignedTranscribeResult(ret.text, ret.subwords if feasible else [], ret.segments if feasible else [],
                                  hyp if raw_hypothesis and feasible else None, token_ids=ret.token_ids,
                                  token_logprobs=ret.token_logprobs, confidence=ret.confidence if feasible else None,
                                  subword_logprobs=ret.subword_logprobs if feasible else [],
                                  segment_confidence=ret.segment_confidence if feasible else [],
                                  log_likelihood=float(log_likelihood), alignment_log_prob=float(alignment_log_prob),
                                  norm_log_likelihood=float(log_likelihood) / max(len(ids), 1), feasible=bool(feasible))
    return out


def align_text_batch(model, audios, texts, config=None):
    """Align a list of (AudioData, text) pairs in batched passes: front-end and encoder as `transcribe_batch` runs them, then the
    lattice of every pair on the device.  `texts[i]`: a string (tokenised by `model.tokenizer.text_to_ids`; ValueError when the
    vocabulary cannot spell it) or a sequence of token ids.  A text that has no alignment returns `feasible=False`, it does not
    raise.

    Returns:
      list[AlignedTranscribeResult]
    """
    if config is None:
        config = TranscribeConfig(verbose=False)
    if len(audios) != len(texts):
        raise ValueError(f"align_text_batch: {len(audios)} audios but {len(texts)} texts")
    labels = [text_ids(model, t) for t in texts]
    waves = [np.ascontiguousarray(w, dtype=np.float32) for w in norm_batch(model, audios, norm_audio)]
    res = model.align_waveforms(waves, labels)
    return [aligned_result(model, labels[i], res.frames[i], res.token_logprobs[i], res.log_likelihood[i], res.alignment_log_prob[i],
                           res.feasible[i], config.raw_hypothesis) for i in range(len(waves))]


def score_texts_batch(model, audios, texts_per_audio, config=None):
    """Score several candidate transcripts per audio on one lattice each (include/rs_asr.h rs_rnnt_align_rows): `texts_per_audio[i]` is
    a list of texts for `audios[i]`, each a string or a sequence of token ids, tokenised as `align_text` tokenises.  Every audio goes
    through the front-end and the encoder ONCE, and the texts of an audio share the lattice cells of their common prefixes.

    Returns:
      list[list[AlignedTranscribeResult]]: per audio, one result per text in the order given; each equals what `align_text` returns
      for that (audio, text) pair, field for field.
    """
    if config is None:
        config = TranscribeConfig(verbose=False)
    if len(audios) != len(texts_per_audio):
        raise ValueError(f"score_texts_batch: {len(audios)} audios but {len(texts_per_audio)} lists of texts")
    labels = [[text_ids(model, t) for t in texts] for texts in texts_per_audio]
    waves = [np.ascontiguousarray(w, dtype=np.float32) for w in norm_batch(model, audios, norm_audio)]
    res, _ = model.align_candidates(waves, labels)
    return [[aligned_result(model, ids, r.frames[j], r.token_logprobs[j], r.log_likelihood[j], r.alignment_log_prob[j], r.feasible[j],
                            config.raw_hypothesis) for j, ids in enumerate(labels[i])] for i, r in enumerate(res)]


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
        model: what `load_model()` returned
        audio (AudioData): the audio
        text: a string, or a sequence of token ids
        config (TranscribeConfig): additional settings

    Returns:
        AlignedTranscribeResult
    """
    return align_text_batch(model, [audio], [text], config)[0]
