"""`align_text()` / `align_text_batch()` — additive: a KNOWN text placed on the audio and scored by the transducer lattice
(include/rs_asr.h rs_rnnt_align, one label per frame: how every search of this package moves).  The audio takes the way of
`transcribe` (`norm_audio`, PAD_SECONDS of silence on both sides), so times mean what they mean there."""
from .interface import AlignedTranscribeResult, Subword, mean_confidence
from .transcribe import _prepare_batch


def text_ids(model, text):
    """a string by the character lookup in tokens.txt that the hotwords use (white space is skipped, a repeated symbol takes its
    first id); a character that is no token raises ValueError.  A sequence of token ids is taken as it is."""
    if not isinstance(text, str):
        return [int(i) for i in text]
    table = {s: i for i, s in reversed(list(enumerate(model.tokens)))}
    chars = [c for c in text if not c.isspace()]
    bad = [c for c in chars if c not in table or table[c] in (model.cfg.blank_id, model.cfg.unk_id)]
    if bad:
        raise ValueError(f"align_text: {bad[0]!r} is not in tokens.txt (pass token ids to bring another tokenisation)")
    return [table[c] for c in chars]


def aligned_result(model, ids, frames, logprobs, log_likelihood, alignment_log_prob, feasible):
    """`K2Model.convert` over (ids, frames): tokens and timestamps as `transcribe` gives them; an infeasible text has no times"""
    r = model.convert(ids, frames if feasible else [0] * len(ids), list(logprobs))
    subwords = [Subword(token=t, seconds=s) for t, s in zip(r.tokens, r.timestamps)] if feasible else []
    lp = list(logprobs)
    return AlignedTranscribeResult(r.text, subwords, token_ids=list(ids), token_logprobs=lp, confidence=mean_confidence(lp) if feasible else None,
                                   subword_logprobs=lp if feasible else [], log_likelihood=float(log_likelihood),
                                   alignment_log_prob=float(alignment_log_prob), norm_log_likelihood=float(log_likelihood) / max(len(ids), 1),
                                   feasible=bool(feasible))


def align_text_batch(model, audios, texts, config=None):
    """Align a list of (AudioData, text) pairs in batched passes.  `texts[i]`: a string (one token per character, `text_ids`) or a
    sequence of token ids.  A text with more tokens than the audio has frames has no alignment: `feasible=False`, no exception.

    Returns:
      list[AlignedTranscribeResult]
    """
    if len(audios) != len(texts):
        raise ValueError(f"align_text_batch: {len(audios)} audios but {len(texts)} texts")
    labels = [text_ids(model, t) for t in texts]
    waves = [a.waveform for a in _prepare_batch(model, audios)]
    res = model.am.align_waveforms(waves, labels)
    return [aligned_result(model, labels[i], res.frames[i], res.token_logprobs[i], res.log_likelihood[i], res.alignment_log_prob[i],
                           res.feasible[i]) for i in range(len(waves))]


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
    waves = [a.waveform for a in _prepare_batch(model, audios)]
    res, _ = model.am.align_candidates(waves, labels)
    return [[aligned_result(model, ids, r.frames[j], r.token_logprobs[j], r.log_likelihood[j], r.alignment_log_prob[j], r.feasible[j])
             for j, ids in enumerate(labels[i])] for i, r in enumerate(res)]


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
        model (K2Model): what `load_model()` returned
        audio (AudioData): the audio
        text: a string, or a sequence of token ids
        config (TranscribeConfig): additional settings

    Returns:
        AlignedTranscribeResult
    """
    return align_text_batch(model, [audio], [text], config)[0]
