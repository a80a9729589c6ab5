"""`transcribe()` of `reazonspeech.k2.asr` (pkg/k2-asr/src/transcribe.py:7-45): normalise to 16 kHz mono, pad PAD_SECONDS of
silence on both sides, warn above TOO_LONG_SECONDS, decode one stream, pair tokens with timestamps."""
import warnings

from ...runtime import fusion
from ...runtime.resample import norm_batch
from .interface import (AudioData, TranscribeConfig, TranscribeResult, ScoredTranscribeResult, NBestTranscribeResult, RescoredTranscribeResult,
                        Subword, mean_confidence)
from .audio import pad_audio, norm_audio, SAMPLERATE

PAD_SECONDS = 0.9
TOO_LONG_SECONDS = 30.0


def _prepare_batch(model, audios):
    """`_prepare` for a list, normalised where `model.resample` says (host or device): -> [AudioData]"""
    return [_pad_and_warn(AudioData(w, SAMPLERATE)) for w in norm_batch(model, audios, norm_audio)]


def _prepare(audio):
    return _pad_and_warn(norm_audio(audio))


def _pad_and_warn(audio):
    """16 kHz mono in: the reference's padding and its warning"""
    audio = pad_audio(audio, PAD_SECONDS)
    duration = audio.waveform.shape[0] / audio.samplerate
    if duration > TOO_LONG_SECONDS:      # the reference's warning (transcribe.py:27-34): upstream's memory grows with T^2
        warnings.warn(
            f"Passing a long audio input ({duration:.1f}s) is not recommended, "
            "because K2 will require a large amount of memory. "
            "Read the upstream discussion for more details: "
            "https://github.com/k2-fsa/icefall/issues/1680"
        )
    return audio


def _entry(r):
    """one result of `stream.result.nbest` -> NBestTranscribeResult without its own list"""
    subwords = [Subword(token=t, seconds=s) for t, s in zip(r.tokens, r.timestamps)]
    lp = r.token_log_probs
    scored = {} if lp is None else dict(token_ids=list(r.token_ids), token_logprobs=list(lp), confidence=mean_confidence(lp), subword_logprobs=list(lp))
    if getattr(r, "log_likelihood", None) is not None:        # a model loaded with rescore=: the list was re-ranked by full likelihood
        return RescoredTranscribeResult(r.text, subwords, log_prob=r.log_prob, norm_log_prob=r.norm_log_prob, log_likelihood=r.log_likelihood,
                                        alignment_log_prob=r.alignment_log_prob, norm_log_likelihood=r.norm_log_likelihood,
                                        search_rank=r.search_rank, **scored)
    return NBestTranscribeResult(r.text, subwords, log_prob=r.log_prob, norm_log_prob=r.norm_log_prob, **scored)


def _result(stream):
    if getattr(stream.result, "nbest", None) is not None:     # a model loaded with nbest=N: entry 0 is the result itself
        entries = [_entry(r) for r in stream.result.nbest]
        if not entries:                                        # no frames: no hypothesis was ranked
            return (RescoredTranscribeResult if getattr(stream.result, "rescore_key", None) else NBestTranscribeResult)(stream.result.text, [])
        head = _entry(stream.result.nbest[0])
        head.nbest = entries
        return head
    subwords = [Subword(token=t, seconds=s) for t, s in zip(stream.result.tokens, stream.result.timestamps)]
    lp = getattr(stream.result, "token_log_probs", None)
    if lp is not None:                   # a model loaded with token_scores=True
        return ScoredTranscribeResult(stream.result.text, subwords, token_ids=list(stream.result.token_ids), token_logprobs=list(lp),
                                      confidence=mean_confidence(lp), subword_logprobs=list(lp))
    return TranscribeResult(stream.result.text, subwords)


def _streams(model, audios, hotwords):
    """one stream per prepared audio; `hotwords`: None, one specification (a string) for all, or a list with one entry per audio"""
    # (no graph of its own leaves a stream at None: the model's is put in at decode time, `stream_graphs`)
    make = lambda spec: model.hotword_graph(spec)         # (asked of the model only when a call has hotwords: a bare recogniser has none)
    per_audio = fusion.per_item(fusion.K2, hotwords, len(audios), None, make, "audio") or [None] * len(audios)
    streams = []
    for a, g in zip(audios, per_audio):
        st = model.create_stream() if g is None else model.create_stream(hotwords=g)     # (no hotwords: the reference's call)
        st.accept_waveform(a.samplerate, a.waveform)
        streams.append(st)
    return streams


def transcribe(model, audio, config=None, hotwords=None, ngram_lm_alpha=None):
    """Inference audio data using the K2 model (transcribe.py:10-45).

    Args:
        model (K2Model): what `load_model()` returned
        audio (AudioData): Audio data to transcribe
        config (TranscribeConfig): Additional settings
        hotwords: phrases to favour in this call INSTEAD OF the model's (`create_stream(hotwords=...)`): a string of phrases
            separated by `/`, or a list of phrases, each with an optional ` :score`; None = the model's hotwords, if any
        ngram_lm_alpha: the weight of the model's n-gram LM in this call: None = `model.ngram_lm_alpha`, 0 = this call without the
            LM; a value while the model has no LM raises ValueError

    Returns:
        TranscribeResult

    The search is the model's: a model built with `load_model(decoding_method="modified_beam_search", max_active_paths=K)` is
    decoded by the beam search, nothing changes here.
    """
    if config is None:
        config = TranscribeConfig()
    audio = _prepare_batch(model, [audio])[0]
    stream = _streams(model, [audio], None if hotwords is None else [hotwords])[0]
    if ngram_lm_alpha is None:
        model.decode_stream(stream)                       # (the reference's call)
    else:
        model.decode_streams([stream], ngram_lm_alpha=ngram_lm_alpha)
    return _result(stream)


def transcribe_batch(model, audios, config=None, hotwords=None):
    """Additive: many utterances as one (or several pipelined) batches on the device; per utterance the same result as
    `transcribe` (every kernel masks by the utterance's own length).  The search (greedy or modified beam search) is the one the
    model was built with (`load_model(decoding_method=...)`).  `hotwords`: None (the model's, if any), one string of phrases
    separated by `/` for all audios, or a list with one entry per audio (None / a string / a list of phrases): every utterance is
    biased by its own graph inside the one batch.  A model loaded with an n-gram LM decodes every batch with `model.ngram_lm` at
    `model.ngram_lm_alpha`; the per-call weight is on `transcribe` only."""
    streams = _streams(model, _prepare_batch(model, audios), hotwords)
    model.decode_streams(streams)
    return [_result(st) for st in streams]
