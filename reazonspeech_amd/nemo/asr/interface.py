"""Result / config value types of the `reazonspeech.nemo.asr` API.

Field names, order and defaults follow pkg/nemo-asr/src/interface.py:4-36 so that
callers (CLI writers, the evaluation harness, notebooks) can switch packages without
touching their code.  `Hypothesis` is new: it is the adapter object that stands in for
NeMo's `Hypothesis` at the two attributes the reference reads (`y_sequence`,
`timestamp`; pkg/nemo-asr/src/decode.py:40,44).
"""
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np


@dataclass
class AudioData:
    """A waveform plus its sample rate (interface.py:4-8)."""
    waveform: np.ndarray
    samplerate: int


@dataclass
class Subword:
    """One emitted subword and the time (seconds, single point) it was emitted at
    (interface.py:10-17)."""
    seconds: float
    token_id: int
    token: str


@dataclass
class Segment:
    """A run of subwords with start/end seconds (interface.py:19-24)."""
    start_seconds: float
    end_seconds: float
    text: str


@dataclass
class TranscribeResult:
    """What `transcribe()` returns (interface.py:26-31).  `hypothesis` is only filled
    when `TranscribeConfig.raw_hypothesis` is set (transcribe.py:57-58)."""
    text: str
    subwords: List[Subword]
    segments: List[Segment]
    hypothesis: object = None


@dataclass
class ScoredTranscribeResult(TranscribeResult):
    """What `transcribe()` returns from a model loaded with `token_scores=True` (additive: a TranscribeResult with these fields
    after the reference's).  `token_logprobs[i]` = log-probability of `token_ids[i]` under the model's own distribution at the
    frame it was emitted (include/rs_asr.h rs_rnnt_token_scores); `subword_logprobs` is aligned with `subwords` (pieces that
    decode to "" are dropped from both, so it can be shorter than `token_logprobs`); `segment_confidence[k]` = exp(mean of the
    log-probabilities of the subwords of `segments[k]`); `confidence` = exp(mean(token_logprobs)), None without tokens."""
    token_ids: List[int] = field(default_factory=list)
    token_logprobs: List[float] = field(default_factory=list)
    confidence: Optional[float] = None
    subword_logprobs: List[float] = field(default_factory=list)
    segment_confidence: List[float] = field(default_factory=list)


@dataclass
class AlignedTranscribeResult(ScoredTranscribeResult):
    """What `align_text()` returns (additive): the given text placed on the audio by the transducer lattice (include/rs_asr.h
    rs_rnnt_align).  The result fields are built from (token ids, Viterbi frames) the way `transcribe` builds them from a search;
    `token_logprobs[i]` = log-probability of `token_ids[i]` at its frame; `log_likelihood` = log P(text | audio) summed over ALL
    alignments; `alignment_log_prob` = the best alignment's own score (<= log_likelihood); `norm_log_likelihood` =
    log_likelihood / max(len(token_ids), 1); `feasible` False (scores -inf, no times) when the text has no alignment on this
    audio: no frames, or more tokens than frames for a model that emits one token per frame."""
    log_likelihood: float = float("-inf")
    alignment_log_prob: float = float("-inf")
    norm_log_likelihood: float = float("-inf")
    feasible: bool = False


@dataclass
class NBestTranscribeResult(TranscribeResult):
    """What `transcribe()` returns from a model loaded with `nbest=N` and the ALSD search (additive; NeMo's beam decoding with
    `return_best_hypothesis=False`): the result as ever, plus `nbest` — the N best finished hypotheses as results of this same type,
    ranked on the device by `norm_score` (score / (labels + 1) with the search's score normalisation; include/rs_asr.h
    rs_rnnt_alsd_nbest), equal label sequences kept once, entry 0 equal to the result itself in text, subwords, segments and score.
    `score` is the hypothesis's log-probability with hotword and LM terms inside.  The token fields are those of
    ScoredTranscribeResult: filled for entry 0 when the model also has `token_scores=True`, None for every other entry.  With
    `raw_hypothesis`, `hypothesis` is an NBestHypotheses whose `n_best_hypotheses` are the entries' Hypothesis objects."""
    score: Optional[float] = None
    norm_score: Optional[float] = None
    nbest: List["NBestTranscribeResult"] = field(default_factory=list)
    token_ids: Optional[List[int]] = None
    token_logprobs: Optional[List[float]] = None
    confidence: Optional[float] = None
    subword_logprobs: Optional[List[float]] = None
    segment_confidence: Optional[List[float]] = None


@dataclass
class RescoredTranscribeResult(NBestTranscribeResult):
    """What `transcribe()` returns from a model loaded with `nbest=N, rescore="likelihood" | "norm_likelihood"` (additive): an
    NBestTranscribeResult whose list was re-ranked by full likelihood.  Every entry has `log_likelihood` = log P(text | audio) summed
    over ALL alignments of its tokens (include/rs_asr.h rs_rnnt_align_rows; what `align_text` gives for that text),
    `alignment_log_prob` = the best alignment's own score, `norm_log_likelihood` = log_likelihood / max(tokens, 1) and `search_rank`
    = its position in the search's own list.  The list is in descending order of the chosen key (ties in the search's order) and
    the result itself is its entry 0.  With `token_scores=True` every entry carries the token fields, not entry 0 alone.  With
    `raw_hypothesis` the four fields are also attributes of the Hypothesis objects of `hypothesis.n_best_hypotheses`."""
    log_likelihood: Optional[float] = None
    alignment_log_prob: Optional[float] = None
    norm_log_likelihood: Optional[float] = None
    search_rank: Optional[int] = None


class NBestHypotheses:
    """[UPSTREAM] NeMo's NBestHypotheses: what `raw_hypothesis` carries when the lists are on"""

    def __init__(self, n_best_hypotheses):
        self.n_best_hypotheses = list(n_best_hypotheses)


def mean_confidence(logprobs):
    """exp(mean(logprobs)), None for an empty list"""
    return float(np.exp(np.mean(np.asarray(logprobs, np.float64)))) if len(logprobs) else None


@dataclass
class TranscribeConfig:
    """Per-call options (interface.py:33-36)."""
    verbose: bool = True
    raw_hypothesis: bool = False


#: What the beam search's `timestamp[idx]` holds relative to the alignment step i = frame + labels emitted before
#: (the index the device kernel records): `timestamp[idx] = i + ALSD_TIMESTAMP_OFFSET`.  With 1 the reference's
#: conversion `frame = step - idx - 1` (decode.py:48) returns the emission frame itself, i.e. subword time =
#: 0.08 * frame - 0.5 s — the semantics this package documents.  NeMo's own ALSD bookkeeping is [UPSTREAM] and could
#: not be checked here (a +-1 frame = 80 ms ambiguity in subword / segment times; text and ids
#: are unaffected): if a real NeMo hypothesis shows `timestamp[idx] = i`, set this to 0 — the one place to flip.
ALSD_TIMESTAMP_OFFSET = 1


class _IdSequence(list):
    """A list of ints that also answers `.tolist()` like the tensor NeMo returns
    (decode.py:40 calls `hyp.y_sequence.tolist()`)."""

    def tolist(self):
        return list(self)


def _int_list(values):
    """python ints from an integer ndarray / tensor (one C call) or any iterable"""
    out = values.tolist() if hasattr(values, "tolist") else list(values)
    return out if all(type(v) is int for v in out) else [int(v) for v in out]


@dataclass
class Hypothesis:
    """Greedy-decode result shaped like NeMo's ALSD `Hypothesis`.

    The reference post-processor was written for ALSD beam search output: it drops the
    first element of `y_sequence` (a prepended blank, decode.py:38-40) and converts
    `timestamp[idx]` (an alignment *step* = frames + symbols so far) back to a frame
    with `step - idx - 1` (decode.py:48).  The greedy kernel reports plain encoder frame
    indices, so the adapter stores `[blank] + ids` and `frame + idx + 1`; the
    reference formula then yields `seconds = max(0.08*frame - 0.5, 0)` unchanged.
    """
    y_sequence: _IdSequence
    timestamp: List[int]
    frames: List[int] = field(default_factory=list)
    score: Optional[float] = None
    token_confidence: Optional[List[float]] = None      # token_scores: exp(log-probability) per label ([UPSTREAM] NeMo preserve_token_confidence, method max_prob)

    @classmethod
    def from_greedy(cls, ids, frames, blank_id):
        ids, frames = _int_list(ids), _int_list(frames)
        steps = [f + idx + 1 for idx, f in enumerate(frames)]
        return cls(_IdSequence([int(blank_id)] + ids), steps, frames)

    @classmethod
    def from_alsd(cls, ids, steps, blank_id, offset=None):
        """Beam-search result: `steps[idx]` is the alignment index i = frame + labels before (what rs_rnnt_alsd
        records); the timestamps handed to the reference post-processor are `i + ALSD_TIMESTAMP_OFFSET`."""
        off = ALSD_TIMESTAMP_OFFSET if offset is None else int(offset)
        ids, steps = _int_list(ids), _int_list(steps)
        frames = [s - idx for idx, s in enumerate(steps)]
        return cls(_IdSequence([int(blank_id)] + ids), [s + off for s in steps], frames)
