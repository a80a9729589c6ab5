"""Value types of the `reazonspeech.espnet.asr` API.

Names, field order and defaults follow pkg/espnet-asr/src/interface.py:4-25 so that the reference's callers (its CLI, the
subtitle writers, evaluation notebooks) keep working unchanged.  This family reports SEGMENTS only: the window loop of
`transcribe()` produces one `Segment` per 30 s window with the window's bounds as its times (pkg/espnet-asr/src/transcribe.py:54-74).
"""
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np


@dataclass
class AudioData:
    """Mono waveform (float32 samples) and its sample rate in Hz (interface.py:4-8)."""
    waveform: np.ndarray
    samplerate: int


@dataclass
class Segment:
    """Text decoded from one window of the input, with the window's start and end in seconds of the original audio
    (interface.py:10-15)."""
    start_seconds: float
    end_seconds: float
    text: str


@dataclass
class TranscribeResult:
    """What `transcribe()` returns: the windows' texts concatenated, and the windows (interface.py:17-20)."""
    text: str
    segments: List[Segment] = field(default_factory=list)


@dataclass
class ScoredTranscribeResult(TranscribeResult):
    """What `transcribe()` returns from a model loaded with `token_scores=True` (additive: a TranscribeResult with these fields
    after the reference's).  `token_logprobs[i]` = log-probability of `token_ids[i]` under the model's own distribution at the
    frame it was emitted (include/rs_asr.h rs_rnnt_token_scores); the pieces of a long recording are concatenated in order;
    `confidence` = exp(mean(token_logprobs)), None without tokens."""
    token_ids: List[int] = field(default_factory=list)
    token_logprobs: List[float] = field(default_factory=list)
    confidence: Optional[float] = None


@dataclass
class AlignedTranscribeResult(ScoredTranscribeResult):
    """What `align_text()` returns (additive): the given text placed on the audio by the transducer lattice (include/rs_asr.h
    rs_rnnt_align).  The result fields are built from (token ids, Viterbi frames) the way `transcribe` builds them from a search;
    `token_logprobs[i]` = log-probability of `token_ids[i]` at its frame; `log_likelihood` = log P(text | audio) summed over ALL
    alignments; `alignment_log_prob` = the best alignment's own score (<= log_likelihood); `norm_log_likelihood` =
    log_likelihood / max(len(token_ids), 1); `feasible` False (scores -inf, no times) when the text has no alignment on this
    audio: no frames, or more tokens than frames for a model that emits one token per frame."""
    token_seconds: List[float] = field(default_factory=list)     # frame x the encoder's stride, minus the padding `transcribe` adds
    log_likelihood: float = float("-inf")
    alignment_log_prob: float = float("-inf")
    norm_log_likelihood: float = float("-inf")
    feasible: bool = False


def mean_confidence(logprobs):
    """exp(mean(logprobs)), None for an empty list"""
    return float(np.exp(np.mean(np.asarray(logprobs, np.float64)))) if len(logprobs) else None


def make_result(text, segments, scored=None):
    """the plain result, or — `scored` = [(token ids, log-probabilities) per piece, in order] — the scored one"""
    if scored is None:
        return TranscribeResult(text, segments)
    ids = [i for piece in scored for i in piece[0]]
    lps = [v for piece in scored for v in piece[1]]
    return ScoredTranscribeResult(text, segments, token_ids=ids, token_logprobs=lps, confidence=mean_confidence(lps))


@dataclass
class TranscribeConfig:
    """Per-call options (interface.py:22-25).  `verbose` turns the progress output of the window loop on."""
    verbose: bool = True
