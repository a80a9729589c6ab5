"""Value types of the `reazonspeech.k2.asr` API.

Names, field order and defaults are the ones callers of the reference package construct and read
(pkg/k2-asr/src/interface.py:4-26), so that switching packages needs no change on their side.  Compared with the NeMo
package there are no segments and no token ids: the sherpa-onnx result the reference consumes has only token strings and one
time stamp per token (pkg/k2-asr/src/transcribe.py:41-45).
"""
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np


@dataclass
class AudioData:
    """Mono waveform (float32 samples in [-1, 1]) and its sample rate in Hz (interface.py:4-8)."""
    waveform: np.ndarray
    samplerate: int


@dataclass
class Subword:
    """One emitted token and the single point in time at which the transducer emitted it, in seconds of the PADDED audio the
    recogniser saw: like the reference, the 0.9 s of leading padding (transcribe.py:7,31-33) is NOT subtracted
    (interface.py:10-14; transcribe.py:43)."""
    seconds: float
    token: str


@dataclass
class TranscribeResult:
    """What `transcribe()` returns: the text (tokens joined) and the tokens with their times (interface.py:16-19)."""
    text: str
    subwords: List[Subword] = field(default_factory=list)


@dataclass
class ScoredTranscribeResult(TranscribeResult):
    """What `transcribe()` returns from a model loaded with `token_scores=True` (additive: a TranscribeResult with these fields
    after the reference's).  `token_logprobs[i]` = log-probability of `token_ids[i]` under the model's own distribution at the
    frame it was emitted — no blank penalty, no hotword bonus (include/rs_asr.h rs_rnnt_token_scores); `subword_logprobs` is
    aligned with `subwords` (here one subword per token); `confidence` = exp(mean(token_logprobs)), None without tokens."""
    token_ids: List[int] = field(default_factory=list)
    token_logprobs: List[float] = field(default_factory=list)
    confidence: Optional[float] = None
    subword_logprobs: List[float] = field(default_factory=list)


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
    """What `transcribe()` returns from a model loaded with `nbest=N` (this project's addition; sherpa-onnx has no n-best): the
    result as ever, plus `nbest` — the N best hypotheses of the modified beam search's last set as results of this same type,
    ranked by `norm_log_prob` (log_prob / len(ys) as sherpa-onnx normalises it), entry 0 equal to the result itself, fewer than N
    when the last set is smaller.  `log_prob` is the hypothesis's total log-probability with hotword and LM terms inside.  The
    token fields are those of ScoredTranscribeResult: filled for the result and entry 0 when the model also has `token_scores=True`,
    None for every other entry (and for all of them with `token_scores` off)."""
    log_prob: Optional[float] = None
    norm_log_prob: Optional[float] = None
    nbest: List["NBestTranscribeResult"] = field(default_factory=list)
    token_ids: Optional[List[int]] = None
    token_logprobs: Optional[List[float]] = None
    confidence: Optional[float] = None
    subword_logprobs: Optional[List[float]] = None


@dataclass
class RescoredTranscribeResult(NBestTranscribeResult):
    """What `transcribe()` returns from a model loaded with `nbest=N, rescore="likelihood" | "norm_likelihood"` (additive): an
    NBestTranscribeResult whose list was re-ranked by full likelihood.  Every entry has `log_likelihood` = log P(text | audio) summed
    over ALL alignments of its tokens (include/rs_asr.h rs_rnnt_align_rows; what `align_text` gives for that text),
    `alignment_log_prob` = the best alignment's own score, `norm_log_likelihood` = log_likelihood / max(tokens, 1) and `search_rank`
    = its position in the search's own list.  The list is in descending order of the chosen key (ties in the search's order) and
    the result itself is its entry 0.  With `token_scores=True` every entry carries the token fields, not entry 0 alone."""
    log_likelihood: Optional[float] = None
    alignment_log_prob: Optional[float] = None
    norm_log_likelihood: Optional[float] = None
    search_rank: Optional[int] = None


def mean_confidence(logprobs):
    """exp(mean(logprobs)), None for an empty list"""
    return float(np.exp(np.mean(np.asarray(logprobs, np.float64)))) if len(logprobs) else None


@dataclass
class TranscribeConfig:
    """Per-call options (interface.py:21-26).  `verbose` only controls the long-audio warning."""
    verbose: bool = True
