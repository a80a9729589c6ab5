"""`load_model()` / `transcribe()` — the drop-in pair (pkg/nemo-asr/src/transcribe.py:9-60),
plus the additive batched entry point `transcribe_batch()` the RTFx metric is quoted on.

What changes underneath: NeMo's `EncDecRNNTBPEModel` is replaced by
`reazonspeech_amd.runtime.model.AsrModel` (HIP kernels behind include/rs_asr.h); padding is
folded into the front-end kernel instead of `np.pad`; decoding is the checkpoint's strategy — batched
greedy or ALSD beam search on the device — adapted to the ALSD-shaped `Hypothesis` the reference
post-processor expects (interface.Hypothesis).
"""
import os
import sys

import numpy as np
import torch

from .interface import TranscribeConfig, Hypothesis
from .decode import decode_hypothesis, PAD_SECONDS
from .audio import norm_audio
from ...runtime import fusion, nemo_hotwords
from ...runtime.resample import norm_batch

#: where a real checkpoint is looked for; the reference downloads
#: 'reazon-research/reazonspeech-nemo-v2' from the HF hub (transcribe.py:26-28), which an
#: offline box cannot do.
CHECKPOINT_ENV = "REAZONSPEECH_NEMO_CHECKPOINT"
HF_REPO = "reazon-research/reazonspeech-nemo-v2"      # transcribe.py:27


def resolve_checkpoint(checkpoint=None, allow_download=True):
    """Where the model's `.nemo` archive comes from, in the order a user of the reference would expect:
      1. the `checkpoint` argument, 2. $REAZONSPEECH_NEMO_CHECKPOINT,
      3. the Hugging Face cache of 'reazon-research/reazonspeech-nemo-v2' (what the reference's
         `from_pretrained` fills, transcribe.py:26-28), 4. a download of that repository when the hub is reachable
         (not with HF_HUB_OFFLINE=1).
    -> path of the archive, or None when there is none (the caller then falls back to synthetic weights, loudly)."""
    import glob
    path = checkpoint or os.environ.get(CHECKPOINT_ENV)
    if path:
        if not os.path.exists(path):
            raise FileNotFoundError(f"checkpoint {path!r} does not exist")
        return path
    try:
        from huggingface_hub import snapshot_download
    except ImportError:
        return None
    for local_only in (True, False):
        if not local_only and (not allow_download or os.environ.get("HF_HUB_OFFLINE", "0") not in ("", "0")):
            break
        try:
            root = snapshot_download(HF_REPO, local_files_only=local_only, allow_patterns=["*.nemo"], etag_timeout=5)
        except Exception as e:             # not cached / no network / authentication / disk: remembered for the caller's warning
            resolve_checkpoint.last_error = f"{'cache lookup' if local_only else 'download'}: {type(e).__name__}: {e}"
            continue
        found = sorted(glob.glob(os.path.join(root, "**", "*.nemo"), recursive=True))
        if found:
            return found[0]
    return None


SYNTHETIC_ENV = "REAZONSPEECH_AMD_SYNTHETIC"


def load_model(device=None, checkpoint=None, config=None, seed=0, pos_cap=None, decoding=None, beam_size=None,
               precision="bf16", synthetic=False, resample="host", token_scores=False, nbest=0, hotwords_file="", hotwords_score=1.5, hotwords=None,
               ngram_lm_model=None, ngram_lm_alpha=0.0, ngram_lm_tokens="nemo", rescore=None):
    """Load the ReazonSpeech FastConformer-RNNT model onto a ROCm GPU.

    Args:
      device (str): "cuda" / "cuda:N" (ROCm devices report as cuda).  None picks "cuda" when
        available, like the reference (transcribe.py:18-22); there is no CPU execution path
        in this package, so "cpu" raises.
      checkpoint (str): path of a `.nemo` archive.  Defaults to $REAZONSPEECH_NEMO_CHECKPOINT, then to the Hugging Face
        cache / hub copy of 'reazon-research/reazonspeech-nemo-v2' (`resolve_checkpoint`).  When none can be found or
        downloaded this RAISES, as `from_pretrained` does in the reference (transcribe.py:26-28) — a transient hub error
        must not produce a model with made-up weights.
      config (ModelConfig), seed (int), synthetic (bool): SEEDED SYNTHETIC weights are loaded only on request — `config=`
        (an architecture; no checkpoint lookup is made), `synthetic=True` or $REAZONSPEECH_AMD_SYNTHETIC=1 (benchmarks /
        tests: timings are valid, transcripts meaningless), and a warning says so.
      decoding (str): override the checkpoint's decoding strategy: "greedy_batch", "alsd" (alignment-length
        synchronous beam search, what the reference checkpoint ships with: decode.py:29,38-41) or "beam" ([UPSTREAM] NeMo's
        `strategy: beam`, the default Graves beam search — the one ESPnet runs, csrc/k_rnnt_beam.hip).
      beam_size (int): override the beam size ("alsd": 1..8, "beam": 1..64).
      precision (str): "bf16" (default): the throughput mode — bf16 matrix-core operands, float32 accumulation, float32
        residual stream, exact float32 decode.  "fp32": the parity mode — float32 weights, activations and arithmetic end
        to end, i.e. what the reference computes (transcribe.py:26-28, :48-53 run NeMo in float32 without autocast; the
        same keyword as `reazonspeech.k2.asr.load_model(precision=...)`, pkg/k2-asr/src/huggingface.py:16); ~20x slower.
        "fp32x3": the float32 mode with every float32 PRODUCT of its GEMMs formed from three bf16 matrix-core terms (hi / lo split,
        float32 accumulation): twice the float32 mode's speed; not an IEEE chain, but every id of the 256-row float32-oracle goldens
        is reproduced (tests/test_gpu_fullsize.py).
      resample (str): where input at another rate than 16 kHz, or with several channels, is normalised (`norm_audio`: resample,
        then average the channels).  "host" (default) = scipy / soxr on the calling thread, one utterance at a time, as before;
        "device" = one HIP launch per (rate, channel count) group of a `transcribe_batch` call (`AsrModel.resample_batch`,
        rs_resample) with the host path's Kaiser filter — float32 rounding apart from the host path's result without soxr.
        Stored as `model.resample`, may be changed later.  Anything else raises ValueError.
      nbest (int): N in 1..8, at most `beam_size`, with `decoding="alsd"`: every result is an `NBestTranscribeResult` (interface.py)
        whose `nbest` holds the N best finished hypotheses — NeMo's `return_best_hypothesis=False`: `sort_nbest(final)` with equal
        label sequences kept once, ranked inside the search's selection kernel (rs_rnnt_alsd_nbest); entry 0 is the result itself;
        with `raw_hypothesis`, `hypothesis.n_best_hypotheses`.  0 (default): today's objects.  N above the beam, or N > 1 with a
        greedy decoding, raises ValueError.  Stored as `model.nbest`; `transcribe(..., nbest=N)` takes a count for one call.
      rescore (str): None (default), "likelihood" or "norm_likelihood", with `nbest >= 2`: every entry of the n-best list is scored
        by log P(text | audio) over ALL alignments, on the device right after the search (include/rs_asr.h rs_rnnt_align_rows: one
        lattice per utterance, the entries' common prefixes computed once), and the list is re-ranked by that (or by that divided
        by max(tokens, 1)), descending, ties in the search's order.  Results are `RescoredTranscribeResult` (interface.py): each entry
        has `log_likelihood`, `alignment_log_prob`, `norm_log_likelihood` and `search_rank`; the result itself is the new entry 0;
        with `token_scores=True` EVERY entry carries its token log-probabilities.  Needs `decoding="alsd"` and `nbest >= 2`
        (ValueError before anything is loaded).  Stored as `model.rescore`, may be set later; `transcribe(..., rescore=)` per call.
        A batch whose lists are beyond one call's lattice bound is scored over several calls; only lists of more than 2047 labels per entry, or ONE utterance's lists beyond the bound, raise ValueError (window the audio).
      token_scores (bool): every result is a `ScoredTranscribeResult` (interface.py): the log-probability of every emitted token
        under the model's own distribution, per subword, and confidences per segment and utterance (exp of the mean) — computed on
        the device right after the search (rs_rnnt_token_scores), valid with every `precision` and `decoding`; with
        `raw_hypothesis`, `Hypothesis.token_confidence` = exp(log-probability) like NeMo's `max_prob` method.  Off (default):
        today's objects.  Stored as `model.token_scores`, may be changed later.
      hotwords_file (str), hotwords_score (float), hotwords: contextual biasing of the ALSD beam search, with the keyword names and
        defaults of the k2 package ("" / 1.5 / None): a file with one phrase per line (an optional trailing ` :2.0` is that phrase's
        own score), and / or `hotwords` = the same as a string of phrases separated by `/` or a list (strings, or sequences of token
        ids).  Phrases are tokenised with the model's SentencePiece vocabulary, both as a word start and as the word reads in the
        middle of a sentence (runtime/nemo_hotwords.py); one the vocabulary cannot spell is skipped with a warning.  The search
        adds the score per matched token to hypotheses that spell a phrase out, inside its ranking, and takes it back when the
        match breaks off (include/rs_asr.h rs_rnnt_alsd_hotwords).  The graph is built and uploaded once, here;
        `transcribe(..., hotwords=...)` replaces it per call.  Non-empty hotwords with a decoding other than "alsd" raise ValueError.
      ngram_lm_model (str or NgramLm), ngram_lm_alpha (float), ngram_lm_tokens (str): shallow fusion of a backoff n-gram language
        model into the ALSD beam search, with NeMo's keyword names (`decoding.beam.ngram_lm_model` / `ngram_lm_alpha`): an ARPA text
        file (`.gz` allowed; a KenLM binary raises ValueError: only ARPA text is read) or an `NgramLm` built by
        runtime/ngram_lm.py.  Every label expansion's score gets `ngram_lm_alpha` x the LM's natural-log probability of the token
        after the hypothesis's labels, inside the ranking (include/rs_asr.h rs_rnnt_alsd_lm); no end-of-sentence term.
        `ngram_lm_tokens` says how a word of the file names a token: "nemo" (default) = one character chr(id + 100), which is
        [UPSTREAM, UNVERIFIED] believed to be what NeMo's train_kenlm.py writes for BPE models; "pieces" = the vocabulary's piece
        strings; "ids" = decimal ids.  Checked before anything is loaded: FileNotFoundError for a missing file, ValueError for an
        alpha that is no finite number >= 0, an unknown `ngram_lm_tokens`, or an LM with a decoding other than "alsd".  Stored as
        `model.ngram_lm` and `model.ngram_lm_alpha`, both may be set later; alpha 0 = the search without the LM.  The
        `decoding.beam.ngram_lm_model` key of a checkpoint's yaml is NOT read (it is a path of the training machine).
      pos_cap (int): encoder frames (80 ms each) the resident relative-position tables cover at load time
        (default 1024, about 82 s); longer utterances grow the tables on first use.

    Returns:
      reazonspeech_amd.runtime.model.AsrModel
    """
    from ...runtime.config import FASTCONFORMER_619M
    from ...runtime.model import AsrModel
    from ...runtime.tokenizer import SentencePieceTokenizer, SyntheticTokenizer
    from ...runtime import weights as W
    from ...runtime.resample import check_mode

    check_mode(resample)
    from ...runtime import rescore as rescoring
    rescoring.check(rescore, nbest, decoding is None or str(decoding) in ("alsd", "beam"))
    fusion.check_file("hotwords_file", hotwords_file)
    if decoding is not None:               # (a checkpoint's own strategy is only known once it is read: checked again below)
        fusion.check_hotword_keywords(fusion.NEMO, str(decoding), hotwords_file, hotwords_score, hotwords)
    has_lm = fusion.check_lm_keywords(fusion.NEMO, None if decoding is None else str(decoding), ngram_lm_model, ngram_lm_alpha, ngram_lm_tokens)
    fusion.check_file("ngram_lm_model", ngram_lm_model)
    if device is None:
        device = "cuda" if torch.cuda.is_available() else "cpu"
    if str(device).startswith("cpu"):
        raise RuntimeError("reazonspeech_amd runs on MI355X (gfx950) only; no CPU path exists "
                           "(use the reference package for CPU inference)")
    if config is not None and checkpoint is None:
        if os.environ.get(CHECKPOINT_ENV):
            print(f"[reazonspeech_amd] WARNING: ${CHECKPOINT_ENV} is set but ignored because an explicit `config` was passed "
                  f"(synthetic weights of that architecture are generated); pass `checkpoint=` to load the archive.", file=sys.stderr, flush=True)
    resolve_checkpoint.last_error = None
    want_synthetic = config is not None or synthetic or os.environ.get(SYNTHETIC_ENV, "0") not in ("", "0")
    checkpoint = None if want_synthetic and checkpoint is None else resolve_checkpoint(checkpoint)
    if not checkpoint and not want_synthetic:
        raise FileNotFoundError(
            f"no checkpoint: neither the `checkpoint` argument, ${CHECKPOINT_ENV}, nor a cached / downloadable copy of '{HF_REPO}' was found"
            + (f" (last lookup failure — {resolve_checkpoint.last_error})" if getattr(resolve_checkpoint, "last_error", None) else "")
            + f".  Seeded synthetic weights are loaded only on request: config=..., synthetic=True or ${SYNTHETIC_ENV}=1.")
    if checkpoint:
        cfg, sd, tok_bytes = W.read_nemo(checkpoint)
        tokenizer = SentencePieceTokenizer(tok_bytes) if tok_bytes else SyntheticTokenizer(cfg.vocab_size)
    else:
        if config is None:
            print("[reazonspeech_amd] WARNING: SEEDED SYNTHETIC weights of the 619M architecture were requested "
                  f"(`synthetic=True` / ${SYNTHETIC_ENV}): timings are valid, transcripts are meaningless.", file=sys.stderr, flush=True)
        cfg = config or FASTCONFORMER_619M
        sd = W.synthetic_state_dict(cfg, seed)
        tokenizer = SyntheticTokenizer(cfg.vocab_size, seed)
    if decoding is not None:
        cfg = cfg.with_(decoding=str(decoding))
    if beam_size is not None:
        cfg = cfg.with_(beam_size=int(beam_size))
    cfg.validate()
    kw = {} if pos_cap is None else {"pos_cap": int(pos_cap)}
    has_hotwords = fusion.check_hotword_keywords(fusion.NEMO, cfg.decoding, hotwords_file, hotwords_score, hotwords)
    fusion.check_lm_keywords(fusion.NEMO, cfg.decoding, ngram_lm_model, ngram_lm_alpha, ngram_lm_tokens)      # the checkpoint's own strategy is known now
    model = AsrModel(cfg, sd, tokenizer, device=device, pad_seconds=PAD_SECONDS, precision=precision, resample=resample, token_scores=token_scores, nbest=nbest, rescore=rescore,
                     **kw)
    model.hotwords_score = float(hotwords_score)
    if has_hotwords:
        model.hotwords = _model_graph(model, hotwords, hotwords_file)                  # the model's graph (None = nothing left to bias)
        if model.hotwords is not None:
            model.hotword_set((model.hotwords,))                                       # checked and uploaded once, at load
    model.ngram_lm_alpha = float(ngram_lm_alpha)
    if has_lm:
        model.ngram_lm = fusion.model_lm(fusion.NEMO, cfg, tokenizer, ngram_lm_model, ngram_lm_tokens)
        model.ngram_set(model.ngram_lm)                                                # checked and uploaded once, at load
    return model


def _model_graph(model, spec, hotwords_file=""):
    """`spec` -> the HotwordGraph `model` (an AsrModel of the NeMo family) decodes it with; None for nothing"""
    cfg = model.cfg
    graph = nemo_hotwords.make_graph(spec, model.tokenizer, cfg.blank_id, cfg.vocab_size, model.hotwords_score, hotwords_file)
    return fusion.check_graph(fusion.NEMO, cfg, graph)


def _call_graphs(model, hotwords, n):
    """the `hotwords` argument of a call over n audios -> None (no utterance has a graph) or one HotwordGraph / None per audio
    (fusion.per_item: None / "" = the model's graph)"""
    return fusion.per_item(fusion.NEMO, hotwords, n, getattr(model, "hotwords", None), lambda spec: _model_graph(model, spec), "audio")


def transcribe_batch(model, audios, config=None, distributed=False, hotwords=None):
    """Transcribe a list of AudioData in one batched pass.

    Each utterance is processed exactly as `transcribe()` would process it alone
    (per-utterance padding, masking and normalisation inside the kernels).

    With `distributed=True` and `torch.distributed` initialised (one process per GPU; the reference's
    multi-GPU mechanism, pkg/evaluation/src/base.py:194-212) every rank passes the same list, decodes a
    length-balanced shard on its own GPU and gets every result back, in the caller's order, through the
    path's one collective (an RCCL all_gather of the hypotheses).

    `hotwords`: None (the model's, if any: `load_model(hotwords=...)`), one string of phrases separated by `/` for all audios, or
    a list with one entry per audio (None / a string / a list of phrases) INSTEAD OF the model's: every utterance is biased by
    its own graph inside the one batch.  Needs `decoding="alsd"` (ValueError otherwise).  Without hotwords every result is what
    it was.

    A model loaded with an n-gram LM (`load_model(ngram_lm_model=...)`) decodes every batch with `model.ngram_lm` at
    `model.ngram_lm_alpha`; both may be set between calls (alpha 0 = without the LM).  `transcribe(..., ngram_lm_alpha=)` takes
    the weight per call.

    Returns:
      list[TranscribeResult]
    """
    if config is None:
        config = TranscribeConfig()
    return _transcribe_graphs(model, audios, config, distributed, _call_graphs(model, hotwords, len(audios)))


def _nbest_result(ret, score, norm):
    """a decoded hypothesis as an NBestTranscribeResult (the token fields only where `decode_hypothesis` scored it)"""
    from .interface import NBestTranscribeResult
    scored = {k: getattr(ret, k) for k in ("token_ids", "token_logprobs", "confidence", "subword_logprobs", "segment_confidence") if hasattr(ret, k)}
    return NBestTranscribeResult(ret.text, ret.subwords, ret.segments, ret.hypothesis, score=score, norm_score=norm, **scored)


def _rescored(model, decoded, k, hyp, config):
    """utterance k of a `RescoredBatch` -> the RescoredTranscribeResult: every entry scored, the list re-ranked by `model.rescore`
    (descending, ties in the search's order), the best entry's fields on the result itself"""
    from ...runtime import rescore as rescoring
    from .interface import NBestHypotheses, RescoredTranscribeResult
    entries, hyps = [], []
    for r, ((y, fr, score, norm), (ll, best, lp)) in enumerate(zip(decoded.nbest[k], decoded.rescored[k])):
        h = hyp if r == 0 else Hypothesis.from_alsd(y, [f + idx for idx, f in enumerate(fr)], model.cfg.blank_id)
        h.score = score
        if lp is not None:
            h.token_confidence = [float(np.exp(v)) for v in lp]
        ret = decode_hypothesis(model, h, lp)
        scored = {f: getattr(ret, f) for f in ("token_ids", "token_logprobs", "confidence", "subword_logprobs", "segment_confidence") if hasattr(ret, f)}
        extra = dict(log_likelihood=ll, alignment_log_prob=best, norm_log_likelihood=rescoring.norm(ll, len(y)), search_rank=r)
        for f, v in extra.items():
            setattr(h, f, v)
        entries.append(RescoredTranscribeResult(ret.text, ret.subwords, ret.segments, h if config.raw_hypothesis else None, score=score,
                                                norm_score=norm, **scored, **extra))
        hyps.append(h)
    if not entries:
        return None
    order = rescoring.order([e.log_likelihood for e in entries], [len(y) for y, _, _, _ in decoded.nbest[k]], model.rescore)
    entries, hyps = [entries[r] for r in order], [hyps[r] for r in order]
    head = RescoredTranscribeResult(**{f: getattr(entries[0], f) for f in entries[0].__dataclass_fields__})
    head.nbest = entries
    if config.raw_hypothesis:
        head.hypothesis = NBestHypotheses(hyps)
    return head


def _transcribe_graphs(model, audios, config, distributed, graphs, ngram_lm_alpha=None, nbest=None):
    """`transcribe_batch` with the hotwords resolved: `graphs` = None, or one HotwordGraph / None per audio; `ngram_lm_alpha`: the
    n-gram LM's weight in this call (None = the model's value, 0 = without the LM; a value with no LM loaded raises ValueError)"""
    lm = fusion.call_alpha(fusion.NEMO, model, ngram_lm_alpha)
    # 16 kHz mono float32 waveforms (transcribe.py:44 minus the padding, which the kernel applies)
    waves = [np.ascontiguousarray(w, dtype=np.float32) for w in norm_batch(model, audios, norm_audio)]
    if config.verbose:
        # the reference forwards `verbose` to NeMo (transcribe.py:52), which draws a tqdm bar on stderr
        print(f"[reazonspeech_amd] transcribing {len(waves)} utterance(s), "
              f"{sum(len(w) for w in waves) / 16000.0:.1f} s of audio on {model.device}", file=sys.stderr, flush=True)
    results = [None] * len(waves)

    def to_results(indices, decoded):
        # ids -> text / subwords / segments (decode.py:28-66).  Called per batch while the GPU works on the next ones.
        for k, i in enumerate(indices):
            ids, frames = decoded.ids[k], decoded.frames[k]
            if decoded.scores is not None:
                # beam search: alignment steps (frame + labels before) through the adapter with the documented offset
                hyp = Hypothesis.from_alsd(ids, [f + idx for idx, f in enumerate(frames)], model.cfg.blank_id)
                hyp.score = decoded.scores[k]
            else:
                hyp = Hypothesis.from_greedy(ids, frames, model.cfg.blank_id)
            lp = decoded.token_logprobs[k] if decoded.token_logprobs is not None else None
            if lp is not None:
                hyp.token_confidence = [float(np.exp(v)) for v in lp]
            ret = decode_hypothesis(model, hyp, lp)
            if config.raw_hypothesis:
                ret.hypothesis = hyp
            rescored = _rescored(model, decoded, k, hyp, config) if getattr(decoded, "rescored", None) is not None else None
            if rescored is not None:                      # the list re-ranked by full likelihood: its best entry is the result
                ret = rescored
            elif getattr(decoded, "rescored", None) is not None:      # no hypothesis was ranked: the same type, an empty list
                from .interface import RescoredTranscribeResult
                scored = {f: getattr(ret, f) for f in ("token_ids", "token_logprobs", "confidence", "subword_logprobs", "segment_confidence") if hasattr(ret, f)}
                ret = RescoredTranscribeResult(ret.text, ret.subwords, ret.segments, ret.hypothesis, **scored)
            elif decoded.nbest is not None:               # the ranked list: entry 0 is the result itself
                from .interface import NBestHypotheses
                entries, hyps = [], []
                for r, (y, fr, score, norm) in enumerate(decoded.nbest[k]):
                    h = hyp if r == 0 else Hypothesis.from_alsd(y, [f + idx for idx, f in enumerate(fr)], model.cfg.blank_id)
                    h.score = score
                    e = _nbest_result(ret if r == 0 else decode_hypothesis(model, h), score, norm)
                    entries.append(e)
                    hyps.append(h)
                ret = _nbest_result(ret, decoded.nbest[k][0][2], decoded.nbest[k][0][3]) if entries else _nbest_result(ret, None, None)
                ret.nbest = entries
                if config.raw_hypothesis:
                    ret.hypothesis = NBestHypotheses(hyps)
                    for e, h in zip(entries, hyps):
                        e.hypothesis = h
            results[i] = ret

    if distributed and getattr(model, "token_scores", False):
        raise ValueError("token_scores is on: the distributed path does not gather token log-probabilities (transcribe_batch(distributed=False) "
                         "on each rank, or load the model without token_scores)")
    if distributed:
        to_results(list(range(len(waves))), model.transcribe_waveforms_sharded(waves, hotwords=graphs, ngram_lm=lm))
    else:
        model.transcribe_waveforms(waves, on_batch=to_results, hotwords=graphs, nbest=nbest, ngram_lm=lm)
    return results


def transcribe(model, audio, config=None, hotwords=None, ngram_lm_alpha=None, nbest=None, rescore=None):
    """Inference of one utterance (transcribe.py:30-60).

    Args:
        model: what `load_model()` returned
        audio (AudioData): audio to transcribe
        config (TranscribeConfig): additional settings
        hotwords: phrases to favour in this call INSTEAD OF the model's: a string of phrases separated by `/`, or a list of
            phrases, each with an optional ` :score`; None = the model's hotwords, if any (needs `decoding="alsd"`)
        ngram_lm_alpha: the weight of the model's n-gram LM in this call: None = `model.ngram_lm_alpha`, 0 = this call without the
            LM; a value when no LM is loaded raises ValueError
        nbest: entries of the n-best list in this call: None = `model.nbest`, 0 = without the list, N = the N best finished
            hypotheses (`NBestTranscribeResult.nbest`; needs `decoding="alsd"` and N <= beam_size, ValueError otherwise).
            `transcribe_batch` decodes with `model.nbest`.
        rescore: n-best rescoring in this call: None = `model.rescore`, False = without it, "likelihood" / "norm_likelihood" = the
            list of this call re-ranked by that key (needs a list of at least two: ValueError otherwise; see `load_model`)

    Returns:
        TranscribeResult
    """
    if config is None:
        config = TranscribeConfig()
    graphs = _call_graphs(model, None if hotwords is None else [hotwords], 1)     # the argument is ONE audio's entry, whatever its type
    if rescore is None:
        return _transcribe_graphs(model, [audio], config, False, graphs, ngram_lm_alpha, nbest)[0]
    plan = model.rescore_plan(rescore, nbest)             # (ValueError before anything runs, and the model's own option stays)
    own, model.rescore = model.rescore, plan
    try:
        return _transcribe_graphs(model, [audio], config, False, graphs, ngram_lm_alpha, nbest)[0]
    finally:
        model.rescore = own
