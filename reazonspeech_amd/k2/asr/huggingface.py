"""`load_model()` of `reazonspeech.k2.asr` (pkg/k2-asr/src/huggingface.py:16-83).

The reference resolves (language, precision) to four files of a Hugging Face repository — tokens.txt and the encoder / decoder /
joiner ONNX graphs (:26-66) — looks them up in the local cache before going online (:68-71) and hands them to sherpa-onnx
(:73-83: one thread, 16 kHz, 80-dim features, greedy search).  Here the same files are read WITHOUT onnx / onnxruntime /
sherpa-onnx (runtime/onnx_lite.py) and run by the HIP kernels of csrc/k_zipformer.hip; argument checking and error messages
follow the reference."""
import os
import sys

import torch

REPOS = {                 # language -> (repository, epochs in the file names)      huggingface.py:26-35
    "ja": ("reazon-research/reazonspeech-k2-v2", 99),
    "ja-en": ("reazon-research/reazonspeech-k2-v2-ja-en", 35),
    "ja-en-mls-5k": ("reazon-research/reazonspeech-k2-v2-ja-en-mls-5k-corrected", 21),
}
CHECKPOINT_ENV = "REAZONSPEECH_K2_CHECKPOINT"


def repo_files(language, precision):
    """-> (repository id, {tokens, encoder, decoder, joiner} file names); ValueError like the reference (:37-38, :61-62)"""
    if language not in REPOS:
        raise ValueError(f"Unknown language: '{language}'")
    repo, epochs = REPOS[language]
    stem = {part: f"{part}-epoch-{epochs}-avg-1" for part in ("encoder", "decoder", "joiner")}
    files = {
        "fp32": {"tokens": "tokens.txt", **{p: s + ".onnx" for p, s in stem.items()}},
        "int8": {"tokens": "tokens.txt", **{p: s + ".int8.onnx" for p, s in stem.items()}},
        "int8-fp32": {"tokens": "tokens.txt", "encoder": stem["encoder"] + ".int8.onnx", "decoder": stem["decoder"] + ".onnx",
                      "joiner": stem["joiner"] + ".int8.onnx"},
    }
    if precision not in files:
        raise ValueError("Unknown precision: '%s'" % precision)
    return repo, files[precision]


SYNTHETIC_ENV = "REAZONSPEECH_AMD_SYNTHETIC"


def resolve_checkpoint(language, precision, checkpoint=None):
    """directory holding the four files: the argument, $REAZONSPEECH_K2_CHECKPOINT, the Hugging Face cache
    (`snapshot_download(local_files_only=True)`, :68-69), then the hub (:70-71).  Like the reference, a failed lookup RAISES
    (a missing `huggingface_hub`, no cache entry while offline, a network / authentication error, a partial download): a
    caller with a transient hub error must not get a model with made-up weights."""
    repo, files = repo_files(language, precision)
    for cand in (checkpoint, os.environ.get(CHECKPOINT_ENV)):
        if cand:
            if not os.path.isdir(cand):
                raise FileNotFoundError(f"checkpoint directory {cand!r} does not exist")
            return cand, files
    import huggingface_hub as hf
    try:
        return hf.snapshot_download(repo, local_files_only=True), files
    except hf.utils.LocalEntryNotFoundError:
        return hf.snapshot_download(repo), files


def load_model(device=None, precision="fp32", language="ja", checkpoint=None, config=None, seed=0, compute=None, synthetic=False,
               decoding_method="greedy_search", max_active_paths=4, blank_penalty=0.0, resample="host", hotwords_file="",
               hotwords_score=1.5, hotwords=None, token_scores=False, nbest=0, rescore=None, ngram_lm_model=None, ngram_lm_alpha=0.0,
               ngram_lm_tokens="pieces"):
    """Load the ReazonSpeech k2 model onto a ROCm GPU (huggingface.py:16-83).

    Args:
      device (str): "cuda" / "cuda:N"; None picks "cuda".  The reference's default is "cpu" (sherpa-onnx's provider); this
        package has no CPU path — "cpu" and "coreml" raise.
      precision (str): "fp32", "int8" or "int8-fp32": which ONNX files are read, validated like the reference (:61-62).  The
        float32 files run in the `compute` mode below; the int8 files ("int8": encoder, decoder and joiner *.int8.onnx;
        "int8-fp32": the decoder's float file) are read by runtime/k2_onnx.py: read_k2_onnx_quantized and run in the int8 mode.
      language (str): "ja", "ja-en" or "ja-en-mls-5k" (:26-38)
      checkpoint (str): directory with tokens.txt and the three ONNX files (default: $REAZONSPEECH_K2_CHECKPOINT, then the
        Hugging Face cache, then the hub)
      config (ZipformerConfig), seed, synthetic: SEEDED SYNTHETIC weights are loaded only on request — `config=` (an architecture),
        `synthetic=True` or $REAZONSPEECH_AMD_SYNTHETIC=1 (benchmarks, tests: timings are valid, transcripts meaningless).  Without
        such a request a checkpoint that cannot be found or downloaded raises, as `hf.snapshot_download` does in the reference.
      compute (str): "bf16" (default): the throughput mode — bf16 matrix-core operands, float32 accumulation and residual stream,
        exact float32 decode.  "fp32": the parity mode — float32 weights, activations and arithmetic end to end, i.e. what
        onnxruntime computes from the reference's default float32 graphs; greedy ids identical to the float32 oracle, ~6x slower.
        "fp32x3": the float32 mode with its products formed from three bf16 matrix-core terms (2x faster; same 256-row golden, ids identical).
        None (default): "bf16" for the float32 files, the int8 mode for the int8 files.  The INT8 mode is onnxruntime's int8 graph
        restated: the float32 mode with every quantized Linear as DynamicQuantizeLinear (scale and zero point per utterance) +
        MatMulInteger on the int8 matrix cores + the scale Mul (csrc/k_int8.hip); not bit-exact against onnxruntime, which has never
        run here.  An explicit "bf16" / "fp32" / "fp32x3" with the int8 files raises ValueError.  With `synthetic` weights and an int8
        `precision`, the float weights are quantized with onnxruntime's QInt8 recipe (runtime/k2_weights.py: quantize_k2_linears).
        (`precision` keeps the reference's meaning: WHICH files are read.)
      decoding_method (str), max_active_paths (int), blank_penalty (float): the keywords of
        `sherpa_onnx.OfflineRecognizer.from_transducer` with its defaults.  "greedy_search" is what the reference passes (:81);
        "modified_beam_search" keeps `max_active_paths` (1..8, default 4) hypotheses per utterance (rs_rnnt_mbs,
        csrc/k_rnnt_mbs.hip).  Valid with every `precision` / `compute`; anything else raises ValueError.
      hotwords_file (str), hotwords_score (float): sherpa-onnx's contextual biasing, its names and defaults ("" / 1.5): a file with one
        phrase per line (blank lines ignored, an optional trailing ` :<float>` = the phrase's own score), every character looked up
        in tokens.txt; a phrase with a character that is no token is skipped with a warning.  The modified beam search then adds
        hotwords_score per matched token to hypotheses that spell a phrase out and takes it back when the match breaks off
        (rs_rnnt_mbs_hotwords, runtime/k2_hotwords.py).  `hotwords` = the same as an in-memory list (strings, or sequences of token
        ids).  The graph is built and uploaded once, here; `create_stream(hotwords=...)` / `transcribe(..., hotwords=...)` replace it
        per utterance.  With "greedy_search" non-empty hotwords raise ValueError, as upstream refuses them.
      ngram_lm_model (str or NgramLm), ngram_lm_alpha (float), ngram_lm_tokens (str): shallow fusion of a backoff n-gram language
        model of the user's own text into the modified beam search, the slot of icefall's modified_beam_search_lm_shallow_fusion
        ([UPSTREAM, UNVERIFIED]; sherpa-onnx's `lm=` is a neural LM and is not offered): an ARPA text file (`.gz` allowed; a KenLM
        binary raises ValueError) or an `NgramLm` built by runtime/ngram_lm.py.  A candidate that survives a frame's top-K selection
        and appends a token gets `ngram_lm_alpha` x the LM's natural-log probability of that token after the hypothesis's tokens
        (include/rs_asr.h rs_rnnt_mbs_lm); no end-of-sentence term.  `ngram_lm_tokens`: "pieces" (default) = the words of the file
        are the symbols of tokens.txt as written there, "ids" = decimal ids; "nemo" and anything else raise ValueError, as do an
        alpha that is no finite number >= 0 and an LM with "greedy_search".  Stored as `model.ngram_lm` / `model.ngram_lm_alpha`,
        both may be set later; `transcribe(..., ngram_lm_alpha=)` takes a weight for one call.
      nbest (int): this project's addition — sherpa-onnx returns one hypothesis per stream.  N in 1..8 with "modified_beam_search"
        makes `stream.result.nbest` (and `transcribe(...).nbest`) the N best hypotheses of the search's last set, ranked on the
        device by the rule that picks the winner (include/rs_asr.h rs_rnnt_mbs_nbest): results with tokens / timestamps / text /
        log_prob; entry 0 is the result itself; fewer than N when the last set is smaller.  0 (default) = off, today's objects.
        N above `max_active_paths`, or N > 1 with "greedy_search", raises ValueError.  Stored as `model.nbest`, may be set later.
      rescore (str): None (default), "likelihood" or "norm_likelihood", with nbest >= 2: every entry of the list is scored by
        log P(text | audio) over ALL alignments on the device right after the search (include/rs_asr.h rs_rnnt_align_rows: one
        lattice per utterance, the entries' common prefixes computed once) and the list is re-ranked by it (or by it divided by
        max(tokens, 1)), descending, ties in the search's order: `stream.result.nbest[k].log_likelihood`, `.alignment_log_prob`,
        `.norm_log_likelihood`, `.search_rank`; `transcribe(...)` returns a `RescoredTranscribeResult` whose entry 0 is the result
        itself; with `token_scores=True` every entry carries its token log-probabilities.  ValueError for another value,
        "greedy_search" or nbest < 2.  Stored as `model.rescore`, may be set later.
        A batch whose lists are beyond one call's lattice bound is scored over several calls; only lists of more than 2047 labels per entry, or ONE utterance's lists beyond the bound, raise ValueError (window the audio).
      resample (str): where `transcribe` / `transcribe_batch` normalise input at another rate than 16 kHz or with several channels
        (`norm_audio`): "host" (default) = scipy / soxr per utterance as before; "device" = one HIP launch per (rate, channel count)
        group of a call (`AsrModel.resample_batch`, rs_resample; the host path's Kaiser filter).  Stored as `model.resample`;
        anything else raises ValueError.  `K2Model.decode_streams` still expects 16 kHz streams.

    A real icefall export has never been read by runtime/k2_onnx.py (no file is reachable from the build environment): the reader
    is verified against files written in the documented export layout only, and checks itself after loading (every expected
    tensor found exactly once, parameter count == cfg.n_params(), folded softmax constants summing to 1) — treat a first real
    checkpoint as UNVERIFIED until one transcript has been compared with sherpa-onnx.

    Returns:
      K2Model (answers sherpa_onnx.OfflineRecognizer's create_stream / decode_stream)
    """
    from ...runtime.k2_config import ZIPFORMER_159M
    from ...runtime.k2_weights import synthetic_state_dict_k2
    from .model import K2Model, read_tokens, synthetic_tokens
    repo_files(language, precision)                       # argument errors first, like the reference
    from ...runtime.resample import check_mode
    check_mode(resample)
    from .model import search_config
    search_config(ZIPFORMER_159M, decoding_method, max_active_paths, blank_penalty, hotwords_file, hotwords_score, hotwords,
                  ngram_lm_model, ngram_lm_alpha, ngram_lm_tokens, nbest)
    from ...runtime import rescore as rescoring
    rescoring.check(rescore, nbest, decoding_method == "modified_beam_search")
    from ...runtime import fusion
    fusion.check_file("ngram_lm_model", ngram_lm_model)
    fusion.check_file("hotwords_file", hotwords_file)
    search = dict(decoding_method=decoding_method, max_active_paths=max_active_paths, blank_penalty=blank_penalty, resample=resample,
                  hotwords_file=hotwords_file, hotwords_score=hotwords_score, hotwords=hotwords, token_scores=token_scores,
                  ngram_lm_model=ngram_lm_model, ngram_lm_alpha=ngram_lm_alpha, ngram_lm_tokens=ngram_lm_tokens, nbest=nbest,
                  rescore=rescore)
    if device is None:
        device = "cuda"
    if not str(device).startswith("cuda"):
        raise RuntimeError(f"device {device!r}: reazonspeech_amd runs on MI355X (gfx950) only; no CPU / CoreML path exists "
                           "(use the reference package for those)")
    if not torch.cuda.is_available():
        raise RuntimeError("reazonspeech_amd needs a ROCm GPU: torch.cuda.is_available() is False")
    if compute not in (None, "bf16", "fp32", "fp32x3"):
        raise ValueError(f"compute must be None, 'bf16', 'fp32' or 'fp32x3', not {compute!r}")
    quantized = precision in ("int8", "int8-fp32")
    if quantized and compute is not None:
        raise ValueError(f"precision {precision!r} reads the int8 ONNX files, which run in the int8 mode only: leave compute at None "
                         f"(got {compute!r}; compute applies to precision='fp32')")
    want_synthetic = config is not None or synthetic or os.environ.get(SYNTHETIC_ENV, "0") not in ("", "0")
    if want_synthetic and not checkpoint:
        basedir, files = None, None
    else:
        basedir, files = resolve_checkpoint(language, precision, checkpoint)
    paths = [os.path.join(basedir, files[p]) for p in ("encoder", "decoder", "joiner")] if basedir else None
    q = None
    if basedir and quantized:
        from ...runtime.k2_onnx import read_k2_onnx_quantized
        cfg, sd, q = read_k2_onnx_quantized(*paths)
    elif basedir:
        from ...runtime.k2_onnx import read_k2_onnx
        cfg, sd = read_k2_onnx(*paths)
    if basedir:
        tokens = read_tokens(os.path.join(basedir, files["tokens"]))
        if len(tokens) != cfg.vocab_size:
            raise ValueError(f"tokens.txt has {len(tokens)} symbols, the joiner {cfg.vocab_size} outputs")
        cfg = cfg.with_(unk_id=tokens.index("<unk>") if "<unk>" in tokens else -1)
        if quantized:
            return K2Model(cfg, sd, tokens, device=device, precision="int8", qweights=q, **search)
        return K2Model(cfg, sd, tokens, device=device, precision=compute or "bf16", **search)
    cfg = config or ZIPFORMER_159M
    print(f"[reazonspeech_amd] WARNING: SEEDED SYNTHETIC weights of the {cfg.n_params() / 1e6:.0f}M Zipformer architecture were requested "
          f"(`config=` / `synthetic=True` / ${SYNTHETIC_ENV}): timings are valid, transcripts are meaningless.", file=sys.stderr, flush=True)
    sd = synthetic_state_dict_k2(cfg, seed)
    if quantized:
        from ...runtime.k2_weights import quantize_k2_linears, dequantize_k2_linears
        q = quantize_k2_linears(cfg, sd)
        return K2Model(cfg, dequantize_k2_linears(sd, q), synthetic_tokens(cfg.vocab_size, seed), device=device, precision="int8", qweights=q, **search)
    return K2Model(cfg, sd, synthetic_tokens(cfg.vocab_size, seed), device=device, precision=compute or "bf16", **search)
