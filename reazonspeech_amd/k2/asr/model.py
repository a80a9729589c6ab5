"""The object `reazonspeech.k2.asr.load_model()` returns here: icefall's Zipformer2 transducer on one MI355X.

It stands where `sherpa_onnx.OfflineRecognizer` stands in the reference (pkg/k2-asr/src/huggingface.py:73-83) and answers the
calls the reference makes on it (transcribe.py:36-45):
    stream = model.create_stream(); stream.accept_waveform(samplerate, waveform); model.decode_stream(stream)
    stream.result.tokens / .timestamps / .text
plus the batched form `decode_streams` (sherpa-onnx has it too) and the recognizer's hotwords: `hotwords_file=` / `hotwords_score=`
at construction, `create_stream(hotwords=...)` per utterance (runtime/k2_hotwords.py; the modified beam search only).  [UPSTREAM] conventions of sherpa-onnx's result conversion
(offline-recognizer-transducer-impl.h Convert, symbol-table.cc): a token's text is its tokens.txt symbol with a leading U+2581 replaced by
a space and `<0xNN>` byte tokens joined into UTF-8; text = the tokens concatenated; timestamp = frame index x 0.04 s."""
import re

import numpy as np

from ...runtime import fusion, k2_hotwords
from ...runtime import rescore as rescoring
from ...runtime.model import AsrModel

_BYTE = re.compile(r"^<0x([0-9A-Fa-f]{2})>$")


class _Result:
    def __init__(self, tokens, timestamps, text, token_ids=None, token_log_probs=None, log_prob=None, norm_log_prob=None, nbest=None):
        self.tokens, self.timestamps, self.text = tokens, timestamps, text
        # n-best (this project's addition: sherpa-onnx returns one hypothesis): `nbest` = the ranked results of the last set, each
        # with tokens / timestamps / text / log_prob (the hypothesis's total log-probability, hotword and LM terms inside) and
        # norm_log_prob (what they are ranked by); entry 0 is this result.  None unless the model was loaded with nbest=N.
        self.log_prob, self.norm_log_prob, self.nbest = log_prob, norm_log_prob, nbest
        # token_scores: the ids behind `tokens` and the log-probability of each ([UPSTREAM] sherpa-onnx keeps per-token log-probs in
        # its hypotheses); None with the option off
        self.token_ids, self.token_log_probs = token_ids, token_log_probs
        # rescore: log P(text | audio) over all alignments, the best alignment's score, the former / max(tokens, 1) and the position
        # in the search's own list — on every entry of `nbest`, which is then in descending order of the chosen key; None when off
        self.log_likelihood = self.alignment_log_prob = self.norm_log_likelihood = self.search_rank = None
        self.rescore_key = None          # the key the list was re-ranked by (also on a result whose list is empty), None when off


class _Stream:
    """sherpa_onnx.OfflineStream: holds one utterance's samples, then its result"""

    def __init__(self, hotwords=None):
        self.hotwords = hotwords          # HotwordGraph of this stream (it replaces the model's), None = the model's
        self.samples = np.zeros((0,), np.float32)
        self.sample_rate = 16000
        self.result = _Result([], [], "")

    def accept_waveform(self, sample_rate, waveform):
        self.sample_rate = int(sample_rate)
        self.samples = np.concatenate([self.samples, np.asarray(waveform, dtype=np.float32).reshape(-1)])


def read_tokens(path):
    """tokens.txt: one `symbol id` pair per line ([UPSTREAM] sherpa-onnx SymbolTable) -> list indexed by id"""
    table = {}
    with open(path, encoding="utf-8") as fp:
        for line in fp:
            line = line.rstrip("\n")
            if not line.strip():
                continue
            sym, _, idx = line.rpartition(" ")
            table[int(idx)] = sym if sym else " "
    return [table.get(i, "<unk>") for i in range(max(table) + 1)]


def synthetic_tokens(vocab_size, seed=0):
    """an icefall-style tokens.txt for synthetic-weight runs: <blk> 0, <sos/eos> 1, <unk> 2, then punctuation and characters"""
    fixed = ["<blk>", "<sos/eos>", "<unk>", "。", "、", "?", "!", "▁"]
    pool = [chr(c) for c in range(0x3041, 0x3097)] + [chr(c) for c in range(0x30A1, 0x30FB)] + [chr(c) for c in range(0x4E00, 0x4E00 + 16384)]
    rng = np.random.default_rng(seed)
    rng.shuffle(pool)
    toks = (fixed + pool)[:vocab_size]
    assert len(toks) == vocab_size and len(set(toks)) == vocab_size
    return toks


DECODING_METHODS = ("greedy_search", "modified_beam_search")      # sherpa-onnx's offline transducer methods


def search_config(cfg, decoding_method="greedy_search", max_active_paths=4, blank_penalty=0.0, hotwords_file="", hotwords_score=1.5,
                  hotwords=None, ngram_lm_model=None, ngram_lm_alpha=0.0, ngram_lm_tokens="pieces", nbest=0):
    """`cfg` with the search sherpa_onnx.OfflineRecognizer.from_transducer's keywords ask for (its names and defaults);
    ValueError for anything it does not have or this package does not run.  Needs no GPU.  The hotwords keywords are checked
    here (upstream refuses them with greedy_search too); the graph itself is the model's, not the configuration's.  So are the
    n-gram LM keywords (runtime/fusion.py: check_lm_keywords): an LM with greedy_search raises.  `nbest` (this project's
    addition, 0 = off) must be an integer in 0..8, at most max_active_paths, and above 1 needs the modified beam search."""
    if not (isinstance(nbest, int) and not isinstance(nbest, bool) and 0 <= nbest <= 8):
        raise ValueError(f"nbest must be an integer in 0..8, not {nbest!r}")
    if nbest > 1 and decoding_method == "greedy_search":
        raise ValueError(f"nbest={nbest} needs decoding_method='modified_beam_search' (greedy_search keeps one hypothesis)")
    # (a method this package does not have is refused in its turn, below: hotwords are refused with the greedy search only)
    fusion.check_hotword_keywords(fusion.K2, decoding_method if decoding_method in DECODING_METHODS else None, hotwords_file, hotwords_score, hotwords)
    if decoding_method not in DECODING_METHODS:
        raise ValueError(f"decoding_method must be 'greedy_search' or 'modified_beam_search', not {decoding_method!r}")
    fusion.check_lm_keywords(fusion.K2, decoding_method, ngram_lm_model, ngram_lm_alpha, ngram_lm_tokens)
    if not float(blank_penalty) >= 0.0:
        raise ValueError(f"blank_penalty must be >= 0, not {blank_penalty!r}")
    if decoding_method == "greedy_search":
        if float(blank_penalty) != 0.0:
            raise ValueError("blank_penalty applies to decoding_method='modified_beam_search' only")
        return cfg.with_(decoding="greedy_batch", beam_size=1, blank_penalty=0.0)
    if not (isinstance(max_active_paths, int) and 1 <= max_active_paths <= 8):
        raise ValueError(f"max_active_paths must be an integer in 1..8, not {max_active_paths!r}")
    if nbest > max_active_paths:
        raise ValueError(f"nbest={nbest} is above max_active_paths={max_active_paths}: the search keeps no more hypotheses than that")
    return cfg.with_(decoding="modified_beam_search", beam_size=int(max_active_paths), blank_penalty=float(blank_penalty))


def stream_graphs(model_graph, streams):
    """the graph each stream is decoded with: its own (create_stream(hotwords=...)) INSTEAD OF the model's, else the model's;
    None when no stream has one"""
    graphs = [st.hotwords if st.hotwords is not None else model_graph for st in streams]
    return graphs if any(g is not None for g in graphs) else None


class K2Model(fusion.ForwardedOptions):
    rule, lm_vocabulary = fusion.K2, "tokens"

    def __init__(self, cfg, state_dict, tokens, device="cuda", pad_seconds=0.0, precision="bf16", qweights=None,
                 decoding_method="greedy_search", max_active_paths=4, blank_penalty=0.0, pos_cap=None, resample="host",
                 hotwords_file="", hotwords_score=1.5, hotwords=None, token_scores=False, ngram_lm_model=None, ngram_lm_alpha=0.0,
                 ngram_lm_tokens="pieces", nbest=0, rescore=None):
        """rescore: None (default), "likelihood" or "norm_likelihood", with nbest >= 2 and the modified beam search: every entry of
        `stream.result.nbest` gets `log_likelihood` (log P(text | audio) over ALL alignments, one label per frame as the search
        moves; include/rs_asr.h rs_rnnt_align_rows on the lists, right after the search), `alignment_log_prob`,
        `norm_log_likelihood` and `search_rank`; the list is re-ranked by the key, descending, ties in the search's order, and
        `stream.result` is its new entry 0.  With token_scores every entry carries `token_log_probs`.  Stored as `model.rescore`,
        may be set later.  ValueError (before anything is loaded) for another value, greedy_search or nbest < 2.
        nbest: this project's addition (sherpa-onnx returns one hypothesis per stream): N >= 1 with the modified beam search makes
        `stream.result.nbest` the N best hypotheses of the search's last set, ranked on the device by log_prob / len(ys) as the
        winner is chosen (include/rs_asr.h rs_rnnt_mbs_nbest) — results with tokens / timestamps / text / log_prob / norm_log_prob,
        entry 0 the result itself, fewer than N when the last set is smaller.  0 (default): `result.nbest` is None.  N above
        max_active_paths, or N > 1 with greedy_search, raises ValueError.  With token_scores, entry 0 carries the token
        log-probabilities and the other entries None.
        ngram_lm_model / ngram_lm_alpha / ngram_lm_tokens: shallow fusion of a backoff n-gram language model into the modified beam
        search (include/rs_asr.h rs_rnnt_mbs_lm: the LM term is added to the K survivors of a frame, after the selection): an ARPA
        text file (`.gz` allowed) or an `NgramLm` of runtime/ngram_lm.py, its weight, and how a word of the file names a token:
        "pieces" (default) = the symbols of tokens.txt as written there, "ids" = decimal ids; "nemo" raises ValueError.  Stored as
        `model.ngram_lm` / `model.ngram_lm_alpha`, both settable; alpha 0 = the search without the LM.  With greedy_search an LM
        raises ValueError.  The table is checked (rs_ngram_check) and uploaded once, here.
        token_scores: `stream.result.token_log_probs` (and `.token_ids`) are filled: the log-probability of every token under the
        model's own distribution (no blank penalty, no hotword bonus), computed on the device right after the search
        (rs_rnnt_token_scores); valid with every precision and decoding method.  Stored as `model.token_scores`, may be changed later.
        hotwords_file / hotwords_score: sherpa-onnx's keywords and defaults (contextual biasing of the modified beam search:
        runtime/k2_hotwords.py for the file format, include/rs_asr.h rs_rnnt_mbs_hotwords for what a hotword does); `hotwords` = the
        same as an in-memory list (strings "phrase" / "phrase :2.0", or token-id sequences).  The model's graph is built and
        uploaded once here; with greedy_search they raise ValueError.
        decoding_method / max_active_paths / blank_penalty: sherpa_onnx.OfflineRecognizer.from_transducer's keywords with its
        defaults (pkg/k2-asr/src/huggingface.py:73-83 passes "greedy_search"): "modified_beam_search" keeps max_active_paths (1..8)
        hypotheses per utterance (csrc/k_rnnt_mbs.hip, rs_rnnt_mbs); valid with every precision — the search only consumes the
        encoder projection.  Anything else raises ValueError.
        precision: "bf16" = the throughput mode; "fp32" = float32 weights, activations and arithmetic end to end (what
        onnxruntime computes from the reference's default float32 graphs: pkg/k2-asr/src/huggingface.py:16,40-45); "fp32x3" = the
        float32 mode with three-term bf16 products; "int8" = onnxruntime's int8 graph restated (the "int8" / "int8-fp32" files):
        the float32 mode with every Linear of `qweights` ({icefall name: (Wq int8 [out][in], sw, zw)}: read_k2_onnx_quantized or
        quantize_k2_linears) as a dynamically quantized MatMul, scales per utterance; `state_dict` then holds the dequantized weights
        resample: "host" / "device": where `transcribe` / `transcribe_batch` normalise their input (runtime/resample.py)
        pos_cap: rows of relative positions the resident position tables start with (|rel| < pos_cap; None = the runtime's default);
        a longer utterance grows them (AsrModel.ensure_pos_cap), so this only moves the first growth"""
        assert cfg.family == "k2" and len(tokens) == cfg.vocab_size
        cfg = search_config(cfg, decoding_method, max_active_paths, blank_penalty, hotwords_file, hotwords_score, hotwords,
                            ngram_lm_model, ngram_lm_alpha, ngram_lm_tokens, nbest)
        rescoring.check(rescore, nbest, cfg.decoding == "modified_beam_search")
        self.cfg = cfg
        self.tokens = list(tokens)
        self.hotwords_score = float(hotwords_score)
        self.hotwords = self.hotword_graph(hotwords, hotwords_file)       # the model's graph (None = no hotwords)
        # the reference pads with np.pad before handing the samples over (transcribe.py:24); a stream's samples arrive padded
        cap = {} if pos_cap is None else {"pos_cap": int(pos_cap)}
        self.am = AsrModel(cfg, state_dict, None, device=device, pad_seconds=pad_seconds, precision=precision, qweights=qweights, resample=resample, token_scores=token_scores,
                           nbest=nbest if cfg.decoding == "modified_beam_search" else 0, rescore=rescore, **cap)
        self.device = self.am.device
        if self.hotwords is not None:
            self.am.hotword_set((self.hotwords,))         # checked and uploaded once, at load
        self.ngram_lm_alpha = ngram_lm_alpha
        if fusion.given(ngram_lm_model):
            self.ngram_lm = fusion.model_lm(fusion.K2, cfg, self.tokens, ngram_lm_model, ngram_lm_tokens)

    def hotword_graph(self, hotwords, hotwords_file=""):
        """a hotwords argument (a string of phrases separated by `/`, or a list; each phrase with an optional ` :score`) -> its
        HotwordGraph, None for nothing; phrases without a score of their own take the model's hotwords_score"""
        if isinstance(hotwords, k2_hotwords.HotwordGraph):
            return hotwords
        graph = k2_hotwords.make_graph(hotwords, self.tokens, self.cfg.blank_id, self.cfg.unk_id, self.hotwords_score, hotwords_file)
        return fusion.check_graph(fusion.K2, self.cfg, graph)

    # entries of `stream.result.nbest` (0 = off): the runtime model's option, settable
    @fusion.ForwardedOptions.nbest.setter
    def nbest(self, n):
        self.am.nbest = self.am.nbest_plan(n)

    # ---- sherpa-onnx's surface ------------------------------------------------------------------------------------------
    def create_stream(self, hotwords=None):
        """hotwords: sherpa-onnx's per-stream hotwords — a string of phrases separated by `/` (or a list), each with an optional
        ` :score`; the stream is then decoded with ITS graph instead of the model's"""
        return _Stream(self.hotword_graph(hotwords))

    def decode_stream(self, stream):
        self.decode_streams([stream])

    def decode_streams(self, streams, ngram_lm_alpha=None):
        """ngram_lm_alpha: the weight of the model's n-gram LM in this call (None = `model.ngram_lm_alpha`, 0 = without the LM)"""
        lm = None if ngram_lm_alpha is None else fusion.call_alpha(fusion.K2, self, ngram_lm_alpha)
        for st in streams:
            if st.sample_rate != self.cfg.sample_rate:
                raise ValueError(f"sample rate {st.sample_rate}: the model expects {self.cfg.sample_rate} Hz (sherpa-onnx resamples; resample with norm_audio first)")
        res = self.am.transcribe_waveforms([st.samples for st in streams], hotwords=stream_graphs(self.hotwords, streams), ngram_lm=lm)
        for k, (st, ids, frames) in enumerate(zip(streams, res.ids, res.frames)):
            st.result = self.convert(ids, frames, res.token_logprobs[k] if res.token_logprobs is not None else None)
            if getattr(res, "rescored", None) is not None and not res.nbest[k]:  # no hypothesis was ranked: an empty list of the same kind
                st.result.nbest, st.result.rescore_key = [], self.am.rescore
            elif getattr(res, "rescored", None) is not None:                     # the list re-ranked by full likelihood
                entries = [self.convert(y, fr, lp) for (y, fr, _, _), (_, _, lp) in zip(res.nbest[k], res.rescored[k])]
                for rank, (r, (y, _, lp, norm), (ll, best, _)) in enumerate(zip(entries, res.nbest[k], res.rescored[k])):
                    r.log_prob, r.norm_log_prob, r.search_rank = lp, norm, rank
                    r.log_likelihood, r.alignment_log_prob, r.norm_log_likelihood = ll, best, rescoring.norm(ll, len(y))
                order = rescoring.order([r.log_likelihood for r in entries], [len(y) for y, _, _, _ in res.nbest[k]], self.am.rescore)
                st.result = entries[order[0]]
                st.result.nbest, st.result.rescore_key = [entries[r] for r in order], self.am.rescore
            elif res.nbest is not None:                   # the ranked list; entry 0 is the result itself
                entries = [self.convert(y, fr) for y, fr, _, _ in res.nbest[k][1:]]
                for r, (_, _, lp, norm) in zip([st.result] + entries, res.nbest[k]):
                    r.log_prob, r.norm_log_prob = lp, norm
                st.result.nbest = ([st.result] + entries) if res.nbest[k] else []

    # ---- result conversion ------------------------------------------------------------------------------------------------
    def symbol(self, i):
        """[UPSTREAM] sherpa-onnx SymbolTable: only a LEADING U+2581 (the SentencePiece word boundary) becomes a space"""
        s = self.tokens[i]
        return " " + s[1:] if s.startswith("▁") else s

    def convert(self, ids, frames, logprobs=None):
        syms = [self.symbol(i) for i in ids]
        # byte-fallback pieces (<0xE3> ...) join into UTF-8 text; the token list keeps them as they are
        out, pending = [], bytearray()
        for s in syms:
            m = _BYTE.match(s)
            if m:
                pending.append(int(m.group(1), 16))
                continue
            if pending:
                out.append(pending.decode("utf-8", errors="replace"))
                pending = bytearray()
            out.append(s)
        if pending:
            out.append(pending.decode("utf-8", errors="replace"))
        step = self.cfg.seconds_per_frame()
        scored = {} if logprobs is None else dict(token_ids=list(ids), token_log_probs=list(logprobs))
        return _Result(syms, [float(np.float32(step * t)) for t in frames], "".join(out), **scored)
