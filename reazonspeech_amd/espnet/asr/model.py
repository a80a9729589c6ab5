"""The object `reazonspeech.espnet.asr.load_model()` returns here: the ESPnet2 Conformer-Transducer on one MI355X.

It stands where `espnet2.bin.asr_inference.Speech2Text` stands in the reference (pkg/espnet-asr/src/transcribe.py:26-32)
and answers the calls the reference makes on it:
    model(padded_samples)[0][0]            -> text of the best hypothesis            (transcribe.py:69)
    model.asr_model.blank_id / .token_list                                           (ctc.py:36,67)
    model.asr_model.encode(speech, length)[0], model.asr_model.ctc.softmax(enc)      (ctc.py:24-26)
    model.dtype, model.device                                                        (ctc.py:19-21)
so that the reference's own ctc.py runs against it unmodified (tests/test_espnet_host.py does exactly that); the package's
own code uses the direct forms `recognize` / `ctc_posteriors`.  Decoding on the device follows `beam_size` the way
[UPSTREAM] BeamSearchTransducer does: beam_size <= 1 is greedy_search (one symbol per frame), anything larger the "default"
beam search with score normalisation (k_rnnt_beam.hip) — the reference's setting is Speech2Text's default, beam_size 20
(transcribe.py:27-31 overrides only lm_weight)."""
import numpy as np
import torch

from ...runtime import fusion, k2_hotwords
from ...runtime import rescore as rescoring
from ...runtime.model import AsrModel

PADDING = (16000, 8000)          # transcribe.py:10
SEGMENTATION_MODES = ("host", "device")


class _Ctc:
    def __init__(self, owner):
        self._owner = owner

    def softmax(self, enc):
        """CTC.softmax(enc) of an `encode` result: the posteriors the same encoder pass produced"""
        if enc is not self._owner._last_enc:
            raise RuntimeError("ctc.softmax expects the tensor the last asr_model.encode call returned")
        return self._owner._last_ctc


class _AsrModelView:
    """the attributes of `Speech2Text.asr_model` the reference touches"""

    def __init__(self, owner):
        self._owner = owner
        self.blank_id = owner.cfg.blank_id
        self.token_list = owner.token_list
        self.ctc = _Ctc(owner)

    def encode(self, speech, length):
        o = self._owner
        wav = speech.detach().float().cpu().numpy().reshape(-1)[:int(length.reshape(-1)[0])]
        enc, probs = o._encode_with_ctc(wav)
        o._last_enc, o._last_ctc = enc, probs
        return enc, torch.tensor([enc.shape[1]], dtype=torch.long)


class _ScoredHypothesis:
    """4th element of an n-best entry with `token_scores` on: the ids and the log-probability of each"""

    def __init__(self, yseq, token_logprobs):
        self.yseq, self.token_logprobs = list(yseq), list(token_logprobs)


class _NBestHypothesis:
    """4th element of an n-best entry of a model loaded with `nbest=N`: [UPSTREAM] the fields of espnet2's transducer Hypothesis a
    caller of Speech2Text reads — `yseq` (the ids; upstream's leading blank is not repeated here) and `score` (the hypothesis's
    log-probability, not normalised; NaN for the one entry of a window the greedy search decoded, which keeps no score) — plus `norm_score` (score / len(yseq) counting that blank: what sort_nbest ranks by) and,
    with `token_scores` on, `token_logprobs` for entry 0 (None for the other entries)"""

    def __init__(self, yseq, score, norm_score, token_logprobs=None):
        self.yseq, self.score, self.norm_score = list(yseq), float(score), float(norm_score)
        self.token_logprobs = None if token_logprobs is None else list(token_logprobs)


class _RescoredHypothesis(_NBestHypothesis):
    """4th element of an n-best entry of a model loaded with `nbest=N, rescore=...`: an _NBestHypothesis with `log_likelihood` (log
    P(text | audio) over ALL alignments of yseq: include/rs_asr.h rs_rnnt_align_rows), `alignment_log_prob` (the best alignment's own
    score), `norm_log_likelihood` (log_likelihood / max(len(yseq), 1)) and `search_rank` (the entry's position in the search's own
    list); the list is in descending order of the chosen key.  With `token_scores` on EVERY entry has `token_logprobs`."""

    def __init__(self, yseq, score, norm_score, token_logprobs, log_likelihood, alignment_log_prob, search_rank):
        super().__init__(yseq, score, norm_score, token_logprobs)
        self.log_likelihood, self.alignment_log_prob, self.search_rank = float(log_likelihood), float(alignment_log_prob), int(search_rank)
        self.norm_log_likelihood = rescoring.norm(self.log_likelihood, len(self.yseq))


def check_nbest(nbest, beam_size):
    """the `nbest=` keyword of load_model / EspnetModel (upstream's Speech2Text(nbest=)): None or 1 with any search, 2..8 with the
    beam search and not above beam_size; ValueError with the reason otherwise.  -> the count the search is run with (0 = off)"""
    if nbest is None:
        return 0
    if not (isinstance(nbest, int) and not isinstance(nbest, bool) and 1 <= nbest <= 8):
        raise ValueError(f"nbest must be an integer in 1..8, not {nbest!r}")
    beam = 1 if beam_size is None else int(beam_size)
    if beam <= 1:
        if nbest > 1:
            raise ValueError(f"nbest={nbest} needs the beam search (beam_size > 1): greedy_search keeps one hypothesis")
        return 0
    if nbest > beam:
        raise ValueError(f"nbest={nbest} is above beam_size={beam}")
    return nbest


_SPACE = "\ue000"              # stands for '<space>' while a phrase is encoded (runtime/k2_hotwords.py encode drops real whitespace)


def check_fusion_keywords(beam_size, ngram_lm_model=None, ngram_lm_alpha=0.0, ngram_lm_tokens="pieces", hotwords_file="", hotwords_score=1.5):
    """the hotword and n-gram LM keywords of load_model / EspnetModel, checked before anything is loaded: ValueError for an alpha or
    a hotwords_score that is no finite number (alpha >= 0), an unknown token encoding, and — as the k2 package refuses them with
    greedy_search — an LM or a hotwords file with beam_size <= 1.  Needs no GPU."""
    search = "greedy_batch" if beam_size is None or int(beam_size) <= 1 else fusion.ESPNET.decoding
    for decoding in (None, search):          # every value is looked at before the search is: a bad score is told before an LM is refused
        fusion.check_lm_keywords(fusion.ESPNET, decoding, ngram_lm_model, ngram_lm_alpha, ngram_lm_tokens)
        fusion.check_hotword_keywords(fusion.ESPNET, decoding, hotwords_file, hotwords_score)


def lm_pieces(token_list, blank_id):
    """the word of an ARPA file that names token i with ngram_lm_tokens="pieces": the symbol of token_list as written there,
    '<space>' included.  '<blank>', '<unk>' and '<sos/eos>' name no token of an n-gram: the file's `<unk>` is the model's unknown-word
    entry, `<s>` its start state, and the search appends none of the three to a hypothesis."""
    special = {"<unk>", "<sos/eos>"}
    return [None if (i == blank_id or p in special) else p for i, p in enumerate(token_list)]


def encode_phrases(phrases, token_list, blank_id, hotwords_score=k2_hotwords.DEFAULT_SCORE):
    """[(phrase, own score)] (runtime/k2_hotwords.py parse_hotwords) -> [(token ids, score)] against an ESPnet character token list:
    one token per character; whitespace is '<space>' when the list has it and is dropped otherwise; a phrase with a character
    outside the list is skipped with the warning the k2 package gives"""
    tokens = list(token_list)
    unk_id = tokens.index("<unk>") if "<unk>" in tokens else -1
    if "<space>" in tokens:
        tokens[tokens.index("<space>")] = _SPACE
        phrases = [("".join(_SPACE if c.isspace() else c for c in body.strip()) if isinstance(body, str) else body, own) for body, own in phrases]
    return k2_hotwords.encode(phrases, tokens, blank_id, unk_id, hotwords_score)


class EspnetModel(fusion.ForwardedOptions):
    rule, lm_vocabulary = fusion.ESPNET, "token_list"
    hotwords = None                 # the model's HotwordGraph (None = no hotwords)
    hotwords_score = k2_hotwords.DEFAULT_SCORE

    def __init__(self, cfg, state_dict, token_list, device="cuda", beam_size=1, max_pops=0, precision="bf16", segmentation="host",
                 resample="host", token_scores=False, nbest=None, ngram_lm_model=None, ngram_lm_alpha=0.0, ngram_lm_tokens="pieces",
                 hotwords_file="", hotwords_score=1.5, rescore=None):
        """rescore: None (default), "likelihood" or "norm_likelihood", with nbest >= 2 and the beam search: every entry of the list of
        `model(speech)` / `recognize_batch(..., nbest=)` is scored by log P(text | audio) over ALL alignments on the device right
        after the search (include/rs_asr.h rs_rnnt_align_rows on the lists, the entries' common prefixes computed once):
        `hyp.log_likelihood`, `hyp.alignment_log_prob`, `hyp.norm_log_likelihood`, `hyp.search_rank`; the list is re-ranked by the key,
        descending, ties in the search's order, so `transcribe` follows the re-ranked best.  The list of one of a window the greedy
        fall-back decoded is scored too.  With token_scores every entry has `token_logprobs`.  Stored as `model.rescore`, settable.
        ngram_lm_model / ngram_lm_alpha / ngram_lm_tokens: shallow fusion of a backoff n-gram language model into the default beam
        search ([UPSTREAM] the `lm_weight * lm_scores` slot of default_beam_search, which the reference closes with lm_weight = 0;
        include/rs_asr.h rs_rnnt_beam_lm): an ARPA text file (`.gz` allowed) or an `NgramLm` of runtime/ngram_lm.py, its weight, and
        how a word of the file names a token: "pieces" (default) = the symbols of token_list, '<space>' included, "ids" = decimal
        ids.  Stored as `model.ngram_lm` / `model.ngram_lm_alpha`, both settable; alpha 0 = the search without the LM.
        hotwords_file / hotwords_score: contextual biasing from a phrase list (runtime/k2_hotwords.py for the file format: one phrase
        per line with an optional ` :score`; include/rs_asr.h rs_rnnt_beam_lm for what a hotword does); phrases are encoded per
        character against token_list.  The model's graph is `model.hotwords`; `model(speech, hotwords=...)` and
        `recognize_batch(..., hotwords=...)` take a call's own.  Both need beam_size > 1: with the greedy search they raise ValueError.
        nbest: upstream's `Speech2Text(nbest=N)`: `model(speech)` returns the N best hypotheses of the beam search — upstream's
        `sort_nbest(kept_hyps)[:nbest]`, ranked on the device (include/rs_asr.h rs_rnnt_beam_nbest) — as N tuples (text, tokens, ids,
        hyp) with `hyp.score` set; `recognize_batch(..., nbest=)` gives the same per window.  None (default): one tuple, as ever.
        N above beam_size, or N > 1 with beam_size <= 1, raises ValueError.  Stored as `model.nbest`.
        token_scores: the searches are followed by rs_rnnt_token_scores on the device; `recognize_batch_scored` and the 4th element
        of `model(speech)`'s n-best entry carry the log-probability of every token.  Stored as `model.token_scores`."""
        assert cfg.espnet and len(token_list) == cfg.vocab_size
        self.segmentation = segmentation
        n_best = check_nbest(nbest, beam_size)
        rescoring.check(rescore, n_best, beam_size is not None and int(beam_size) > 1)
        check_fusion_keywords(beam_size, ngram_lm_model, ngram_lm_alpha, ngram_lm_tokens, hotwords_file, hotwords_score)
        if beam_size is not None and int(beam_size) > 1:
            cfg = cfg.with_(decoding="beam", beam_size=int(beam_size), beam_score_norm=True, beam_max_pops=int(max_pops))
        self.beam_size = cfg.beam_size if cfg.decoding == "beam" else 1
        self.cfg = cfg
        self.token_list = list(token_list)
        self.am = AsrModel(cfg, state_dict, None, device=device, pad_seconds=0.0, precision=precision, resample=resample, token_scores=token_scores,
                           nbest=n_best, rescore=rescore)
        self.device = self.am.device
        self.dtype = "float32"
        self._last_enc = self._last_ctc = None
        self.asr_model = _AsrModelView(self)
        self.hotwords_score = float(hotwords_score)
        self.hotwords = self.hotword_graph(None, hotwords_file)          # the model's graph (None = no hotwords)
        if self.hotwords is not None:
            self.am.hotword_set((self.hotwords,))         # checked (rs_hotwords_check) and uploaded once, at load
        self.ngram_lm_alpha = ngram_lm_alpha
        if fusion.given(ngram_lm_model):
            self.ngram_lm = fusion.model_lm(fusion.ESPNET, cfg, self.token_list, ngram_lm_model, ngram_lm_tokens)

    # ---- hotwords and the n-gram LM ------------------------------------------------------------------------------------
    def hotword_graph(self, hotwords, hotwords_file=""):
        """a hotwords argument (a string of phrases separated by `/`, or a list; each phrase with an optional ` :score`; or a
        HotwordGraph) -> its HotwordGraph, None for nothing; phrases without a score of their own take the model's hotwords_score"""
        if isinstance(hotwords, k2_hotwords.HotwordGraph):
            graph = hotwords
        else:
            phrases = (k2_hotwords.read_hotwords_file(hotwords_file) if hotwords_file else []) + k2_hotwords.parse_hotwords(hotwords)
            graph = k2_hotwords.build_graph(encode_phrases(phrases, self.token_list, self.cfg.blank_id, self.hotwords_score))
        return fusion.check_graph(fusion.ESPNET, self.cfg, graph)

    def call_graphs(self, hotwords, n):
        """the `hotwords=` of a call over n windows -> one HotwordGraph or None per window, or None when no window has one.  None =
        the model's graph for every window; a string (phrases separated by `/`) or a HotwordGraph = that one for every window,
        INSTEAD OF the model's; a list = one entry per window, each a string, a list of phrases, a HotwordGraph or None (= the
        model's)."""
        if isinstance(hotwords, k2_hotwords.HotwordGraph):
            hotwords = [hotwords] * n
        return fusion.per_item(fusion.ESPNET, hotwords, n, self.hotwords, self.hotword_graph, "window")

    def call_lm(self, ngram_lm_alpha):
        """the `ngram_lm_alpha=` of a call -> what AsrModel.stage takes: None = the model's LM at the model's weight, else (NgramLm or
        None, alpha); 0 = this call without the LM; a value with no LM loaded raises ValueError"""
        return None if ngram_lm_alpha is None else (self.ngram_lm, fusion.given_alpha(self, ngram_lm_alpha))

    # ---- the reference's call forms -------------------------------------------------------------------------------
    def __call__(self, speech, hotwords=None, ngram_lm_alpha=None):
        """Speech2Text.__call__: n-best list of (text, tokens, token ids, hypothesis): one entry (upstream's default), or
        `model.nbest` of them from a model loaded with `nbest=N`.  `hotwords`: this call's phrases instead of the model's (a string of
        phrases separated by `/`, a list of phrases, or a HotwordGraph); `ngram_lm_alpha`: the LM's weight in this call (None = `model.ngram_lm_alpha`, 0 = without the LM)."""
        wav = np.asarray(speech.detach().cpu().numpy() if isinstance(speech, torch.Tensor) else speech, dtype=np.float32).reshape(-1)
        res = self._search([wav], hotwords=self.call_graphs(None if hotwords is None else [hotwords], 1), ngram_lm=self.call_lm(ngram_lm_alpha))
        if res.nbest is not None:
            return self._nbest_entries(res, 0)
        ids = res.ids[0]
        tokens = [self.token_list[i] for i in ids]
        hyp = _ScoredHypothesis(ids, res.token_logprobs[0]) if res.token_logprobs is not None else None
        return [(self.tokens2text(tokens), tokens, ids, hyp)]

    # ---- direct forms -----------------------------------------------------------------------------------------------
    @staticmethod
    def tokens2text(tokens):
        """[UPSTREAM] espnet2 CharTokenizer.tokens2text (token_type: char): '<space>' stands for ' ', the rest joins as is"""
        return "".join(" " if t == "<space>" else t for t in tokens)

    def ids_to_text(self, ids):
        return self.tokens2text([self.token_list[i] for i in ids])

    def _nbest_entries(self, res, b):
        """window b of a search that ran with lists -> [(text, tokens, ids, hyp)], best first; a window the greedy fall-back decoded
        has the one entry"""
        out = []
        rescored = getattr(res, "rescored", None)
        for r, (ids, _, score, norm) in enumerate(res.nbest[b]):
            tokens = [self.token_list[i] for i in ids]
            if rescored is not None:
                ll, best, lp = rescored[b][r]
                hyp = _RescoredHypothesis(ids, score, norm, lp, ll, best, r)
            else:
                lp = res.token_logprobs[b] if res.token_logprobs is not None and r == 0 else None
                hyp = _NBestHypothesis(ids, score, norm, lp)
            out.append((self.tokens2text(tokens), tokens, ids, hyp))
        if rescored is not None:                           # re-ranked by full likelihood; ties keep the search's order
            order = rescoring.order([e[3].log_likelihood for e in out], [len(e[2]) for e in out], self.am.rescore)
            out = [out[r] for r in order]
        return out

    def _best(self, res):
        """per window (ids, token log-probabilities or None) of the hypothesis a search returns: the search's own best — or, when the
        lists were rescored (`model.rescore`), the re-ranked best, so that `recognize_batch`, `recognize_batch_scored` and with them
        `transcribe_batch` give what `model(speech)[0]` and `transcribe` give"""
        lp = res.token_logprobs
        out = [(ids, lp[b] if lp is not None else None) for b, ids in enumerate(res.ids)]
        if getattr(res, "rescored", None) is not None:
            for b in range(len(out)):
                entries = self._nbest_entries(res, b)
                if entries:
                    out[b] = (entries[0][2], entries[0][3].token_logprobs if lp is not None else None)
        return out

    def recognize_batch(self, waves, isolate_overflow=False, nbest=None, hotwords=None, ngram_lm_alpha=None, rescore=None):
        """padded like the reference pads each window (np.pad(samples, PADDING), transcribe.py:69) -> [text].
        `isolate_overflow`: see `_search`.  `nbest=N`: per window the list of `model(speech)` instead — N tuples (text, tokens, ids,
        hyp), best first (one where the greedy fall-back decoded the window).  `hotwords`: one spec for every window (a string) or
        a list with one entry per window (see `call_graphs`); `ngram_lm_alpha`: the LM's weight in this call (0 = without the LM).
        `rescore`: n-best rescoring in this call: None = `model.rescore`, False = without it, a key = the lists of this call
        re-ranked by it (ValueError for lists shorter than two)."""
        if rescore is not None:                            # `model.rescore` for the call's duration
            plan = self.am.rescore_plan(rescore, check_nbest(nbest, self.beam_size) if nbest is not None else None)
            own, self.am.rescore = self.am.rescore, plan   # (a refused value raised above: the model's own option stays)
            try:
                return self.recognize_batch(waves, isolate_overflow, nbest, hotwords, ngram_lm_alpha)
            finally:
                self.am.rescore = own
        padded = [np.pad(np.asarray(w, np.float32), PADDING, mode="constant") for w in waves]
        fused = dict(hotwords=self.call_graphs(hotwords, len(padded)), ngram_lm=self.call_lm(ngram_lm_alpha))
        if nbest is None:
            return [self.ids_to_text(ids) for ids, _ in self._best(self._search(padded, isolate_overflow=isolate_overflow, **fused))]
        res = self._search(padded, isolate_overflow=isolate_overflow, nbest=check_nbest(nbest, self.beam_size) or 1, **fused)
        return [self._nbest_entries(res, b) for b in range(len(padded))]

    def recognize_batch_scored(self, waves, isolate_overflow=False, hotwords=None, ngram_lm_alpha=None):
        """`recognize_batch` of a model with `token_scores` on -> ([text], [(token ids, log-probabilities)]); the log-probabilities
        are the model's own, without hotword bonus or LM term"""
        res = self._search([np.pad(np.asarray(w, np.float32), PADDING, mode="constant") for w in waves], isolate_overflow=isolate_overflow,
                           hotwords=self.call_graphs(hotwords, len(waves)), ngram_lm=self.call_lm(ngram_lm_alpha))
        if res.token_logprobs is None:
            raise ValueError("recognize_batch_scored needs token_scores=True")
        best = self._best(res)
        return [self.ids_to_text(ids) for ids, _ in best], best

    def _search(self, waves, max_batch=256, isolate_overflow=False, nbest=None, hotwords=None, ngram_lm=None):
        """the transducer search over a batch of (padded) windows.  Upstream's default beam search has no bound on the
        prediction-network evaluations a frame may take; the device search has one (`max_pops`, which sizes its workspace)
        and reports RS_EOVERFLOW instead of truncating.  The front end and the encoder run ONCE per batch; a decode that hits
        the bound is retried on the same joint projection with 4x and 16x the bound, then done greedily with a warning — one
        pathological window must not abort a whole file — and the result says so (`DecodedBatch.degraded`).  The overrides are
        arguments of the decode call: nothing is written into the shared model configuration.

        `isolate_overflow` (default off: a chunk that still overflows turns greedy as a whole): the windows of such a chunk are
        decoded again one by one, each with the retry ladder above, so that only the window that overflows turns greedy and its
        chunk-mates keep the beam search's result — what a caller that pools unrelated windows into one chunk needs to return
        what the window-by-window path returns.

        `nbest`: entries per window for this call (None = `model.nbest`).  With lists on, `DecodedBatch.nbest` holds every window's;
        the retry ladder is the same, and a window the greedy fall-back decoded has a list of one (score NaN: the greedy search
        keeps none) and `degraded`.

        `hotwords`: None, or one HotwordGraph / None per window (`call_graphs`); `ngram_lm`: None = the model's LM and weight, or
        (NgramLm or None, alpha) for this call (`call_lm`).  Positive bonuses can make a frame take more pops: the ladder is the same,
        and the greedy fall-back runs without either and stays flagged `degraded`."""
        from ...runtime.capi import RsError, RS_EOVERFLOW
        from ...runtime.model import DecodedBatch, RescoredBatch
        am = self.am
        n_best = am.nbest if nbest is None else nbest
        rescoring_on = am.cfg.decoding == "beam" and am.rescore_plan(None, n_best) is not None
        if am.cfg.decoding != "beam":
            res = am.transcribe_waveforms(waves)
            if n_best:                                    # (nbest = 1 with the greedy search: the one hypothesis as a list)
                res.nbest = [[(ids, fr, float("nan"), float("nan"))] for ids, fr in zip(res.ids, res.frames)]
            return res
        bound = am.cfg.beam_max_pops or 16 * am.cfg.beam_size
        out = DecodedBatch([], [], [], [], [], token_logprobs=[] if am.token_scores else None, nbest=[] if n_best else None)
        if rescoring_on:
            out = RescoredBatch([], [], [], [], [], token_logprobs=out.token_logprobs, nbest=[], rescored=[])
        for lo in range(0, len(waves), max_batch):
            graphs = None if hotwords is None else list(hotwords[lo:lo + max_batch])
            buf = am.stage([np.asarray(w, np.float32) for w in waves[lo:lo + max_batch]], nbest=n_best,
                           hotwords=am.graph_plan(graphs, len(graphs)) if graphs is not None else None, ngram_lm=ngram_lm)
            with torch.cuda.device(am.device):
                stream = torch.cuda.current_stream().cuda_stream
                am.run_encoder(buf, stream)
                used = None
                for factor in (1, 4, 16):
                    try:
                        am.decode(am.ctx, buf, buf.ws, stream, max_pops=bound * factor)
                        used = "beam"
                        break
                    except RsError as e:
                        if e.code != RS_EOVERFLOW:
                            raise
                if used is None and isolate_overflow and buf.B > 1:
                    for k, w in enumerate(waves[lo:lo + max_batch]):
                        one = self._search([w], max_batch=1, nbest=n_best, hotwords=None if graphs is None else [graphs[k]], ngram_lm=ngram_lm)
                        out.ids += one.ids; out.frames += one.frames; out.enc_lens += one.enc_lens
                        out.scores += one.scores; out.degraded += one.degraded
                        if out.nbest is not None:
                            out.nbest += one.nbest
                        if out.token_logprobs is not None:
                            out.token_logprobs += one.token_logprobs
                        if rescoring_on:
                            out.rescored += one.rescored
                    continue
                if used is None:
                    import warnings
                    warnings.warn(f"beam search: a frame needed more than {16 * bound} prediction-network evaluations; this batch of windows "
                                  "is decoded with the greedy search instead", RuntimeWarning, stacklevel=3)
                    am.decode(am.ctx, buf, buf.ws, stream, decoding="greedy_batch")
                    used = "greedy_batch"
                am.score(am.ctx, buf, stream, decoding=used)
                if rescoring_on:                          # (the greedy fall-back's list of one is scored too)
                    am.rescore_step(am.ctx, buf, stream, decoding=used, single=True)
                res = am.collect(buf, decoding=used)
            out.ids += res.ids; out.frames += res.frames; out.enc_lens += res.enc_lens
            out.scores += res.scores if res.scores is not None else [float("nan")] * buf.B
            out.degraded += [used != "beam"] * buf.B
            if out.token_logprobs is not None:
                out.token_logprobs += res.token_logprobs
            if out.nbest is not None:                     # (the greedy fall-back ran without lists: its one hypothesis each)
                out.nbest += res.nbest if res.nbest is not None else [[(ids, fr, float("nan"), float("nan"))] for ids, fr in zip(res.ids, res.frames)]
            if rescoring_on:
                out.rescored += res.rescored
        return out

    def recognize(self, samples):
        return self.recognize_batch([samples])[0]

    def _encode_with_ctc(self, wav):
        am = self.am
        buf = am.stage([np.asarray(wav, np.float32)])
        M = buf.B * buf.tp_max
        vp = (self.cfg.n_logits + 3) // 4 * 4      # row pitch of the posteriors (include/rs_asr.h: rs_encoder_set_ctc_out)
        probs = torch.empty((M, vp), dtype=torch.float32, device=am.device)
        enc = torch.empty((buf.B, buf.tp_max, self.cfg.d_model), dtype=torch.float32, device=am.device)
        with torch.cuda.device(am.device):
            stream = torch.cuda.current_stream().cuda_stream
            am.ctx.set_ctc_out(probs, None)
            try:
                am.ctx.frontend(buf.audio, buf.lens, 0, 0, buf.t_max, buf.feats, buf.n_frames, buf.ws, stream)
                am.ctx.encoder(buf.feats, buf.n_frames, buf.B, buf.t_max, enc, buf.joint_enc, buf.enc_lens, buf.ws, stream)
            finally:
                am.ctx.set_ctc_out(None, None)
            torch.cuda.synchronize(am.device)
        n = int(buf.enc_lens.cpu()[0])
        return enc[:, :n].cpu(), probs.view(buf.B, buf.tp_max, vp)[:, :n, :self.cfg.n_logits].contiguous().cpu()

    def ctc_posteriors(self, samples):
        """softmax(ctc_lo(encoder(samples))) as float32 numpy [T'][vocab] (ctc.py:12-27 — no padding)"""
        return self._encode_with_ctc(samples)[1][0].numpy()

    # ---- segmentation = "device" -------------------------------------------------------------------------------------
    @property
    def segmentation(self):
        """where the time stamps of a recognised text are computed: "host" = one encoder pass and one run of the numpy aligner
        per window (ctc.get_timings); "device" = one encoder pass and one rs_ctc_align launch per batch (`align_batch`), and the
        blank finder reads only the blank column.  Same results; may be changed at any time."""
        return self._segmentation

    @segmentation.setter
    def segmentation(self, value):
        if value not in SEGMENTATION_MODES:
            raise ValueError(f"segmentation must be one of {SEGMENTATION_MODES}, got {value!r}")
        self._segmentation = value

    def blank_posteriors(self, samples):
        """the blank column of `ctc_posteriors(samples)`, float32 numpy [T']: only that column leaves the device"""
        am = self.am
        buf = am.stage([np.asarray(samples, np.float32)])
        col = torch.empty((buf.B * buf.tp_max,), dtype=torch.float32, device=am.device)
        with torch.cuda.device(am.device):
            stream = torch.cuda.current_stream().cuda_stream
            am.ctx.set_ctc_out(None, col)
            try:
                am.ctx.frontend(buf.audio, buf.lens, 0, 0, buf.t_max, buf.feats, buf.n_frames, buf.ws, stream)
                am.ctx.encoder(buf.feats, buf.n_frames, buf.B, buf.t_max, None, buf.joint_enc, buf.enc_lens, buf.ws, stream)
            finally:
                am.ctx.set_ctc_out(None, None)
            n = int(buf.enc_lens.cpu()[0])
            return col[:n].cpu().numpy()

    def _blank_pass(self, buf, col, stream):
        """front-end + encoder of a staged batch with only the blank column registered (asynchronous on `stream`)"""
        am = self.am
        am.ctx.set_ctc_out(None, col)
        try:
            am.ctx.frontend(buf.audio, buf.lens, 0, 0, buf.t_max, buf.feats, buf.n_frames, buf.ws, stream)
            am.ctx.encoder(buf.feats, buf.n_frames, buf.B, buf.t_max, None, buf.joint_enc, buf.enc_lens, buf.ws, stream)
        finally:
            am.ctx.set_ctc_out(None, None)

    def find_blank_batch(self, windows, threshold=0.98, max_batch=256):
        """`ctc.find_blank(self, windows[i], threshold)` for a batch of windows -> [Blank].  Per chunk of `max_batch` windows:
        ONE front-end + encoder pass with the blank column kept on the device, one rs_ctc_find_blank launch, and only the cut
        points (B x 2 int32) copied back."""
        from .ctc import Blank
        am = self.am
        out = []
        for lo in range(0, len(windows), max_batch):
            chunk = [np.asarray(w, np.float32) for w in windows[lo:lo + max_batch]]
            buf = am.stage(chunk)
            B = buf.B
            with torch.cuda.device(am.device):
                stream = torch.cuda.current_stream().cuda_stream
                col = torch.empty((B * buf.tp_max,), dtype=torch.float32, device=am.device)
                cuts = torch.empty((B, 2), dtype=torch.int32, device=am.device)
                self._blank_pass(buf, col, stream)
                am.ctx.ctc_find_blank(col, buf.enc_lens, buf.lens, B, buf.tp_max, threshold, cuts, stream)
                cuts = cuts.cpu().numpy()
            out += [Blank(int(s), int(e)) for s, e in cuts]
        return out

    def align_batch(self, waves, texts, max_batch=256):
        """`ctc.get_timings(self, waves[i], texts[i])` for a batch: -> [float64 array, one sample position per kept character of
        the text, or None where the host path raises (more symbols than frames, ...)].  Per chunk of `max_batch` windows: ONE
        front-end + encoder pass over the un-padded windows with the posteriors kept on the device, the ground truths packed on
        the host while it runs, one rs_ctc_align launch, and only the frame indices and the status words copied back."""
        from . import ctc_segmentation
        assert len(waves) == len(texts)
        am, cfg = self.am, self.cfg
        params = ctc_segmentation.CtcSegmentationParameters(char_list=self.token_list[:-1])     # as ctc.get_timings
        vp = (cfg.n_logits + 3) // 4 * 4            # row pitch of the posteriors (include/rs_asr.h: rs_encoder_set_ctc_out)
        out = []
        for lo in range(0, len(waves), max_batch):
            chunk = [np.asarray(w, np.float32) for w in waves[lo:lo + max_batch]]
            buf = am.stage(chunk)
            B = buf.B
            with torch.cuda.device(am.device):
                stream = torch.cuda.current_stream().cuda_stream
                probs = torch.empty((B * buf.tp_max, vp), dtype=torch.float32, device=am.device)
                am.ctx.set_ctc_out(probs, None)
                try:
                    am.ctx.frontend(buf.audio, buf.lens, 0, 0, buf.t_max, buf.feats, buf.n_frames, buf.ws, stream)
                    am.ctx.encoder(buf.feats, buf.n_frames, B, buf.t_max, None, buf.joint_enc, buf.enc_lens, buf.ws, stream)
                finally:
                    am.ctx.set_ctc_out(None, None)
                # (the launches above are asynchronous: the packing below runs on the host while the encoder runs)
                gt, gt_lens, bounds = ctc_segmentation.pack_ground_truth(params, texts[lo:lo + max_batch])
                c_max, S = gt.shape[1], gt.shape[2]
                if S > 8:
                    raise ValueError(f"segmentation='device' aligns token lists whose longest token has at most 8 characters, got {S}")
                d_gt = torch.from_numpy(gt).to(am.device, non_blocking=True)
                d_len = torch.from_numpy(gt_lens).to(am.device, non_blocking=True)
                frames = torch.empty((B, c_max), dtype=torch.int32, device=am.device)
                status = torch.empty((B,), dtype=torch.int32, device=am.device)
                ws = torch.empty((am.ctx.ctc_align_workspace_bytes(B, buf.tp_max, c_max, S),), dtype=torch.uint8, device=am.device)
                am.ctx.ctc_align(probs, buf.enc_lens, B, buf.tp_max, d_gt, d_len, params.blank, frames, status, ws, stream)
                frames, status, enc_lens = frames.cpu().numpy(), status.cpu().numpy(), buf.enc_lens.cpu().numpy()
            for b, w in enumerate(chunk):
                if status[b] != 0:
                    out.append(None)
                    continue
                index_duration = len(w) / (int(enc_lens[b]) + 1)
                per_symbol = frames[b, :gt_lens[b]].astype(np.float64) * index_duration
                out.append(per_symbol[bounds[b][0] + 1:bounds[b][1]])
        return out


def synthetic_token_list(vocab_size: int, seed: int = 0):
    """An ESPnet-style character token list for synthetic-weight runs: '<blank>', '<unk>', punctuation the segmenter looks
    for (ctc.py:6-8), kana / kanji, '<sos/eos>' last ([UPSTREAM] ESPnet2 token_list layout, token_type: char)."""
    fixed = ["<blank>", "<unk>", "。", "、", "?", "!", ","]
    pool = [chr(c) for c in range(0x3041, 0x3097)] + [chr(c) for c in range(0x30A1, 0x30FB)] + [chr(c) for c in range(0x4E00, 0x4E00 + 8192)]
    rng = np.random.default_rng(seed)
    rng.shuffle(pool)
    body = pool[:max(0, vocab_size - len(fixed) - 1)]
    toks = (fixed + body)[:vocab_size - 1] + ["<sos/eos>"]
    assert len(toks) == vocab_size and len(set(toks)) == vocab_size
    return toks
