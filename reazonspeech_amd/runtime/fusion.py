"""The host side of the two search options the three packages share — hotwords (contextual biasing, runtime/k2_hotwords.py) and
n-gram LM shallow fusion (runtime/ngram_lm.py): which decoding of which family can fuse them and in which words the others are
refused, stated ONCE per family (`Rule`: NEMO, K2, ESPNET), and the keyword checks, the model's LM, a call's weight and a call's
graphs as one function each that takes the rule.  Needs no GPU.

What stays with its family: how phrases become token ids (nemo_hotwords.encode, k2_hotwords.encode, espnet's encode_phrases), how a
vocabulary names the words of an ARPA file (`Rule.pieces`), and the order in which a loader runs these checks."""
import os
from typing import Callable, NamedTuple

import numpy as np

from . import ngram_lm
from .k2_hotwords import DEFAULT_SCORE, HotwordGraph


def _nemo_pieces(cfg, tokenizer):
    return tokenizer.ids_to_tokens(range(cfg.vocab_size))


def _k2_pieces(cfg, tokens):
    # the file's `<unk>` is the model's unknown-word entry, never a token of an n-gram: tokens.txt's own <unk> symbol names no id here
    return [None if i == cfg.unk_id else p for i, p in enumerate(list(tokens)[:cfg.vocab_size])]


def _espnet_pieces(cfg, token_list):
    from ..espnet.asr.model import lm_pieces
    return lm_pieces(token_list, cfg.blank_id)


class Rule(NamedTuple):
    """one family's answers.  The refusals are `str.format` templates over the repr of the decoding that was asked for."""
    family: str
    decoding: str                   # the one decoding of the family whose search has a hotword and an LM form
    token_modes: tuple              # the `ngram_lm_tokens` the package reads ...
    default_tokens: str             # ... and the one it reads when none is given
    tokens_note: str                # what the refusal of an unknown `ngram_lm_tokens` adds
    foreign_tokens: tuple           # ((mode, refusal), ...): modes of ANOTHER package, refused in words of their own
    lm_refusal: str                 # an LM / hotwords with another decoding, as the package says it ...
    hotwords_refusal: str
    plan_lm_refusal: str            # ... and as AsrModel.lm_plan / graph_plan say it, which a call reaches only past the package
    plan_hotwords_refusal: str
    pieces: Callable                # (cfg, the model's vocabulary) -> the word of an ARPA file per token id, None = names no token
    # `hotwords=` of a call (`per_item`)
    list_hint: str                  # what a list of the wrong length is told, a template over the unit word
    empty_is_own: bool              # an empty string means the model's own graph (else: a spec that holds nothing, so NO graph)
    share_objects: bool             # the same object twice in a list is built once (equal strings always are)


_NEMO_LM, _NEMO_HW = "an n-gram LM needs decoding='alsd', not {}", "hotwords need decoding='alsd', not {}"
_K2_LM, _K2_HW = "an n-gram LM needs decoding_method='modified_beam_search', not {}", "hotwords need decoding_method='modified_beam_search'"

NEMO = Rule(
    family="nemo", decoding="alsd", token_modes=ngram_lm.TOKEN_MODES, default_tokens="nemo", tokens_note="", foreign_tokens=(),
    lm_refusal=_NEMO_LM, hotwords_refusal=_NEMO_HW, plan_lm_refusal=_NEMO_LM, plan_hotwords_refusal=_NEMO_HW, pieces=_nemo_pieces,
    list_hint="a list is one entry per {0}; pass a string of phrases separated by '/' to use one specification for all",
    empty_is_own=True, share_objects=False)
K2 = NEMO._replace(
    family="k2", decoding="modified_beam_search", token_modes=("pieces", "ids"), default_tokens="pieces",
    foreign_tokens=(("nemo", "ngram_lm_tokens='nemo' is the NeMo package's word encoding; the k2 package reads 'pieces' (the symbols of tokens.txt) or 'ids'"),),
    lm_refusal=_K2_LM, hotwords_refusal=_K2_HW + " (greedy_search has no hypotheses to bias)", plan_lm_refusal=_K2_LM,
    plan_hotwords_refusal=_K2_HW, pieces=_k2_pieces)
# (the plan keeps the nemo package's words for an espnet model: EspnetModel refuses in its own before a call gets that far)
ESPNET = NEMO._replace(
    family="espnet", decoding="beam", token_modes=("pieces", "ids"), default_tokens="pieces", tokens_note=" ('pieces' = the symbols of token_list)",
    lm_refusal="an n-gram LM needs the beam search (beam_size > 1): greedy_search has no hypotheses to re-rank",
    hotwords_refusal="hotwords need the beam search (beam_size > 1): greedy_search has no hypotheses to bias", pieces=_espnet_pieces,
    list_hint="a list has one entry per {0}; one spec for all is a string", empty_is_own=False, share_objects=True)
RULES = {r.family: r for r in (NEMO, K2, ESPNET)}
FUSED = frozenset(r.decoding for r in RULES.values())      # the searches the device runs with graphs and an LM, whatever the family


def rule_of(cfg):
    return RULES[getattr(cfg, "family", "nemo")]


def given(value):
    """whether a `ngram_lm_model` / `hotwords_file` keyword names anything: None and the empty string do not"""
    return value is not None and not (isinstance(value, str) and not value)


def check_file(name, path):
    """the `hotwords_file` / `ngram_lm_model` keyword `name`, where it is a path: FileNotFoundError when no such file exists"""
    if given(path) and isinstance(path, (str, os.PathLike)) and not os.path.isfile(path):
        raise FileNotFoundError(f"{name} {str(path)!r} does not exist")


# ---- the keywords of a loader ---------------------------------------------------------------------------------------------------------
def check_tokens(rule, ngram_lm_tokens):
    for mode, refusal in rule.foreign_tokens:
        if ngram_lm_tokens == mode:
            raise ValueError(refusal)
    return ngram_lm.check_tokens(ngram_lm_tokens, rule.token_modes, rule.tokens_note)


def check_lm_keywords(rule, decoding, ngram_lm_model=None, ngram_lm_alpha=0.0, ngram_lm_tokens=None):
    """the LM keywords of a `load_model`, checked before anything is loaded -> True when there is an LM.  ValueError for an alpha that
    is no finite number >= 0, a token encoding the package does not read, and an LM with a decoding other than the rule's (the only
    search of the family with a "rank the adjusted score" slot: the greedy searches have no hypotheses to re-rank); `decoding` None =
    not known yet (a checkpoint's own strategy: checked again later)."""
    ngram_lm.check_alpha(ngram_lm_alpha)
    check_tokens(rule, rule.default_tokens if ngram_lm_tokens is None else ngram_lm_tokens)
    has = given(ngram_lm_model)
    if has and decoding is not None and decoding != rule.decoding:
        raise ValueError(rule.lm_refusal.format(repr(decoding)))
    return has


def check_hotword_keywords(rule, decoding, hotwords_file="", hotwords_score=DEFAULT_SCORE, hotwords=None):
    """the hotword keywords of a `load_model`, checked before anything is loaded -> True when there are hotwords: ValueError for a
    score that is no finite number and for non-empty hotwords with a decoding other than the rule's (greedy has no hypotheses to
    bias; nemo's "beam" has no hotword form); `decoding` None = not known yet, or refused by the caller in its turn"""
    if not (isinstance(hotwords_score, (int, float)) and not isinstance(hotwords_score, bool) and np.isfinite(hotwords_score)):
        raise ValueError(f"hotwords_score must be a finite number, not {hotwords_score!r}")
    has = bool(hotwords_file) or isinstance(hotwords, HotwordGraph) or (hotwords is not None and len(hotwords) > 0)
    if has and decoding is not None and decoding != rule.decoding:
        raise ValueError(rule.hotwords_refusal.format(repr(decoding)))
    return has


# ---- the model's LM and graph -----------------------------------------------------------------------------------------------------------
def model_lm(rule, cfg, vocabulary, ngram_lm_model, ngram_lm_tokens=None):
    """`ngram_lm_model` (a path to ARPA text, `.gz` allowed, or an NgramLm) -> the NgramLm a model with configuration `cfg` decodes
    with; the table's n_logits must be the model's.  `vocabulary`: what `rule.pieces` reads (nemo: the tokenizer; k2: the symbols of
    tokens.txt; espnet: token_list).  A KenLM binary is refused by the reader."""
    if cfg.decoding != rule.decoding:
        raise ValueError(rule.lm_refusal.format(repr(cfg.decoding)))
    if isinstance(ngram_lm_model, ngram_lm.NgramLm):
        if ngram_lm_model.n_logits != cfg.n_logits:
            raise ValueError(f"the n-gram LM was built for {ngram_lm_model.n_logits} logits, the model has {cfg.n_logits}")
        return ngram_lm_model
    mode = check_tokens(rule, rule.default_tokens if ngram_lm_tokens is None else ngram_lm_tokens)
    pieces = rule.pieces(cfg, vocabulary) if mode == "pieces" else None
    return ngram_lm.load(ngram_lm_model, cfg.vocab_size, cfg.blank_id, mode, pieces, cfg.n_logits)


def check_graph(rule, cfg, graph):
    """a call's or the model's HotwordGraph (None = nothing to bias) -> the same, refused when `cfg`'s search cannot be biased"""
    if graph is not None and cfg.decoding != rule.decoding:
        raise ValueError(rule.hotwords_refusal.format(repr(cfg.decoding)))
    return graph


# ---- the options of one call ------------------------------------------------------------------------------------------------------------
def given_alpha(model, ngram_lm_alpha):
    """an `ngram_lm_alpha=` that was given -> the weight as a float; a value above 0 with no LM loaded raises ValueError"""
    alpha = ngram_lm.check_alpha(ngram_lm_alpha)
    if getattr(model, "ngram_lm", None) is None and alpha > 0:
        raise ValueError("ngram_lm_alpha given, but the model has no n-gram LM (load_model(ngram_lm_model=...))")
    return alpha


def call_alpha(rule, model, ngram_lm_alpha):
    """the `ngram_lm_alpha` of transcribe / transcribe_batch -> (NgramLm or None, alpha) of this call: None = the model's value,
    0 = this call without the LM; a value with no LM loaded raises ValueError"""
    lm = getattr(model, "ngram_lm", None)
    if ngram_lm_alpha is None:
        alpha = ngram_lm.check_alpha(getattr(model, "ngram_lm_alpha", 0.0), "model.ngram_lm_alpha")
    else:
        alpha = given_alpha(model, ngram_lm_alpha)
    if lm is None or alpha == 0.0:
        return None, 0.0
    if model.cfg.decoding != rule.decoding:
        raise ValueError(rule.lm_refusal.format(repr(model.cfg.decoding)))
    return lm, alpha


def check_entries(rule, hotwords, n, unit):
    if len(hotwords) != n:
        raise ValueError(f"hotwords: {len(hotwords)} entries for {n} {unit}s ({rule.list_hint.format(unit)})")


def per_item(rule, hotwords, n, own, make, unit):
    """the `hotwords=` of a call over n items (`unit`: "audio", "window") -> None (no item has a graph) or one HotwordGraph / None per
    item.  None = `own`, the model's graph, for every item; a string = one specification for all; a list = one entry per item: None =
    `own`, else a string, a list of phrases or a HotwordGraph, which `make` turns into the graph the item is decoded with INSTEAD OF
    the model's.  Equal strings are built once.  The rule says what an empty string means and whether one object is built once."""
    def is_own(h):
        return h is None or (rule.empty_is_own and isinstance(h, str) and not h)
    if hotwords is None or isinstance(hotwords, str):
        graphs = [own if is_own(hotwords) else make(hotwords)] * n
    else:
        check_entries(rule, hotwords, n, unit)
        made, graphs = {}, []
        for h in hotwords:
            if is_own(h):
                graphs.append(own)
            elif isinstance(h, str) or rule.share_objects:
                key = h if isinstance(h, str) else id(h)
                if key not in made:
                    made[key] = make(h)
                graphs.append(made[key])
            else:
                graphs.append(make(h))
    return graphs if any(g is not None for g in graphs) else None


# ---- what K2Model and EspnetModel forward to their runtime model ------------------------------------------------------------------------
class ForwardedOptions:
    """the options of a package's model that are its runtime model's (`self.am`), checked on the way in.  The class names its `rule`
    and, as `lm_vocabulary`, the attribute that holds what `rule.pieces` reads."""
    rule = None
    lm_vocabulary = None

    # the model's n-gram LM (an NgramLm, None = no fusion) and its weight, both settable
    @property
    def ngram_lm(self):
        return self.am.ngram_lm

    @ngram_lm.setter
    def ngram_lm(self, lm):
        if lm is not None:
            lm = model_lm(self.rule, self.cfg, getattr(self, self.lm_vocabulary), lm)
            self.am.ngram_set(lm)                         # checked (rs_ngram_check) and uploaded once, found again by NgramLm.key
        self.am.ngram_lm = lm

    @property
    def ngram_lm_alpha(self):
        return self.am.ngram_lm_alpha

    @ngram_lm_alpha.setter
    def ngram_lm_alpha(self, alpha):
        self.am.ngram_lm_alpha = ngram_lm.check_alpha(alpha)

    @property
    def token_scores(self):
        return self.am.token_scores

    @token_scores.setter
    def token_scores(self, value):
        self.am.token_scores = bool(value)

    # entries of the n-best list (0 = off)
    @property
    def nbest(self):
        return self.am.nbest

    # n-best rescoring by full likelihood (None = off, "likelihood", "norm_likelihood"): the runtime model's option, settable
    @property
    def rescore(self):
        return self.am.rescore

    @rescore.setter
    def rescore(self, key):
        self.am.rescore = None if key is None else self.am.rescore_plan(key)      # (a refused value leaves the option as it was)

    # where `transcribe` / `transcribe_batch` normalise their input ("host" / "device")
    @property
    def resample(self):
        return self.am.resample

    @resample.setter
    def resample(self, value):
        from .resample import check_mode
        self.am.resample = check_mode(value)

    def resample_batch(self, waveforms, rates):
        return self.am.resample_batch(waveforms, rates)
