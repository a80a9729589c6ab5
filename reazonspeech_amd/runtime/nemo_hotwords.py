"""Hotwords (contextual biasing) of the NeMo family's ALSD beam search (rs_rnnt_alsd_hotwords, csrc/k_rnnt_alsd.hip): phrases ->
token ids with the model's SentencePiece vocabulary -> the context graph of runtime/k2_hotwords.py.  Needs no GPU.

The phrase syntax (file, `/`-separated string, list, optional ` :<float>` score), the graph and its flat arrays are
runtime/k2_hotwords.py's; only the tokenisation differs.  A text phrase is encoded by the tokenizer's `text_to_ids`, which returns
every reading the phrase can have inside a transcript (SentencePiece marks a word start with U+2581; the same word in the middle
of a Japanese sentence has none), and EVERY reading enters the graph with the phrase's score.  A phrase the vocabulary cannot
spell is skipped with a warning naming it; a phrase given as token ids is checked as k2_hotwords.encode checks it (integers,
inside the vocabulary, never the blank)."""
import warnings

import numpy as np

from . import k2_hotwords
from .k2_hotwords import DEFAULT_SCORE, HotwordGraph, build_graph, parse_hotwords, read_hotwords_file


def encode(phrases, tokenizer, blank_id, vocab_size, hotwords_score=DEFAULT_SCORE):
    """[(phrase, own score)] -> [(token ids, score)] ready for `build_graph`; a text phrase gives one entry per reading"""
    out = []
    for body, own in phrases:
        if not isinstance(body, str):
            out.extend(k2_hotwords.encode([(body, own)], range(vocab_size), blank_id, -1, hotwords_score))
            continue
        score = float(own) if own != 0.0 else float(hotwords_score)
        if not np.isfinite(score):
            raise ValueError(f"hotwords: score {score!r} is not finite")
        readings = [tuple(int(i) for i in r) for r in tokenizer.text_to_ids(body)]
        readings = [r for r in readings if r and all(0 <= i < vocab_size and i != blank_id for i in r)]
        if not readings:
            warnings.warn(f"hotwords: phrase {body!r} skipped: the vocabulary cannot spell it")
            continue
        for r in dict.fromkeys(readings):
            out.append((r, score))
    return out


def make_graph(spec, tokenizer, blank_id, vocab_size, hotwords_score=DEFAULT_SCORE, hotwords_file=""):
    """a hotwords argument (k2_hotwords.parse_hotwords) and / or a hotwords file -> HotwordGraph or None"""
    if isinstance(spec, HotwordGraph):
        return spec
    phrases = (read_hotwords_file(hotwords_file) if hotwords_file else []) + parse_hotwords(spec)
    return build_graph(encode(phrases, tokenizer, blank_id, vocab_size, hotwords_score))


def check_keywords(decoding, hotwords_file="", hotwords_score=DEFAULT_SCORE, hotwords=None):
    """the hotword keywords of `load_model`, checked before anything is loaded: ValueError for a score that is no finite number and
    for non-empty hotwords with a decoding other than "alsd" (greedy has no hypotheses to bias; "beam" has no hotword form)"""
    if not (isinstance(hotwords_score, (int, float)) and not isinstance(hotwords_score, bool) and np.isfinite(hotwords_score)):
        raise ValueError(f"hotwords_score must be a finite number, not {hotwords_score!r}")
    has = bool(hotwords_file) or isinstance(hotwords, HotwordGraph) or (hotwords is not None and len(hotwords) > 0)
    if has and decoding != "alsd":
        raise ValueError(f"hotwords need decoding='alsd', not {decoding!r}")
    return has


def model_graph(model, spec, hotwords_file=""):
    """`spec` -> the HotwordGraph `model` (an AsrModel of the NeMo family) decodes it with; None for nothing"""
    cfg = model.cfg
    graph = make_graph(spec, model.tokenizer, cfg.blank_id, cfg.vocab_size, model.hotwords_score, hotwords_file)
    if graph is not None and cfg.decoding != "alsd":
        raise ValueError(f"hotwords need decoding='alsd', not {cfg.decoding!r}")
    return graph


def per_audio(model, hotwords, n, single=False):
    """the `hotwords` argument of transcribe / transcribe_batch -> None (no utterance has a graph) or one HotwordGraph / None per
    audio.  None = the model's graph; a string = one specification for all audios; a list = one entry per audio (None / "" = the
    model's graph, a string, a list of phrases or a HotwordGraph INSTEAD OF the model's).  `single`: the argument is ONE
    audio's entry, whatever its type (transcribe)."""
    own = getattr(model, "hotwords", None)
    if single and hotwords is not None:
        hotwords = [hotwords]
    if hotwords is None or isinstance(hotwords, str):
        g = model_graph(model, hotwords) if hotwords else own
        graphs = [g] * n
    else:
        if len(hotwords) != n:
            raise ValueError(f"hotwords: {len(hotwords)} entries for {n} audios (a list is one entry per audio; pass a string of phrases "
                             "separated by '/' to use one specification for all)")
        cache, graphs = {}, []
        for h in hotwords:
            if h is None or (isinstance(h, str) and not h):
                graphs.append(own)
            elif isinstance(h, str):
                if h not in cache:
                    cache[h] = model_graph(model, h)
                graphs.append(cache[h])
            else:
                graphs.append(model_graph(model, h))
    return None if all(g is None for g in graphs) else graphs
