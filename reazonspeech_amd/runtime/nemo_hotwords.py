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
