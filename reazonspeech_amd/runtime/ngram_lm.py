"""N-gram language models for shallow fusion in the transducer beam searches — ALSD (rs_rnnt_alsd_lm, csrc/k_rnnt_alsd.hip) and the
k2 package's modified beam search (rs_rnnt_mbs_lm, csrc/k_rnnt_mbs.hip); the rules are stated in include/rs_asr.h: ARPA text -> the flat arrays the device walks (csrc/k_rnnt_ngram.h).  Needs no GPU and nothing beyond numpy.

  read_arpa(path, vocab_size, blank_id, ngram_lm_tokens=, pieces=) -> Ngrams     the file's n-grams over token ids
  build(ngrams, vocab_size, blank_id) -> NgramLm                                 the flat table (natural logarithms, float32)
  load(path, ...) = build(read_arpa(path, ...))

The file: `\\data\\`, `ngram N=count` lines, `\\N-grams:` sections of `log10p <TAB> w1 ... wN [<TAB> log10 backoff]`, `\\end\\`; a
`.gz` file is read through gzip.  Only ARPA TEXT is read: a KenLM binary file (recognised by the magic text at its head) raises
ValueError — reading one needs the kenlm package, which is not a dependency of this project.

How a "word" of the file names a token (`ngram_lm_tokens`):
  "nemo"    one character, chr(id + 100).  [UPSTREAM, not vendored, UNVERIFIED] believed to be what NeMo's
            scripts/asr_language_modeling/ngram_lm/train_kenlm.py writes for BPE models (TOKEN_OFFSET = 100) and what the beam
            search's compute_ngram_score looks up; NeMo is not available to this project, so the encoding is an assumption.
  "pieces"  the vocabulary's piece strings (tokenizer.ids_to_tokens; k2: the symbols of tokens.txt as written there, which is what an
            icefall token-level LM is trained on — the k2 package's default)
  "ids"     decimal ids
`<s>`, `</s>` and `<unk>` are special in all three.  N-grams that contain `</s>` (the search never emits it), that have `<s>`
anywhere but first, or that hold a word which maps to no id below vocab_size or to the blank are dropped; ONE warning gives the
number dropped per reason.  An n-gram whose prefix (all words but the last) is not an (n-1)-gram of the file raises ValueError."""
import gzip
import hashlib
import math
import warnings

import numpy as np

MAX_ORDER = 8
TOKEN_OFFSET = 100                 # "nemo": word = chr(id + TOKEN_OFFSET)
TOKEN_MODES = ("nemo", "pieces", "ids")
BOS = -1                           # `<s>` inside an n-gram of token ids
KENLM_MAGIC = b"mmap lm http://kheafield.com/code format version"
LN10 = math.log(10.0)


def check_tokens(ngram_lm_tokens, modes=TOKEN_MODES, note=""):
    """`modes`: the encodings a caller reads (a package reads fewer than this reader: runtime/fusion.py), `note`: what it adds"""
    if ngram_lm_tokens not in modes:
        raise ValueError(f"ngram_lm_tokens must be one of {modes}, not {ngram_lm_tokens!r}{note}")
    return ngram_lm_tokens


class Ngrams:
    """the n-grams of a file over token ids: `entries` {(ids...): (log10 p, log10 backoff)} with BOS (-1) for `<s>` (first position
    only; the unigram (BOS,) is `<s>` itself), `order`, `unk` = `<unk>`'s log10 p or None, `floor` = the lowest unigram log10 p of
    the file (`<s>` aside), `dropped` = {reason: count}"""

    def __init__(self, order, entries, unk=None, floor=None, dropped=None):
        self.order, self.entries, self.unk, self.floor, self.dropped = int(order), dict(entries), unk, floor, dict(dropped or {})


def _open_text(path):
    with open(path, "rb") as fh:
        head = fh.read(len(KENLM_MAGIC))
    if head.startswith(KENLM_MAGIC[:8]):
        raise ValueError(f"{path}: a KenLM binary file; only ARPA text is read (convert it back, or keep the .arpa the binary was built from)")
    if head[:2] == b"\x1f\x8b" or str(path).endswith(".gz"):
        return gzip.open(path, "rt", encoding="utf-8", newline="\n")
    return open(path, "r", encoding="utf-8", newline="\n")


def _number(text, path, no, what):
    try:
        v = float(text)
    except ValueError:
        raise ValueError(f"{path}:{no}: {what} {text!r} is not a number") from None
    if not math.isfinite(v):
        raise ValueError(f"{path}:{no}: {what} {text!r} is not finite")
    return v


def parse_arpa(path):
    """-> (order, [[(words, log10 p, log10 backoff, line number)] per n]): the file as written, every refusal of the format"""
    counts, sections, cur, cur_line, state = {}, {}, 0, 0, "head"
    with _open_text(path) as fh:
        for no, raw in enumerate(fh, 1):
            line = raw.rstrip("\r\n")                         # (never str.strip(): chr(133) and chr(160) are "nemo" words)
            if not line.strip(" \t"):
                continue
            if state == "head":
                if line.strip(" \t") != "\\data\\":
                    raise ValueError(f"{path}:{no}: expected \\data\\, found {line[:40]!r}")
                state = "counts"
                continue
            if line.startswith("\\"):
                tag = line.strip(" \t")
                if cur and len(sections[cur]) != counts[cur]:
                    raise ValueError(f"{path}:{cur_line}: the header gives {counts[cur]} {cur}-grams, the section has {len(sections[cur])}")
                if tag == "\\end\\":
                    state = "end"
                    break
                if not (tag.endswith("-grams:") and tag[1:-7].isdigit()):
                    raise ValueError(f"{path}:{no}: malformed section line {line[:40]!r}")
                n = int(tag[1:-7])
                if n != cur + 1 or n not in counts:
                    raise ValueError(f"{path}:{no}: section {n}-grams out of order or without a count")
                cur, cur_line, state = n, no, "grams"
                sections[n] = []
                continue
            if state == "counts":
                body = line.strip(" \t")
                if not body.startswith("ngram ") or "=" not in body:
                    raise ValueError(f"{path}:{no}: malformed count line {line[:40]!r}")
                k, _, c = body[6:].partition("=")
                if not (k.strip().isdigit() and c.strip().isdigit()):
                    raise ValueError(f"{path}:{no}: malformed count line {line[:40]!r}")
                k = int(k)
                if k != len(counts) + 1:
                    raise ValueError(f"{path}:{no}: count of order {k} out of sequence")
                if k > MAX_ORDER:
                    raise ValueError(f"{path}:{no}: order {k} is above the {MAX_ORDER} this reader takes")
                counts[k] = int(c)
                continue
            fields = line.split("\t")
            if len(fields) in (2, 3):
                words, bo = fields[1].split(" "), fields[2] if len(fields) == 3 else None
            else:                                                 # written with blanks only
                toks = [t for t in line.split(" ") if t]
                fields, words, bo = toks[:1], toks[1:1 + cur], toks[1 + cur] if len(toks) == cur + 2 else None
                if len(toks) not in (cur + 1, cur + 2):
                    words = []
            if len(words) != cur or any(w == "" for w in words):
                raise ValueError(f"{path}:{no}: malformed {cur}-gram line {line[:60]!r}")
            p = _number(fields[0].strip(" "), path, no, "log-probability")
            b = _number(bo.strip(" "), path, no, "backoff") if bo is not None else 0.0
            sections[cur].append((tuple(words), p, b, no))
    if state != "end":
        raise ValueError(f"{path}: no \\end\\ line")
    if not counts or cur != len(counts):
        raise ValueError(f"{path}: the header counts {len(counts)} orders, the file has sections up to {cur}")
    return len(counts), [sections[n] for n in range(1, len(counts) + 1)]


def word_map(ngram_lm_tokens, vocab_size, pieces=None):
    """-> word -> token id or None, for one encoding"""
    check_tokens(ngram_lm_tokens)
    if ngram_lm_tokens == "nemo":
        return lambda w: ord(w) - TOKEN_OFFSET if len(w) == 1 and 0 <= ord(w) - TOKEN_OFFSET < vocab_size else None
    if ngram_lm_tokens == "ids":
        return lambda w: int(w) if w.isascii() and w.isdigit() and int(w) < vocab_size else None
    if pieces is None:
        raise ValueError("ngram_lm_tokens='pieces' needs the vocabulary's piece strings")
    index = {}
    for i, p in enumerate(list(pieces)[:vocab_size]):
        index.setdefault(p, i)
    return index.get


def read_arpa(path, vocab_size, blank_id, ngram_lm_tokens="nemo", pieces=None):
    """the n-grams of an ARPA file over token ids (Ngrams); see the head of this module for what is dropped and what is refused"""
    to_id = word_map(ngram_lm_tokens, vocab_size, pieces)
    order, sections = parse_arpa(path)
    dropped = {"</s>": 0, "<s> not first": 0, "no token id": 0, "blank": 0}
    entries, seen, unk, floor = {}, set(), None, None
    for n, sec in enumerate(sections, 1):
        for words, p, b, no in sec:
            if words in seen:
                raise ValueError(f"{path}:{no}: the {n}-gram {' '.join(words)!r} occurs twice")
            if n > 1 and words[:-1] not in seen:
                raise ValueError(f"{path}:{no}: the prefix of the {n}-gram {' '.join(words)!r} is not a {n - 1}-gram of the file")
            seen.add(words)
            if n == 1 and words[0] != "<s>":
                floor = p if floor is None else min(floor, p)
            if n == 1 and words[0] == "<unk>":
                unk = p
                continue
            if "</s>" in words:
                dropped["</s>"] += 1
                continue
            if "<s>" in words[1:]:
                dropped["<s> not first"] += 1
                continue
            ids = [BOS if (k == 0 and w == "<s>") else to_id(w) for k, w in enumerate(words)]
            if any(i is None for i in ids):
                dropped["no token id"] += 1
                continue
            if blank_id in ids:
                dropped["blank"] += 1
                continue
            entries[tuple(ids)] = (p, b)
    if any(dropped.values()):
        warnings.warn(f"ngram lm {path}: n-grams dropped: " + ", ".join(f"{v} ({k})" for k, v in dropped.items() if v))
    return Ngrams(order, entries, unk, floor, dropped)


ARRAYS = ("child_begin", "child_tok", "child_node", "root_child", "logp", "backoff", "suffix", "level")   # the pointer fields of rs_ngram
FLOATS = ("logp", "backoff")


class NgramLm:
    """a backoff n-gram model as the flat table of include/rs_asr.h (rs_ngram): `arrays` (ARRAYS, numpy), `start`, `order`, `unk_logp`
    and `key`, a hash of the content by which a model uploads a table once"""

    def __init__(self, arrays, start, order, unk_logp):
        self.arrays = {k: np.ascontiguousarray(arrays[k], dtype=np.float32 if k in FLOATS else np.int32) for k in ARRAYS}
        self.start, self.order, self.unk_logp = int(start), int(order), np.float32(unk_logp)
        h = hashlib.sha1()
        for k in ARRAYS:
            h.update(self.arrays[k].tobytes())
        h.update(np.asarray([self.start, self.order], np.int32).tobytes() + np.float32(self.unk_logp).tobytes())
        self.key = h.hexdigest()

    n_nodes = property(lambda self: len(self.arrays["logp"]))
    n_children = property(lambda self: len(self.arrays["child_tok"]))
    n_logits = property(lambda self: len(self.arrays["root_child"]))


def _ln(log10_value):
    return np.float32(float(log10_value) * LN10)              # the product in float64, rounded once


def build(ngrams, vocab_size, blank_id, n_logits=None):
    """Ngrams (or {(ids...): (log10 p, log10 backoff)} with BOS for `<s>`) -> NgramLm.  Node 0 is the root; the nodes follow by
    (level, ids).  `<s>` is a level-1 node that is in no child list: no token reaches it."""
    if not isinstance(ngrams, Ngrams):
        ent = dict(ngrams)
        ngrams = Ngrams(max((len(k) for k in ent), default=1), ent)
    n_logits = int(n_logits) if n_logits is not None else max(int(vocab_size), int(blank_id) + 1)
    ent = ngrams.entries
    if not 1 <= ngrams.order <= MAX_ORDER:
        raise ValueError(f"ngram lm: order {ngrams.order} outside 1..{MAX_ORDER}")
    for ids, (p, b) in ent.items():
        if not ids or len(ids) > ngrams.order:
            raise ValueError(f"ngram lm: n-gram {ids} does not fit order {ngrams.order}")
        if any((i == BOS and k > 0) or (i != BOS and not 0 <= i < vocab_size) or i == blank_id for k, i in enumerate(ids)):
            raise ValueError(f"ngram lm: n-gram {ids} has a token outside the vocabulary, the blank, or <s> past the first place")
        if not (math.isfinite(p) and math.isfinite(b)):
            raise ValueError(f"ngram lm: n-gram {ids} has a non-finite value")
        if len(ids) > 1 and ids[:-1] not in ent:
            raise ValueError(f"ngram lm: the prefix of {ids} is not an n-gram of the model")
    keys = sorted(ent, key=lambda k: (len(k), k))
    node = {(): 0}
    for k in keys:
        node[k] = len(node)
    N = len(node)
    logp, backoff = np.zeros(N, np.float32), np.zeros(N, np.float32)
    suffix, level = np.zeros(N, np.int32), np.zeros(N, np.int32)
    kids = [[] for _ in range(N)]
    for k in keys:
        n = node[k]
        logp[n], backoff[n], level[n] = _ln(ent[k][0]), _ln(ent[k][1]), len(k)
        s = k[1:]
        while s and s not in node:                               # the longest proper suffix present in the file
            s = s[1:]
        suffix[n] = node[s]
        if k != (BOS,):
            kids[node[k[:-1]]].append((k[-1], n))
    child_begin = np.zeros(N + 1, np.int32)
    tok, nod = [], []
    for n in range(N):
        kids[n].sort()
        tok.extend(t for t, _ in kids[n])
        nod.extend(c for _, c in kids[n])
        child_begin[n + 1] = len(tok)
    root_child = np.full(n_logits, -1, np.int32)
    for t, c in kids[0]:
        root_child[t] = c
    unigrams = [ent[k][0] for k in keys if len(k) == 1 and k != (BOS,)]
    unk = ngrams.unk if ngrams.unk is not None else ngrams.floor if ngrams.floor is not None else min(unigrams, default=0.0)
    arrays = dict(child_begin=child_begin, child_tok=np.asarray(tok, np.int32), child_node=np.asarray(nod, np.int32),
                  root_child=root_child, logp=logp, backoff=backoff, suffix=suffix, level=level)
    return NgramLm(arrays, node.get((BOS,), 0), ngrams.order, _ln(unk))


def load(path, vocab_size, blank_id, ngram_lm_tokens="nemo", pieces=None, n_logits=None):
    return build(read_arpa(path, vocab_size, blank_id, ngram_lm_tokens, pieces), vocab_size, blank_id, n_logits)


# ---- the weight (the keywords themselves are checked in runtime/fusion.py) ----------------------------------------------------------
def check_alpha(alpha, name="ngram_lm_alpha"):
    if not (isinstance(alpha, (int, float, np.floating, np.integer)) and not isinstance(alpha, bool) and math.isfinite(alpha) and alpha >= 0):
        raise ValueError(f"{name} must be a finite number >= 0, not {alpha!r}")
    return float(alpha)
