"""Hotwords (contextual biasing) of the Zipformer family's modified beam search: phrase parsing and the context graph as the
flat arrays `rs_rnnt_mbs_hotwords` walks (include/rs_asr.h: rs_hotwords; csrc/k_rnnt_mbs.hip).  Needs no GPU.

[UPSTREAM, not vendored, PARITY UNPINNED] sherpa-onnx's `hotwords_file=` / `hotwords_score=` / `create_stream(hotwords=)` and its
ContextGraph::Build / FillFailOutput, restated from the specification in include/rs_asr.h:
  file       one phrase per line, blank lines ignored; an optional trailing ` :<float>` is the phrase's own score
  string     phrases separated by `/` (what `create_stream(hotwords=...)` takes), each with the optional ` :<float>`
  tokens     modeling_unit "cjkchar": every character of a phrase (white space dropped) is looked up in tokens.txt; a phrase with a
             character that is no token is skipped with a warning naming it (upstream logs and skips).  A phrase may also be a
             sequence of token ids — any tokenisation can be used that way; the blank or <unk> id in one raises ValueError
  score      of phrase i: its own if given and non-zero, else `hotwords_score` (default 1.5, upstream's)

Only the graph is built here; the walk (ForwardOneStep, non-strict, and Finalize) is the kernel's."""
import re
import warnings
from collections import deque

import numpy as np

DEFAULT_SCORE = 1.5
INT_ARRAYS = ("child_begin", "child_tok", "child_node", "fail", "output", "is_end", "level", "graph_root")
FLOAT_ARRAYS = ("token_score", "node_score", "output_score")
_SCORE = re.compile(r"^(.*?)(?:\s+:(\S*))?\s*$", re.S)


def parse_phrase(text):
    """"phrase :2.0" -> ("phrase", 2.0); "phrase" -> ("phrase", 0.0) (0 = no score of its own)"""
    m = _SCORE.match(text)
    body, score = m.group(1).strip(), m.group(2)
    if score is None:
        return body, 0.0
    try:
        return body, float(score)
    except ValueError:
        raise ValueError(f"hotwords: {text!r}: the score after ' :' is not a number") from None


def parse_hotwords(spec):
    """a hotwords argument -> [(phrase, own score)]: phrase = str (characters) or tuple of token ids.
    spec: None / "" -> []; a string of phrases separated by `/`; or a list whose entries are strings ("phrase" / "phrase :2"),
    sequences of token ids, or (phrase or ids, score) pairs."""
    if spec is None:
        return []
    if isinstance(spec, str):
        return [p for p in (parse_phrase(part) for part in spec.split("/")) if p[0]]
    out = []
    for item in spec:
        if isinstance(item, str):
            p = parse_phrase(item)
            if p[0]:
                out.append(p)
            continue
        item = tuple(item) if not isinstance(item, np.ndarray) else tuple(item.tolist())
        if len(item) == 2 and not isinstance(item[0], (int, np.integer)) and isinstance(item[1], (int, float, np.floating)):
            body, score = item
            body = parse_phrase(body)[0] if isinstance(body, str) else tuple(body)
            out.append((body, float(score)))
        else:
            out.append((item, 0.0))
    return out


def read_hotwords_file(path):
    with open(path, encoding="utf-8") as fp:
        return [p for p in (parse_phrase(line.rstrip("\n")) for line in fp if line.strip()) if p[0]]


def encode(phrases, tokens, blank_id, unk_id, hotwords_score=DEFAULT_SCORE):
    """[(phrase, own score)] -> [(token ids, score)] ready for `build_graph`"""
    table = None
    out = []
    for body, own in phrases:
        if isinstance(body, str):
            if table is None:
                table = {s: i for i, s in reversed(list(enumerate(tokens)))}      # a repeated symbol: its first id
            chars = [c for c in body if not c.isspace()]
            missing = [c for c in chars if c not in table or table[c] in (blank_id, unk_id)]
            if missing or not chars:
                warnings.warn(f"hotwords: phrase {body!r} skipped: {missing[0]!r} is not in tokens.txt" if missing else
                              f"hotwords: empty phrase {body!r} skipped")
                continue
            ids = tuple(table[c] for c in chars)
        else:
            ids = tuple(body)
            if not ids:
                raise ValueError("hotwords: an empty token-id phrase")
            for i in ids:
                if not isinstance(i, (int, np.integer)) or isinstance(i, bool):
                    raise ValueError(f"hotwords: token ids must be integers, got {i!r}")
                if i == blank_id or i == unk_id:
                    raise ValueError(f"hotwords: token id {i} is the blank or <unk>: it can never be appended to a hypothesis")
                if not 0 <= i < len(tokens):
                    raise ValueError(f"hotwords: token id {i} outside the vocabulary of {len(tokens)}")
            ids = tuple(int(i) for i in ids)
        score = float(own) if own != 0.0 else float(hotwords_score)
        if not np.isfinite(score):
            raise ValueError(f"hotwords: score {score!r} is not finite")
        out.append((ids, score))
    return out


class HotwordGraph:
    """one context graph as flat arrays with LOCAL node indices (root = node 0); `key` identifies it by content"""

    def __init__(self, encoded):
        self.key = tuple(encoded)
        tok, par, tsc, nsc, end, lvl, kids = [-1], [0], [0.0], [0.0], [0], [0], [{}]
        for ids, s in encoded:                                   # ContextGraph::Build
            cur = 0
            for j, t in enumerate(ids):
                last = j == len(ids) - 1
                nxt = kids[cur].get(t)
                if nxt is None:
                    nxt = len(tok)
                    kids[cur][t] = nxt
                    tok.append(t); par.append(cur); tsc.append(s); nsc.append(nsc[cur] + s); end.append(int(last))
                    lvl.append(lvl[cur] + 1); kids.append({})
                else:
                    tsc[nxt] = max(s, tsc[nxt])
                    nsc[nxt] = nsc[cur] + tsc[nxt]
                    end[nxt] = int(end[nxt] or last)
                cur = nxt
        n = len(tok)
        osc = [nsc[i] if end[i] else 0.0 for i in range(n)]
        fail, output = [0] * n, [-1] * n
        queue = deque(kids[0].values())                          # FillFailOutput: breadth-first, the root's children fail to the root
        while queue:
            cur = queue.popleft()
            for t, c in kids[cur].items():
                f = fail[cur]
                while t not in kids[f] and f != 0:
                    f = fail[f]
                fail[c] = kids[f].get(t, 0)
                o = fail[c]
                while o != 0 and not end[o]:
                    o = fail[o]
                if o != 0:
                    output[c] = o
                    osc[c] += osc[o]
                queue.append(c)
        begin, ctok, cnode = [0], [], []
        for i in range(n):
            for t in sorted(kids[i]):
                ctok.append(t); cnode.append(kids[i][t])
            begin.append(len(ctok))
        i32 = lambda x: np.asarray(x, dtype=np.int32)             # noqa: E731
        f32 = lambda x: np.asarray(x, dtype=np.float32)           # noqa: E731
        self.arrays = dict(child_begin=i32(begin), child_tok=i32(ctok), child_node=i32(cnode), fail=i32(fail), output=i32(output),
                           is_end=i32(end), level=i32(lvl), token_score=f32(tsc), node_score=f32(nsc), output_score=f32(osc))
        self.n_nodes, self.n_children, self.max_level = n, len(ctok), max(lvl)
        self.n_phrases = len(encoded)


def build_graph(encoded):
    """[(token ids, score)] -> HotwordGraph, or None when nothing is left to bias"""
    return HotwordGraph(encoded) if encoded else None


def make_graph(spec, tokens, blank_id, unk_id, hotwords_score=DEFAULT_SCORE, hotwords_file=""):
    """a hotwords argument (see `parse_hotwords`) and / or a hotwords file -> HotwordGraph or None"""
    phrases = (read_hotwords_file(hotwords_file) if hotwords_file else []) + parse_hotwords(spec)
    return build_graph(encode(phrases, tokens, blank_id, unk_id, hotwords_score))


def concat(graphs):
    """the graphs of a call as ONE table with global indices (rs_hotwords): dict of numpy arrays + "max_level" """
    out = {k: [] for k in INT_ARRAYS + FLOAT_ARRAYS}
    node0 = child0 = 0
    for g in graphs:
        a = g.arrays
        out["graph_root"].append(np.asarray([node0], np.int32))
        out["child_begin"].append(a["child_begin"][:-1] + child0)
        out["child_node"].append(a["child_node"] + node0)
        out["fail"].append(a["fail"] + node0)
        out["output"].append(np.where(a["output"] >= 0, a["output"] + node0, -1).astype(np.int32))
        for k in ("child_tok", "is_end", "level") + FLOAT_ARRAYS:
            out[k].append(a[k])
        node0 += g.n_nodes
        child0 += g.n_children
    out["child_begin"].append(np.asarray([child0], np.int32))
    table = {k: np.ascontiguousarray(np.concatenate(v) if v else np.zeros((0,)), dtype=np.float32 if k in FLOAT_ARRAYS else np.int32)
             for k, v in out.items()}
    table["max_level"] = max((g.max_level for g in graphs), default=0)
    return table
