"""Helpers of the n-gram LM tests (tests/test_ngram_lm_host.py, tests/test_alsd_lm_host.py, tests/test_gpu_alsd_lm.py).
TEST INFRASTRUCTURE.

  write_arpa(path, entries, ...)  an ARPA file from {(words...): (log10 p, log10 backoff or None)}
  ArpaDict                        the textbook dictionary implementation of ARPA backoff, float64
  step(lm, state, tok)            include/rs_asr.h's `step` over the flat arrays of an NgramLm, in float32
  (the C checker with an LM is alsd_hotwords_ref.alsd_checker, tests/alsd_checker.c, given lm and alpha)
  lm_float64(...)                 oracle/alsd.py's search plus the hotword rules plus the LM rule, in float64
  toy_lm(plain, cfg)              an order-3 LM cut from the plain search's results; random_lm(...) a large synthetic one"""
import math
import os

import numpy as np
import torch

from oracle import alsd as oalsd
from reazonspeech_amd.runtime import ngram_lm as NL

HERE = os.path.dirname(os.path.abspath(__file__))
TOY_ARPA = os.path.join(HERE, "golden", "toy_3gram.arpa")
BOS = NL.BOS
LN10 = math.log(10.0)


# ---- ARPA text -------------------------------------------------------------------------------------------------------------------
def word_of(tok, mode, pieces=None):
    if tok == BOS:
        return "<s>"
    return chr(tok + NL.TOKEN_OFFSET) if mode == "nemo" else str(tok) if mode == "ids" else pieces[tok]


def write_arpa(path, entries, mode="ids", pieces=None, extra=(), order=None, counts=None, gz=False):
    """entries {(ids... | words...): (log10 p, log10 backoff or None)}; ids are written in `mode`, strings as they are (`<unk>`,
    `</s>`); `extra` = lines appended verbatim to their section [(n, line)]; `counts` overrides the header's"""
    import gzip
    order = order or max(len(k) for k in entries)
    secs = {n: [] for n in range(1, order + 1)}
    for k, (p, b) in entries.items():
        words = [w if isinstance(w, str) else word_of(w, mode, pieces) for w in k]
        secs[len(k)].append(f"{p!r}\t{' '.join(words)}" + (f"\t{b!r}" if b is not None else ""))     # repr: the float64 round-trips
    for n, line in extra:
        secs[n].append(line)
    lines = ["\\data\\"] + [f"ngram {n}={(counts or {}).get(n, len(secs[n]))}" for n in secs] + [""]
    for n in secs:
        lines += [f"\\{n}-grams:"] + secs[n] + [""]
    lines.append("\\end\\")
    text = "\n".join(lines) + "\n"
    with (gzip.open(path, "wt", encoding="utf-8", newline="\n") if gz else open(path, "w", encoding="utf-8", newline="\n")) as fh:
        fh.write(text)
    return path


class ArpaDict:
    """textbook ARPA backoff over a dictionary {(ids...): (log10 p, log10 backoff)} (BOS for `<s>`), float64, natural logarithms:
    p(w | h) = p(h w) if the model has it, else backoff(h) (1 if the model has no h) x p(w | h without its first word);
    a word without a unigram: `unk`"""

    def __init__(self, entries, order, unk_log10):
        self.ent, self.order, self.unk = dict(entries), order, float(unk_log10) * LN10

    def logp(self, hist, w):
        hist = tuple(hist)[-(self.order - 1):] if self.order > 1 else ()
        acc = 0.0
        while True:
            e = self.ent.get(hist + (w,))
            if e is not None:
                return acc + e[0] * LN10
            if not hist:
                return acc + self.unk
            acc += self.ent[hist][1] * LN10 if hist in self.ent else 0.0
            hist = hist[1:]


def step(lm, state, tok):
    """include/rs_asr.h: step(state, token) -> (lp, next, backoffs) over the flat arrays, float32"""
    a = lm.arrays
    n, acc, c, nb = int(state), np.float32(0.0), -1, 0
    for _ in range(lm.order + 1):
        if n == 0:
            c = int(a["root_child"][tok]) if 0 <= tok < lm.n_logits else -1
        else:
            lo, hi = int(a["child_begin"][n]), int(a["child_begin"][n + 1])
            k = lo + int(np.searchsorted(a["child_tok"][lo:hi], tok))
            c = int(a["child_node"][k]) if k < hi and a["child_tok"][k] == tok else -1
        if c >= 0 or n == 0:
            break
        acc = np.float32(acc + a["backoff"][n])
        n = int(a["suffix"][n])
        nb += 1
    if c < 0:
        return np.float32(acc + lm.unk_logp), 0, nb
    return np.float32(acc + a["logp"][c]), (c if a["level"][c] < lm.order else int(a["suffix"][c])), nb


def walk(lm, tokens, state=None):
    """the state after `tokens` from `state` (default: the model's start)"""
    s = lm.start if state is None else state
    for t in tokens:
        _, s, _ = step(lm, s, t)
    return s


def totals(rows, order):
    """the LM counters of a batch, summed: {hits: [level 1..order], backoffs, unk, full_order_pops, recombinations}"""
    return dict(hits=[sum(r["hits"][k] for r in rows) for k in range(1, order + 1)], backoffs=sum(r["backoffs"] for r in rows),
                unk=sum(r["unk"] for r in rows), full_order_pops=sum(r["full_order_pops"] for r in rows),
                recombinations=sum(r["recombinations"] for r in rows))


def all_counted(t):
    return all(h > 0 for h in t["hits"]) and all(t[k] > 0 for k in ("backoffs", "unk", "full_order_pops", "recombinations"))


# ---- the search in float64 -------------------------------------------------------------------------------------------------------
def lm_float64(cfg, sd, f, t_len, graph=None, arpa=None, alpha=0.0, bos=False, beam=4, max_target_len=2.0, score_norm=True,
               recombine="upstream"):
    """AR.hw_float64 plus the LM rule: a label expansion adds alpha x arpa.logp(history, label) after the hotword delta; the history is
    the hypothesis's labels (after `<s>` when `bos`).  -> (labels, alignment steps, score) of the winner."""
    blank = cfg.blank_id
    Wo, bo = sd["joint.joint_net.2.weight"].double(), sd["joint.joint_net.2.bias"].double()
    V1 = Wo.shape[0]
    non_blank = torch.tensor([k for k in range(V1) if k != blank])
    beam = min(beam, V1 - 1)
    pn = oalsd._PredNet(cfg, sd)
    u_max = int(max_target_len * t_len) if isinstance(max_target_len, float) else int(max_target_len)
    root = graph.root if graph is not None else None
    hyps = [dict(y=[blank], score=0.0, ts=[], st=pn.zero_state(), ctx=root)]
    final = []
    for i in range(t_len + u_max):
        live = [(h, i - (len(h["y"]) - 1)) for h in hyps]
        live = [(h, t) for h, t in live if t <= t_len - 1]
        if not live:
            break
        cands = []
        for h, t in live:
            g, new_state = pn.score(oalsd.Hyp(h["y"], h["score"], h["ts"], h["st"]))
            with torch.no_grad():
                logp = torch.log_softmax(torch.relu(f[t].double() + g.double()) @ Wo.t() + bo, dim=-1)
                top_v, top_i = logp[non_blank].topk(beam)
            bh = dict(y=h["y"][:], score=h["score"] + float(logp[blank]), ts=h["ts"][:], st=h["st"], ctx=h["ctx"])
            cands.append(bh)
            if t == t_len - 1:
                final.append(bh)
            for lp, k in zip(top_v.tolist(), non_blank[top_i].tolist()):
                delta, ctx = graph.step(h["ctx"], int(k)) if graph is not None else (0.0, None)
                term = alpha * arpa.logp(((BOS,) if bos else ()) + tuple(h["y"][1:]), int(k)) if arpa is not None and alpha else 0.0
                cands.append(dict(y=h["y"] + [int(k)], score=h["score"] + float(lp) + delta + term, ts=h["ts"] + [i], st=new_state, ctx=ctx))
        kept = sorted(cands, key=lambda c: c["score"], reverse=True)[:beam]      # stable: ties keep expansion order
        merged = []
        for c in kept:
            for m in merged:
                if m["y"] == c["y"]:
                    m["score"] = float(np.logaddexp(m["score"], c["score"]))
                    break
            else:
                merged.append(c)
        hyps = kept if recombine == "upstream" else merged
    out = final if final else hyps
    done = [(h, h["score"] + (graph.finalize(h["ctx"])[0] if graph is not None else 0.0)) for h in out]
    key = (lambda e: e[1] / len(e[0]["y"])) if score_norm else (lambda e: e[1])
    best, score = sorted(done, key=key, reverse=True)[0]
    return best["y"][1:], best["ts"], score


# ---- fixtures --------------------------------------------------------------------------------------------------------------------
def toy_lm(plain, cfg, skip=5):
    """an order-3 model cut from the PLAIN search's results `plain` (AR.alsd_checker at beam 4), so that the search meets it at every
    level; every log10 value is a multiple of 1/8.  Unigrams for every token but those with id % skip == skip - 1 (a candidate
    without one is an unknown word); `<s>` and the bigram `<s>` + each winner's first label; the bigrams and trigrams of the
    winners' labels and of the best beam entry that differs, prefix-closed as a file is
    -> entries {(ids...): (log10 p, log10 backoff)}; there is no `<unk>`: an unknown word costs the lowest unigram"""
    V = cfg.vocab_size
    ent = {(t,): (-(1.0 + (t % 9) / 8.0), -(t % 3) / 8.0) for t in range(V) if t % skip != skip - 1}
    ent[(BOS,)] = (-99.0, -0.25)
    seqs = []
    for r in plain:
        seqs.append(r["ids"])
        seqs += [y for y, *_ in r["beam"] if y != r["ids"]][:1]
    for y in seqs:
        y = [t for t in y]
        if y and (y[0],) in ent:
            ent[(BOS, y[0])] = (-0.125, -0.125)
        for k in range(len(y) - 1):
            a, b = y[k], y[k + 1]
            if (a,) in ent and (b,) in ent:
                ent[(a, b)] = (-0.25, -0.125 * (k % 2))
        for k in range(len(y) - 2):
            a, b, c = y[k:k + 3]
            if (a, b) in ent and (c,) in ent:
                ent[(a, b, c)] = (-0.125, 0.0)
    if len(seqs[0]) >= 2 and (BOS, seqs[0][0]) in ent and (seqs[0][1],) in ent:
        ent[(BOS, seqs[0][0], seqs[0][1])] = (-0.125, 0.0)
    assert all(v * 8 == int(v * 8) for e in ent.values() for v in e)
    return ent


def random_lm(cfg, seqs, n_high=3000, order=4, seed=4):
    """an order-`order` model with a unigram for every token, every n-gram (up to `order`, also after `<s>`) of the label sequences
    `seqs` (what the plain search proposes: the search meets the model at every level) and about `n_high` more higher-order n-grams
    drawn around their labels, prefix-closed: long child lists below frequent contexts, and root_child for everything else"""
    rng = np.random.default_rng(seed)
    V = cfg.vocab_size
    q = lambda lo, hi: float(rng.integers(lo * 8, hi * 8)) / 8.0                    # noqa: E731  multiples of 1/8
    ent = {(t,): (-q(1, 5), -q(0, 1)) for t in range(V)}
    ent[(BOS,)] = (-99.0, -q(0, 1))
    seen = sorted({int(t) for y in seqs for t in y})
    for y in seqs:
        y = (BOS,) + tuple(int(t) for t in y)
        for k in range(len(y)):
            for m in range(2, min(order, len(y) - k) + 1):
                ent.setdefault(y[k:k + m], (-q(0, 1), -q(0, 1) if m < order else 0.0))
    for _ in range(n_high):
        n = int(rng.integers(2, order + 1))
        words = tuple(int(rng.choice(seen)) if rng.random() < 0.7 else int(rng.integers(0, V)) for _ in range(n))
        for k in range(2, n + 1):
            ent.setdefault(words[:k], (-q(0, 3), -q(0, 1) if k < order else 0.0))
    return ent
