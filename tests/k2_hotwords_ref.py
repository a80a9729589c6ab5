"""Helpers of the hotword tests (tests/test_k2_hotwords_host.py, tests/test_gpu_k2_hotwords.py).  TEST INFRASTRUCTURE.

  ContextGraph           a pointer-and-dict restatement of sherpa-onnx's ContextGraph from the specification in include/rs_asr.h
                         (Build, FillFailOutput, ForwardOneStep strict and non-strict, Finalize) — written independently of the
                         product's flat builder (reazonspeech_amd/runtime/k2_hotwords.py), which it is compared with
  flat_step / FlatView   a numpy walker over the flat table the device reads (strict and non-strict; the product builds only the
                         non-strict walk, in the kernel)
  hw_float64(...)        k2_mbs_ref.mbs_float64 plus the context rules, in float64
The C checker with hotwords is k2_mbs_ref.mbs_checker (tests/k2_mbs_checker.c), given a table and graph_of.
"""
import math

import numpy as np
import torch

import k2_mbs_ref as R


# ---- the graph, with pointers ------------------------------------------------------------------------------------------------
class Node:
    def __init__(self, token, parent):
        self.token, self.parent, self.next = token, parent, {}
        self.token_score = self.node_score = self.output_score = 0.0
        self.is_end, self.level = False, 0 if parent is None else parent.level + 1
        self.fail = self.output = None

    def path(self):
        out, n = [], self
        while n.parent is not None:
            out.append(n.token)
            n = n.parent
        return tuple(reversed(out))


class ContextGraph:
    def __init__(self, phrases):
        """phrases: [(token ids, score)]"""
        self.root = Node(-1, None)
        self.root.fail = self.root
        for ids, score in phrases:
            node = self.root
            for j, tok in enumerate(ids):
                last = j == len(ids) - 1
                if tok not in node.next:
                    child = Node(tok, node)
                    child.token_score = score
                    child.node_score = node.node_score + score
                    child.is_end = last
                    node.next[tok] = child
                else:
                    child = node.next[tok]
                    child.token_score = max(score, child.token_score)
                    child.node_score = node.node_score + child.token_score
                    child.is_end = child.is_end or last
                child.output_score = child.node_score if child.is_end else 0.0
                node = child
        level = list(self.root.next.values())          # breadth-first; the root's children fail to the root and have no output
        for child in level:
            child.fail = self.root
        while level:
            nxt = []
            for cur in level:
                for tok, c in cur.next.items():
                    f = cur.fail
                    while tok not in f.next and f is not self.root:
                        f = f.fail
                    c.fail = f.next.get(tok, self.root)
                    o = c.fail
                    while o is not self.root and not o.is_end:
                        o = o.fail
                    c.output = None if o is self.root else o
                    if c.output is not None:
                        c.output_score += c.output.output_score
                    nxt.append(c)
            level = nxt

    def step(self, state, tok, strict=False):
        if tok in state.next:
            n = state.next[tok]
            score = n.token_score
        else:
            n = state.fail
            while tok not in n.next:
                n = n.fail
                if n is self.root:
                    break
            if tok in n.next:
                n = n.next[tok]
            score = n.node_score - state.node_score
        if not strict and n.output_score != 0:
            out = n.node_score if n.is_end else (n.output.node_score if n.output is not None else n.node_score)
            return score + out - n.node_score, self.root
        return score + n.output_score, n

    def finalize(self, state):
        return -state.node_score, self.root


# ---- the flat table, walked with numpy ------------------------------------------------------------------------------------------
class FlatView:
    """a flat table (reazonspeech_amd.runtime.k2_hotwords.concat) with the token path of every node, for comparisons"""

    def __init__(self, table):
        self.t = table
        n = len(table["fail"])
        self.parent, self.token = np.full(n, -1), np.full(n, -1)
        for p in range(n):
            for c in range(table["child_begin"][p], table["child_begin"][p + 1]):
                self.parent[table["child_node"][c]] = p
                self.token[table["child_node"][c]] = table["child_tok"][c]

    def path(self, n):
        out = []
        while self.parent[n] >= 0:
            out.append(int(self.token[n]))
            n = self.parent[n]
        return tuple(reversed(out))

    def child(self, n, tok):
        t = self.t
        lo, hi = t["child_begin"][n], t["child_begin"][n + 1]
        i = lo + int(np.searchsorted(t["child_tok"][lo:hi], tok))
        return int(t["child_node"][i]) if i < hi and t["child_tok"][i] == tok else -1

    def step(self, root, state, tok, strict=False):
        t = self.t
        n = self.child(state, tok)
        if n >= 0:
            score = float(t["token_score"][n])
        else:
            n = int(t["fail"][state])
            while self.child(n, tok) < 0 and n != root:
                n = int(t["fail"][n])
            c = self.child(n, tok)
            n = c if c >= 0 else n
            score = float(t["node_score"][n]) - float(t["node_score"][state])
        if not strict and t["output_score"][n] != 0:
            o = int(t["output"][n])
            out = t["node_score"][n] if t["is_end"][n] else (t["node_score"][o] if o >= 0 else t["node_score"][n])
            return score + float(out) - float(t["node_score"][n]), root
        return score + float(t["output_score"][n]), n

    def finalize(self, root, state):
        return -float(self.t["node_score"][state]), root


# ---- the search in float64 -------------------------------------------------------------------------------------------------------
def hw_float64(cfg, sd, f, graph, K=4, blank_penalty=0.0, length_norm=True, logits_fn=None, n_frames=None):
    """k2_mbs_ref.mbs_float64 with a ContextGraph (None = the plain search): the K best are selected without bonus; a selected
    candidate that appends a label steps the graph from its parent's state and adds the delta; merged candidates keep the first
    one's tokens, timestamps and state; Finalize before the winner.  Returns the fields of mbs_float64 that the tests read, plus
    `states` = the token path of every final hypothesis's state BEFORE Finalize and `bonus` = the deltas each final hypothesis
    itself collected (Finalize included)."""
    cs, blank, unk = cfg.context_size, cfg.blank_id, cfg.unk_id
    if logits_fn is None:
        logits_fn = R.model_logits_fn(cfg, sd, f)
        n_frames = len(f)
    hyps = [dict(ys=[-1] * (cs - 1) + [blank], ts=[], lp=0.0, ctx=graph.root if graph else None, bonus=0.0)]
    merges, frame_gaps = 0, []
    with torch.no_grad():
        for t in range(n_frames):
            rows = []
            for h in hyps:
                logits = torch.as_tensor(logits_fn(t, h["ys"]), dtype=torch.float64).clone()
                if blank_penalty > 0:
                    logits[blank] -= blank_penalty
                rows.append(torch.log_softmax(logits, 0) + h["lp"])
            flat = torch.cat(rows)
            V = rows[0].numel()
            order = torch.sort(flat, descending=True, stable=True).indices[:K + 1].tolist()
            vals = [float(flat[c]) for c in order]
            frame_gaps.append(min((a - b for a, b in zip(vals, vals[1:])), default=math.inf))
            new = []
            for c, lp in zip(order[:K], vals[:K]):
                h, v = hyps[c // V], c % V
                ys, ts, ctx, bonus = list(h["ys"]), list(h["ts"]), h["ctx"], h["bonus"]
                if v != blank and v != unk:
                    ys.append(v)
                    ts.append(t)
                    if graph is not None:
                        delta, ctx = graph.step(ctx, v)
                        lp, bonus = lp + delta, bonus + delta
                same = [e for e in new if e["ys"] == ys]
                if same:
                    same[0]["lp"] = float(np.logaddexp(same[0]["lp"], lp))
                    merges += 1
                else:
                    new.append(dict(ys=ys, ts=ts, lp=lp, ctx=ctx, bonus=bonus))
            hyps = new
    states = [h["ctx"].path() if graph else () for h in hyps]
    if graph is not None and n_frames > 0:
        for h in hyps:
            delta, h["ctx"] = graph.finalize(h["ctx"])
            h["lp"], h["bonus"] = h["lp"] + delta, h["bonus"] + delta
    norm = [h["lp"] / len(h["ys"]) if length_norm else h["lp"] for h in hyps]
    win = max(range(len(hyps)), key=lambda k: (norm[k], -k))
    top = sorted(norm, reverse=True)
    gi = int(np.argmin(frame_gaps)) if frame_gaps else -1
    return dict(ids=hyps[win]["ys"][cs:], frames=hyps[win]["ts"], score=hyps[win]["lp"], merges=merges,
                final=[(h["ys"][cs:], h["lp"]) for h in hyps], states=states, bonus=[h["bonus"] for h in hyps], frame_gaps=frame_gaps,
                min_gap=frame_gaps[gi] if frame_gaps else math.inf, min_gap_frame=gi,
                final_gap=top[0] - top[1] if len(top) > 1 else math.inf)


EMPTY_TABLE = R.EMPTY_TABLE


# ---- the graphs of the toy-geometry tests ---------------------------------------------------------------------------------------
def toy_graphs(plain, score=4.0):
    """Three phrase lists [(token ids, score)] chosen from the PLAIN search's results `plain` (mbs_checker at K = 4) so that the
    graphs are met by what the search proposes:
      A  cut from the final sets: per utterance the first tokens of the winner, the whole of its best runner-up that differs, and
         the winner's last two tokens followed by one that does not come (a match still pending at the last frame: Finalize)
      B  overlapping phrases over one winner's tokens w (the longest): w[0:4] + a token that does not follow (a partial match that
         is given up), its inner pieces w[1:3], w[2:4], w[1:5] (suffixes of each other: fail and output links) and w[3:4]
      C  one single-token phrase: the most frequent token of the winners"""
    a, seen = [], set()
    for r in plain:
        if len(r["ids"]) >= 2:
            a.append((tuple(r["ids"][:3]), score))
            a.append((tuple(r["ids"][-2:]) + (r["ids"][0],), score))
        others = [y for y, _ in r["final"] if y != r["ids"] and len(y) >= 1]
        if others:
            a.append((tuple(others[0]), score))
    a = [p for p in a if not (p in seen or seen.add(p))]
    w = max((r["ids"] for r in plain), key=len)
    assert len(w) >= 5, "the toy utterances must emit at least five tokens somewhere"
    b = [(tuple(w[0:4]) + (w[0],), 1.5), (tuple(w[1:3]), 2.0), (tuple(w[2:4]), 1.0), (tuple(w[1:5]), 1.5), (tuple(w[3:4]), 1.0)]
    flat = [t for r in plain for t in r["ids"]]
    c = [((max(set(flat), key=lambda t: (flat.count(t), -t)),), score)]
    return a, b, c
