"""Helpers of the tests of the n-gram LM in the modified beam search (tests/test_k2_mbs_lm_host.py, tests/test_gpu_k2_mbs_lm.py).
TEST INFRASTRUCTURE.

  mbs_lm_checker(...)   tests/k2_mbs_lm_checker.c through ctypes: the search of csrc/k_rnnt_mbs.hip restated in the device's float32
                        order — plain, with hotwords, with an n-gram LM — and its counters.  `inject` replaces decoder and joiner
                        by a table of logits (the hand-built cases).
  lm_float64(...)       k2_hotwords_ref.hw_float64 plus the LM rule of include/rs_asr.h (rs_rnnt_mbs_lm), in float64 over the
                        textbook dictionary backoff of ngram_lm_ref.ArpaDict; `dtype=torch.float32` runs the same text in float32
                        (how far rounding alone moves the scores: where the test's LINE comes from)
  toy_lm(plain, cfg)    an order-3 model cut from the plain search's final sets; random_lm(...) a large synthetic one
"""
import ctypes
import math
import os

import numpy as np
import torch

import checker_lib
import k2_mbs_ref as R
from ngram_lm_ref import ArpaDict, BOS  # noqa: F401
from oracle import greedy as og, zipformer as oz

MAX_K = 8
LM_COUNTERS = 14
vp, i32, f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_float


class HwTable(ctypes.Structure):
    _fields_ = [(k, vp) for k in ("child_begin", "child_tok", "child_node", "fail", "output", "is_end", "token_score", "node_score",
                                  "output_score", "graph_root")] + [("n_graphs", i32)]


class LmTable(ctypes.Structure):
    _fields_ = [(k, vp) for k in ("child_begin", "child_tok", "child_node", "root_child", "suffix", "level", "logp", "backoff")] + \
               [("n_nodes", i32), ("order", i32), ("start", i32), ("unk_logp", f32)]


def lib():
    L = checker_lib.load("k2_mbs_lm_checker.c")
    L.rs_k2_mbs_lm_checker.restype = ctypes.c_int
    return L


def _hw_struct(table):
    """-> (HwTable, the arrays it points into) of a flat hotword table (reazonspeech_amd.runtime.k2_hotwords.concat)"""
    keep = {k: np.ascontiguousarray(table[k], dtype=np.float32 if k.endswith("_score") else np.int32) for k, _ in HwTable._fields_[:-1]}
    return HwTable(*[keep[k].ctypes.data for k, _ in HwTable._fields_[:-1]], len(keep["graph_root"])), keep


def _lm_struct(lm):
    """-> (LmTable, the arrays it points into) of an NgramLm"""
    keep = {k: np.ascontiguousarray(lm.arrays[k], dtype=np.float32 if k in ("logp", "backoff") else np.int32) for k, _ in LmTable._fields_[:8]}
    return LmTable(*[keep[k].ctypes.data for k, _ in LmTable._fields_[:8]], lm.n_nodes, lm.order, lm.start, float(lm.unk_logp)), keep


def mbs_lm_checker(cfg, sd, f, enc_lens, table=None, graph_of=None, lm=None, alpha=0.0, K=4, blank_penalty=0.0, length_norm=True,
                   out_cap=None, workers=None, inject=None):
    """As k2_mbs_ref.mbs_checker (the same fields per utterance), plus `lm` (an NgramLm, None = no model) at weight `alpha`, and per
    utterance final_lm (the LM state of every final entry), hits [level 0..8], backoffs, unk, full_order_pops, state_mismatches,
    walks.  `inject` float32 [Tp][V][V]: logits of frame t for a hypothesis whose last token is u = inject[t][u]; then `sd` and `f`
    are not read (`f` only gives B and Tp, `cfg` V, blank_id and unk_id)."""
    L = lib()
    og.lib().rs_oracle_set_joint_act(1)                      # the Zipformer joiner is tanh
    f = np.ascontiguousarray(f, dtype=np.float32)
    B, Tp, J = f.shape
    fp, ip = og._fp, og._ip
    if inject is None:
        a = R.k2_arrays(sd)
        weights = [fp(a[k]) for k in ("embed", "conv_w", "wp", "bp", "wo", "bo")]
        D, inj = cfg.decoder_dim, None
    else:
        inject = np.ascontiguousarray(inject, dtype=np.float32)
        assert inject.shape == (Tp, cfg.vocab_size, cfg.vocab_size)
        weights, D, inj = [None] * 6, 0, fp(inject)
    enc_lens = np.ascontiguousarray(enc_lens, dtype=np.int32)
    hw, hw_keep = _hw_struct(table) if table is not None else (None, None)
    graph_of = None if graph_of is None else np.ascontiguousarray(graph_of, dtype=np.int32)
    assert graph_of is None or len(graph_of) == B
    lms, lm_keep = _lm_struct(lm) if lm is not None else (None, None)
    if out_cap is None:
        out_cap = max(Tp, 1)
    ids, frames = np.zeros((B, out_cap), np.int32), np.zeros((B, out_cap), np.int32)
    n_ids, merges, fin_n = np.zeros((B,), np.int32), np.zeros((B,), np.int32), np.zeros((B,), np.int32)
    scores = np.zeros((B,), np.float32)
    fin_len, fin_lp, fin_lm = np.zeros((B, MAX_K), np.int32), np.zeros((B, MAX_K), np.float32), np.zeros((B, MAX_K), np.int32)
    fin_y = np.zeros((B, MAX_K, out_cap), np.int32)
    counters, fin_total = np.zeros((B, 3), np.int32), np.zeros((B,), np.float32)
    lcnt = np.zeros((B, LM_COUNTERS), np.int32)

    def rows(b0, b1):
        return L.rs_k2_mbs_lm_checker(
            fp(f[b0:b1]), ip(enc_lens[b0:b1]), b1 - b0, Tp, J, D, cfg.vocab_size, cfg.blank_id, cfg.unk_id, *weights, inj, int(K),
            ctypes.c_float(blank_penalty), int(bool(length_norm)), int(out_cap), ip(ids[b0:b1]), ip(frames[b0:b1]), ip(n_ids[b0:b1]),
            fp(scores[b0:b1]), ip(merges[b0:b1]), ip(fin_n[b0:b1]), ip(fin_len[b0:b1]), fp(fin_lp[b0:b1]), ip(fin_lm[b0:b1]),
            ip(fin_y[b0:b1]), ctypes.byref(hw) if hw is not None else None, ip(graph_of[b0:b1]) if graph_of is not None else None,
            ip(counters[b0:b1]), fp(fin_total[b0:b1]), ctypes.byref(lms) if lms is not None else None, ctypes.c_float(alpha),
            ip(lcnt[b0:b1]))

    if workers is None:
        workers = min(16, os.cpu_count() or 1)
    if B > 1 and workers > 1:
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max_workers=min(workers, B)) as pool:
            rc = min(pool.map(lambda b: rows(b, b + 1), range(B)))
    else:
        rc = rows(0, B) if B else 0
    if rc != 0:
        raise RuntimeError(f"k2 mbs lm checker failed ({rc}; -5 = more than out_cap={out_cap} tokens)")
    out = []
    for b in range(B):
        final = [(fin_y[b, k, :fin_len[b, k]].tolist(), float(fin_lp[b, k])) for k in range(fin_n[b])]
        out.append(dict(ids=ids[b, :n_ids[b]].tolist(), frames=frames[b, :n_ids[b]].tolist(), score=float(scores[b]),
                        score_bits=int(scores[b:b + 1].view(np.int32)[0]), merges=int(merges[b]), final=final,
                        final_bits=[int(x) for x in fin_lp[b, :fin_n[b]].view(np.int32)], final_lm=fin_lm[b, :fin_n[b]].tolist(),
                        child_hits=int(counters[b, 0]), fail_transitions=int(counters[b, 1]), exits=int(counters[b, 2]),
                        finalize=float(fin_total[b]), hits=lcnt[b, :9].tolist(), backoffs=int(lcnt[b, 9]), unk=int(lcnt[b, 10]),
                        full_order_pops=int(lcnt[b, 11]), state_mismatches=int(lcnt[b, 12]), walks=int(lcnt[b, 13])))
    return out


def totals(rows, order):
    """the LM counters of a batch, summed"""
    return dict(hits=[sum(r["hits"][k] for r in rows) for k in range(1, order + 1)], backoffs=sum(r["backoffs"] for r in rows),
                unk=sum(r["unk"] for r in rows), full_order_pops=sum(r["full_order_pops"] for r in rows),
                state_mismatches=sum(r["state_mismatches"] for r in rows), walks=sum(r["walks"] for r in rows))


def all_counted(t):
    """found at level >= 2, backoff steps, unknown token, full-order pops: all met (and no merge of two different LM states)"""
    return sum(t["hits"][1:]) > 0 and all(t[k] > 0 for k in ("backoffs", "unk", "full_order_pops")) and t["state_mismatches"] == 0


RECHOOSE = "the LM is not met at every level on this projection: re-choose the inputs (tests/k2_mbs_lm_ref.py toy_lm)"


# ---- the search in float64 (or, for the rounding measurement, the same text in float32) --------------------------------------------
def lm_float64(cfg, sd, f, arpa=None, alpha=0.0, bos=False, graph=None, K=4, blank_penalty=0.0, length_norm=True, logits_fn=None,
               n_frames=None, dtype=torch.float64):
    """k2_hotwords_ref.hw_float64 plus the LM rule: the K best are selected without bonus and without LM term; a selected candidate
    that appends a label v adds the graph's delta, then alpha x arpa.logp(history, v), the history being the hypothesis's tokens (after
    `<s>` when `bos`).  Returns the fields of mbs_float64."""
    cs, blank, unk = cfg.context_size, cfg.blank_id, cfg.unk_id
    num = float if dtype == torch.float64 else np.float32
    if logits_fn is None:
        keys = ("decoder.embedding.weight", "decoder.conv.weight", "joiner.decoder_proj.weight", "joiner.decoder_proj.bias",
                "joiner.output_linear.weight", "joiner.output_linear.bias")
        sdt = {k: sd[k].to(dtype) for k in keys}
        ft = torch.as_tensor(np.asarray(f), dtype=dtype)
        wo, bo, cache = sdt["joiner.output_linear.weight"], sdt["joiner.output_linear.bias"], {}

        def logits_fn(t, ys):
            key = tuple(ys[-cs:])
            if key not in cache:
                cache[key] = oz.decoder_out(cfg, sdt, list(key)).to(dtype)
            return torch.tanh(ft[t] + cache[key]) @ wo.t() + bo
        n_frames = len(f)
    hyps = [dict(ys=[-1] * (cs - 1) + [blank], ts=[], lp=num(0.0), ctx=graph.root if graph else None)]
    merges, frame_gaps = 0, []
    with torch.no_grad():
        for t in range(n_frames):
            rows = []
            for h in hyps:
                logits = torch.as_tensor(logits_fn(t, h["ys"]), dtype=dtype).clone()
                if blank_penalty > 0:
                    logits[blank] -= blank_penalty
                rows.append(torch.log_softmax(logits, 0) + torch.as_tensor(h["lp"], dtype=dtype))
            flat = torch.cat(rows)
            V = rows[0].numel()
            order = torch.sort(flat, descending=True, stable=True).indices[:K + 1].tolist()
            vals = [num(flat[c]) for c in order]
            frame_gaps.append(min((float(a) - float(b) for a, b in zip(vals, vals[1:])), default=math.inf))
            new = []
            for c, lp in zip(order[:K], vals[:K]):
                h, v = hyps[c // V], c % V
                ys, ts, ctx = list(h["ys"]), list(h["ts"]), h["ctx"]
                if v != blank and v != unk:
                    if graph is not None:
                        delta, ctx = graph.step(ctx, v)
                        lp = num(lp + num(delta))
                    if arpa is not None and alpha:
                        term = arpa.logp(((BOS,) if bos else ()) + tuple(h["ys"][cs:]), v)
                        lp = num(lp + num(num(alpha) * num(term)))
                    ys.append(v)
                    ts.append(t)
                same = [e for e in new if e["ys"] == ys]
                if same:
                    same[0]["lp"] = num(np.logaddexp(same[0]["lp"], lp))
                    merges += 1
                else:
                    new.append(dict(ys=ys, ts=ts, lp=lp, ctx=ctx))
            hyps = new
    if graph is not None and n_frames > 0:
        for h in hyps:
            delta, h["ctx"] = graph.finalize(h["ctx"])
            h["lp"] = num(h["lp"] + num(delta))
    norm = [float(h["lp"]) / len(h["ys"]) if length_norm else float(h["lp"]) for h in hyps]
    win = max(range(len(hyps)), key=lambda k: (norm[k], -k))
    top = sorted(norm, reverse=True)
    gi = int(np.argmin(frame_gaps)) if frame_gaps else -1
    return dict(ids=hyps[win]["ys"][cs:], frames=hyps[win]["ts"], score=float(hyps[win]["lp"]), merges=merges,
                final=[(h["ys"][cs:], float(h["lp"])) for h in hyps], frame_gaps=frame_gaps,
                min_gap=frame_gaps[gi] if frame_gaps else math.inf, min_gap_frame=gi,
                final_gap=top[0] - top[1] if len(top) > 1 else math.inf)


# ---- fixtures --------------------------------------------------------------------------------------------------------------------
def toy_lm(plain, cfg, against_every=1):
    """an order-3 model cut from the PLAIN search's results `plain` (a checker's rows at K = 4), so that the search meets it at every
    level; every log10 value is a multiple of 1/8.  Unigrams for every token the final sets contain (another candidate is an unknown
    word: there is no `<unk>`, it costs the lowest unigram); `<s>` and the bigram `<s>` + the first token of every final entry; the
    bigrams and trigrams of the final entries with high probability — except a few that contradict the search: in every
    `against_every`-th row whose winner and a runner-up part ways at some token, the winner's bigram and trigram that end in its token
    there are unlikely (the runner-up's stay likely)
    -> entries {(ids...): (log10 p, log10 backoff)}"""
    bad = {cfg.blank_id, cfg.unk_id}
    seqs, against, n_forks = [], [], 0
    for r in plain:
        w = list(r["ids"])
        finals = [list(y) for y, _ in r["final"] if y]
        seqs += [y for y in [w] + finals if y and y not in seqs]
        for o in finals:
            k = next((q for q in range(min(len(w), len(o))) if w[q] != o[q]), None)
            if k is not None and k >= 1:
                n_forks += 1
                if n_forks % against_every == 0:
                    against.append(tuple(w[max(0, k - 2):k + 1]))
                break
    toks = sorted({t for y in seqs for t in y} - bad)
    assert toks, "the plain search must emit tokens"
    ent = {(t,): (-(1.0 + (t % 9) / 8.0), -(t % 3) / 8.0) for t in toks}
    ent[(BOS,)] = (-99.0, -0.25)
    for g in against:                                            # first: the n-grams of the other sequences do not overwrite them
        ent.setdefault(g[-2:], (-3.0, -0.125))
        if len(g) == 3:
            ent.setdefault(g[:2], (-0.25, -0.125))
            ent.setdefault(g, (-2.5, 0.0))
    for y in seqs:
        ent.setdefault((BOS, y[0]), (-0.125, -0.125))
        for k in range(len(y) - 1):
            ent.setdefault((y[k], y[k + 1]), (-0.25, -0.125 * (k % 2)))
        for k in range(len(y) - 2):
            ent.setdefault(tuple(y[k:k + 3]), (-0.125, 0.0))
        if len(y) >= 2:
            ent.setdefault((BOS, y[0], y[1]), (-0.125, 0.0))
    assert all(v * 8 == int(v * 8) for e in ent.values() for v in e)
    return ent


def random_lm(cfg, seqs, n_high=3000, order=4, seed=4):
    """an order-`order` model with a unigram for every token but the blank and <unk>, every n-gram (up to `order`, also after `<s>`) of
    the token sequences `seqs` (what the plain search proposes) and about `n_high` more higher-order n-grams drawn around their
    tokens, prefix-closed: long child lists below frequent contexts (the bisection), root_child for everything else"""
    rng = np.random.default_rng(seed)
    bad = {cfg.blank_id, cfg.unk_id}
    vocab = [t for t in range(cfg.vocab_size) if t not in bad]
    q = lambda lo, hi: float(rng.integers(lo * 8, hi * 8)) / 8.0                    # noqa: E731  multiples of 1/8
    ent = {(t,): (-q(1, 5), -q(0, 1)) for t in vocab}
    ent[(BOS,)] = (-99.0, -q(0, 1))
    seen = sorted({int(t) for y in seqs for t in y} - bad)
    for y in seqs:
        y = (BOS,) + tuple(int(t) for t in y)
        for k in range(len(y)):
            for m in range(2, min(order, len(y) - k) + 1):
                ent.setdefault(y[k:k + m], (-q(0, 1), -q(0, 1) if m < order else 0.0))
    for _ in range(n_high):
        n = int(rng.integers(2, order + 1))
        words = tuple(int(rng.choice(seen)) if rng.random() < 0.7 else int(rng.choice(vocab)) for _ in range(n))
        for k in range(2, n + 1):
            ent.setdefault(words[:k], (-q(0, 3), -q(0, 1) if k < order else 0.0))
    return ent


def unk_log10(ent):
    """what an unknown word costs in a model without `<unk>`: the lowest unigram (runtime/ngram_lm.py build)"""
    return min(p for k, (p, _) in ent.items() if len(k) == 1 and k != (BOS,))
