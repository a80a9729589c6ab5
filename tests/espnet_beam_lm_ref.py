"""Helpers of the tests of hotwords and n-gram LM fusion in ESPnet's default beam search (tests/test_espnet_beam_lm_host.py,
tests/test_gpu_espnet_beam_lm.py).  TEST INFRASTRUCTURE.

  lm_checker(...)        tests/espnet_beam_lm_checker.c through ctypes: the search of csrc/k_rnnt_beam.hip restated in the device's
                         float32 order in all its forms — plain, n-best, hotwords, LM, both — and the counters that show which edge
                         a fixture reaches.  `inject` replaces prediction network and joint by a table of logits (the hand-built cases).
  beam_lm_float64(...)   [UPSTREAM, not vendored, UNVERIFIED] espnet2 BeamSearchTransducer.default_beam_search + sort_nbest with the
                         LM term on every label extension it opens, written from the algorithm in include/rs_asr.h
                         (rs_rnnt_beam_lm) in float64 over the textbook dictionary backoff of ngram_lm_ref.ArpaDict and the
                         pointer graph of k2_hotwords_ref.ContextGraph — nothing of the product's tables or walks
  as_plain(rows)         a checker's rows in the shape the fixtures of k2_hotwords_ref.toy_graphs / k2_mbs_lm_ref.toy_lm read
"""
import ctypes
import os
import types

import numpy as np

import checker_lib
from espnet_beam_nbest_ref import bits, f32, model_logp_fn  # noqa: F401
from k2_mbs_lm_ref import LM_COUNTERS, _hw_struct, _lm_struct
from ngram_lm_ref import BOS
from oracle import greedy as og

NB_COUNTERS = 6


def lib():
    L = checker_lib.load("espnet_beam_lm_checker.c")
    L.rs_espnet_beam_lm_checker.restype = ctypes.c_int
    return L


def lm_checker(cfg, sd, f, enc_lens, nbest=0, beam=20, score_norm=True, max_pops=None, out_cap=None, table=None, graph_of=None, lm=None,
               alpha=0.0, workers=None, inject=None, check=True):
    """-> per utterance dict(entries=[(ids, frames, score bits, norm bits)] best first (n_hyps of them; nbest = 0: the one result),
    n_ids, pops, kept, duplicates, ties, norm_reorders, pop_ties, finalize_reorders, child_hits, fail_transitions, exits, finalize,
    hits [level 0..8], backoffs, unk, full_order_pops, walks).  f float32 [B][Tp][J].  `table` = a flat hotword table
    (runtime.k2_hotwords.concat) with `graph_of` [B]; `lm` = an NgramLm at weight `alpha`.  `inject` float32 [Tp][V][V]: the logits of
    frame t for a hypothesis whose last label is u = inject[t][u]; then `sd` and `f` are not read.  `check` False: an overflow returns
    what was written."""
    L = lib()
    og.lib().rs_oracle_set_joint_act(1 if getattr(cfg, "espnet", False) else 0)
    f = np.ascontiguousarray(f, dtype=np.float32)
    B, Tp, J = f.shape
    fp, ip = og._fp, og._ip
    PF = ctypes.POINTER(ctypes.c_float)
    if inject is None:
        arr = og.decoder_arrays(cfg, sd)
        wl = (PF * cfg.pred_layers)(*[fp(w) for w in arr["lstm_w"]])
        bl = (PF * cfg.pred_layers)(*[fp(b) for b in arr["lstm_b"]])
        weights = [fp(arr["embed"]), wl, bl, fp(arr["Wp"]), fp(arr["bp"]), fp(arr["Wo"]), fp(arr["bo"])]
        inj = None
    else:
        inject = np.ascontiguousarray(inject, dtype=np.float32)
        assert inject.shape == (Tp, cfg.n_logits, cfg.n_logits)
        weights, inj = [None] * 7, fp(inject)
    enc_lens = np.ascontiguousarray(enc_lens, dtype=np.int32)
    hw, hw_keep = _hw_struct(table) if table is not None else (None, None)
    graph_of = None if graph_of is None else np.ascontiguousarray(graph_of, dtype=np.int32)
    assert graph_of is None or len(graph_of) == B
    lms, lm_keep = _lm_struct(lm) if lm is not None else (None, None)
    if max_pops is None:
        max_pops = 16 * int(beam)
    if out_cap is None:
        out_cap = max(1, Tp * 4)
    N = max(int(nbest), 1)
    ids, frames = np.zeros((B, N, out_cap), np.int32), np.zeros((B, N, out_cap), np.int32)
    n_ids, n_hyps = np.full((B, N), -1, np.int32), np.full((B,), -1, np.int32)
    scores, norms = np.zeros((B, N), np.float32), np.zeros((B, N), np.float32)
    pops, nbc = np.zeros((B,), np.int32), np.zeros((B, NB_COUNTERS), np.int32)
    hcnt, fin_total, lcnt = np.zeros((B, 3), np.int32), np.zeros((B,), np.float32), np.zeros((B, LM_COUNTERS), np.int32)

    def rows(b0, b1):
        return L.rs_espnet_beam_lm_checker(
            fp(f[b0:b1]), ip(enc_lens[b0:b1]), b1 - b0, Tp, J, cfg.pred_hidden, cfg.pred_layers, cfg.n_logits, cfg.blank_id, *weights, inj,
            int(beam), int(bool(score_norm)), int(max_pops), int(nbest), int(out_cap), ip(ids[b0:b1]), ip(frames[b0:b1]), ip(n_ids[b0:b1]),
            fp(scores[b0:b1]), fp(norms[b0:b1]), ip(n_hyps[b0:b1]), ip(pops[b0:b1]), ip(nbc[b0:b1]),
            ctypes.byref(hw) if hw is not None else None, ip(graph_of[b0:b1]) if graph_of is not None else None, ip(hcnt[b0:b1]),
            fp(fin_total[b0:b1]), ctypes.byref(lms) if lms is not None else None, ctypes.c_float(alpha), ip(lcnt[b0:b1]))

    if workers is None:
        workers = min(16, os.cpu_count() or 1)
    if B > 1 and workers > 1:
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max_workers=min(workers, B)) as pool:
            rc = min(pool.map(lambda b: rows(b, b + 1), range(B)))
    else:
        rc = rows(0, B) if B else 0
    if rc == -1 or (rc != 0 and check):
        raise RuntimeError(f"espnet beam lm checker failed ({rc}; -5 = overflow of max_pops={max_pops} / out_cap={out_cap}, -1 = nbest outside 0..beam)")
    sb, nb = scores.view(np.int32), norms.view(np.int32)
    out = []
    for b in range(B):
        entries = [(ids[b, r, :n_ids[b, r]].tolist(), frames[b, r, :n_ids[b, r]].tolist(), int(sb[b, r]), int(nb[b, r])) for r in range(n_hyps[b])]
        out.append(dict(entries=entries, n_ids=n_ids[b].tolist(), pops=int(pops[b]), kept=int(nbc[b, 0]), duplicates=int(nbc[b, 1]),
                        ties=int(nbc[b, 2]), norm_reorders=int(nbc[b, 3]), pop_ties=int(nbc[b, 4]), finalize_reorders=int(nbc[b, 5]),
                        child_hits=int(hcnt[b, 0]), fail_transitions=int(hcnt[b, 1]), exits=int(hcnt[b, 2]), finalize=float(fin_total[b]),
                        hits=lcnt[b, :9].tolist(), backoffs=int(lcnt[b, 9]), unk=int(lcnt[b, 10]), full_order_pops=int(lcnt[b, 11]),
                        walks=int(lcnt[b, 13])))
    return out


def as_plain(rows):
    """a checker's n-best rows as the fixtures of the k2 tests read a search's results: ids = the winner, final = the whole list"""
    return [dict(ids=list(r["entries"][0][0]) if r["entries"] else [], final=[(list(e[0]), f32(e[2])) for e in r["entries"]]) for r in rows]


def fixture_cfg(cfg):
    """what k2_mbs_lm_ref.toy_lm / random_lm read of a configuration; ESPnet's token list has no id the LM must avoid but the blank"""
    return types.SimpleNamespace(blank_id=cfg.blank_id, unk_id=-1, vocab_size=cfg.n_logits)


def toy_lm(plain, cfg, disliked=-6.0):
    """k2_mbs_lm_ref.toy_lm (order 3, cut from the plain search's lists `plain`, so that the search meets it at every level: hits at
    levels 1..3, backoffs, unknown tokens, full-order pops) with one change that makes the model contradict the search at EVERY beam:
    the most frequent label of the lists is unlikely (log10 p = `disliked`) in every context the model has for it
    -> entries {(ids...): (log10 p, log10 backoff)}"""
    from k2_mbs_lm_ref import toy_lm as k2_toy_lm
    ent = k2_toy_lm(plain, fixture_cfg(cfg))
    flat = [t for r in plain for y, _ in r["final"] for t in y]
    x = max(set(flat), key=lambda t: (flat.count(t), -t))
    for k in list(ent):
        if k[-1] == x:
            ent[k] = (float(disliked), ent[k][1])
    return ent


# ---- the search in float64 ---------------------------------------------------------------------------------------------------------
def beam_lm_float64(logp_fn, n_frames, V, blank, beam=20, score_norm=True, arpa=None, alpha=0.0, bos=True, graph=None, nbest=None):
    """default_beam_search with the terms of include/rs_asr.h (rs_rnnt_beam_lm), in float64, over `logp_fn(t, yseq) -> float64
    log-softmax [V]` (yseq includes the leading blank).  `arpa`: an ngram_lm_ref.ArpaDict at weight `alpha` (`bos`: histories start
    after `<s>`); `graph`: a k2_hotwords_ref.ContextGraph.  The states are functions of the label sequence: the LM reads the labels,
    the graph's node is carried.
    -> (ranked [(ids, score, norm)] over the kept list (the first `nbest`), the least distance between two scores the search compared)"""
    beam = min(beam, V)
    beam_k = min(beam, V - 1)
    labels = [v for v in range(V) if v != blank]
    kept = [dict(score=0.0, yseq=[blank], ctx=graph.root if graph is not None else None)]
    min_gap = np.inf
    for t in range(n_frames):
        hyps, kept = kept, []
        while True:
            mi = max(range(len(hyps)), key=lambda i: (hyps[i]["score"], -i))
            mh = hyps.pop(mi)
            logp = np.asarray(logp_fn(t, mh["yseq"]), np.float64)
            order = sorted(labels, key=lambda v: (-logp[v], v))[:beam_k]          # logp[1:].topk(beam_k): no term inside
            kept.append(dict(score=mh["score"] + float(logp[blank]), yseq=mh["yseq"], ctx=mh["ctx"]))
            for v in order:
                sc, ctx = mh["score"] + float(logp[v]), mh["ctx"]
                if graph is not None:
                    delta, ctx = graph.step(ctx, v)
                    sc += delta
                if arpa is not None and alpha:
                    sc += alpha * arpa.logp(((BOS,) if bos else ()) + tuple(mh["yseq"][1:]), v)
                hyps.append(dict(score=sc, yseq=mh["yseq"] + [v], ctx=ctx))
            hmax = max(h["score"] for h in hyps)
            best = sorted([h for h in kept if h["score"] > hmax], key=lambda h: h["score"])
            every = sorted(h["score"] for h in kept + hyps)
            min_gap = min(min_gap, min((b - a for a, b in zip(every, every[1:])), default=np.inf))
            if len(best) >= beam:
                kept = best
                break
    if graph is not None and n_frames > 0:
        for h in kept:
            h["score"] += graph.finalize(h["ctx"])[0]
    norm = lambda h: h["score"] / len(h["yseq"]) if score_norm else h["score"]       # noqa: E731
    ranked = sorted(kept, key=norm, reverse=True)                                    # Python's sort: stable, as upstream's
    norms = sorted((norm(h) for h in kept), reverse=True)
    min_gap = min(min_gap, min((a - b for a, b in zip(norms, norms[1:])), default=np.inf))
    return [(h["yseq"][1:], h["score"], norm(h)) for h in ranked][:nbest], min_gap


# ---- fixtures shared by the host and the device tests ---------------------------------------------------------------------------------
TOY_LENS = [24, 17, 1, 9, 0, 20, 13]          # seven ragged utterances, one of a single frame and one without frames
TOY_GRAPH_OF = [0, 1, 2, -1, 0, 2, -1]        # graphs A, B, C and "none" over the seven rows
TOY_ALPHA = 0.5
TOY_SCORE = 2.5                               # per token of a phrase of graphs A and C: above it a row's search stops converging (a bonus
                                              # that outweighs every label's log-probability extends a hypothesis without end: RS_EOVERFLOW)
TOY_SEED, TOY_BIAS = 11, 12.0                 # chosen so that the float64 restatement agrees on every row (tests/test_espnet_beam_lm_host.py)
_toy = {}


def toy():
    """the toy geometry, computed once and left unchanged: ESPNET_TINY with synthetic weights, the float32 ORACLE's projection of seven
    2 s utterances cut to 24 frames (so that the host and the device tests search the same numbers), the plain search's lists on
    the first five rows (beam 4), three graphs and an order-3 LM cut from them
    -> dict(cfg, sd, f [7][24][J], lens, plain, phrases (A, B, C), graphs, table, lm_entries, lm, arpa)"""
    if not _toy:
        from ngram_lm_ref import ArpaDict
        import k2_hotwords_ref as H
        from k2_mbs_lm_ref import unk_log10
        from reazonspeech_amd.runtime import k2_hotwords as kh, ngram_lm as NL
        from reazonspeech_amd.runtime.config import ESPNET_TINY as cfg
        from test_oracle_espnet_beam import _inputs
        sd, f, _ = _inputs(cfg, TOY_SEED, len(TOY_LENS), 2.0, TOY_BIAS)
        f = np.ascontiguousarray(f.numpy()[:, :24])
        lens = np.asarray(TOY_LENS, np.int32)
        plain = as_plain(lm_checker(cfg, sd, f[:5], lens[:5], 4, beam=4))
        phrases = H.toy_graphs(plain, score=TOY_SCORE)
        graphs = [kh.build_graph(p) for p in phrases]
        ent = toy_lm(plain, cfg)
        lm = NL.build(ent, cfg.n_logits, cfg.blank_id)
        _toy.update(cfg=cfg, sd=sd, f=f, lens=lens, plain=plain, phrases=phrases, graphs=graphs, table=kh.concat(graphs), lm_entries=ent, lm=lm,
                    arpa=ArpaDict(ent, lm.order, unk_log10(ent)))
    return _toy


# the hand-built edges: the `flat_model` idiom of tests/test_gpu_nbest_espnet.py — lin_out.weight = 0, the bias gives the label
# probabilities, the same at every frame for every hypothesis.  Labels A, B, C; every case is one utterance of T frames.
A, B, C = 10, 11, 12
EDGE_PROBS = {0: .4, A: .3, B: .25, C: .04}
TIE_PROBS = {0: .5, A: .25, B: .125, C: .05}  # a bonus of log 2 lifts B onto A; that the two scores then tie bit for bit is asserted where it is used
EDGES = dict(
    lm_changes_the_winner=dict(T=2, beam=2, nbest=2, lm={(A,): (-2.0, 0.0), (B,): (-0.125, 0.0)}, alpha=1.0),
    lm_backoff_and_unk=dict(T=2, beam=3, nbest=3, lm={(A,): (-0.5, -0.25), (B,): (-0.5, -0.125), (A, B): (-0.125, 0.0)}, alpha=0.5),
    lm_order_1=dict(T=2, beam=2, nbest=2, lm={(A,): (-1.0, 0.0), (B,): (-0.25, 0.0), (C,): (-0.5, 0.0)}, alpha=1.0),
    phrase_completed=dict(T=2, beam=4, nbest=4, phrases=[((A, B), 1.2)], max_pops=400),
    phrase_abandoned=dict(T=2, beam=6, nbest=6, phrases=[((B, C, C), 0.5)], max_pops=400),
    phrase_open_at_the_end=dict(T=1, beam=2, nbest=2, phrases=[((A, B, C), 1.0)]),
    overlapping_phrases=dict(T=3, beam=3, nbest=3, phrases=[((A, B, C), 0.5), ((B,), 1.0)], max_pops=400),
    more_pops=dict(T=3, beam=3, nbest=3, phrases=[((A,), 1.0)], max_pops=200),
    tie_after_the_terms=dict(T=1, beam=2, nbest=2, probs=TIE_PROBS, phrases=[((B,), float(np.log(2.0)))]),
)


def flat_sd(probs, cfg=None):
    """an ESPnet-shaped toy whose joint ignores its inputs: label v has probability probs[v] (up to the softmax's normalisation) at
    every frame for every hypothesis, the rest of the vocabulary lies far below -> (cfg, state dict)"""
    import torch
    from reazonspeech_amd.runtime.config import ESPNET_TINY
    from reazonspeech_amd.runtime.weights_espnet import synthetic_state_dict_espnet
    cfg = cfg or ESPNET_TINY
    sd = synthetic_state_dict_espnet(cfg, 7, blank_bias=0.0, dec_gain=8.0)
    bias = np.full((cfg.n_logits,), np.log(1e-9), np.float32)
    for v, p in probs.items():
        bias[v] = np.float32(np.log(p))
    sd["joint_network.lin_out.weight"] = torch.zeros_like(sd["joint_network.lin_out.weight"])
    sd["joint_network.lin_out.bias"] = torch.from_numpy(bias)
    return cfg, sd


def flat_logp(probs, cfg):
    """the float64 log-softmax of `flat_sd`'s joint row"""
    z = np.full((cfg.n_logits,), np.log(1e-9), np.float32)
    for v, p in probs.items():
        z[v] = np.float32(np.log(p))
    z = z.astype(np.float64)
    return z - np.log(np.exp(z).sum())


def edge_tables(case, cfg):
    """-> (graphs or None, NgramLm or None, alpha) of a case of EDGES"""
    from reazonspeech_amd.runtime import k2_hotwords as kh, ngram_lm as NL
    graphs = [kh.build_graph(case["phrases"])] if case.get("phrases") else None
    lm = NL.build(case["lm"], cfg.n_logits, cfg.blank_id) if case.get("lm") else None
    return graphs, lm, case.get("alpha", 0.0)


def run_edge(name, with_terms=True, **over):
    """the checker on a case of EDGES (`with_terms` False: the plain search on the same model) -> its row"""
    from reazonspeech_amd.runtime import k2_hotwords as kh
    case = dict(EDGES[name], **over)
    cfg, sd = flat_sd(case.get("probs", EDGE_PROBS))
    graphs, lm, alpha = edge_tables(case, cfg) if with_terms else (None, None, 0.0)
    T = case["T"]
    return lm_checker(cfg, sd, np.zeros((1, T, cfg.joint_hidden), np.float32), [T], case["nbest"], beam=case["beam"],
                      max_pops=case.get("max_pops"), table=kh.concat(graphs) if graphs else None, graph_of=[0] if graphs else None, lm=lm,
                      alpha=alpha)[0]
