"""Helpers of the ALSD hotword and LM tests (tests/test_alsd_hotwords_host.py, tests/test_alsd_lm_host.py and their GPU tests).
TEST INFRASTRUCTURE.

  alsd_checker(...)      tests/alsd_checker.c through ctypes: the device's float32 order with hotwords and LM, and its counters
  hw_float64(...)        oracle/alsd.py's search plus the context rules of include/rs_asr.h (rs_rnnt_alsd_hotwords), in float64,
                         over the pointer graph of tests/k2_hotwords_ref.py (ContextGraph)
  toy_batch / toy_graphs the ragged toy-geometry batch of the GPU test and three phrase lists cut from the plain search's results
"""
import ctypes

import numpy as np
import torch

import checker_lib
import k2_mbs_ref as R
from oracle import alsd as oalsd, greedy as og
from reazonspeech_amd.runtime import k2_hotwords

MAX_BEAM = 8
COUNTERS = ("child_hits", "fail_transitions", "exits", "finalized", "recombinations", "state_mismatches")
LM_COUNTERS = 14
EMPTY_TABLE = R.EMPTY_TABLE


def lib():
    L = checker_lib.load("alsd_checker.c")
    L.rs_alsd_checker.restype = ctypes.c_int
    return L


def table_of(phrase_lists):
    """[[(token ids, score)], ...] -> the flat table of the graphs, one per list (runtime/k2_hotwords.py)"""
    return k2_hotwords.concat([k2_hotwords.build_graph(p) for p in phrase_lists])


def alsd_checker(cfg, sd, f, enc_lens, table=None, graph_of=None, lm=None, alpha=0.0, beam=4, max_target_len=2.0, score_norm=True,
                 merge=False, out_cap=None, inject=None, dims=None):
    """as oracle.greedy.rnnt_alsd, with the flat table of the call's graphs (None = no graph), graph_of int [B] (-1 = none), and an
    NgramLm with its weight (None / 0 = no LM).
    -> per utterance a dict: ids, steps, score, score_bits, the COUNTERS, finalize (the Finalize delta inside the score), hits
    [order + 1] (by level), backoffs, unk, full_order_pops, lm_mismatches, and beam = [(labels, score, hotword state, LM state)] as the
    search left it.
    inject [Tp][V][V] with dims = (V, blank): logits by (frame, last label + 1) instead of the networks (cfg, sd, f unused)."""
    L = lib()
    enc_lens = np.ascontiguousarray(enc_lens, dtype=np.int32)
    B = len(enc_lens)
    PF = ctypes.POINTER(ctypes.c_float)
    fp, ip = og._fp, og._ip
    if inject is None:
        arr = og.decoder_arrays(cfg, sd)
        f = np.ascontiguousarray(f, dtype=np.float32)
        assert f.shape[0] == B
        _, Tp, J = f.shape
        H, NL, V, blank = cfg.pred_hidden, cfg.pred_layers, cfg.n_logits, cfg.blank_id
        wl = (PF * NL)(*[fp(w) for w in arr["lstm_w"]])
        bl = (PF * NL)(*[fp(b) for b in arr["lstm_b"]])
        net = (fp(f), fp(arr["embed"]), wl, bl, fp(arr["Wp"]), fp(arr["bp"]), fp(arr["Wo"]), fp(arr["bo"]))
        og.lib().rs_oracle_set_joint_act(0)
        inj = None
    else:
        inject = np.ascontiguousarray(inject, dtype=np.float32)
        V, blank = dims
        Tp = inject.shape[0]
        assert inject.shape == (Tp, V, V)
        J, H, NL = 1, 1, 1
        net = (None,) * 8
        inj = fp(inject)
    u_max = og.alsd_budget(enc_lens, max_target_len)
    if out_cap is None:
        out_cap = max(1, int((enc_lens + u_max).max())) if B else 1
    table = table if table is not None else EMPTY_TABLE
    tab = {k: np.ascontiguousarray(v, dtype=np.float32 if k.endswith("_score") else np.int32) for k, v in table.items() if k != "max_level"}
    graph_of = np.ascontiguousarray(graph_of if graph_of is not None else np.full(B, -1), dtype=np.int32)
    assert len(graph_of) == B
    ids, steps = np.zeros((B, out_cap), np.int32), np.zeros((B, out_cap), np.int32)
    n_ids, scores = np.zeros((B,), np.int32), np.zeros((B,), np.float32)
    counters, fin = np.zeros((B, len(COUNTERS)), np.int32), np.zeros((B,), np.float32)
    beam_n, beam_len, beam_state = np.zeros((B,), np.int32), np.zeros((B, MAX_BEAM), np.int32), np.zeros((B, MAX_BEAM), np.int32)
    beam_score, beam_y = np.zeros((B, MAX_BEAM), np.float32), np.zeros((B, MAX_BEAM, out_cap), np.int32)
    lmc, beam_lm = np.zeros((B, LM_COUNTERS), np.int32), np.zeros((B, MAX_BEAM), np.int32)
    if lm is not None:
        assert lm.n_logits == V, (lm.n_logits, V)
        a = lm.arrays
        lm_args = (ip(a["child_begin"]), ip(a["child_tok"]), ip(a["child_node"]), ip(a["root_child"]), fp(a["logp"]), fp(a["backoff"]),
                   ip(a["suffix"]), ip(a["level"]), lm.n_nodes, lm.order, lm.start, ctypes.c_float(float(lm.unk_logp)))
    else:
        lm_args = (None,) * 8 + (0, 1, 0, ctypes.c_float(0.0))
    rc = L.rs_alsd_checker(
        net[0], ip(enc_lens), B, Tp, J, H, NL, V, blank, net[1], net[2], net[3], net[4], net[5], net[6], net[7], int(beam), ip(u_max),
        int(bool(score_norm)), int(bool(merge)), int(out_cap), ip(ids), ip(steps), ip(n_ids), fp(scores),
        ip(tab["child_begin"]), ip(tab["child_tok"]), ip(tab["child_node"]), ip(tab["fail"]), ip(tab["output"]), ip(tab["is_end"]),
        fp(tab["token_score"]), fp(tab["node_score"]), fp(tab["output_score"]), ip(tab["graph_root"]), len(tab["graph_root"]),
        ip(graph_of), ip(counters), fp(fin), inj, ip(beam_n), ip(beam_len), ip(beam_state), fp(beam_score), ip(beam_y),
        *lm_args, ctypes.c_float(float(alpha)), ip(lmc), ip(beam_lm))
    if rc != 0:
        raise RuntimeError(f"alsd checker failed ({rc}; -5 = more than out_cap={out_cap} labels)")
    out = []
    for b in range(B):
        d = dict(ids=ids[b, :n_ids[b]].tolist(), steps=steps[b, :n_ids[b]].tolist(), score=float(scores[b]),
                 score_bits=int(scores[b:b + 1].view(np.int32)[0]), finalize=float(fin[b]),
                 beam=[(beam_y[b, k, :beam_len[b, k]].tolist(), float(beam_score[b, k]), int(beam_state[b, k]), int(beam_lm[b, k]))
                       for k in range(beam_n[b])],
                 hits=lmc[b, :9].tolist(), backoffs=int(lmc[b, 9]), unk=int(lmc[b, 10]), full_order_pops=int(lmc[b, 11]),
                 lm_mismatches=int(lmc[b, 13]))
        d.update({name: int(counters[b, i]) for i, name in enumerate(COUNTERS)})
        assert d["recombinations"] == lmc[b, 12]             # counted once among the hotword counters, once among the LM's
        out.append(d)
    return out


# ---- the search in float64 -------------------------------------------------------------------------------------------------------
def hw_float64(cfg, sd, f, t_len, graph=None, beam=4, max_target_len=2.0, score_norm=True, recombine="upstream"):
    """oracle/alsd.py: alsd_decode for ONE utterance with a KR.ContextGraph (None = the plain search): a label expansion steps the
    graph from its hypothesis's state and carries the delta INTO the ranking; the blank keeps score and state; recombination keeps
    the first occurrence; a finished hypothesis (and, when nothing finished, every beam entry) gets Finalize before the winner is
    chosen.  -> (labels, alignment steps, score) of the winner."""
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
                cands.append(dict(y=h["y"] + [int(k)], score=h["score"] + float(lp) + delta, ts=h["ts"] + [i], st=new_state, ctx=ctx))
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


# ---- the toy-geometry fixture ------------------------------------------------------------------------------------------------------
TOY_GRAPH_OF = [0, 1, -1, 2, -1, 1, 0]


def toy_batch(cfg, seed=7, B=7, Tp=21):
    """B ragged rows on a random projection (as tests/test_gpu_alsd.py builds one): one row with zero frames, one of full length"""
    g = torch.Generator().manual_seed(seed)
    f = torch.randn((B, Tp, cfg.joint_hidden), generator=g) * (0.7 + 0.6 * torch.rand((B, 1, 1), generator=g))
    lens = torch.randint(6, Tp + 1, (B,), generator=g, dtype=torch.int32)
    lens[2] = 0
    lens[5] = Tp
    return f, lens


def toy_graphs(plain):
    """Three phrase lists [(token ids, score)] chosen from the PLAIN search's results `plain` (alsd_checker without a table at beam
    4), so that the graphs are met by what the search proposes; every score is a multiple of 0.5:
      A  cut from the winners: per utterance the winner's first three labels, the labels of its best beam entry that differs, and
         the winner's last two labels followed by one that does not come (a match still pending at the end: Finalize)
      B  overlapping phrases over one winner's labels w (the longest): w[0:4] + a label that does not follow (a partial match that
         is given up), its inner pieces w[1:3], w[2:4], w[1:5] (suffixes of each other: fail and output links) and w[3:4]
      C  one single-token phrase: the most frequent label of the winners"""
    a, seen = [], set()
    for r in plain:
        if len(r["ids"]) >= 2:
            a.append((tuple(r["ids"][:3]), 2.0))
            a.append((tuple(r["ids"][-2:]) + (r["ids"][0],), 2.0))
        others = [y for y, *_ in r["beam"] if y != r["ids"] and len(y) >= 1]
        if others:
            a.append((tuple(others[0]), 2.0))
    a = [p for p in a if not (p in seen or seen.add(p))]
    w = max((r["ids"] for r in plain), key=len)
    assert len(w) >= 5, "the toy utterances must emit at least five labels somewhere"
    b = [(tuple(w[0:4]) + (w[0],), 1.5), (tuple(w[1:3]), 2.0), (tuple(w[2:4]), 1.0), (tuple(w[1:5]), 1.5), (tuple(w[3:4]), 1.0)]
    flat = [t for r in plain for t in r["ids"]]
    c = [((max(set(flat), key=lambda t: (flat.count(t), -t)),), 2.0)]
    return a, b, c


def same_bits(a, b):
    return np.float32(a).tobytes() == np.float32(b).tobytes()


def bits(x):
    return int(np.asarray([x], np.float32).view(np.int32)[0])

