"""Helpers of the tests of the n-best lists of the ALSD beam search (tests/test_nbest_alsd_host.py, tests/test_gpu_nbest_alsd.py).
TEST INFRASTRUCTURE.

  nbest_checker(...)    tests/alsd_nbest_checker.c through ctypes: the search of csrc/k_rnnt_alsd.hip with the ranked list of
                        rs_rnnt_alsd_nbest restated in the device's float32 order — plain, hotwords, n-gram LM, both; merge on and off —
                        and the counters that show which edge a fixture reaches.  Arguments as alsd_hotwords_ref.alsd_checker.
  final_float64(...)    oracle/alsd.py's search in float64 with its whole `final` list (alsd_hotwords_ref.hw_float64 returns the
                        winner only), ranked by the rule of include/rs_asr.h with equal label sequences removed
"""
import ctypes

import numpy as np
import torch

import checker_lib
from alsd_hotwords_ref import EMPTY_TABLE, LM_COUNTERS, MAX_BEAM
from oracle import alsd as oalsd, greedy as og

NB_COUNTERS = ("offered", "evicted", "equal_met", "equal_replaced", "cross_step_ties", "budget_exit", "finalize_reorders")


def lib():
    L = checker_lib.load("alsd_nbest_checker.c")
    L.rs_alsd_nbest_checker.restype = ctypes.c_int
    return L


def bits(x):
    return int(np.asarray([x], np.float32).view(np.int32)[0])


def f32(b):
    return float(np.asarray([b], np.int32).view(np.float32)[0])


def nbest_checker(cfg, sd, f, enc_lens, nbest, table=None, graph_of=None, lm=None, alpha=0.0, beam=4, max_target_len=2.0, score_norm=True,
                  merge=False, out_cap=None, inject=None, dims=None):
    """-> per utterance dict(entries=[(ids, steps, score bits, norm bits)] best first (n_hyps of them), n_ids=[nbest counts], the
    NB_COUNTERS, beam=[(labels, score)] as the search left it).  inject [Tp][V][V] with dims = (V, blank): logits by (frame, last
    label + 1) instead of the networks (cfg, sd, f unused)."""
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
    N = int(nbest)
    ids, steps = np.zeros((B, N, out_cap), np.int32), np.zeros((B, N, out_cap), np.int32)
    n_ids, n_hyps, nbc = np.full((B, N), -1, np.int32), np.full((B,), -1, np.int32), np.zeros((B, len(NB_COUNTERS)), np.int32)
    scores, norms = np.zeros((B, N), np.float32), np.zeros((B, N), np.float32)
    counters, fin = np.zeros((B, 6), np.int32), np.zeros((B,), np.float32)
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
    rc = L.rs_alsd_nbest_checker(
        net[0], ip(enc_lens), B, Tp, J, H, NL, V, blank, net[1], net[2], net[3], net[4], net[5], net[6], net[7], int(beam), ip(u_max),
        int(bool(score_norm)), int(bool(merge)), N, int(out_cap), ip(ids), ip(steps), ip(n_ids), fp(scores), fp(norms), ip(n_hyps), ip(nbc),
        ip(tab["child_begin"]), ip(tab["child_tok"]), ip(tab["child_node"]), ip(tab["fail"]), ip(tab["output"]), ip(tab["is_end"]),
        fp(tab["token_score"]), fp(tab["node_score"]), fp(tab["output_score"]), ip(tab["graph_root"]), len(tab["graph_root"]),
        ip(graph_of), ip(counters), fp(fin), inj, ip(beam_n), ip(beam_len), ip(beam_state), fp(beam_score), ip(beam_y),
        *lm_args, ctypes.c_float(float(alpha)), ip(lmc), ip(beam_lm))
    if rc != 0:
        raise RuntimeError(f"alsd n-best checker failed ({rc}; -5 = more than out_cap={out_cap} labels, -1 = beam or nbest out of range)")
    sb, nb = scores.view(np.int32), norms.view(np.int32)
    out = []
    for b in range(B):
        d = dict(entries=[(ids[b, r, :n_ids[b, r]].tolist(), steps[b, r, :n_ids[b, r]].tolist(), int(sb[b, r]), int(nb[b, r])) for r in range(n_hyps[b])],
                 n_ids=n_ids[b].tolist(), recombinations=int(counters[b, 4]),
                 beam=[(beam_y[b, k, :beam_len[b, k]].tolist(), float(beam_score[b, k])) for k in range(beam_n[b])])
        d.update({name: int(nbc[b, i]) for i, name in enumerate(NB_COUNTERS)})
        out.append(d)
    return out


def final_float64(cfg, sd, f, t_len, beam=4, max_target_len=2.0, score_norm=True):
    """oracle/alsd.py's ALSD for ONE utterance in float64 (recombination as alsd_hotwords_ref.hw_float64's "upstream" mode: scores add
    into the first occurrence, duplicates stay in the beam), keeping every finished hypothesis
    -> [(labels, score, norm)] ranked by norm descending (ties: the earlier-finished first), equal label sequences removed (the
    better norm stays)"""
    blank = cfg.blank_id
    Wo, bo = sd["joint.joint_net.2.weight"].double(), sd["joint.joint_net.2.bias"].double()
    V1 = Wo.shape[0]
    non_blank = torch.tensor([k for k in range(V1) if k != blank])
    beam = min(beam, V1 - 1)
    pn = oalsd._PredNet(cfg, sd)
    u_max = int(max_target_len * t_len) if isinstance(max_target_len, float) else int(max_target_len)
    hyps = [dict(y=[blank], score=0.0, ts=[], st=pn.zero_state())]
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
            bh = dict(y=h["y"][:], score=h["score"] + float(logp[blank]), ts=h["ts"][:], st=h["st"])
            cands.append(bh)
            if t == t_len - 1:
                final.append(bh)
            for lp, k in zip(top_v.tolist(), non_blank[top_i].tolist()):
                cands.append(dict(y=h["y"] + [int(k)], score=h["score"] + float(lp), ts=h["ts"] + [i], st=new_state))
        hyps = sorted(cands, key=lambda c: c["score"], reverse=True)[:beam]       # stable: ties keep expansion order
        first = []
        for c in hyps:                                           # recombination: the first occurrence takes the sum, the duplicates stay
            for m in first:                                      # (a finished hypothesis is the same object: it reads the sum too)
                if m["y"] == c["y"]:
                    m["score"] = float(np.logaddexp(m["score"], c["score"]))
                    break
            else:
                first.append(c)
    out = final if final else hyps
    norm = (lambda h: h["score"] / len(h["y"])) if score_norm else (lambda h: h["score"])
    ranked, seen = [], set()
    for h in sorted(out, key=norm, reverse=True):            # stable: the earlier-finished first on a tie
        if tuple(h["y"]) not in seen:
            seen.add(tuple(h["y"]))
            ranked.append((h["y"][1:], h["score"], norm(h)))
    return ranked
