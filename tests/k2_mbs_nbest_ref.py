"""Helpers of the tests of the n-best lists of the modified beam search (tests/test_nbest_host.py, tests/test_gpu_nbest.py).
TEST INFRASTRUCTURE.

  nbest_checker(...)    tests/k2_mbs_nbest_checker.c through ctypes: the search of csrc/k_rnnt_mbs.hip with the ranked list of
                        rs_rnnt_mbs_nbest restated in the device's float32 order — plain, with hotwords, with an n-gram LM, with
                        both — and the counters that show which edge a fixture reaches.  `inject` replaces decoder and joiner by a
                        table of logits (the hand-built cases).
  ranked_float64(...)   the ranked list of the float64 restatement k2_mbs_lm_ref.lm_float64: its final set under the same rule
"""
import ctypes
import os

import numpy as np

import checker_lib
import k2_mbs_lm_ref as LR
import k2_mbs_ref as R
from oracle import greedy as og

MAX_K = LR.MAX_K


def lib():
    L = checker_lib.load("k2_mbs_nbest_checker.c")
    L.rs_k2_mbs_nbest_checker.restype = ctypes.c_int
    return L


def bits(x):
    return int(np.asarray([x], np.float32).view(np.int32)[0])


def nbest_checker(cfg, sd, f, enc_lens, nbest, table=None, graph_of=None, lm=None, alpha=0.0, K=4, blank_penalty=0.0, length_norm=True,
                  out_cap=None, workers=None, inject=None):
    """-> per utterance dict(entries=[(ids, frames, score bits, norm bits)] best first (n_hyps of them), n_ids=[nbest counts],
    last_set, ties, last_merges, finalize_reorders, merges, final=[(ids, log_prob)] in the order of entry).  Arguments as
    k2_mbs_lm_ref.mbs_lm_checker."""
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
    hw, hw_keep = LR._hw_struct(table) if table is not None else (None, None)
    graph_of = None if graph_of is None else np.ascontiguousarray(graph_of, dtype=np.int32)
    assert graph_of is None or len(graph_of) == B
    lms, lm_keep = LR._lm_struct(lm) if lm is not None else (None, None)
    if out_cap is None:
        out_cap = max(Tp, 1)
    N = int(nbest)
    ids, frames = np.zeros((B, N, out_cap), np.int32), np.zeros((B, N, out_cap), np.int32)
    n_ids, n_hyps, nbc = np.full((B, N), -1, np.int32), np.full((B,), -1, np.int32), np.zeros((B, 4), np.int32)
    scores, norms = np.zeros((B, N), np.float32), np.zeros((B, N), np.float32)
    merges, fin_n = np.zeros((B,), np.int32), np.zeros((B,), np.int32)
    fin_len, fin_lp, fin_lm = np.zeros((B, MAX_K), np.int32), np.zeros((B, MAX_K), np.float32), np.zeros((B, MAX_K), np.int32)
    fin_y = np.zeros((B, MAX_K, out_cap), np.int32)
    counters, fin_total = np.zeros((B, 3), np.int32), np.zeros((B,), np.float32)
    lcnt = np.zeros((B, LR.LM_COUNTERS), np.int32)

    def rows(b0, b1):
        return L.rs_k2_mbs_nbest_checker(
            fp(f[b0:b1]), ip(enc_lens[b0:b1]), b1 - b0, Tp, J, D, cfg.vocab_size, cfg.blank_id, cfg.unk_id, *weights, inj, int(K),
            ctypes.c_float(blank_penalty), int(bool(length_norm)), N, int(out_cap), ip(ids[b0:b1]), ip(frames[b0:b1]), ip(n_ids[b0:b1]),
            fp(scores[b0:b1]), fp(norms[b0:b1]), ip(n_hyps[b0:b1]), ip(nbc[b0:b1]), ip(merges[b0:b1]), ip(fin_n[b0:b1]),
            ip(fin_len[b0:b1]), fp(fin_lp[b0:b1]), ip(fin_lm[b0:b1]), ip(fin_y[b0:b1]), ctypes.byref(hw) if hw is not None else None,
            ip(graph_of[b0:b1]) if graph_of is not None else None, ip(counters[b0:b1]), fp(fin_total[b0:b1]),
            ctypes.byref(lms) if lms is not None else None, ctypes.c_float(alpha), ip(lcnt[b0:b1]))

    if workers is None:
        workers = min(16, os.cpu_count() or 1)
    if B > 1 and workers > 1:
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max_workers=min(workers, B)) as pool:
            rc = min(pool.map(lambda b: rows(b, b + 1), range(B)))
    else:
        rc = rows(0, B) if B else 0
    if rc != 0:
        raise RuntimeError(f"k2 mbs n-best checker failed ({rc}; -5 = more than out_cap={out_cap} tokens, -1 = nbest outside 1..K)")
    sb, nb = scores.view(np.int32), norms.view(np.int32)
    out = []
    for b in range(B):
        entries = [(ids[b, r, :n_ids[b, r]].tolist(), frames[b, r, :n_ids[b, r]].tolist(), int(sb[b, r]), int(nb[b, r])) for r in range(n_hyps[b])]
        out.append(dict(entries=entries, n_ids=n_ids[b].tolist(), last_set=int(nbc[b, 0]), ties=int(nbc[b, 1]), last_merges=int(nbc[b, 2]),
                        finalize_reorders=int(nbc[b, 3]), merges=int(merges[b]), finalize=float(fin_total[b]),
                        final=[(fin_y[b, k, :fin_len[b, k]].tolist(), float(fin_lp[b, k])) for k in range(fin_n[b])]))
    return out


def f32(bits_):
    return float(np.asarray([bits_], np.int32).view(np.float32)[0])


def ranked_float64(ref, length_norm=True, context=2):
    """the list of a k2_mbs_lm_ref.lm_float64 result: its final set [(ids, log_prob)] under the rule of rs_rnnt_mbs_nbest
    -> [(ids, log_prob, norm)] best first, ties in the order of entry"""
    rows = [(y, lp, lp / (len(y) + context) if length_norm else lp) for y, lp in ref["final"]]
    order = sorted(range(len(rows)), key=lambda k: (-rows[k][2], k))
    return [rows[k] for k in order]
