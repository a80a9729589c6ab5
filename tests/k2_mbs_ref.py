"""Helpers of the modified-beam-search tests (tests/test_k2_mbs_host.py, tests/test_gpu_k2_mbs.py).  TEST INFRASTRUCTURE.

  mbs_checker(...)   tests/k2_mbs_checker.c through ctypes: the search of csrc/k_rnnt_mbs.hip restated in the device's float32 order,
                     without or with hotwords, and its counters.  Built by tests/checker_lib.py and linked against the oracle
                     library, whose decoder, projection and joint-logit routines it calls.
  mbs_float64(...)   a readable torch-float64 restatement of the algorithm (include/rs_asr.h, rs_rnnt_mbs) with Python-float
                     log_prob like upstream; also reports how close the search came to a tie.
"""
import ctypes
import math
import os

import numpy as np
import torch

import checker_lib
from oracle import greedy as og, zipformer as oz

MAX_K = 8
# the flat hotword table (reazonspeech_amd.runtime.k2_hotwords.concat) of no graph at all
EMPTY_TABLE = dict(child_begin=np.zeros(1, np.int32), child_tok=np.zeros(0, np.int32), child_node=np.zeros(0, np.int32),
                   fail=np.zeros(0, np.int32), output=np.zeros(0, np.int32), is_end=np.zeros(0, np.int32), level=np.zeros(0, np.int32),
                   token_score=np.zeros(0, np.float32), node_score=np.zeros(0, np.float32), output_score=np.zeros(0, np.float32),
                   graph_root=np.zeros(0, np.int32), max_level=0)


def lib():
    L = checker_lib.load("k2_mbs_checker.c")
    L.rs_k2_mbs_checker.restype = ctypes.c_int
    return L


def k2_arrays(sd):
    c = lambda k: np.ascontiguousarray(sd[k].numpy(), dtype=np.float32)  # noqa: E731
    return dict(embed=c("decoder.embedding.weight"), conv_w=c("decoder.conv.weight"), wp=c("joiner.decoder_proj.weight"),
                bp=c("joiner.decoder_proj.bias"), wo=c("joiner.output_linear.weight"), bo=c("joiner.output_linear.bias"))


def mbs_checker(cfg, sd, f, enc_lens, table=None, graph_of=None, K=4, blank_penalty=0.0, length_norm=True, out_cap=None, workers=None):
    """f float32 [B, Tp, J] (numpy) = joiner.encoder_proj(encoder output), enc_lens int [B], the flat table of the call's graphs
    (None = no graph) and graph_of int [B] (-1 = none) -> per utterance a dict(ids, frames, score (float32 log_prob of the winner),
    score_bits, merges, final = [(tokens, float32 log_prob)] of the last set in the order of entry, child_hits, fail_transitions,
    exits (non-strict), finalize (the sum of the Finalize deltas)).  Utterances are independent: rows run on `workers` threads."""
    L = lib()
    og.lib().rs_oracle_set_joint_act(1)                      # the Zipformer joiner is tanh (as oracle/k2_greedy.c sets it)
    a = k2_arrays(sd)
    f = np.ascontiguousarray(f, dtype=np.float32)
    B, Tp, J = f.shape
    enc_lens = np.ascontiguousarray(enc_lens, dtype=np.int32)
    table = table if table is not None else EMPTY_TABLE
    tab = {k: np.ascontiguousarray(v, dtype=np.float32 if k.endswith("_score") else np.int32) for k, v in table.items() if k != "max_level"}
    graph_of = np.ascontiguousarray(graph_of if graph_of is not None else np.full(B, -1), dtype=np.int32)
    assert len(graph_of) == B
    if out_cap is None:
        out_cap = max(Tp, 1)
    ids, frames = np.zeros((B, out_cap), np.int32), np.zeros((B, out_cap), np.int32)
    n_ids, merges, fin_n = np.zeros((B,), np.int32), np.zeros((B,), np.int32), np.zeros((B,), np.int32)
    scores = np.zeros((B,), np.float32)
    fin_len, fin_lp = np.zeros((B, MAX_K), np.int32), np.zeros((B, MAX_K), np.float32)
    fin_y = np.zeros((B, MAX_K, out_cap), np.int32)
    counters, fin_total = np.zeros((B, 3), np.int32), np.zeros((B,), np.float32)
    fp, ip = og._fp, og._ip

    def rows(b0, b1):
        return L.rs_k2_mbs_checker(
            fp(f[b0:b1]), ip(enc_lens[b0:b1]), b1 - b0, Tp, J, cfg.decoder_dim, cfg.vocab_size, cfg.blank_id, cfg.unk_id, fp(a["embed"]),
            fp(a["conv_w"]), fp(a["wp"]), fp(a["bp"]), fp(a["wo"]), fp(a["bo"]), int(K), ctypes.c_float(blank_penalty),
            int(bool(length_norm)), int(out_cap), ip(ids[b0:b1]), ip(frames[b0:b1]), ip(n_ids[b0:b1]), fp(scores[b0:b1]),
            ip(merges[b0:b1]), ip(fin_n[b0:b1]), ip(fin_len[b0:b1]), fp(fin_lp[b0:b1]), ip(fin_y[b0:b1]),
            ip(tab["child_begin"]), ip(tab["child_tok"]), ip(tab["child_node"]), ip(tab["fail"]), ip(tab["output"]), ip(tab["is_end"]),
            fp(tab["token_score"]), fp(tab["node_score"]), fp(tab["output_score"]), ip(tab["graph_root"]), len(tab["graph_root"]),
            ip(graph_of[b0:b1]), ip(counters[b0:b1]), fp(fin_total[b0:b1]))

    if workers is None:
        workers = min(16, os.cpu_count() or 1)
    if B > 1 and workers > 1:
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max_workers=min(workers, B)) as pool:
            rc = min(pool.map(lambda b: rows(b, b + 1), range(B)))
    else:
        rc = rows(0, B) if B else 0
    if rc != 0:
        raise RuntimeError(f"k2 mbs checker failed ({rc}; -5 = more than out_cap={out_cap} tokens)")
    out = []
    for b in range(B):
        final = [(fin_y[b, k, :fin_len[b, k]].tolist(), float(fin_lp[b, k])) for k in range(fin_n[b])]
        out.append(dict(ids=ids[b, :n_ids[b]].tolist(), frames=frames[b, :n_ids[b]].tolist(), score=float(scores[b]),
                        score_bits=int(scores[b:b + 1].view(np.int32)[0]), merges=int(merges[b]), final=final,
                        child_hits=int(counters[b, 0]), fail_transitions=int(counters[b, 1]), exits=int(counters[b, 2]),
                        finalize=float(fin_total[b])))
    return out


def model_logits_fn(cfg, sd, f):
    """float64 logits of (frame t, token history ys): output_linear(tanh(f[t] + decoder_proj(decoder(last context_size tokens))))"""
    sd64 = {k: sd[k].double() for k in ("decoder.embedding.weight", "decoder.conv.weight", "joiner.decoder_proj.weight",
                                        "joiner.decoder_proj.bias", "joiner.output_linear.weight", "joiner.output_linear.bias")}
    f64 = torch.as_tensor(np.asarray(f), dtype=torch.float64)
    wo, bo = sd64["joiner.output_linear.weight"], sd64["joiner.output_linear.bias"]
    cache = {}

    def fn(t, ys):
        key = tuple(ys[-cfg.context_size:])
        if key not in cache:
            cache[key] = oz.decoder_out(cfg, sd64, list(key))
        return torch.tanh(f64[t] + cache[key]) @ wo.t() + bo
    return fn


def mbs_float64(cfg, sd, f, K=4, blank_penalty=0.0, length_norm=True, logits_fn=None, n_frames=None):
    """One utterance, f [T][J].  The algorithm as include/rs_asr.h states it, in float64 with Python-float log_prob:
    returns dict(ids, frames, score, merges, final = [(tokens, log_prob)] in the order of entry,
                 frame_gaps = per frame the smallest gap between adjacent values among the K + 1 best candidates,
                 min_gap / min_gap_frame, final_gap = gap between the two best final (normalised) scores).
    logits_fn(t, ys) replaces decoder and joiner (hand-built cases); n_frames is then the number of frames."""
    cs, blank, unk = cfg.context_size, cfg.blank_id, cfg.unk_id
    if logits_fn is None:
        logits_fn = model_logits_fn(cfg, sd, f)
        n_frames = len(f)
    hyps = [dict(ys=[-1] * (cs - 1) + [blank], ts=[], lp=0.0)]
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
            order = torch.sort(flat, descending=True, stable=True).indices[:K + 1].tolist()     # equal values: lower flat index first
            vals = [float(flat[c]) for c in order]
            frame_gaps.append(min((a - b for a, b in zip(vals, vals[1:])), default=math.inf))
            new = []
            for c, lp in zip(order[:K], vals[:K]):
                h, v = hyps[c // V], c % V
                ys, ts = list(h["ys"]), list(h["ts"])
                if v != blank and v != unk:
                    ys.append(v)
                    ts.append(t)
                same = [e for e in new if e["ys"] == ys]
                if same:                                      # Hypotheses::Add: the first one keeps its tokens / timestamps
                    same[0]["lp"] = float(np.logaddexp(same[0]["lp"], lp))
                    merges += 1
                else:
                    new.append(dict(ys=ys, ts=ts, lp=lp))
            hyps = new
    norm = [h["lp"] / len(h["ys"]) if length_norm else h["lp"] for h in hyps]
    win = max(range(len(hyps)), key=lambda k: (norm[k], -k))                                   # equal scores: first entered
    top = sorted(norm, reverse=True)
    gi = int(np.argmin(frame_gaps)) if frame_gaps else -1
    return dict(ids=hyps[win]["ys"][cs:], frames=hyps[win]["ts"], score=hyps[win]["lp"], merges=merges,
                final=[(h["ys"][cs:], h["lp"]) for h in hyps], frame_gaps=frame_gaps,
                min_gap=frame_gaps[gi] if frame_gaps else math.inf, min_gap_frame=gi,
                final_gap=top[0] - top[1] if len(top) > 1 else math.inf)
