"""Helpers of the tests of the n-best lists of ESPnet's default beam search (tests/test_nbest_espnet_host.py, tests/test_gpu_nbest_espnet.py).
TEST INFRASTRUCTURE.

  nbest_checker(...)    tests/espnet_beam_nbest_checker.c through ctypes: the search of csrc/k_rnnt_beam.hip with upstream's
                        sort_nbest(kept_hyps)[:nbest] restated in the device's float32 order, and the counters that show which edge a
                        fixture reaches.  `inject` replaces prediction network and joint by a table of logits (the hand-built cases).
  beam_float64(...)     [UPSTREAM] espnet2 BeamSearchTransducer.default_beam_search + sort_nbest restated in float64 WITH its kept
                        list (oracle/espnet.py's restatement returns the best hypothesis only) -> (ranked list, kept list)
  model_logp_fn(...)    the float64 log-softmax of an ESPnet-shaped decoder's joint row, cached by label sequence
"""
import ctypes
import os

import numpy as np
import torch

import checker_lib
from oracle import greedy as og


def lib():
    L = checker_lib.load("espnet_beam_nbest_checker.c")
    L.rs_espnet_beam_nbest_checker.restype = ctypes.c_int
    return L


def bits(x):
    return int(np.asarray([x], np.float32).view(np.int32)[0])


def f32(b):
    return float(np.asarray([b], np.int32).view(np.float32)[0])


def nbest_checker(cfg, sd, f, enc_lens, nbest, beam=20, score_norm=True, max_pops=None, out_cap=None, workers=None, inject=None, check=True):
    """-> per utterance dict(entries=[(ids, frames, score bits, norm bits)] best first (n_hyps of them), n_ids=[nbest counts], pops,
    kept, duplicates, ties, norm_reorders).  f float32 [B][Tp][J], as oracle.greedy.espnet_beam takes it.  `inject` float32
    [Tp][V][V]: the logits of frame t for a hypothesis whose last label is u = inject[t][u]; then `sd` and `f` are not read (`f` only
    gives B and Tp, `cfg` n_logits, blank_id, pred_hidden and pred_layers).  `check` False: an overflow returns what was written."""
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
    if max_pops is None:
        max_pops = 8 * int(beam)
    if out_cap is None:
        out_cap = max(1, Tp * 4)
    N = int(nbest)
    ids, frames = np.zeros((B, N, out_cap), np.int32), np.zeros((B, N, out_cap), np.int32)
    n_ids, n_hyps = np.full((B, N), -1, np.int32), np.full((B,), -1, np.int32)
    scores, norms = np.zeros((B, N), np.float32), np.zeros((B, N), np.float32)
    pops, nbc = np.zeros((B,), np.int32), np.zeros((B, 4), np.int32)

    def rows(b0, b1):
        return L.rs_espnet_beam_nbest_checker(
            fp(f[b0:b1]), ip(enc_lens[b0:b1]), b1 - b0, Tp, J, cfg.pred_hidden, cfg.pred_layers, cfg.n_logits, cfg.blank_id, *weights, inj,
            int(beam), int(bool(score_norm)), int(max_pops), N, int(out_cap), ip(ids[b0:b1]), ip(frames[b0:b1]), ip(n_ids[b0:b1]),
            fp(scores[b0:b1]), fp(norms[b0:b1]), ip(n_hyps[b0:b1]), ip(pops[b0:b1]), ip(nbc[b0:b1]))

    if workers is None:
        workers = min(16, os.cpu_count() or 1)
    if B > 1 and workers > 1:
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max_workers=min(workers, B)) as pool:
            rcs = list(pool.map(lambda b: rows(b, b + 1), range(B)))
        rc = min(rcs)
    else:
        rc = rows(0, B) if B else 0
    if rc == -1 or (rc != 0 and check):
        raise RuntimeError(f"espnet beam n-best checker failed ({rc}; -5 = overflow of max_pops={max_pops} / out_cap={out_cap}, -1 = nbest outside 1..beam)")
    sb, nb = scores.view(np.int32), norms.view(np.int32)
    out = []
    for b in range(B):
        entries = [(ids[b, r, :n_ids[b, r]].tolist(), frames[b, r, :n_ids[b, r]].tolist(), int(sb[b, r]), int(nb[b, r])) for r in range(n_hyps[b])]
        out.append(dict(entries=entries, n_ids=n_ids[b].tolist(), pops=int(pops[b]), kept=int(nbc[b, 0]), duplicates=int(nbc[b, 1]),
                        ties=int(nbc[b, 2]), norm_reorders=int(nbc[b, 3])))
    return out


# ---- the search in float64, with its kept list ---------------------------------------------------------------------------------------
def beam_float64(logp_fn, n_frames, V, blank, beam=20, score_norm=True):
    """[UPSTREAM] default_beam_search + sort_nbest, statement for statement as oracle/espnet.py restates it (which see), in float64,
    over `logp_fn(t, yseq) -> float64 log-softmax [V]` (yseq includes the leading blank).
    -> (ranked [(ids, score, norm)] over the whole kept list, min gap between an end-of-frame decision's sides)"""
    beam = min(beam, V)
    beam_k = min(beam, V - 1)
    labels = [v for v in range(V) if v != blank]
    kept = [dict(score=0.0, yseq=[blank])]
    min_gap = np.inf
    for t in range(n_frames):
        hyps, kept = kept, []
        while True:
            mi = max(range(len(hyps)), key=lambda i: (hyps[i]["score"], -i))
            mh = hyps.pop(mi)
            logp = np.asarray(logp_fn(t, mh["yseq"]), np.float64)
            order = sorted(labels, key=lambda v: (-logp[v], v))[:beam_k]
            kept.append(dict(score=mh["score"] + float(logp[blank]), yseq=mh["yseq"]))
            for v in order:
                hyps.append(dict(score=mh["score"] + float(logp[v]), yseq=mh["yseq"] + [v]))
            hmax = max(h["score"] for h in hyps)
            best = sorted([h for h in kept if h["score"] > hmax], key=lambda h: h["score"])
            every = sorted(h["score"] for h in kept + hyps)
            min_gap = min(min_gap, min((b - a for a, b in zip(every, every[1:])), default=np.inf))
            if len(best) >= beam:
                kept = best
                break
    norm = lambda h: h["score"] / len(h["yseq"]) if score_norm else h["score"]       # noqa: E731
    ranked = sorted(kept, key=norm, reverse=True)                                    # Python's sort: stable, as upstream's
    return [(h["yseq"][1:], h["score"], norm(h)) for h in ranked], min_gap


def model_logp_fn(cfg, sd, f_row):
    """float64 log-softmax of the ESPnet-shaped joint for (frame t, label sequence), the LSTM state cached by sequence"""
    assert getattr(cfg, "espnet", False)
    H = cfg.pred_hidden
    lstms = []
    for l in range(cfg.pred_layers):
        m = torch.nn.LSTM(H, H, 1, batch_first=True).double()
        with torch.no_grad():
            for nm in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
                getattr(m, nm + "_l0").copy_(sd[f"decoder.decoder.{l}.{nm}_l0"].double())
        lstms.append(m)
    emb, wd = sd["decoder.embed.weight"].double(), sd["joint_network.lin_dec.weight"].double()
    wo, bo = sd["joint_network.lin_out.weight"].double(), sd["joint_network.lin_out.bias"].double()
    ft = torch.as_tensor(np.asarray(f_row), dtype=torch.float64)
    zero = [(torch.zeros(1, 1, H, dtype=torch.float64), torch.zeros(1, 1, H, dtype=torch.float64)) for _ in lstms]
    cache = {}

    def state(yseq):                                   # -> (decoder output after yseq's last label, LSTM state after it)
        key = tuple(yseq)
        if key not in cache:
            prev = zero if len(key) == 1 else state(key[:-1])[1]
            x = emb[key[-1]].view(1, 1, H)
            new = []
            for l, m in enumerate(lstms):
                x, st = m(x, prev[l])
                new.append(st)
            cache[key] = (x[0, 0] @ wd.t(), new)
        return cache[key]

    def fn(t, yseq):
        with torch.no_grad():
            return torch.log_softmax(torch.tanh(ft[t] + state(yseq)[0]) @ wo.t() + bo, dim=-1).numpy()
    return fn
