"""Helpers of the transducer alignment tests (tests/test_rnnt_align_host.py, tests/test_gpu_rnnt_align.py).  TEST INFRASTRUCTURE.

  align_checker(...)     tests/rnnt_align_checker.c through ctypes: rs_rnnt_align (csrc/k_rnnt_align.hip) restated serially in the
                         device's float32 order on the oracle library's routines.
  lattice_float64(...)   ONE utterance: (lb, ly) of every lattice cell in torch float64, read off the model.
  forward_float64 / viterbi_float64   the definition of the two recursions over a given lattice, both topologies.
  enumerate_paths(...)   every alignment path of a small lattice, listed (no DP): what pins the definition.
"""
import ctypes
import itertools
import math

import numpy as np
import torch

import checker_lib
from oracle import greedy as og, zipformer as oz
from token_scores_ref import is_k2, pack  # noqa: F401  (re-exported)

NEG = -math.inf


def lib():
    L = checker_lib.load("rnnt_align_checker.c")
    L.rs_rnnt_align_checker.restype = ctypes.c_int
    return L


def align_checker(cfg, sd, f, enc_lens, ids, n_ids, one_per_frame=False, want_rc=0, want_lattice=False):
    """f float32 [B, Tp, J], enc_lens int [B], ids int32 [B, u_cap], n_ids int32 [B] -> dict(loglik, best float32 [B]; frames int32,
    logp float32 [B, u_cap]; lattice float32 [B, Tp, u_cap + 1, 2] when asked).  Slots the checker leaves alone hold -2 / NaN
    (frames / logp)."""
    L = lib()
    f = np.ascontiguousarray(f, dtype=np.float32)
    B, Tp, J = f.shape
    enc_lens = np.ascontiguousarray(enc_lens, dtype=np.int32)
    ids, n_ids = (np.ascontiguousarray(a, dtype=np.int32) for a in (ids, n_ids))
    u_cap = ids.shape[1]
    loglik = np.full((B,), np.nan, np.float32)
    best = np.full((B,), np.nan, np.float32)
    logp = np.full((B, u_cap), np.nan, np.float32)
    frames = np.full((B, u_cap), -2, np.int32)
    lattice = np.full((B, Tp, u_cap + 1, 2), np.nan, np.float32) if want_lattice else None
    fp, ip = og._fp, og._ip
    PF = ctypes.POINTER(ctypes.c_float)
    lat = fp(lattice) if want_lattice else None
    if is_k2(cfg):
        og.lib().rs_oracle_set_joint_act(1)
        c = lambda k: np.ascontiguousarray(sd[k].numpy(), dtype=np.float32)  # noqa: E731
        embed, conv_w = c("decoder.embedding.weight"), c("decoder.conv.weight")
        wp, bp = c("joiner.decoder_proj.weight"), c("joiner.decoder_proj.bias")
        wo, bo = c("joiner.output_linear.weight"), c("joiner.output_linear.bias")
        rc = L.rs_rnnt_align_checker(fp(f), ip(enc_lens), B, Tp, J, cfg.decoder_dim, 1, cfg.vocab_size, cfg.blank_id, fp(embed), None, None,
                                     fp(conv_w), fp(wp), fp(bp), fp(wo), fp(bo), ip(ids), ip(n_ids), u_cap, int(bool(one_per_frame)),
                                     fp(loglik), fp(best), ip(frames), fp(logp), lat)
    else:
        og.lib().rs_oracle_set_joint_act(1 if getattr(cfg, "espnet", False) else 0)
        arr = og.decoder_arrays(cfg, sd)
        wl = (PF * cfg.pred_layers)(*[fp(w) for w in arr["lstm_w"]])
        bl = (PF * cfg.pred_layers)(*[fp(b) for b in arr["lstm_b"]])
        rc = L.rs_rnnt_align_checker(fp(f), ip(enc_lens), B, Tp, J, cfg.pred_hidden, cfg.pred_layers, cfg.n_logits, cfg.blank_id,
                                     fp(arr["embed"]), wl, bl, None, fp(arr["Wp"]), fp(arr["bp"]), fp(arr["Wo"]), fp(arr["bo"]),
                                     ip(ids), ip(n_ids), u_cap, int(bool(one_per_frame)), fp(loglik), fp(best), ip(frames), fp(logp), lat)
    assert rc == want_rc, f"align checker returned {rc}, expected {want_rc}"
    out = dict(loglik=loglik, best=best, frames=frames, logp=logp)
    if want_lattice:
        out["lattice"] = lattice
    return out


def lattice_float64(cfg, sd, f, ids):
    """ONE utterance: f [T][J], its labels -> (lb float64 [T][U + 1], ly float64 [T][U] ): the prediction network consumes
    [start, y_1, .., y_u] for g(u), u = 0..U; the joint scores every (t, u); log_softmax."""
    f64 = torch.as_tensor(np.asarray(f), dtype=torch.float64)
    ids = [int(i) for i in ids]
    gs = []
    with torch.no_grad():
        if is_k2(cfg):
            sd64 = {k: sd[k].double() for k in ("decoder.embedding.weight", "decoder.conv.weight", "joiner.decoder_proj.weight",
                                                "joiner.decoder_proj.bias", "joiner.output_linear.weight", "joiner.output_linear.bias")}
            wo, bo = sd64["joiner.output_linear.weight"], sd64["joiner.output_linear.bias"]
            act = torch.tanh
            ys = [-1] * (cfg.context_size - 1) + [cfg.blank_id]
            for u in range(len(ids) + 1):
                gs.append(oz.decoder_out(cfg, sd64, ys[-cfg.context_size:]))
                if u < len(ids):
                    ys.append(ids[u])
            blank = cfg.blank_id
        else:
            arr = {k: ([torch.from_numpy(x).double() for x in v] if isinstance(v, list) else torch.from_numpy(v).double())
                   for k, v in og.decoder_arrays(cfg, sd).items()}
            wo, bo = arr["Wo"], arr["bo"]
            H, L = cfg.pred_hidden, cfg.pred_layers
            h = [torch.zeros(H, dtype=torch.float64) for _ in range(L)]
            c = [torch.zeros(H, dtype=torch.float64) for _ in range(L)]
            act = torch.tanh if getattr(cfg, "espnet", False) else torch.relu
            token = cfg.blank_id
            for u in range(len(ids) + 1):
                x = arr["embed"][token]
                for l in range(L):                                # gate order i, f, g, o; W = [W_ih | W_hh], bias = b_ih + b_hh
                    z = arr["lstm_w"][l] @ torch.cat([x, h[l]]) + arr["lstm_b"][l]
                    i, fg, gg, o = torch.sigmoid(z[:H]), torch.sigmoid(z[H:2 * H]), torch.tanh(z[2 * H:3 * H]), torch.sigmoid(z[3 * H:])
                    c[l] = fg * c[l] + i * gg
                    h[l] = o * torch.tanh(c[l])
                    x = h[l]
                gs.append(arr["Wp"] @ h[L - 1] + arr["bp"])
                if u < len(ids):
                    token = ids[u]
            blank = cfg.blank_id
        g = torch.stack(gs)                                                       # [U + 1][J]
        lp = torch.log_softmax(act(f64[:, None, :] + g[None, :, :]) @ wo.t() + bo, -1)      # [T][U + 1][V]
        lb = lp[:, :, blank].numpy()
        ly = np.stack([lp[:, u, ids[u]].numpy() for u in range(len(ids))], 1) if ids else np.zeros((f64.shape[0], 0))
    return lb, ly


def _lae(a, b):
    m = max(a, b)
    return m if m == NEG else m + math.log(math.exp(a - m) + math.exp(b - m))


def _sweep(lb, ly, one, combine):
    """the recursion of the issue, cell by cell -> table a[t][u] (t = 0..T with `one`, else 0..T-1)"""
    T, U = lb.shape[0], ly.shape[1]
    rows = T + 1 if one else T
    a = [[NEG] * (U + 1) for _ in range(rows)]
    for t in range(rows):
        for u in range(U + 1):
            if t == 0 and u == 0:
                a[t][u] = 0.0
                continue
            blank = a[t - 1][u] + lb[t - 1][u] if t >= 1 else NEG
            if one:
                label = a[t - 1][u - 1] + ly[t - 1][u - 1] if (t >= 1 and u >= 1) else NEG
            else:
                label = a[t][u - 1] + ly[t][u - 1] if u >= 1 else NEG
            a[t][u] = combine(blank, label)
    return a


def forward_float64(lb, ly, one=False):
    """log P(text | audio): lb [T][U + 1], ly [T][U] float64"""
    T, U = lb.shape[0], ly.shape[1]
    if T == 0:
        return 0.0 if U == 0 else NEG
    if one and U > T:
        return NEG
    a = _sweep(lb, ly, one, _lae)
    return a[T][U] if one else a[T - 1][U] + lb[T - 1][U]


def viterbi_float64(lb, ly, one=False):
    """(best score, frames) with ties to the blank predecessor"""
    T, U = lb.shape[0], ly.shape[1]
    if T == 0:
        return (0.0, []) if U == 0 else (NEG, [-1] * U)
    if one and U > T:
        return NEG, [-1] * U
    v = _sweep(lb, ly, one, max)
    t, u, frames = (T if one else T - 1), U, [0] * U
    while u > 0:
        blank = v[t - 1][u] + lb[t - 1][u] if t >= 1 else NEG
        if one:
            label = v[t - 1][u - 1] + ly[t - 1][u - 1] if t >= 1 else NEG
        else:
            label = v[t][u - 1] + ly[t][u - 1]
        if label > blank:
            frames[u - 1] = t - 1 if one else t
            u -= 1
            t -= 1 if one else 0
        else:
            t -= 1
    return (v[T][U] if one else v[T - 1][U] + lb[T - 1][U]), frames


def enumerate_paths(lb, ly, one=False):
    """every alignment listed, without a DP -> [(score, frames)].  Standard: label u + 1 is emitted at any frame, frames
    non-decreasing; every frame ends in a blank taken at the label count reached so far.  One per frame: every frame emits a blank or
    exactly one label, so the label frames are strictly increasing."""
    T, U = lb.shape[0], ly.shape[1]
    out = []
    if one:
        for frames in itertools.combinations(range(T), U):
            s, u = 0.0, 0
            for t in range(T):
                if u < U and frames[u] == t:
                    s += ly[t][u]
                    u += 1
                else:
                    s += lb[t][u]
            out.append((s, list(frames)))
        return out
    for frames in itertools.combinations_with_replacement(range(T), U):
        s, u = 0.0, 0
        for t in range(T):
            while u < U and frames[u] == t:
                s += ly[t][u]
                u += 1
            s += lb[t][u]
        out.append((s, list(frames)))
    return out


def path_sum_f32(lattice, frames, one=False):
    """float32 sum of the lattice entries along the Viterbi path of ONE utterance in the DP's order of additions: lattice
    [T][U + 1][2] float32 (lb, ly), frames [U]"""
    T, U = lattice.shape[0], len(frames)
    s, u = np.float32(0.0), 0
    for t in range(T):
        if one:
            if u < U and frames[u] == t:
                s = np.float32(s + lattice[t, u, 1])
                u += 1
            else:
                s = np.float32(s + lattice[t, u, 0])
        else:
            while u < U and frames[u] == t:
                s = np.float32(s + lattice[t, u, 1])
                u += 1
            s = np.float32(s + lattice[t, u, 0])
    return s
