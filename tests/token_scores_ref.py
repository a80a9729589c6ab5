"""Helpers of the token-score tests (tests/test_token_scores_host.py, tests/test_gpu_token_scores.py).  TEST INFRASTRUCTURE.

  scores_checker(...)   tests/token_scores_checker.c through ctypes: rs_rnnt_token_scores (csrc/k_rnnt_scores.hip) restated in the
                        device's float32 order.  Compiled here with the flags of oracle/build.py and linked against the oracle
                        library, whose LSTM step, stateless decoder, dot product, joint logits and log-sum-exp it calls.
  scores_float64(...)   a readable torch-float64 restatement: teacher-forced prediction network, joint, log_softmax.
  pack / unpack         ragged per-utterance lists <-> the [B][u_cap] arrays of the C ABI
"""
import ctypes

import numpy as np
import torch

import checker_lib
from oracle import greedy as og, zipformer as oz


def lib():
    L = checker_lib.load("token_scores_checker.c")
    L.rs_token_scores_checker.restype = ctypes.c_int
    return L


def is_k2(cfg):
    return getattr(cfg, "family", "") == "k2"


def pack(rows, u_cap, fill=0):
    """[[int]] -> int32 [B][u_cap], counts int32 [B]"""
    out = np.full((len(rows), u_cap), fill, np.int32)
    for b, r in enumerate(rows):
        out[b, :len(r)] = r
    return out, np.asarray([len(r) for r in rows], np.int32)


def scores_checker(cfg, sd, f, enc_lens, ids, frames, n_ids, frames_are_steps=False, want_rc=0):
    """f float32 [B, Tp, J], enc_lens int [B], ids / frames int32 [B, u_cap], n_ids int32 [B] -> (logp float32 [B, u_cap],
    top1 int32 [B, u_cap]); slots past n_ids hold NaN / -2 (the checker leaves them alone)"""
    L = lib()
    f = np.ascontiguousarray(f, dtype=np.float32)
    B, Tp, J = f.shape
    enc_lens = np.ascontiguousarray(enc_lens, dtype=np.int32)
    ids, frames, n_ids = (np.ascontiguousarray(a, dtype=np.int32) for a in (ids, frames, n_ids))
    u_cap = ids.shape[1]
    logp = np.full((B, u_cap), np.nan, np.float32)
    top1 = np.full((B, u_cap), -2, np.int32)
    fp, ip = og._fp, og._ip
    PF = ctypes.POINTER(ctypes.c_float)
    if is_k2(cfg):
        og.lib().rs_oracle_set_joint_act(1)
        c = lambda k: np.ascontiguousarray(sd[k].numpy(), dtype=np.float32)  # noqa: E731
        embed, conv_w = c("decoder.embedding.weight"), c("decoder.conv.weight")
        wp, bp = c("joiner.decoder_proj.weight"), c("joiner.decoder_proj.bias")
        wo, bo = c("joiner.output_linear.weight"), c("joiner.output_linear.bias")
        rc = L.rs_token_scores_checker(fp(f), ip(enc_lens), B, Tp, J, cfg.decoder_dim, 1, cfg.vocab_size, cfg.blank_id, fp(embed), None, None,
                                       fp(conv_w), fp(wp), fp(bp), fp(wo), fp(bo), ip(ids), ip(frames), ip(n_ids), u_cap,
                                       int(bool(frames_are_steps)), fp(logp), ip(top1))
    else:
        og.lib().rs_oracle_set_joint_act(1 if getattr(cfg, "espnet", False) else 0)
        arr = og.decoder_arrays(cfg, sd)
        wl = (PF * cfg.pred_layers)(*[fp(w) for w in arr["lstm_w"]])
        bl = (PF * cfg.pred_layers)(*[fp(b) for b in arr["lstm_b"]])
        rc = L.rs_token_scores_checker(fp(f), ip(enc_lens), B, Tp, J, cfg.pred_hidden, cfg.pred_layers, cfg.n_logits, cfg.blank_id,
                                       fp(arr["embed"]), wl, bl, None, fp(arr["Wp"]), fp(arr["bp"]), fp(arr["Wo"]), fp(arr["bo"]),
                                       ip(ids), ip(frames), ip(n_ids), u_cap, int(bool(frames_are_steps)), fp(logp), ip(top1))
    assert rc == want_rc, f"token score checker returned {rc}, expected {want_rc}"
    return logp, top1


def scores_float64(cfg, sd, f, ids, frames, frames_are_steps=False):
    """ONE utterance: f [T][J], its ids and frames (lists) -> (log-probabilities float64 [n], argmax [n]).  The definition, read
    off the model: the prediction network consumes [start, y_0, .., y_(u-1)], the joint scores frame t of token u, log_softmax."""
    f64 = torch.as_tensor(np.asarray(f), dtype=torch.float64)
    out, best = [], []
    with torch.no_grad():
        if is_k2(cfg):
            sd64 = {k: sd[k].double() for k in ("decoder.embedding.weight", "decoder.conv.weight", "joiner.decoder_proj.weight",
                                                "joiner.decoder_proj.bias", "joiner.output_linear.weight", "joiner.output_linear.bias")}
            wo, bo = sd64["joiner.output_linear.weight"], sd64["joiner.output_linear.bias"]
            ys = [-1] * (cfg.context_size - 1) + [cfg.blank_id]
            for u, (y, t) in enumerate(zip(ids, frames)):
                t = t - u if frames_are_steps else t
                g = oz.decoder_out(cfg, sd64, ys[-cfg.context_size:])
                lp = torch.log_softmax(torch.tanh(f64[t] + g) @ wo.t() + bo, 0)
                out.append(float(lp[y])); best.append(int(lp.argmax()))
                ys.append(y)
            return np.asarray(out, np.float64), best
        arr = {k: ([torch.from_numpy(x).double() for x in v] if isinstance(v, list) else torch.from_numpy(v).double())
               for k, v in og.decoder_arrays(cfg, sd).items()}
        H, L = cfg.pred_hidden, cfg.pred_layers
        h = [torch.zeros(H, dtype=torch.float64) for _ in range(L)]
        c = [torch.zeros(H, dtype=torch.float64) for _ in range(L)]
        act = torch.tanh if getattr(cfg, "espnet", False) else torch.relu
        token = cfg.blank_id
        for u, (y, t) in enumerate(zip(ids, frames)):
            t = t - u if frames_are_steps else t
            x = arr["embed"][token]
            for l in range(L):                                # gate order i, f, g, o; W = [W_ih | W_hh], bias = b_ih + b_hh
                z = arr["lstm_w"][l] @ torch.cat([x, h[l]]) + arr["lstm_b"][l]
                i, fg, gg, o = torch.sigmoid(z[:H]), torch.sigmoid(z[H:2 * H]), torch.tanh(z[2 * H:3 * H]), torch.sigmoid(z[3 * H:])
                c[l] = fg * c[l] + i * gg
                h[l] = o * torch.tanh(c[l])
                x = h[l]
            g = arr["Wp"] @ h[L - 1] + arr["bp"]
            lp = torch.log_softmax(arr["Wo"] @ act(f64[t] + g) + arr["bo"], 0)
            out.append(float(lp[y])); best.append(int(lp.argmax()))
            token = y
    return np.asarray(out, np.float64), best


def oracle_greedy(cfg, sd, f, enc_lens, u_max=None):
    """the family's greedy search on the CPU oracle -> [(ids, frames)]"""
    return og.k2_greedy(cfg, sd, f, enc_lens, u_max) if is_k2(cfg) else og.rnnt_greedy(cfg, sd, f, enc_lens, u_max)
