"""Fixtures and CPU references of tests/test_gpu_conformer_lengths.py (no GPU code; tests/test_conformer_lengths_host.py runs
everything here on the CPU).

  families   "nemo"    TINY (FastConformer-RNNT toy: 2 layers, d_model 256, 2 heads of 128, conv kernel 9, dw_striding x8)
             "nemo_w"  the same weights with limited-context attention: att_left 20, att_right 10, one global token (the W1 of
                       tests/test_gpu_attention_edges.py)
             "espnet"  ESPNET_TINY (Conformer-Transducer toy: 2 layers, d_model 256, 4 heads of 64, conv kernel 15, Conv2dSubsampling x4)
  weights    synthetic_state_dict / synthetic_state_dict_espnet, one seed per family (WEIGHT_SEED)
  audio      `runtime/synth.py` speech-like audio cut to the sample count that gives exactly T' encoder frames without padding
             (`samples_for`: a multiple of 64, the row alignment of the staging buffers, so a buffer sized to the utterance has the
             utterance's own frame count); one seed per (family, T'): `seed_for`
  oracle     `oracle(family, T', recipe)`: oracle/model.py / oracle/espnet.py run end to end once per case (lru_cache), trimmed to
             the utterance's length: sub_out, layer0, layer1, enc, joint (+ ctc for ESPnet); `greedy(family, T')`: the float32 oracle's
             greedy search; `margin(family, T')`: the smallest decision margin along that path, float64 walk
  comparison `errors` (max, mean and last-row max of |got - ref| per tap) and `violations` (the figures that exceed a tolerance):
             the GPU test and the host test's mutation check share them

The seeds are chosen on the CPU, by the oracle alone: SEEDS lists the (family, T') whose default seed gave a near-tie or, at T' >= 8, no
token; tests/test_conformer_lengths_host.py asserts the property for every utterance the GPU module runs.
"""
import functools
import importlib.util
import os

import numpy as np
import torch

from oracle import espnet as oe, model as om
from reazonspeech_amd.runtime.config import ESPNET_TINY, TINY
from reazonspeech_amd.runtime.synth import synthetic_batch
from reazonspeech_amd.runtime.weights import synthetic_state_dict
from reazonspeech_amd.runtime.weights_espnet import synthetic_state_dict_espnet

HERE = os.path.dirname(os.path.abspath(__file__))
NEAR_TIE = 1e-3                     # the project's near-tie (tests/golden/make_k2_golden.py, make_espnet_golden.py)
TOL_BF16_MAX, TOL_BF16_MEAN = 6e-2, 6e-3          # the toy tolerance of tests/test_gpu_pipeline.py and tests/test_gpu_espnet.py
TOL_CTC_BF16 = 3e-2                 # tests/test_gpu_espnet.py
FACTOR_F32 = 8.0                    # tests/test_gpu_subsample_edges.py: two float32 evaluations that differ in summation order
FLOOR_F32 = 4 * 2.0 ** -23
W1 = (20, 10, 1)                    # tests/test_gpu_attention_edges.py W1
WEIGHT_SEED = {"nemo": 3, "nemo_w": 3, "espnet": 3}
CFGS = {"nemo": TINY, "nemo_w": TINY.with_(att_left=W1[0], att_right=W1[1], n_global=W1[2]), "espnet": ESPNET_TINY}
TAPS = ("sub_out", "layer0", "layer1", "enc", "joint")

LADDER = {"nemo": (1, 2, 3, 4, 5, 8, 9, 31, 32, 33, 47, 48, 49, 63, 64, 65, 95, 96, 97, 159, 160, 161, 191, 192, 193, 319, 320, 321, 385),
          "espnet": (1, 2, 3, 7, 8, 9, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 383, 384, 385, 513)}
UNFUSED_TP = (3, 32, 33, 48, 49, 129)             # section 2, both families
FORM_TP = (9, 33, 129, 161, 193)                  # section 3: the utterances ...
FORM_BUF = (33, 161, 193, 385)                    # ... and the buffers they ride in
WINDOW_TP = (31, 33, 255, 256, 257, 511, 512, 513)
CAP_TP = (20, 200)                                # section 5
PUBLIC_TP = {"nemo": (20, 100, 250), "espnet": (50, 200, 450)}      # section 7, after the package's own padding

# (family, T') -> seed where the default (`seed_for`) gives a near-tie in the oracle or, at T' >= 8, no token
SEEDS = {("nemo", 33): 13033, ("nemo", 48): 14048, ("nemo", 64): 12064, ("nemo", 65): 17065, ("nemo", 129): 30129, ("nemo", 159): 14159,
         ("nemo", 161): 21161, ("nemo", 191): 49191, ("nemo", 192): 13192, ("nemo", 193): 13193, ("nemo", 200): 18200, ("nemo", 319): 14319,
         ("nemo", 320): 113320, ("nemo", 321): 126321, ("nemo", 385): 60385, ("nemo_w", 255): 12255, ("nemo_w", 256): 32256,
         ("nemo_w", 257): 21257, ("nemo_w", 511): 624511, ("nemo_w", 512): 108512, ("nemo_w", 513): 234513}


def utterances():
    """every (family, T') the GPU module runs against the oracle or decodes"""
    out = []
    for fam in ("nemo", "espnet"):
        out += [(fam, t) for t in sorted(set(LADDER[fam]) | set(UNFUSED_TP) | set(FORM_TP) | set(FORM_BUF) | set(CAP_TP))]
    return out + [("nemo_w", t) for t in WINDOW_TP]


def seed_for(fam, tp):
    base = {"nemo": 11000, "nemo_w": 11000, "espnet": 12000}[fam]
    return SEEDS.get((fam, tp), base + tp)


@functools.lru_cache(maxsize=None)
def weights(fam):
    cfg = CFGS[fam]
    return synthetic_state_dict_espnet(cfg, WEIGHT_SEED[fam]) if cfg.espnet else synthetic_state_dict(cfg, WEIGHT_SEED[fam])


def samples_for(cfg, tp):
    """samples of an utterance with exactly tp encoder frames and no padding: the largest multiple of 64 that still gives tp (tp = 0: the
    largest that gives no frame at all)"""
    n = 0
    while cfg.enc_frames(cfg.mel_frames(n + 64)) <= tp:
        n += 64
    assert n > 0 and n % 64 == 0 and cfg.enc_frames(cfg.mel_frames(n)) == tp, (tp, n)
    return n


@functools.lru_cache(maxsize=None)
def wave(fam, tp, seed=None, samples=None):
    cfg = CFGS[fam]
    n = samples_for(cfg, tp) if samples is None else samples
    w = synthetic_batch(1, n / cfg.sample_rate, seed=seed_for(fam, tp) if seed is None else seed)[0][0][:n]
    assert w.shape[0] == n and cfg.enc_frames(cfg.mel_frames(n)) == tp
    w.setflags(write=False)
    return w


def forward(cfg, sd, w, recipe):
    """the oracle end to end on one utterance -> dict of tensors trimmed to its length (TAPS; ctc for ESPnet), enc_len, n_frames"""
    audio, lens = torch.from_numpy(np.array(w, dtype=np.float32))[None], torch.tensor([len(w)])
    taps = {}
    if cfg.espnet:
        ref = oe.forward(cfg, sd, audio, lens, recipe, taps)
        n = int(ref["enc_lens"][0])
        out = {"enc": ref["enc"][0, :n], "joint": ref["joint_enc"][0, :n], "ctc": ref["ctc"][0, :n]}
    else:
        f, el = om.forward_to_joint(cfg, sd, audio, lens, recipe, taps)
        n = int(el[0])
        out = {"enc": taps["enc"][0, :n], "joint": f[0, :n]}
    for name in ("sub_out", "layer0", "layer1"):
        out[name] = taps[name][0, :n]
    out["enc_len"], out["n_frames"], out["feats"] = n, int(taps["n_frames"][0]), taps["feats"][0]
    return out


@functools.lru_cache(maxsize=None)
def oracle(fam, tp, recipe):
    ref = forward(CFGS[fam], weights(fam), wave(fam, tp), recipe)
    assert ref["enc_len"] == tp == CFGS[fam].enc_frames(ref["n_frames"])
    return ref


def frontend_as(cfg, sd, w, dtype):
    """the oracle's own front-end of one utterance with all arithmetic in `dtype` -> (features [1][n][n_mels], n)"""
    audio, lens = torch.from_numpy(np.array(w, dtype=np.float32))[None], torch.tensor([len(w)])
    with torch.no_grad():
        feats, n = (oe.frontend if cfg.espnet else om.frontend)(cfg, sd, audio, lens, dtype=dtype)
    return feats, int(n[0])


@functools.lru_cache(maxsize=None)
def sub_out_yardstick(fam, tp):
    """reference-only yardsticks of the one tap that is not LayerNorm-ed (sub_out holds values of tens), the quantities of
    tests/test_gpu_subsample_edges.py taken over front-end AND subsampling, since here the device computes its own features:
      fp32                 max(FACTOR_F32 * max |oracle32 - oracle64|, FLOOR_F32 * max |oracle64|); oracle64 = the front-end and the subsampling
                           in float64 on the same float32 parameters and audio
      bf16_max, bf16_mean  max / mean |bf16 recipe - oracle32|
    over the whole utterance"""
    cfg, sd = CFGS[fam], weights(fam)
    ref = oracle(fam, tp, "fp32")
    sub = oe.subsampling if cfg.espnet else om.subsampling
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    n = torch.tensor([ref["n_frames"]])
    with torch.no_grad():
        feats64, n64 = frontend_as(cfg, sd, wave(fam, tp), torch.float64)
        assert n64 == ref["n_frames"]
        ref64 = sub(cfg, sd64, feats64, n, "fp32")[0][0, :tp]
        b16 = sub(cfg, sd, ref["feats"][None, :ref["n_frames"]], n, "bf16")[0][0, :tp].double()
    f32 = ref["sub_out"].double()
    gap = (b16 - f32).abs()
    return {"fp32": max(FACTOR_F32 * float((f32 - ref64).abs().max()), FLOOR_F32 * float(ref64.abs().max())),
            "bf16_max": float(gap.max()), "bf16_mean": float(gap.mean())}


@functools.lru_cache(maxsize=None)
def greedy(fam, tp):
    """(ids, frames) of the float32 oracle's own greedy search"""
    cfg, sd = CFGS[fam], weights(fam)
    ref = oracle(fam, tp, "fp32")
    search = oe.greedy_torch if cfg.espnet else om.greedy_torch
    ids, frames = search(cfg, sd, ref["joint"][None], torch.tensor([tp]))[0]
    return list(ids), list(frames)


@functools.lru_cache(maxsize=None)
def _espnet_golden_tools():
    spec = importlib.util.spec_from_file_location("make_espnet_golden", os.path.join(HERE, "golden", "make_espnet_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def nemo_greedy_margins(cfg, sd, f, n, ids, frames):
    """float64 walk along the greedy path of the NeMo joint (relu, up to max_symbols labels per frame, multi-layer LSTM): the smallest
    top-1 minus top-2 margin over every decision; 0 where the walk itself disagrees with the path (a tie at float32 resolution)"""
    H = cfg.pred_hidden
    P = "decoder.prediction.dec_rnn.lstm."
    emb = sd["decoder.prediction.embed.weight"].double()
    lstm = [(sd[P + f"weight_ih_l{l}"].double(), sd[P + f"weight_hh_l{l}"].double(), (sd[P + f"bias_ih_l{l}"] + 0.0).double() + sd[P + f"bias_hh_l{l}"].double())
            for l in range(cfg.pred_layers)]
    wp, bp = sd["joint.pred.weight"].double(), sd["joint.pred.bias"].double()
    wo, bo = sd["joint.joint_net.2.weight"].double(), sd["joint.joint_net.2.bias"].double()
    st = [(torch.zeros(H, dtype=torch.float64), torch.zeros(H, dtype=torch.float64)) for _ in lstm]

    def step(tok):
        x = emb[tok]
        for l, (wi, wh, b) in enumerate(lstm):
            h, c = st[l]
            g = wi @ x + wh @ h + b
            i, fg, gg, o = g[:H].sigmoid(), g[H:2 * H].sigmoid(), g[2 * H:3 * H].tanh(), g[3 * H:].sigmoid()
            c = fg * c + i * gg
            h = o * c.tanh()
            st[l] = (h, c)
            x = h
        return wp @ x + bp
    g = step(cfg.blank_id)
    fd = torch.as_tensor(f).double()
    path = list(zip(frames, ids))
    worst, u = float("inf"), 0
    for t in range(n):
        sym = 0
        while sym < cfg.max_symbols:
            z = wo @ torch.relu(fd[t] + g) + bo
            top = torch.topk(z, 2)
            worst = min(worst, float(top.values[0] - top.values[1]))
            want = path[u][1] if u < len(path) and path[u][0] == t else cfg.blank_id
            if int(top.indices[0]) != want:
                worst = 0.0
            if want == cfg.blank_id:
                break
            g = step(want)
            u += 1
            sym += 1
    if u != len(path):
        worst = 0.0
    return worst


@functools.lru_cache(maxsize=None)
def margin(fam, tp):
    cfg, sd = CFGS[fam], weights(fam)
    ids, frames = greedy(fam, tp)
    f = oracle(fam, tp, "fp32")["joint"]
    if cfg.espnet:
        return _espnet_golden_tools().greedy_margins(cfg, sd, f.numpy(), tp, ids, frames)
    return nemo_greedy_margins(cfg, sd, f, tp, ids, frames)


def errors(got, ref, names=TAPS):
    """per tap: (max, mean, max over the LAST valid row) of |got - ref|; got and ref hold [n][.] tensors of one utterance"""
    out = {}
    for name in names:
        a, r = got[name], ref[name]
        assert a.shape == r.shape and a.shape[0] >= 1, (name, tuple(a.shape), tuple(r.shape))
        e = (a.double() - r.double()).abs()
        out[name] = (float(e.max()), float(e.mean()), float(e[-1].max()))
    return out


def violations(errs, tol_max, tol_mean=None, bounds=None):
    """the figures of `errors` above the tolerance: max and last-row max against tol_max, mean against tol_mean (when given);
    `bounds`: {tap: (tol_max, tol_mean)} for the taps that have a bound of their own"""
    bad = []
    for name, (mx, mean, last) in errs.items():
        t_max, t_mean = (bounds or {}).get(name, (tol_max, tol_mean))
        if not (mx <= t_max and last <= t_max):
            bad.append((name, "max", mx, last, t_max))
        if t_mean is not None and not mean <= t_mean:
            bad.append((name, "mean", mean, t_mean))
    return bad


def forms(fam, tp):
    """the kernel forms a buffer of tp frames selects (csrc/k_attention.hip launch_attention_hd, csrc/k_f32.hip rs_launch_attention_f32,
    csrc/k_layernorm.hip rs_launch_glu_dwconv), as the module docstring of the GPU test tabulates them"""
    cfg = CFGS[fam]
    qb = (tp + 31) // 32
    window = cfg.att_left >= 0 or cfg.att_right >= 0
    if cfg.head_dim == 128 or window:
        nw = min(qb, 6)
        bf16 = f"{'WINDOW' if window else 'staged'}<{cfg.head_dim}> {nw} waves x {(qb + nw - 1) // nw} wg, {(qb + 4) // 5} key chunk(s) of 5"
    elif tp <= 32:
        bf16 = "staged<64,kbc 2> one wave"
    else:
        nw = min(qb, 4)
        bf16 = f"staged<64,kbc 4> {nw} waves x {(qb + nw - 1) // nw} wg, {(qb + 3) // 4} key chunk(s) of 4"
    if window:
        f32 = "keys<4>" if tp <= 256 else "keys<8>" if tp <= 512 else "keys<0>"
    else:
        f32 = f"mfma<{cfg.head_dim}> {(tp + 63) // 64} x 64 queries"
    k = cfg.conv_kernel
    conv = f"dwconv_silu_dma<9,6> {(tp + 47) // 48} x 48" if k == 9 else f"dwconv_act<{k},0> {(tp + 127) // 128} x 128"
    conv0 = f"glu_fast<9,6,1> {(tp + 47) // 48} x 48" if k == 9 else f"glu_generic {(tp + 31) // 32} x 32"
    return {"attention bf16": bf16, "attention fp32": f32, "conv fused": conv, "conv unfused": conv0}
