"""-m gpu: n-best lists from ESPnet's default beam search on the device (rs_rnnt_beam_nbest, csrc/k_rnnt_beam.hip) against its C
checker (tests/espnet_beam_nbest_checker.c): ids, frames, n_ids, scores, norm_scores, n_hyps and the pop count of every utterance BIT
FOR BIT, given the same joint-encoder projection.

  toy geometry               ESPNET_TINY, B = 5, ragged lengths 24, 17, 1, 9 and 0 frames; beam 1, 2, 4, 8 x nbest 1, 2, beam; score norm
                             on and off
  the hand-built edges       a joint whose logits are its bias alone (lin_out.weight = 0): a kept list longer than nbest, a tie resolved
                             by list position, duplicates kept, the norm changing the order — each shown reached by the checker's
                             counters, then compared with the device
  batch invariance           row b alone == row b inside the batch
  the old entry              rs_rnnt_beam returns what oracle/espnet_beam.c says, and entry 0 of the list is its result, bit for bit
  the public surface         EspnetModel(beam_size=6, nbest=3): model(speech) returns 3 tuples with hyp.score; recognize_batch(nbest=);
                             the greedy fall-back returns a list of one and `degraded`; token scores ride on entry 0
  errors                     RS_EINVAL before anything is enqueued for nbest outside 1..8 or above the beam, on a Zipformer context;
                             RS_EWORKSPACE; RS_EOVERFLOW for max_pops and for out_cap
Without the feature these fail at symbol lookup."""
import ctypes

import numpy as np
import pytest
import torch

import espnet_beam_nbest_ref as EB
from oracle import greedy as og
from reazonspeech_amd.espnet.asr.model import EspnetModel, synthetic_token_list
from reazonspeech_amd.k2.asr.model import K2Model, synthetic_tokens
from reazonspeech_amd.runtime import capi
from reazonspeech_amd.runtime.config import ESPNET_TINY
from reazonspeech_amd.runtime.k2_config import ZIPFORMER_TINY
from reazonspeech_amd.runtime.k2_weights import synthetic_state_dict_k2
from reazonspeech_amd.runtime.synth import synthetic_batch
from reazonspeech_amd.runtime.weights_espnet import synthetic_state_dict_espnet

pytestmark = pytest.mark.gpu
LENS = [24, 17, 1, 9, 0]
RS_EWORKSPACE = -3
FILL = -7


def build(cfg, seed, bias, sd=None, **kw):
    sd = sd if sd is not None else synthetic_state_dict_espnet(cfg, seed, blank_bias=bias, dec_gain=8.0)
    return EspnetModel(cfg, sd, synthetic_token_list(cfg.vocab_size, seed), device="cuda:0", **kw), sd


def device_nbest(am, f, lens, beam, nbest, score_norm=True, max_pops=0, out_cap=None, short=0, query=True, with_frames=True):
    """rs_rnnt_beam_nbest on a projection f [B][Tp][J] -> per utterance dict(entries=[(ids, frames, score bits, norm bits)], n_ids,
    pops); `short`: bytes withheld from the workspace; `query` False: the workspace of rs_rnnt_beam (for arguments the n-best query
    refuses)"""
    dev = am.device
    B, Tp, _ = f.shape
    out_cap = out_cap or (2 * Tp + 16)
    N = max(int(nbest), 1)
    f = f.to(dev).contiguous()
    lens = torch.as_tensor(np.asarray(lens), dtype=torch.int32).to(dev)
    ids = torch.zeros((B, N, out_cap), dtype=torch.int32, device=dev)
    frames = torch.zeros_like(ids)
    n_ids = torch.full((B, N), FILL, dtype=torch.int32, device=dev)
    n_hyps = torch.full((B,), FILL, dtype=torch.int32, device=dev)
    pops = torch.full((B,), FILL, dtype=torch.int32, device=dev)
    scores = torch.full((B, N), float("nan"), dtype=torch.float32, device=dev)
    norms = torch.full((B, N), float("nan"), dtype=torch.float32, device=dev)
    if query:
        ws = torch.empty((am.ctx.beam_nbest_workspace_bytes(B, beam, Tp, max_pops, nbest),), dtype=torch.uint8, device=dev)
    else:
        ws = torch.empty((am.ctx.beam_workspace_bytes(B, max(beam, 1), Tp, max_pops),), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    try:
        am.ctx.check(am.ctx.lib.rs_rnnt_beam_nbest(
            am.ctx._h, f.data_ptr(), lens.data_ptr(), B, Tp, int(beam), capi_flag(score_norm), int(max_pops), int(nbest), out_cap,
            ids.data_ptr(), frames.data_ptr() if with_frames else None, n_ids.data_ptr(), scores.data_ptr(), norms.data_ptr(),
            n_hyps.data_ptr(), pops.data_ptr(), ws.data_ptr(), ws.numel() - short, ctypes.c_void_p(stream)))
    finally:
        torch.cuda.synchronize()
        device_nbest.untouched = bool((n_ids.cpu() == FILL).all() and (n_hyps.cpu() == FILL).all() and (pops.cpu() == FILL).all())
    n, nh, hp = n_ids.cpu().numpy(), n_hyps.cpu().numpy(), pops.cpu().numpy()
    sb, nb = scores.cpu().numpy().view(np.int32), norms.cpu().numpy().view(np.int32)
    hi, hf = ids.cpu().numpy(), frames.cpu().numpy()
    return [dict(entries=[(hi[b, r, :n[b, r]].tolist(), hf[b, r, :n[b, r]].tolist(), int(sb[b, r]), int(nb[b, r])) for r in range(nh[b])],
                 n_ids=n[b].tolist(), pops=int(hp[b])) for b in range(B)]


def capi_flag(score_norm):
    return 1 if score_norm else 0                          # RS_BEAM_SCORE_NORM


def check(cfg, sd, am, f, lens, beam, nbest, **kw):
    """device == checker, bits; -> (device rows, checker rows)"""
    got = device_nbest(am, f, lens, beam, nbest, **kw)
    want = EB.nbest_checker(cfg, sd, f.cpu().numpy(), np.asarray(lens, np.int32), nbest, beam=beam, max_pops=kw.get("max_pops") or 16 * beam,
                            out_cap=2 * f.shape[1] + 16, score_norm=kw.get("score_norm", True))
    for b, (g, w) in enumerate(zip(got, want)):
        assert g["n_ids"] == w["n_ids"] and g["pops"] == w["pops"], (beam, nbest, kw, b, g["n_ids"], w["n_ids"], g["pops"], w["pops"])
        assert g["entries"] == w["entries"], (beam, nbest, kw, b, g["entries"], w["entries"])
    return got, want


@pytest.fixture(scope="module")
def tiny(gpu_device):
    """the device's own projection of five 2 s utterances, cut to 24 frames"""
    model, sd = build(ESPNET_TINY, 11, 12.0)
    audio, lens = synthetic_batch(5, 2.0, seed=21)
    am = model.am
    buf = am.stage([audio[b, :int(lens[b])] for b in range(5)])
    with torch.cuda.device(am.device):
        stream = torch.cuda.current_stream().cuda_stream
        am.ctx.frontend(buf.audio, buf.lens, 0, 0, buf.t_max, buf.feats, buf.n_frames, buf.ws, stream)
        am.ctx.encoder(buf.feats, buf.n_frames, buf.B, buf.t_max, None, buf.joint_enc, buf.enc_lens, buf.ws, stream)
        torch.cuda.synchronize()
    assert int(buf.enc_lens.min()) >= 24
    return model, sd, buf.joint_enc[:, :24].contiguous().clone()


@pytest.mark.parametrize("beam,nbest", [(1, 1), (2, 1), (2, 2), (4, 1), (4, 2), (4, 4), (8, 1), (8, 2), (8, 8)])
def test_device_equals_checker_toy_geometry(tiny, beam, nbest):
    model, sd, f = tiny
    for score_norm in (True, False):
        got, want = check(model.cfg, sd, model.am, f, LENS, beam, nbest, score_norm=score_norm)
        assert got[4]["entries"] == [([], [], 0, 0)] and got[4]["pops"] == 0        # no frames: the start hypothesis alone
        assert [len(g["entries"]) for g in got[:4]] == [nbest] * 4
    assert sum(len(e[0]) for g in got for e in g["entries"]) > 0
    no_frames = device_nbest(model.am, f, LENS, beam, nbest, with_frames=False)     # frames may be NULL
    assert [[(e[0], e[2], e[3]) for e in g["entries"]] for g in no_frames] == [[(e[0], e[2], e[3]) for e in g["entries"]] for g in
                                                                              device_nbest(model.am, f, LENS, beam, nbest)]


def flat_model(probs):
    """an ESPnet-shaped toy whose joint ignores its inputs (lin_out.weight = 0): label v has probability probs[v] at every frame for
    every hypothesis (the rest of the vocabulary shares what is left, far below)"""
    cfg = ESPNET_TINY
    sd = synthetic_state_dict_espnet(cfg, 7, blank_bias=0.0, dec_gain=8.0)
    bias = np.full((cfg.n_logits,), np.log(1e-9), np.float32)
    for v, p in probs.items():
        bias[v] = np.float32(np.log(p))
    sd["joint_network.lin_out.weight"] = torch.zeros_like(sd["joint_network.lin_out.weight"])
    sd["joint_network.lin_out.bias"] = torch.from_numpy(bias)
    return build(cfg, 7, 0.0, sd=sd)


def test_the_hand_built_edges_on_the_device(gpu_device):
    cfg = ESPNET_TINY
    A, Bt, C = 10, 11, 12
    model, sd = flat_model({cfg.blank_id: .5, A: .2, Bt: .2, C: .05})
    f = torch.zeros((2, 3, cfg.joint_hidden))
    labels = lambda r: [(e[0], e[1]) for e in r["entries"]]               # noqa: E731
    # one frame, beam 2: the frame ends with 3 kept above the rest — a list longer than nbest — and [A], [B] score the same: the
    # tie goes to [A], kept first
    got, want = check(cfg, sd, model.am, f, [1, 0], 2, 2)
    assert want[0]["kept"] == 3 and want[0]["ties"] == 1                  # the edges are reached
    assert labels(got[0]) == [([], []), ([A], [0])]
    # three frames, beam 4: the same labels reached at different frames are different hypotheses and both stay; the norm reorders
    got, want = check(cfg, sd, model.am, f, [3, 2], 4, 4)
    assert want[0]["duplicates"] >= 1 and want[0]["norm_reorders"] == 1 and want[0]["kept"] > 4     # the edges are reached
    assert len({tuple(e[0]) for e in got[0]["entries"]}) < 4 and len({(tuple(e[0]), tuple(e[1])) for e in got[0]["entries"]}) == 4
    got_off, want_off = check(cfg, sd, model.am, f, [3, 2], 4, 4, score_norm=False)
    assert want_off[0]["norm_reorders"] == 0 and labels(got_off[0]) != labels(got[0])


def test_alone_equals_inside_the_batch(tiny):
    model, _, f = tiny
    together = device_nbest(model.am, f, LENS, 8, 8)
    for b in (0, 1, 2, 3):
        alone = device_nbest(model.am, f[b:b + 1, :LENS[b]], LENS[b:b + 1], 8, 8)
        assert alone[0] == together[b], b


def test_the_old_entry_returns_what_it_returned(tiny):
    model, sd, f = tiny
    am, dev = model.am, model.am.device
    B, Tp, _ = f.shape
    cap = 2 * Tp + 16
    lens = torch.as_tensor(LENS, dtype=torch.int32).to(dev)
    for beam in (2, 4, 8):
        for score_norm in (True, False):
            ids = torch.zeros((B, cap), dtype=torch.int32, device=dev)
            frames = torch.zeros_like(ids)
            n_ids, pops = torch.zeros((B,), dtype=torch.int32, device=dev), torch.zeros((B,), dtype=torch.int32, device=dev)
            scores = torch.zeros((B,), dtype=torch.float32, device=dev)
            ws = torch.empty((am.ctx.beam_workspace_bytes(B, beam, Tp, 0),), dtype=torch.uint8, device=dev)
            am.ctx.rnnt_beam(f, lens, B, Tp, beam, score_norm, 0, ids, n_ids, scores, pops, ws, torch.cuda.current_stream().cuda_stream, frames=frames)
            torch.cuda.synchronize()
            n, sb = n_ids.cpu().numpy(), scores.cpu().numpy().view(np.int32)
            got = [(ids[b, :n[b]].cpu().tolist(), frames[b, :n[b]].cpu().tolist(), int(sb[b]), int(pops[b])) for b in range(B)]
            want = og.espnet_beam(model.cfg, sd, f.cpu().numpy(), np.asarray(LENS, np.int32), beam=beam, score_norm=score_norm, max_pops=16 * beam,
                                  out_cap=cap, with_frames=True)
            assert got == [(w[0], w[1], EB.bits(w[2]), w[3]) for w in want], (beam, score_norm)
            lists = device_nbest(am, f, LENS, beam, beam, score_norm=score_norm)
            for b in range(B):                                             # entry 0 of the list is the old entry's result
                assert lists[b]["entries"][0][:3] == got[b][:3] and lists[b]["pops"] == got[b][3], (beam, score_norm, b)


def test_through_espnetmodel(gpu_device):
    off, sd = build(ESPNET_TINY, 11, 12.0, beam_size=6)
    model, _ = build(ESPNET_TINY, 11, 12.0, sd=sd, beam_size=6, nbest=3)
    assert (off.nbest, model.nbest) == (0, 3)
    audio, lens = synthetic_batch(3, 1.5, seed=4)
    waves = [audio[b, :int(lens[b])] for b in range(3)]
    one = off(waves[0])
    assert len(one) == 1 and one[0][3] is None                            # off: today's one tuple
    got = model(waves[0])
    assert len(got) == 3 and got[0][:3] == one[0][:3]
    for text, tokens, ids, hyp in got:
        assert text == model.ids_to_text(ids) and tokens == [model.token_list[i] for i in ids] and hyp.yseq == ids
        assert hyp.norm_score == float(np.float32(hyp.score) / np.float32(len(ids) + 1)) and hyp.token_logprobs is None
    assert [h.norm_score for *_, h in got] == sorted((h.norm_score for *_, h in got), reverse=True)
    # the lists are the checker's on the device's projection
    res = model._search(waves)
    buf = model.am.stage(waves)
    with torch.cuda.device(model.am.device):
        model.am.run_encoder(buf, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    want = EB.nbest_checker(model.cfg, sd, buf.joint_enc.cpu().numpy(), buf.enc_lens.cpu().numpy(), 3, beam=6, max_pops=96, out_cap=2 * buf.tp_max + 16)
    for b in range(3):
        assert [(y, fr, EB.bits(s), EB.bits(n)) for y, fr, s, n in res.nbest[b]] == want[b]["entries"], b
        assert (res.ids[b], res.frames[b], EB.bits(res.scores[b])) == want[b]["entries"][0][:3]
    assert res.degraded == [False] * 3
    # recognize_batch(nbest=): per call, also on the model loaded without lists
    padded = off.recognize_batch(waves)
    lists = off.recognize_batch(waves, nbest=2)
    assert [len(x) for x in lists] == [2, 2, 2] and [x[0][0] for x in lists] == padded
    assert [[e[:3] for e in x] for x in model.recognize_batch(waves, nbest=2)] == [[e[:3] for e in x] for x in lists]
    # token scores ride on entry 0
    model.token_scores = True
    off.token_scores = True
    scored = model(waves[1])
    assert scored[0][3].token_logprobs == off(waves[1])[0][3].token_logprobs and all(h.token_logprobs is None for *_, h in scored[1:])
    model.token_scores = False
    # the greedy fall-back (every beam decode made to overflow): a list of one, flagged
    import warnings
    real = model.am.decode

    def overflowing(ctx, buf, ws, stream, max_pops=None, decoding=None, nbest=None):
        if decoding is None:
            raise capi.RsError(capi.RS_EOVERFLOW, "beam search: a frame needed more than max_pops")
        return real(ctx, buf, ws, stream, max_pops=max_pops, decoding=decoding, nbest=nbest)
    model.am.decode = overflowing
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            res = model._search(waves)
            called = model(waves[0])
    finally:
        model.am.decode = real
    assert res.degraded == [True] * 3 and any("greedy search instead" in str(x.message) for x in w)
    assert [len(x) for x in res.nbest] == [1, 1, 1] and [x[0][0] for x in res.nbest] == res.ids and len(called) == 1
    with pytest.raises(ValueError, match="above beam_size=6"):
        build(ESPNET_TINY, 11, 12.0, sd=sd, beam_size=6, nbest=7)


def test_errors(tiny):
    model, _, f = tiny
    am = model.am
    # refused from the argument list, before anything is enqueued: the outputs keep their fill
    for beam, nbest, pattern in ((4, 0, "nbest must be 1..8"), (20, 9, "nbest must be 1..8"), (4, -1, "nbest must be 1..8"),
                                 (4, 5, "above the beam"), (2, 3, "above the beam"), (0, 1, "beam size must be >= 1")):
        with pytest.raises(capi.RsError, match=pattern) as e:
            device_nbest(am, f, LENS, beam, nbest, query=False)
        assert e.value.code == capi.RS_EINVAL and device_nbest.untouched, (beam, nbest)
    for args in ((4, 0), (4, 5), (0, 1), (20, 9)):
        with pytest.raises(RuntimeError):
            am.ctx.beam_nbest_workspace_bytes(5, args[0], 24, 0, args[1])
    with pytest.raises(capi.RsError, match="workspace") as e:
        device_nbest(am, f, LENS, 4, 4, short=1)
    assert e.value.code == RS_EWORKSPACE
    with pytest.raises(capi.RsError, match="max_pops") as e:
        device_nbest(am, f, LENS, 8, 8, max_pops=9)
    assert e.value.code == capi.RS_EOVERFLOW
    with pytest.raises(capi.RsError, match="out_cap") as e:               # a returned entry that does not fit
        device_nbest(am, f, LENS, 4, 4, out_cap=1)
    assert e.value.code == capi.RS_EOVERFLOW
    assert device_nbest(am, f, LENS, 2, 2)                                 # and the context is usable afterwards
    k2 = K2Model(ZIPFORMER_TINY, synthetic_state_dict_k2(ZIPFORMER_TINY, 0), synthetic_tokens(ZIPFORMER_TINY.vocab_size, 0), device="cuda:0")
    with pytest.raises(RuntimeError):
        k2.am.ctx.beam_nbest_workspace_bytes(2, 4, 10, 0, 2)
    dev = k2.am.device
    z = lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)          # noqa: E731
    zf = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)       # noqa: E731
    with pytest.raises(capi.RsError, match="rs_rnnt_beam_nbest: not defined for a Zipformer context") as e:
        k2.am.ctx.rnnt_beam_nbest(zf(2, 10, ZIPFORMER_TINY.joiner_dim), z(2) + 10, 2, 10, 4, True, 0, 2, z(2, 2, 10), z(2, 2), zf(2, 2), zf(2, 2),
                                  z(2), z(2), torch.empty((1 << 20,), dtype=torch.uint8, device=dev), 0)
    assert e.value.code == capi.RS_EINVAL
