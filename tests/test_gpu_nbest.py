"""-m gpu: n-best lists from the modified beam search on the device (rs_rnnt_mbs_nbest, csrc/k_rnnt_mbs.hip) against its C checker
(tests/k2_mbs_nbest_checker.c): ids, frames, n_ids, scores, norm_scores and n_hyps of every utterance BIT FOR BIT, given the same
joiner.encoder_proj output.

  toy geometry (V = 97)      B = 5, ragged lengths 24, 17, 1, 9 and 0 frames; max_active_paths 1, 2, 4, 8 x nbest 1, 2, max_active_paths;
                             the plain, hotword, LM and LM + hotword forms
  any-V form                 V = 10 753 (the first above 256 x 42: the selection kernel's NVR = 0 form), B = 3
  159M decoder geometry      V = 10 720, J = D = 512, B = 2 (the <42> form)
  the hand-built edges       a joiner whose logits are its bias alone (output_linear.weight = 0): a last set smaller than nbest with a
                             merge in the last frame and an exact tie in one search; a Finalize that reorders the list; no frames —
                             each shown reached by the checker's counters, then compared with the device
  batch invariance           row b alone == row b inside the batch
  the old entries            rs_rnnt_mbs / _hotwords / _lm return what their existing checkers say, and entry 0 of the list is their
                             result, bit for bit
  the public surface         K2Model(nbest=N): stream.result.nbest, transcribe / transcribe_batch, max_batch < n == one batch,
                             token_scores on entry 0, the settable count
  errors                     RS_EINVAL before anything is enqueued for nbest outside 1..8 or above max_active_paths, on a nemo
                             context; RS_EWORKSPACE; RS_EOVERFLOW; ValueError from the model
Without the feature these fail at symbol lookup."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import k2_hotwords_ref as H
import k2_mbs_lm_ref as LR
import k2_mbs_nbest_ref as NB
import k2_mbs_ref as R
from reazonspeech_amd.k2.asr import interface
from reazonspeech_amd.k2.asr.model import K2Model, synthetic_tokens
from reazonspeech_amd.runtime import capi, k2_hotwords as kh, ngram_lm as NL
from reazonspeech_amd.runtime.config import TINY
from reazonspeech_amd.runtime.k2_config import ZIPFORMER_TINY
from reazonspeech_amd.runtime.k2_weights import synthetic_state_dict_k2
from reazonspeech_amd.runtime.model import AsrModel, _HotwordSet, _NgramSet
from reazonspeech_amd.runtime.synth import synthetic_batch
from reazonspeech_amd.runtime.tokenizer import SyntheticTokenizer
from reazonspeech_amd.runtime.weights import synthetic_state_dict

k2tr = importlib.import_module("reazonspeech_amd.k2.asr.transcribe")

pytestmark = pytest.mark.gpu
PAD = int(0.9 * 16000)
ALPHA = 0.5
LENS = [24, 17, 1, 9, 0]
GRAPH_OF = [0, 1, 2, -1, 1]
RS_EWORKSPACE = -3
FILL = -7


def build(cfg, seed, sd=None, **kw):
    sd = sd if sd is not None else synthetic_state_dict_k2(cfg, seed)
    return K2Model(cfg, sd, synthetic_tokens(cfg.vocab_size, seed), device="cuda:0", **kw), sd


def device_nbest(am, f, lens, K, nbest, lm=None, alpha=0.0, hw=None, graph_of=None, blank_penalty=0.0, length_norm=True, out_cap=None,
                 short=0, query=True):
    """rs_rnnt_mbs_nbest on a projection f [B][Tp][J] -> per utterance dict(entries=[(ids, frames, score bits, norm bits)], n_ids),
    or None when nothing ran (the outputs keep their fill); `short`: bytes withheld from the workspace; `query` False: a workspace
    of the LM entry's size (for arguments the n-best query refuses)"""
    dev = am.device
    B, Tp, _ = f.shape
    out_cap = out_cap or max(Tp, 1)
    N = max(int(nbest), 1)
    f = f.to(dev).contiguous()
    lens = torch.as_tensor(np.asarray(lens), dtype=torch.int32).to(dev)
    ids = torch.zeros((B, N, out_cap), dtype=torch.int32, device=dev)
    frames = torch.zeros_like(ids)
    n_ids = torch.full((B, N), FILL, dtype=torch.int32, device=dev)
    n_hyps = torch.full((B,), FILL, dtype=torch.int32, device=dev)
    scores = torch.full((B, N), float("nan"), dtype=torch.float32, device=dev)
    norms = torch.full((B, N), float("nan"), dtype=torch.float32, device=dev)
    if query:
        ws = torch.empty((am.ctx.mbs_nbest_workspace_bytes(B, K, Tp, out_cap, nbest),), dtype=torch.uint8, device=dev)
    else:
        ws = torch.empty((am.ctx.mbs_workspace_bytes(B, min(max(K, 1), 8), Tp, out_cap, lm=True),), dtype=torch.uint8, device=dev)
    gof = None if graph_of is None else torch.as_tensor(np.asarray(graph_of), dtype=torch.int32).to(dev)
    stream = torch.cuda.current_stream().cuda_stream
    try:
        am.ctx.check(am.ctx.lib.rs_rnnt_mbs_nbest(
            am.ctx._h, f.data_ptr(), lens.data_ptr(), B, Tp, int(K), float(blank_penalty), capi.MBS_LENGTH_NORM if length_norm else 0,
            int(nbest), out_cap, ids.data_ptr(), frames.data_ptr(), n_ids.data_ptr(), scores.data_ptr(), norms.data_ptr(), n_hyps.data_ptr(),
            ctypes.byref(hw.struct) if hw is not None else None, gof.data_ptr() if gof is not None else None,
            ctypes.byref(lm.struct) if lm is not None else None, float(alpha), ws.data_ptr(), ws.numel() - short, ctypes.c_void_p(stream)))
    finally:
        torch.cuda.synchronize()
        device_nbest.untouched = bool((n_ids.cpu() == FILL).all() and (n_hyps.cpu() == FILL).all())
    n, nh = n_ids.cpu().numpy(), n_hyps.cpu().numpy()
    sb, nb = scores.cpu().numpy().view(np.int32), norms.cpu().numpy().view(np.int32)
    hi, hf = ids.cpu().numpy(), frames.cpu().numpy()
    return [dict(entries=[(hi[b, r, :n[b, r]].tolist(), hf[b, r, :n[b, r]].tolist(), int(sb[b, r]), int(nb[b, r])) for r in range(nh[b])],
                 n_ids=n[b].tolist()) for b in range(B)]


def check(cfg, sd, am, f, lens, K, nbest, lm=None, alpha=0.0, graphs=None, graph_of=None, **kw):
    """device == checker, bits; -> (device rows, checker rows)"""
    hw = _HotwordSet(graphs, am.device) if graphs else None
    ns = _NgramSet(lm, am.device) if lm is not None else None
    got = device_nbest(am, f, lens, K, nbest, lm=ns, alpha=alpha, hw=hw, graph_of=graph_of if graphs else None, **kw)
    want = NB.nbest_checker(cfg, sd, f.cpu().numpy(), np.asarray(lens, np.int32), nbest, kh.concat(graphs) if graphs else None,
                            graph_of if graphs else None, lm=lm, alpha=alpha, K=K, **kw)
    for b, (g, w) in enumerate(zip(got, want)):
        assert g["n_ids"] == w["n_ids"] and len(g["entries"]) == len(w["entries"]), (K, nbest, kw, b, g["n_ids"], w["n_ids"])
        assert g["entries"] == w["entries"], (K, nbest, kw, b, g["entries"], w["entries"])
    return got, want


def encoder_projection(model, waves):
    am = model.am
    buf = am.stage(waves, buf=am.new_buffers(len(waves), max(len(w) for w in waves)))
    am.run_device(buf)
    torch.cuda.synchronize()
    got = am.collect(buf)
    return buf.joint_enc.clone(), list(got.enc_lens)


@pytest.fixture(scope="module")
def tiny(gpu_device):
    return build(ZIPFORMER_TINY, 3)


@pytest.fixture(scope="module")
def toy(tiny):
    """the device's own projection of five utterances cut to 24, 17, 1, 9 and 0 frames, the plain search's results on it (checker,
    K = 4), the graphs and the LM cut from them"""
    model, sd = tiny
    audio, n = synthetic_batch(5, 3.0, seed=5, ragged=True, min_seconds=2.0)
    f, lens = encoder_projection(model, [np.pad(audio[b, :n[b]], PAD) for b in range(5)])
    assert min(lens) >= 24
    f = f[:, :24].contiguous()
    plain = R.mbs_checker(ZIPFORMER_TINY, sd, f.cpu().numpy(), np.asarray(LENS, np.int32), K=4)
    graphs = [kh.build_graph(p) for p in H.toy_graphs(plain)]
    lm = NL.build(LR.toy_lm(plain, ZIPFORMER_TINY), ZIPFORMER_TINY.vocab_size, ZIPFORMER_TINY.blank_id)
    return f, graphs, lm


@pytest.mark.parametrize("K,nbest", [(1, 1), (2, 1), (2, 2), (4, 1), (4, 2), (4, 4), (8, 1), (8, 2), (8, 8)])
def test_device_equals_checker_toy_geometry(tiny, toy, K, nbest):
    model, sd = tiny
    f, graphs, lm = toy
    sizes = set()
    for form in (dict(), dict(graphs=graphs, graph_of=GRAPH_OF), dict(lm=lm, alpha=ALPHA), dict(lm=lm, alpha=ALPHA, graphs=graphs, graph_of=GRAPH_OF)):
        got, want = check(ZIPFORMER_TINY, sd, model.am, f, LENS, K, nbest, **form)
        assert got[4]["entries"] == [] and got[4]["n_ids"] == [0] * nbest      # no frames: no entry
        assert len(got[2]["entries"]) == min(nbest, want[2]["last_set"])        # one frame
        sizes |= {len(g["entries"]) for g in got}
    assert nbest in sizes
    check(ZIPFORMER_TINY, sd, model.am, f, LENS, K, nbest, length_norm=False, blank_penalty=1.5)


def test_any_vocabulary_form(gpu_device):
    cfg = ZIPFORMER_TINY.with_(vocab_size=256 * 42 + 1).validate()          # the first vocabulary the <42> form does not take
    model, sd = build(cfg, 0)
    g = torch.Generator().manual_seed(5)
    f = torch.randn((3, 12, cfg.joiner_dim), generator=g) * 0.9
    got, _ = check(cfg, sd, model.am, f, [12, 1, 10], 4, 4)
    assert [len(r["entries"]) for r in got] == [4, 4, 4]
    check(cfg, sd, model.am, f, [12, 1, 10], 4, 2, length_norm=False)


def test_159m_decoder_geometry(gpu_device):
    cfg = ZIPFORMER_TINY.with_(vocab_size=10720, decoder_dim=512, joiner_dim=512).validate()
    model, sd = build(cfg, 0)
    g = torch.Generator().manual_seed(2)
    f = torch.randn((2, 24, cfg.joiner_dim), generator=g) * (0.8 + 0.4 * torch.rand((2, 1, 1), generator=g))
    plain = R.mbs_checker(cfg, sd, f.numpy(), np.asarray([24, 13], np.int32), K=4)
    seqs = [y for r in plain for y, _ in r["final"] if y]
    assert seqs, "the fixture must emit tokens"
    lm = NL.build(LR.random_lm(cfg, seqs, n_high=500, order=3, seed=4), cfg.vocab_size, cfg.blank_id)
    graph = kh.build_graph([(tuple(y[:2]), 2.0) for y in seqs if len(y) >= 2][:20] or [((seqs[0][0],), 2.0)])
    got, _ = check(cfg, sd, model.am, f, [24, 13], 4, 4)
    assert [len(r["entries"]) for r in got] == [4, 4] and sum(len(e[0]) for r in got for e in r["entries"]) > 8
    check(cfg, sd, model.am, f, [24, 13], 8, 8, lm=lm, alpha=0.3, graphs=[graph], graph_of=[0, -1])


# ---- the hand-built edges: logits = the joiner's bias alone, so every frame of every hypothesis offers the same distribution ---------
def flat_model(probs):
    """a toy Zipformer whose joiner ignores its input (output_linear.weight = 0): token v has probability probs[v] (the rest of the
    vocabulary shares what is left, far below)"""
    cfg = ZIPFORMER_TINY
    sd = synthetic_state_dict_k2(cfg, 7)
    bias = np.full((cfg.vocab_size,), np.log(1e-9), np.float32)
    for v, p in probs.items():
        bias[v] = np.float32(np.log(p))
    sd["joiner.output_linear.weight"] = torch.zeros_like(sd["joiner.output_linear.weight"])
    sd["joiner.output_linear.bias"] = torch.from_numpy(bias)
    return build(cfg, 7, sd=sd)


def test_the_hand_built_edges_on_the_device(gpu_device):
    cfg = ZIPFORMER_TINY
    A, Bt, C = 10, 11, 12
    model, sd = flat_model({cfg.blank_id: .3, cfg.unk_id: .2, A: .2, Bt: .2, C: .05})
    f = torch.zeros((2, 3, cfg.joiner_dim))
    # one frame, K = 4: blank, <unk> (merges into the blank's entry), A and B with equal values: 3 entries for 4 places, a merge in
    # the last frame, an exact tie — and a row without frames
    got, want = check(cfg, sd, model.am, f, [1, 0], 4, 4)
    w = want[0]
    assert (w["last_set"], w["last_merges"]) == (3, 1) and w["ties"] >= 1                          # the edges are reached
    assert [e[0] for e in got[0]["entries"]] == [[], [A], [Bt]] and got[0]["n_ids"] == [0, 1, 1, 0]
    assert got[0]["entries"][1][3] == got[0]["entries"][2][3]                                      # equal norms, bits
    assert got[1]["entries"] == [] and want[1]["last_set"] == 0
    # K = 8 lets [C] into the set; the phrase C A gives it a pending + 3.0: before Finalize it leads the whole set, after it it is
    # fourth again
    graph = kh.build_graph([((C, A), 3.0)])
    got, want = check(cfg, sd, model.am, f, [1, 0], 8, 4, graphs=[graph], graph_of=[0, -1], length_norm=False)
    assert want[0]["finalize_reorders"] == 1 and want[0]["finalize"] == -3.0                       # the edge is reached
    assert [e[0] for e in got[0]["entries"]] == [[], [A], [Bt], [C]]
    # three frames of the same distribution: merges in every frame leave 4 entries for 8 places
    got, want = check(cfg, sd, model.am, f, [3, 2], 8, 8)
    assert want[0]["merges"] > 0 and len(got[0]["entries"]) == want[0]["last_set"] == 4


def test_alone_equals_inside_the_batch(tiny, toy):
    model, _ = tiny
    am = model.am
    f, graphs, lm = toy
    hw, ns = _HotwordSet(graphs, am.device), _NgramSet(lm, am.device)
    together = device_nbest(am, f, LENS, 4, 4, lm=ns, alpha=ALPHA, hw=hw, graph_of=GRAPH_OF)
    for b in (0, 1, 2, 3):
        alone = device_nbest(am, f[b:b + 1, :LENS[b]], LENS[b:b + 1], 4, 4, lm=ns, alpha=ALPHA, hw=hw, graph_of=[GRAPH_OF[b]])
        assert alone[0] == together[b], b


def old_entry(am, f, lens, K, entry, lm=None, alpha=0.0, hw=None, graph_of=None):
    """rs_rnnt_mbs / rs_rnnt_mbs_hotwords / rs_rnnt_mbs_lm -> [(ids, frames, score bits)]"""
    dev = am.device
    B, Tp, _ = f.shape
    f = f.to(dev).contiguous()
    lens = torch.as_tensor(np.asarray(lens), dtype=torch.int32).to(dev)
    ids = torch.zeros((B, Tp), dtype=torch.int32, device=dev)
    frames = torch.zeros_like(ids)
    n_ids = torch.zeros((B,), dtype=torch.int32, device=dev)
    scores = torch.zeros((B,), dtype=torch.float32, device=dev)
    gof = None if graph_of is None else torch.as_tensor(np.asarray(graph_of), dtype=torch.int32).to(dev)
    ws = torch.empty((am.ctx.mbs_workspace_bytes(B, K, Tp, Tp, hotwords=entry != "plain", lm=entry == "lm"),), dtype=torch.uint8, device=dev)
    kw = {}
    if entry != "plain":
        kw.update(hotwords=hw.struct, graph_of=gof)
    if entry == "lm":
        kw.update(lm=lm.struct, lm_alpha=alpha)
    am.ctx.rnnt_mbs(f, lens, B, Tp, K, 0.0, True, ids, frames, n_ids, scores, ws, torch.cuda.current_stream().cuda_stream, **kw)
    torch.cuda.synchronize()
    n, bits = n_ids.cpu().numpy(), scores.cpu().numpy().view(np.int32)
    return [(ids[b, :n[b]].cpu().tolist(), frames[b, :n[b]].cpu().tolist(), int(bits[b])) for b in range(B)]


def test_the_old_entries_return_what_they_returned(tiny, toy):
    model, sd = tiny
    am = model.am
    f, graphs, lm = toy
    hw, ns = _HotwordSet(graphs, am.device), _NgramSet(lm, am.device)
    fa, la, table = f.cpu().numpy(), np.asarray(LENS, np.int32), kh.concat(graphs)
    for K in (2, 4, 8):
        cases = (("plain", {}, R.mbs_checker(ZIPFORMER_TINY, sd, fa, la, K=K)),
                 ("hotwords", dict(hw=hw, graph_of=GRAPH_OF), R.mbs_checker(ZIPFORMER_TINY, sd, fa, la, table, GRAPH_OF, K=K)),
                 ("lm", dict(hw=hw, graph_of=GRAPH_OF, lm=ns, alpha=ALPHA),
                  LR.mbs_lm_checker(ZIPFORMER_TINY, sd, fa, la, table, GRAPH_OF, lm=lm, alpha=ALPHA, K=K)))
        for entry, kw, want in cases:
            got = old_entry(am, f, LENS, K, entry, **kw)
            assert got == [(w["ids"], w["frames"], w["score_bits"]) for w in want], (K, entry)
            lists = device_nbest(am, f, LENS, K, K, **kw)
            for b in range(4):                                             # entry 0 of the list is the old entry's result
                assert lists[b]["entries"][0][:3] == got[b], (K, entry, b)
            assert lists[4]["entries"] == [] and got[4] == ([], [], 0)


def test_through_k2model_and_the_transcribe_functions(tiny):
    cfg = ZIPFORMER_TINY
    _, sd = tiny
    mbs = dict(decoding_method="modified_beam_search")
    off, _ = build(cfg, 3, sd=sd, **mbs)
    model, _ = build(cfg, 3, sd=sd, nbest=3, **mbs)
    assert (off.nbest, model.nbest) == (0, 3)
    audio, lens = synthetic_batch(9, 2.0, seed=50, ragged=True, min_seconds=0.5)
    audios = [interface.AudioData(audio[b, :lens[b]], 16000) for b in range(9)]
    conf = interface.TranscribeConfig(verbose=False)
    base = k2tr.transcribe_batch(off, audios, conf)
    assert all(type(r) is interface.TranscribeResult for r in base)         # off: today's objects
    res = k2tr.transcribe_batch(model, audios, conf)
    for r, b in zip(res, base):
        assert type(r) is interface.NBestTranscribeResult and (r.text, r.subwords) == (b.text, b.subwords)
        assert 1 <= len(r.nbest) <= 3 and (r.nbest[0].text, r.nbest[0].subwords, r.nbest[0].log_prob) == (r.text, r.subwords, r.log_prob)
        norms = [e.norm_log_prob for e in r.nbest]
        assert norms == sorted(norms, reverse=True) and len({tuple(s.token for s in e.subwords) for e in r.nbest}) == len(r.nbest)
    assert max(len(r.nbest) for r in res) == 3
    one = k2tr.transcribe(model, audios[4], conf)
    assert [(e.text, e.log_prob) for e in one.nbest] == [(e.text, e.log_prob) for e in res[4].nbest]
    # the runtime's lists are the checker's on the device's projection; a list longer than max_batch == one batch
    am = model.am
    waves = [np.pad(a.waveform, PAD) for a in audios]
    buf = am.stage(waves, buf=am.new_buffers(9, max(len(w) for w in waves)))
    am.run_device(buf)
    torch.cuda.synchronize()
    got = am.collect(buf)
    want = NB.nbest_checker(cfg, sd, buf.joint_enc.cpu().numpy(), np.asarray(got.enc_lens, np.int32), 3, K=4)
    for b in range(9):
        assert [(y, fr, NB.bits(s), NB.bits(n)) for y, fr, s, n in got.nbest[b]] == want[b]["entries"], b
        assert (got.ids[b], got.frames[b], NB.bits(got.scores[b])) == want[b]["entries"][0][:3]
    whole, parts = am.transcribe_waveforms(waves), am.transcribe_waveforms(waves, max_batch=4)
    assert whole.nbest == got.nbest == parts.nbest and (whole.ids, whole.scores) == (parts.ids, parts.scores)
    # per call and settable; token scores ride on entry 0
    assert am.transcribe_waveforms(waves, nbest=0).nbest is None
    assert [l[:2] for l in whole.nbest] == am.transcribe_waveforms(waves, nbest=2).nbest
    model.nbest = 0
    assert all(type(r) is interface.TranscribeResult for r in k2tr.transcribe_batch(model, audios, conf))
    model.nbest, model.token_scores = 2, True
    scored = k2tr.transcribe_batch(model, audios, conf)
    off.token_scores = True
    ref = k2tr.transcribe_batch(off, audios, conf)
    for r, b in zip(scored, ref):
        assert r.token_logprobs == b.token_logprobs and r.nbest[0].token_logprobs == b.token_logprobs
        assert all(e.token_logprobs is None for e in r.nbest[1:])
    with pytest.raises(ValueError, match="above the beam"):
        model.nbest = 5
    with pytest.raises(ValueError, match="above the beam"):
        am.transcribe_waveforms(waves, nbest=5)
    greedy, _ = build(cfg, 3, sd=sd)
    with pytest.raises(ValueError, match="needs a beam search"):
        greedy.am.transcribe_waveforms(waves[:2], nbest=2)


def test_errors(tiny, toy):
    model, _ = tiny
    am = model.am
    f, graphs, lm = toy
    ns = _NgramSet(lm, am.device)
    # refused from the argument list, before anything is enqueued: the outputs keep their fill
    for K, nbest, pattern in ((4, 0, "nbest must be 1..8"), (8, 9, "nbest must be 1..8"), (4, -1, "nbest must be 1..8"),
                              (4, 5, "above max_active_paths"), (2, 3, "above max_active_paths"), (9, 2, "max_active_paths must be 1..8")):
        with pytest.raises(capi.RsError, match=pattern) as e:
            device_nbest(am, f, LENS, K, nbest, query=False)
        assert e.value.code == capi.RS_EINVAL and device_nbest.untouched, (K, nbest)
    with pytest.raises(capi.RsError, match="lm_alpha") as e:
        device_nbest(am, f, LENS, 4, 2, lm=ns, alpha=float("nan"))
    assert e.value.code == capi.RS_EINVAL and device_nbest.untouched
    for args in ((4, 0), (4, 5), (0, 1), (9, 2)):
        with pytest.raises(RuntimeError):
            am.ctx.mbs_nbest_workspace_bytes(5, args[0], 24, 24, args[1])
    with pytest.raises(capi.RsError, match="workspace") as e:
        device_nbest(am, f, LENS, 4, 4, lm=ns, alpha=ALPHA, short=1)       # (the query sizes the LM form's layout, the largest)
    assert e.value.code == RS_EWORKSPACE
    with pytest.raises(capi.RsError, match="out_cap") as e:                # a returned entry that does not fit
        device_nbest(am, f, LENS, 4, 4, out_cap=1)
    assert e.value.code == capi.RS_EOVERFLOW
    nemo = AsrModel(TINY, synthetic_state_dict(TINY, 0), SyntheticTokenizer(TINY.vocab_size), device="cuda:0")
    with pytest.raises(RuntimeError):
        nemo.ctx.mbs_nbest_workspace_bytes(2, 4, 10, 10, 2)
    dev = nemo.device
    z = lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)          # noqa: E731
    zf = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)       # noqa: E731
    with pytest.raises(capi.RsError, match="Zipformer") as e:
        nemo.ctx.rnnt_mbs_nbest(zf(2, 10, TINY.joint_hidden), z(2) + 10, 2, 10, 4, 0.0, True, 2, z(2, 2, 10), z(2, 2, 10), z(2, 2), zf(2, 2),
                                zf(2, 2), z(2), torch.empty((1 << 20,), dtype=torch.uint8, device=dev), 0)
    assert e.value.code == capi.RS_EINVAL
    with pytest.raises(ValueError, match="above the beam"):
        AsrModel(TINY.with_(decoding="alsd", beam_size=4), {}, SyntheticTokenizer(TINY.vocab_size), device="cuda:0", nbest=5)
