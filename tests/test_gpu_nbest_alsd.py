"""-m gpu: n-best lists from the ALSD beam search on the device (rs_rnnt_alsd_nbest, csrc/k_rnnt_alsd.hip) against its C checker
(tests/alsd_nbest_checker.c): ids, alignment steps, n_ids, scores, norm_scores and n_hyps of every utterance BIT FOR BIT, given the
same joint-encoder projection.

  toy geometry               TINY (2 LSTM layers), B = 5, ragged lengths 24, 17, 1, 9 and 0 frames; beam 1, 2, 4, 8 x nbest 1, 2, beam;
                             the plain, hotword, LM and LM + hotword forms; merge on and off, norm on and off, a budget that ends
                             the search
  any-V form                 a vocabulary above 3072 (the selection kernel's NVR = 0 form), B = 3
  619M decoder geometry      V + 1 = 3001, 640-wide decoder and joint (the <48> form), B = 2
  the hand-built edges       a joint whose logits are its bias alone (joint_net.2.weight = 0): eviction from the tail, fewer finish
                             than nbest, nothing finishes, equal sequences finishing in one step, an exact tie across two steps, a
                             Finalize that reorders — each shown reached by the checker's counters, then compared with the device
  batch invariance           row b alone == row b inside the batch
  the old entries            rs_rnnt_alsd / _hotwords / _lm return what tests/alsd_checker.c says, and entry 0 of the list is their
                             result, bit for bit
  the public surface         load_model(decoding="alsd", nbest=N): transcribe / transcribe_batch return NBestTranscribeResult,
                             transcribe(nbest=), raw_hypothesis.n_best_hypotheses, token scores on entry 0, off returns today's objects
  errors                     RS_EINVAL before anything is enqueued for nbest outside 1..8 or above the beam, on a Zipformer context;
                             RS_EWORKSPACE; RS_EOVERFLOW
Without the feature these fail at symbol lookup."""
import ctypes

import numpy as np
import pytest
import torch

import alsd_hotwords_ref as AR
import alsd_nbest_ref as AN
import ngram_lm_ref as NR
from reazonspeech_amd.k2.asr.model import K2Model, synthetic_tokens
from reazonspeech_amd.nemo.asr import interface, load_model, transcribe, transcribe_batch
from reazonspeech_amd.runtime import capi, k2_hotwords as kh, ngram_lm as NL
from reazonspeech_amd.runtime.config import TINY, WIDE2
from reazonspeech_amd.runtime.k2_config import ZIPFORMER_TINY
from reazonspeech_amd.runtime.k2_weights import synthetic_state_dict_k2
from reazonspeech_amd.runtime.model import AsrModel, _HotwordSet, _NgramSet
from reazonspeech_amd.runtime.synth import synthetic_batch
from reazonspeech_amd.runtime.tokenizer import SyntheticTokenizer
from reazonspeech_amd.runtime.weights import synthetic_state_dict

pytestmark = pytest.mark.gpu
LENS = [24, 17, 1, 9, 0]
GRAPH_OF = [0, 1, 2, -1, 1]
ALPHA = 0.5
RS_EWORKSPACE = -3
FILL = -7


def device_nbest(am, f, lens, beam, nbest, max_target_len=2.0, score_norm=True, merge=False, lm=None, alpha=0.0, hw=None, graph_of=None,
                 out_cap=None, short=0, query=True):
    """rs_rnnt_alsd_nbest on a projection f [B][Tp][J] -> per utterance dict(entries=[(ids, steps, score bits, norm bits)], n_ids);
    `short`: bytes withheld from the workspace; `query` False: the workspace of rs_rnnt_alsd_lm plus room for the list (for arguments
    the n-best query refuses)"""
    dev = am.device
    f = torch.as_tensor(np.asarray(f)) if not isinstance(f, torch.Tensor) else f
    B, Tp, _ = f.shape
    budget = int(max_target_len * Tp) if isinstance(max_target_len, float) else int(max_target_len)
    out_cap = out_cap or max(1, Tp + budget)
    N = max(int(nbest), 1)
    f = f.to(dev).contiguous()
    lens = torch.as_tensor(np.asarray(lens), dtype=torch.int32).to(dev)
    ids = torch.zeros((B, N, out_cap), dtype=torch.int32, device=dev)
    steps = torch.zeros_like(ids)
    n_ids = torch.full((B, N), FILL, dtype=torch.int32, device=dev)
    n_hyps = torch.full((B,), FILL, dtype=torch.int32, device=dev)
    scores = torch.full((B, N), float("nan"), dtype=torch.float32, device=dev)
    norms = torch.full((B, N), float("nan"), dtype=torch.float32, device=dev)
    if query:
        ws = torch.empty((am.ctx.alsd_nbest_workspace_bytes(B, beam, Tp, max_target_len, nbest),), dtype=torch.uint8, device=dev)
    else:
        ws = torch.empty((am.ctx.alsd_workspace_bytes(B, min(max(beam, 1), 8), Tp, max_target_len, lm=True) + (1 << 22),), dtype=torch.uint8, device=dev)
    gof = None if graph_of is None else torch.as_tensor(np.asarray(graph_of), dtype=torch.int32).to(dev)
    ratio, abs_len = am.ctx._alsd_budget(max_target_len)
    flags = (capi.ALSD_SCORE_NORM if score_norm else 0) | (capi.ALSD_MERGE if merge else 0)
    try:
        am.ctx.check(am.ctx.lib.rs_rnnt_alsd_nbest(
            am.ctx._h, f.data_ptr(), lens.data_ptr(), B, Tp, int(beam), ratio, abs_len, flags, int(nbest), out_cap, ids.data_ptr(),
            steps.data_ptr(), n_ids.data_ptr(), scores.data_ptr(), norms.data_ptr(), n_hyps.data_ptr(),
            ctypes.byref(hw.struct) if hw is not None else None, gof.data_ptr() if gof is not None else None,
            ctypes.byref(lm.struct) if lm is not None else None, float(alpha), ws.data_ptr(), ws.numel() - short,
            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    finally:
        torch.cuda.synchronize()
        device_nbest.untouched = bool((n_ids.cpu() == FILL).all() and (n_hyps.cpu() == FILL).all())
    n, nh = n_ids.cpu().numpy(), n_hyps.cpu().numpy()
    sb, nb = scores.cpu().numpy().view(np.int32), norms.cpu().numpy().view(np.int32)
    hi, hs = ids.cpu().numpy(), steps.cpu().numpy()
    return [dict(entries=[(hi[b, r, :n[b, r]].tolist(), hs[b, r, :n[b, r]].tolist(), int(sb[b, r]), int(nb[b, r])) for r in range(nh[b])],
                 n_ids=n[b].tolist()) for b in range(B)]


def check(cfg, sd, am, f, lens, beam, nbest, lm=None, alpha=0.0, graphs=None, graph_of=None, **kw):
    """device == checker, bits; -> (device rows, checker rows)"""
    hw = _HotwordSet(graphs, am.device) if graphs else None
    ns = _NgramSet(lm, am.device) if lm is not None else None
    got = device_nbest(am, f, lens, beam, nbest, lm=ns, alpha=alpha, hw=hw, graph_of=graph_of if graphs else None, **kw)
    fa = f.cpu().numpy() if isinstance(f, torch.Tensor) else np.asarray(f)
    want = AN.nbest_checker(cfg, sd, fa, np.asarray(lens, np.int32), nbest, kh.concat(graphs) if graphs else None, graph_of if graphs else None,
                            lm=lm, alpha=alpha, beam=beam, **kw)
    for b, (g, w) in enumerate(zip(got, want)):
        assert g["n_ids"] == w["n_ids"] and len(g["entries"]) == len(w["entries"]), (beam, nbest, kw, b, g["n_ids"], w["n_ids"])
        assert g["entries"] == w["entries"], (beam, nbest, kw, b, g["entries"], w["entries"])
    return got, want


@pytest.fixture(scope="module")
def tiny(gpu_device):
    sd = synthetic_state_dict(TINY, 0)
    return AsrModel(TINY, sd, SyntheticTokenizer(TINY.vocab_size), device="cuda:0"), sd


@pytest.fixture(scope="module")
def toy(tiny):
    """a random projection [5][24][J] as tests/test_gpu_alsd.py builds one, the graphs and the LM cut from the plain search on it"""
    _, sd = tiny
    g = torch.Generator().manual_seed(6)
    f = torch.randn((5, 24, TINY.joint_hidden), generator=g) * (0.7 + 0.6 * torch.rand((5, 1, 1), generator=g))
    plain = AR.alsd_checker(TINY, sd, f.numpy(), np.asarray(LENS, np.int32), beam=4)
    graphs = [kh.build_graph(p) for p in AR.toy_graphs(plain)]
    lm = NL.build(NR.toy_lm(plain, TINY), TINY.vocab_size, TINY.blank_id)
    return f, graphs, lm


@pytest.mark.parametrize("beam,nbest", [(1, 1), (2, 1), (2, 2), (4, 1), (4, 2), (4, 4), (8, 1), (8, 2), (8, 8)])
def test_device_equals_checker_toy_geometry(tiny, toy, beam, nbest):
    model, sd = tiny
    f, graphs, lm = toy
    sizes = set()
    for form in (dict(), dict(graphs=graphs, graph_of=GRAPH_OF), dict(lm=lm, alpha=ALPHA), dict(lm=lm, alpha=ALPHA, graphs=graphs, graph_of=GRAPH_OF)):
        got, _ = check(TINY, sd, model, f, LENS, beam, nbest, **form)
        assert [e[0] for e in got[4]["entries"]] == [[]] and got[4]["entries"][0][2:] == (0, 0)      # no frames: the empty start hypothesis
        sizes |= {len(g["entries"]) for g in got}
    assert nbest in sizes
    check(TINY, sd, model, f, LENS, beam, nbest, merge=True, score_norm=False, max_target_len=7)
    check(TINY, sd, model, f, LENS, beam, nbest, max_target_len=0.5)                                  # the budget ends the search


def test_any_vocabulary_form(gpu_device):
    cfg = TINY.with_(vocab_size=3100)                                      # V + 1 above 64 x 48: the form that re-reads the row
    sd = synthetic_state_dict(cfg, 0)
    model = AsrModel(cfg, sd, SyntheticTokenizer(cfg.vocab_size), device="cuda:0")
    assert cfg.n_logits > 3072
    g = torch.Generator().manual_seed(5)
    f = torch.randn((3, 12, cfg.joint_hidden), generator=g) * 0.9
    got, _ = check(cfg, sd, model, f, [12, 1, 10], 4, 4, max_target_len=1.0)
    assert all(1 <= len(r["entries"]) <= 4 for r in got) and max(len(r["entries"]) for r in got) == 4
    check(cfg, sd, model, f, [12, 1, 10], 4, 2, max_target_len=1.0, score_norm=False, merge=True)


def test_619m_decoder_geometry(gpu_device):
    cfg = WIDE2
    sd = synthetic_state_dict(cfg, 0, blank_bias=6.5)
    model = AsrModel(cfg, sd, SyntheticTokenizer(cfg.vocab_size), device="cuda:0")
    assert (cfg.pred_hidden, cfg.joint_hidden, cfg.n_logits) == (640, 640, 3001)
    g = torch.Generator().manual_seed(15)
    f = torch.randn((2, 12, cfg.joint_hidden), generator=g) * (0.8 + 0.4 * torch.rand((2, 1, 1), generator=g))
    got, _ = check(cfg, sd, model, f, [12, 7], 4, 4, max_target_len=1.0)
    assert max(len(r["entries"]) for r in got) == 4
    plain = AR.alsd_checker(cfg, sd, f.numpy(), np.asarray([12, 7], np.int32), beam=4, max_target_len=1.0)
    seqs = [y for r in plain for y, *_ in r["beam"] + [(r["ids"], 0, 0)] if y]
    lm = NL.build(NR.random_lm(cfg, seqs, n_high=500, order=3), cfg.vocab_size, cfg.blank_id)
    seen = sorted({t for y in seqs for t in y})
    graph = kh.build_graph([((int(seen[0]),), 1.5)])
    check(cfg, sd, model, f, [12, 7], 8, 8, lm=lm, alpha=0.4, graphs=[graph], graph_of=[0, -1], max_target_len=1.0)


# ---- the hand-built edges: logits = the joint's bias alone, so every frame of every hypothesis offers the same distribution ----------
def flat_model(probs, blank):
    """a TINY model whose joint ignores its inputs (joint_net.2.weight = 0): labels 0..3 have probabilities probs, the blank `blank`"""
    sd = synthetic_state_dict(TINY, 7)
    bias = np.full((TINY.n_logits,), np.log(1e-9), np.float32)
    for v, p in enumerate(probs):
        bias[v] = np.float32(np.log(p))
    bias[TINY.blank_id] = np.float32(np.log(blank))
    sd["joint.joint_net.2.weight"] = torch.zeros_like(sd["joint.joint_net.2.weight"])
    sd["joint.joint_net.2.bias"] = torch.from_numpy(bias)
    return AsrModel(TINY, sd, SyntheticTokenizer(TINY.vocab_size), device="cuda:0"), sd


def test_the_hand_built_edges_on_the_device(gpu_device):
    f = torch.zeros((2, 2, TINY.joint_hidden))
    labels = lambda r: [e[0] for e in r["entries"]]               # noqa: E731
    # more finish than nbest, and every later one is better under the norm: the tail is evicted
    model, sd = flat_model([.8, .05, .03, .02], .1)
    got, want = check(TINY, sd, model, f, [1, 0], 2, 2, max_target_len=3)
    assert want[0]["evicted"] >= 2 and want[0]["offered"] > 2 and labels(got[0]) == [[0, 0, 0], [0, 0]]          # the edge is reached
    # fewer finish than nbest (one alignment step), and nothing finishes (two frames, no budget)
    model, sd = flat_model([.2, .15, .1, .05], .5)
    got, want = check(TINY, sd, model, f, [1, 0], 3, 3, max_target_len=0)
    assert want[0]["offered"] == 1 and labels(got[0]) == [[]] and got[0]["n_ids"] == [0, 0, 0]                     # the edge is reached
    model, sd = flat_model([.9, .05, .02, .02], .01)
    got, want = check(TINY, sd, model, f, [2, 2], 2, 2, max_target_len=0)
    assert want[0]["budget_exit"] == 1 and labels(got[0]) == [y for y, _ in want[0]["beam"]]                       # the edge is reached
    # equal sequences finishing in one step, merge off
    model, sd = flat_model([.45, .02, .02, .01], .5)
    got, want = check(TINY, sd, model, f, [2, 1], 4, 4, max_target_len=2, merge=False)
    assert want[0]["equal_met"] >= 1 and len({tuple(y) for y in labels(got[0])}) == len(got[0]["entries"])         # the edge is reached
    # an exact tie of norms across two steps
    model, sd = flat_model([.4, .1, .05, .05], .4)
    got, want = check(TINY, sd, model, f, [1, 0], 3, 3, max_target_len=2)
    assert want[0]["cross_step_ties"] >= 1 and labels(got[0])[:2] == [[], [0]] and got[0]["entries"][0][3] == got[0]["entries"][1][3]
    # a Finalize that reorders the list
    model, sd = flat_model([.25, .3, .02, .03], .4)
    graph = kh.build_graph([((0, 2), 1.0)])
    got, want = check(TINY, sd, model, f, [1, 0], 3, 3, max_target_len=1, score_norm=False, graphs=[graph], graph_of=[0, -1])
    assert want[0]["finalize_reorders"] == 1 and labels(got[0]) == [[], [1], [0]]                                  # the edge is reached


def test_alone_equals_inside_the_batch(tiny, toy):
    model, _ = tiny
    f, graphs, lm = toy
    hw, ns = _HotwordSet(graphs, model.device), _NgramSet(lm, model.device)
    together = device_nbest(model, f, LENS, 4, 4, lm=ns, alpha=ALPHA, hw=hw, graph_of=GRAPH_OF, max_target_len=24)
    for b in (0, 1, 2, 3):
        alone = device_nbest(model, f[b:b + 1, :LENS[b]], LENS[b:b + 1], 4, 4, lm=ns, alpha=ALPHA, hw=hw, graph_of=[GRAPH_OF[b]], max_target_len=24)
        assert alone[0] == together[b], b


def test_the_old_entries_return_what_they_returned(tiny, toy):
    model, sd = tiny
    f, graphs, lm = toy
    dev = model.device
    hw, ns = _HotwordSet(graphs, dev), _NgramSet(lm, dev)
    fa, la, table = f.numpy(), np.asarray(LENS, np.int32), kh.concat(graphs)
    B, Tp, _ = f.shape
    gof = torch.as_tensor(GRAPH_OF, dtype=torch.int32).to(dev)
    for beam in (2, 4, 8):
        cases = (("plain", {}, {}, AR.alsd_checker(TINY, sd, fa, la, beam=beam)),
                 ("hotwords", dict(hotwords=hw.struct, graph_of=gof), dict(hw=hw, graph_of=GRAPH_OF), AR.alsd_checker(TINY, sd, fa, la, table, GRAPH_OF, beam=beam)),
                 ("lm", dict(hotwords=hw.struct, graph_of=gof, lm=ns.struct, lm_alpha=ALPHA), dict(hw=hw, graph_of=GRAPH_OF, lm=ns, alpha=ALPHA),
                  AR.alsd_checker(TINY, sd, fa, la, table, GRAPH_OF, lm, ALPHA, beam=beam)))
        for name, old_kw, new_kw, want in cases:
            cap = 3 * Tp
            ids = torch.zeros((B, cap), dtype=torch.int32, device=dev)
            steps = torch.zeros_like(ids)
            n_ids, scores = torch.zeros((B,), dtype=torch.int32, device=dev), torch.zeros((B,), dtype=torch.float32, device=dev)
            ws = torch.empty((model.ctx.alsd_workspace_bytes(B, beam, Tp, 2.0, hotwords=name != "plain", lm=name == "lm"),), dtype=torch.uint8, device=dev)
            model.ctx.rnnt_alsd(f.to(dev), torch.as_tensor(LENS, dtype=torch.int32).to(dev), B, Tp, beam, 2.0, True, False, ids, steps, n_ids, scores, ws,
                                torch.cuda.current_stream().cuda_stream, **old_kw)
            torch.cuda.synchronize()
            n, sb = n_ids.cpu().numpy(), scores.cpu().numpy().view(np.int32)
            got = [(ids[b, :n[b]].cpu().tolist(), steps[b, :n[b]].cpu().tolist(), int(sb[b])) for b in range(B)]
            assert got == [(w["ids"], w["steps"], w["score_bits"]) for w in want], (beam, name)
            lists = device_nbest(model, f, LENS, beam, beam, **new_kw)
            for b in range(B):                                             # entry 0 of the list is the old entry's result
                assert lists[b]["entries"][0][:3] == got[b], (beam, name, b)


def test_through_load_model_and_the_transcribe_functions(gpu_device):
    off = load_model(device="cuda:0", config=TINY, decoding="alsd", beam_size=4)
    model = load_model(device="cuda:0", config=TINY, decoding="alsd", beam_size=4, nbest=3)
    assert (off.nbest, model.nbest) == (0, 3)
    audio, lens = synthetic_batch(6, 2.0, seed=50, ragged=True, min_seconds=0.5)
    audios = [interface.AudioData(audio[b, :lens[b]], 16000) for b in range(6)]
    conf = interface.TranscribeConfig(verbose=False)
    base = transcribe_batch(off, audios, conf)
    assert all(type(r) is interface.TranscribeResult for r in base)         # off: today's objects
    res = transcribe_batch(model, audios, conf)
    for r, b in zip(res, base):
        assert type(r) is interface.NBestTranscribeResult and (r.text, r.subwords, r.segments) == (b.text, b.subwords, b.segments)
        assert 1 <= len(r.nbest) <= 3 and (r.nbest[0].text, r.nbest[0].subwords, r.nbest[0].score) == (r.text, r.subwords, r.score)
        norms = [e.norm_score for e in r.nbest]
        assert norms == sorted(norms, reverse=True) and r.token_logprobs is None and r.hypothesis is None
        assert len({tuple(s.token_id for s in e.subwords) for e in r.nbest}) <= len(r.nbest)
    assert max(len(r.nbest) for r in res) == 3
    one = transcribe(model, audios[2], conf)
    assert [(e.text, e.score) for e in one.nbest] == [(e.text, e.score) for e in res[2].nbest]
    assert type(transcribe(model, audios[2], conf, nbest=0)) is interface.TranscribeResult
    assert [(e.text, e.score) for e in transcribe(off, audios[2], conf, nbest=2).nbest] == [(e.text, e.score) for e in res[2].nbest[:2]]
    raw = transcribe(model, audios[2], interface.TranscribeConfig(verbose=False, raw_hypothesis=True))
    hyps = raw.hypothesis.n_best_hypotheses
    assert len(hyps) == len(raw.nbest) and [h.score for h in hyps] == [e.score for e in raw.nbest] and raw.nbest[0].hypothesis is hyps[0]
    # the runtime's lists are the checker's on the device's projection
    am = model
    waves = [np.asarray(a.waveform, np.float32) for a in audios]
    buf = am.stage(waves, buf=am.new_buffers(6, max(len(w) for w in waves)))
    am.run_device(buf)
    torch.cuda.synchronize()
    got = am.collect(buf)
    want = AN.nbest_checker(TINY, synthetic_state_dict(TINY, 0), buf.joint_enc.cpu().numpy(), np.asarray(got.enc_lens, np.int32), 3, beam=4,
                            max_target_len=TINY.alsd_max_target_len)
    for b in range(6):
        assert [(y, [fr + k for k, fr in enumerate(frs)], AN.bits(s), AN.bits(n)) for y, frs, s, n in got.nbest[b]] == want[b]["entries"], b
    whole, parts = am.transcribe_waveforms(waves), am.transcribe_waveforms(waves, max_batch=4)
    assert whole.nbest == got.nbest == parts.nbest
    # token scores ride on entry 0
    model.token_scores = off.token_scores = True
    scored, ref = transcribe_batch(model, audios, conf), transcribe_batch(off, audios, conf)
    for r, b in zip(scored, ref):
        assert r.token_logprobs == b.token_logprobs and r.nbest[0].token_logprobs == b.token_logprobs and r.confidence == b.confidence
        assert all(e.token_logprobs is None for e in r.nbest[1:])
    with pytest.raises(ValueError, match="above the beam"):
        transcribe(model, audios[0], conf, nbest=5)
    greedy = load_model(device="cuda:0", config=TINY)
    with pytest.raises(ValueError, match="needs a beam search"):
        transcribe(greedy, audios[0], conf, nbest=2)


def test_errors(tiny, toy):
    model, _ = tiny
    f, graphs, lm = toy
    ns = _NgramSet(lm, model.device)
    for beam, nbest, pattern in ((4, 0, "nbest must be 1..8"), (8, 9, "nbest must be 1..8"), (4, -1, "nbest must be 1..8"),
                                 (4, 5, "above the beam"), (2, 3, "above the beam")):
        with pytest.raises(capi.RsError, match=pattern) as e:
            device_nbest(model, f, LENS, beam, nbest, query=False)
        assert e.value.code == capi.RS_EINVAL and device_nbest.untouched, (beam, nbest)
    with pytest.raises(capi.RsError, match="lm_alpha") as e:
        device_nbest(model, f, LENS, 4, 2, lm=ns, alpha=float("nan"))
    assert e.value.code == capi.RS_EINVAL and device_nbest.untouched
    for args in ((4, 0), (4, 5), (0, 1), (8, 9)):
        with pytest.raises(RuntimeError):
            model.ctx.alsd_nbest_workspace_bytes(5, args[0], 24, 2.0, args[1])
    with pytest.raises(capi.RsError, match="workspace") as e:
        device_nbest(model, f, LENS, 4, 4, lm=ns, alpha=ALPHA, short=1)
    assert e.value.code == RS_EWORKSPACE
    with pytest.raises(capi.RsError, match="out_cap") as e:
        device_nbest(model, f, LENS, 4, 4, out_cap=1)
    assert e.value.code == capi.RS_EOVERFLOW
    assert device_nbest(model, f, LENS, 2, 2)                              # and the context is usable afterwards
    k2 = K2Model(ZIPFORMER_TINY, synthetic_state_dict_k2(ZIPFORMER_TINY, 0), synthetic_tokens(ZIPFORMER_TINY.vocab_size, 0), device="cuda:0")
    with pytest.raises(RuntimeError):
        k2.am.ctx.alsd_nbest_workspace_bytes(2, 4, 10, 2.0, 2)
    dev = k2.am.device
    z = lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)          # noqa: E731
    zf = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)       # noqa: E731
    with pytest.raises(capi.RsError, match="rs_rnnt_alsd_nbest: not defined for a Zipformer context") as e:
        k2.am.ctx.rnnt_alsd_nbest(zf(2, 10, ZIPFORMER_TINY.joiner_dim), z(2) + 10, 2, 10, 4, 2.0, True, False, 2, z(2, 2, 30), z(2, 2, 30), z(2, 2),
                                  zf(2, 2), zf(2, 2), z(2), torch.empty((1 << 20,), dtype=torch.uint8, device=dev), 0)
    assert e.value.code == capi.RS_EINVAL
