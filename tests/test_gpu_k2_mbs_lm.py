"""-m gpu: n-gram LM shallow fusion in the modified beam search on the device (rs_rnnt_mbs_lm, csrc/k_rnnt_mbs.hip) against its C
checker (tests/k2_mbs_lm_checker.c): ids, frames and the float32 score of every utterance BIT FOR BIT, given the device's own
joiner.encoder_proj output.

  toy geometry (V = 97)      the <4> form: K = 1, 2, 4, 8; 7 ragged utterances with a zero-frame row; blank_penalty 1.5 and no length
                             normalisation once each; the LM alone, and the LM with graphs A / B / C / none spread over the rows
                             (tests/k2_hotwords_ref.py toy_graphs).  The LM is tests/k2_mbs_lm_ref.py toy_lm, order 3, cut from the
                             plain search's final sets; the checker's counters show that higher-order hits, backoffs, unknown tokens
                             and full-order pops were all met, and at K >= 2 the LM changes a result
  159M decoder geometry      the <42> form: V = 10 720, J = D = 512, B = 5, Tp = 30, K = 4; an order-4 LM with every unigram and a few
                             thousand random higher-order n-grams (long child lists: the bisection)
  any-V form                 the <0> form: V = 10 753 (the first above 256 x 42), B = 3, Tp = 12, K = 4, an order-2 LM
  no model                   lm = None, an empty table, alpha = 0: rs_rnnt_mbs_hotwords, and without graphs rs_rnnt_mbs, bits
  batch invariance           an utterance alone with LM + graph == the same utterance inside the ragged batch
  the public surface         K2Model(ngram_lm_model=path): transcribe == transcribe_batch row, ngram_lm_alpha = 0 == no LM, the
                             settable weight, 9 utterances at max_batch = 4 == one batch, token scores stay the model's own
  errors                     RS_EINVAL on a nemo context and, before any launch, for a bad alpha or table; RS_EWORKSPACE
"""
import ctypes
import importlib
import types

import numpy as np
import pytest
import torch

import k2_hotwords_ref as H
import k2_mbs_lm_ref as LR
import k2_mbs_ref as R
import ngram_lm_ref as NR
import token_scores_ref as TS
from ngram_lm_ref import BOS
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
TOY_ALPHA = 0.5
GRAPH_OF = [0, 1, -1, 2, -1, 1, 0]            # graphs A, B, C and "none" over the seven rows (row 2 has no frames)
RS_EWORKSPACE = -3


def build(cfg, seed, sd=None, **kw):
    sd = sd if sd is not None else synthetic_state_dict_k2(cfg, seed)
    return K2Model(cfg, sd, synthetic_tokens(cfg.vocab_size, seed), device="cuda:0", **kw), sd


def ragged_waves(n, seconds, seed, min_seconds):
    audio, lens = synthetic_batch(n, seconds, seed=seed, ragged=True, min_seconds=min_seconds)
    return [np.pad(audio[b, :lens[b]], PAD) for b in range(n)]


def device_search(am, f, lens, K, lm=None, alpha=0.0, hw=None, graph_of=None, blank_penalty=0.0, length_norm=True, entry="lm", short=0):
    """rs_rnnt_mbs_lm (or, by `entry`, rs_rnnt_mbs_hotwords / rs_rnnt_mbs) on a projection f [B][Tp][J] -> list of (ids, frames,
    score bits); `short`: bytes withheld from the workspace"""
    dev = am.device
    B, Tp, _ = f.shape
    out_cap = max(Tp, 1)
    f = f.to(dev).contiguous()
    lens = torch.as_tensor(np.asarray(lens), dtype=torch.int32).to(dev)
    ids = torch.zeros((B, out_cap), dtype=torch.int32, device=dev)
    frames = torch.zeros_like(ids)
    n_ids = torch.full((B,), -1, dtype=torch.int32, device=dev)
    scores = torch.full((B,), float("nan"), dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    gof = None if graph_of is None else torch.as_tensor(np.asarray(graph_of), dtype=torch.int32).to(dev)
    hot = dict(hotwords=hw.struct if hw is not None else None, graph_of=gof)
    if entry == "plain":
        ws = torch.empty((am.ctx.mbs_workspace_bytes(B, K, Tp, out_cap),), dtype=torch.uint8, device=dev)
        am.ctx.rnnt_mbs(f, lens, B, Tp, K, blank_penalty, length_norm, ids, frames, n_ids, scores, ws, stream)
    elif entry == "hotwords":
        ws = torch.empty((am.ctx.mbs_workspace_bytes(B, K, Tp, out_cap, hotwords=True),), dtype=torch.uint8, device=dev)
        am.ctx.rnnt_mbs(f, lens, B, Tp, K, blank_penalty, length_norm, ids, frames, n_ids, scores, ws, stream, **hot)
    else:
        ws = torch.empty((am.ctx.mbs_workspace_bytes(B, K, Tp, out_cap, lm=True),), dtype=torch.uint8, device=dev)
        head = (am.ctx._h, f.data_ptr(), lens.data_ptr(), B, Tp, int(K), float(blank_penalty), capi.MBS_LENGTH_NORM if length_norm else 0,
                out_cap, ids.data_ptr(), frames.data_ptr(), n_ids.data_ptr(), scores.data_ptr())
        # straight to rs_rnnt_mbs_lm, also with lm = None and alpha = 0 (Context.rnnt_mbs would pick a narrower entry)
        am.ctx.check(am.ctx.lib.rs_rnnt_mbs_lm(*head, ctypes.byref(hw.struct) if hw is not None else None, gof.data_ptr() if gof is not None else None,
                                               ctypes.byref(lm.struct) if lm is not None else None, float(alpha), ws.data_ptr(),
                                               ws.numel() - short, ctypes.c_void_p(stream)))
    torch.cuda.synchronize()
    n = n_ids.cpu().numpy()
    if (n < 0).any():                                                      # nothing ran: the outputs keep their fill
        return None
    bits = scores.cpu().numpy().view(np.int32)
    return [(ids[b, :n[b]].cpu().tolist(), frames[b, :n[b]].cpu().tolist(), int(bits[b])) for b in range(B)]


def check(cfg, sd, am, f, lens, lm, alpha, graphs=None, graph_of=None, **kw):
    """device == checker, bits; -> (device rows, checker rows)"""
    hw = _HotwordSet(graphs, am.device) if graphs else None
    got = device_search(am, f, lens, lm=_NgramSet(lm, am.device), alpha=alpha, hw=hw, graph_of=graph_of if graphs else None, **kw)
    want = LR.mbs_lm_checker(cfg, sd, f.cpu().numpy(), np.asarray(lens, np.int32), kh.concat(graphs) if graphs else None,
                             graph_of if graphs else None, lm=lm, alpha=alpha, **kw)
    for b, (g, w) in enumerate(zip(got, want)):
        assert g[0] == w["ids"] and g[1] == w["frames"], (kw, b, g[:2], w["ids"], w["frames"])
        assert g[2] == w["score_bits"], (kw, b, g[2], w["score_bits"], w["score"])
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
    """the device's own projection of seven ragged utterances, the plain search's results on it (checker, K = 4), the graphs and the LM"""
    model, sd = tiny
    f, lens = encoder_projection(model, ragged_waves(7, 3.0, 5, 0.7))
    lens[2] = 0
    plain = R.mbs_checker(ZIPFORMER_TINY, sd, f.cpu().numpy(), np.asarray(lens, np.int32), K=4)
    graphs = [kh.build_graph(p) for p in H.toy_graphs(plain)]
    lm = NL.build(LR.toy_lm(plain, ZIPFORMER_TINY), ZIPFORMER_TINY.vocab_size, ZIPFORMER_TINY.blank_id)
    assert lm.order == 3 and lm.start != 0
    return f, lens, graphs, lm


@pytest.mark.parametrize("K,kw", [(1, {}), (2, {}), (4, {}), (8, {}), (4, dict(blank_penalty=1.5)), (4, dict(length_norm=False))])
def test_device_equals_checker_toy_geometry(tiny, toy, K, kw):
    model, sd = tiny
    f, lens, graphs, lm = toy
    plain = device_search(model.am, f, lens, K=K, entry="plain", **kw)
    for with_graphs in (False, True):
        got, want = check(ZIPFORMER_TINY, sd, model.am, f, lens, lm, TOY_ALPHA, graphs if with_graphs else None, GRAPH_OF, K=K, **kw)
        assert got[2] == ([], [], 0)                                      # no frames: no tokens, log_prob 0
        t = LR.totals(want, lm.order)
        differ = [b for b in range(len(lens)) if got[b][0] != plain[b][0]]
        print(f"K = {K} {kw} graphs {with_graphs}: {t}, hotword child hits {sum(w['child_hits'] for w in want)}, rows whose ids differ "
              f"from the search without the LM {differ}")
        if not kw:
            assert LR.all_counted(t), LR.RECHOOSE
        if with_graphs and not kw:
            assert sum(w["child_hits"] for w in want) > 0, LR.RECHOOSE
        if K >= 2:
            assert differ, LR.RECHOOSE


def test_159m_decoder_geometry_long_child_lists(gpu_device):
    cfg = ZIPFORMER_TINY.with_(vocab_size=10720, decoder_dim=512, joiner_dim=512).validate()
    model, sd = build(cfg, 0)
    g = torch.Generator().manual_seed(2)
    B, Tp = 5, 30
    f = torch.randn((B, Tp, cfg.joiner_dim), generator=g) * (0.8 + 0.4 * torch.rand((B, 1, 1), generator=g))
    lens = [30, 17, 0, 25, 9]
    plain = R.mbs_checker(cfg, sd, f.numpy(), np.asarray(lens, np.int32), K=4)
    seqs = [y for r in plain for y, _ in r["final"] if y]                  # what the plain search proposes
    assert seqs, "the fixture must emit tokens"
    lm = NL.build(LR.random_lm(cfg, seqs, n_high=3000, order=4, seed=4), cfg.vocab_size, cfg.blank_id)
    longest = int(np.diff(lm.arrays["child_begin"])[1:].max())
    assert lm.order == 4 and 256 * 4 < cfg.vocab_size <= 256 * 42 and longest >= 16
    got, want = check(cfg, sd, model.am, f, lens, lm, 0.3, K=4)
    t = LR.totals(want, 4)
    print("159M decoder geometry:", t, "longest child list below the root", longest)
    assert sum(t["hits"][1:]) > 0, LR.RECHOOSE
    # ... and with a graph over the same tokens
    graph = kh.build_graph([(tuple(y[:2]), 2.0) for y in seqs if len(y) >= 2][:50] or [((seqs[0][0],), 2.0)])
    check(cfg, sd, model.am, f, lens, lm, 0.3, [graph], [0, 0, 0, -1, 0], K=4)


def test_any_vocabulary_form(gpu_device):
    cfg = ZIPFORMER_TINY.with_(vocab_size=256 * 42 + 1).validate()          # the first vocabulary the <42> form does not take
    model, sd = build(cfg, 0)
    g = torch.Generator().manual_seed(5)
    B, Tp = 3, 12
    f = torch.randn((B, Tp, cfg.joiner_dim), generator=g) * 0.9
    lens = [12, 7, 10]
    plain = R.mbs_checker(cfg, sd, f.numpy(), np.asarray(lens, np.int32), K=4)
    seqs = [y for r in plain for y, _ in r["final"] if y]
    assert seqs, "the fixture must emit tokens"
    lm = NL.build(LR.random_lm(cfg, seqs, n_high=500, order=2, seed=9), cfg.vocab_size, cfg.blank_id)
    got, want = check(cfg, sd, model.am, f, lens, lm, 0.6, K=4)
    print("any-V form:", LR.totals(want, 2))
    assert LR.totals(want, 2)["walks"] > 0


def test_no_model_is_the_search_without_one(tiny, toy):
    model, _ = tiny
    am = model.am
    f, lens, graphs, lm = toy
    hw, ns = _HotwordSet(graphs, am.device), _NgramSet(lm, am.device)
    empty = types.SimpleNamespace(struct=capi.RsNgram())                   # n_nodes == 0
    for K in (2, 4):
        plain = device_search(am, f, lens, K, entry="plain")
        hot = device_search(am, f, lens, K, hw=hw, graph_of=GRAPH_OF, entry="hotwords")
        assert hot != plain
        assert device_search(am, f, lens, K, lm=None, alpha=0.5) == plain                               # a null table, no graphs: rs_rnnt_mbs
        assert device_search(am, f, lens, K, lm=ns, alpha=0.0) == plain                                 # alpha 0
        assert device_search(am, f, lens, K, lm=empty, alpha=0.5) == plain
        assert device_search(am, f, lens, K, lm=None, alpha=0.5, hw=hw, graph_of=GRAPH_OF) == hot       # ... with graphs: rs_rnnt_mbs_hotwords
        assert device_search(am, f, lens, K, lm=ns, alpha=0.0, hw=hw, graph_of=GRAPH_OF) == hot
        with_lm = device_search(am, f, lens, K, lm=ns, alpha=TOY_ALPHA)
        assert with_lm != plain
        assert device_search(am, f, lens, K, lm=ns, alpha=TOY_ALPHA, hw=hw, graph_of=[-1] * 7) == with_lm


def test_alone_equals_inside_a_ragged_batch(tiny, toy):
    model, _ = tiny
    am = model.am
    f, lens, graphs, lm = toy
    hw, ns = _HotwordSet(graphs, am.device), _NgramSet(lm, am.device)
    together = device_search(am, f, lens, 4, lm=ns, alpha=TOY_ALPHA, hw=hw, graph_of=GRAPH_OF)
    for b in (0, 1, 3, 4):
        alone = device_search(am, f[b:b + 1, :lens[b]], lens[b:b + 1], 4, lm=ns, alpha=TOY_ALPHA, hw=hw, graph_of=[GRAPH_OF[b]])
        assert alone[0] == together[b], b


def test_through_k2model_and_the_transcribe_functions(tiny, tmp_path):
    cfg = ZIPFORMER_TINY
    _, sd = tiny
    mbs = dict(decoding_method="modified_beam_search")
    plain_model, _ = build(cfg, 3, sd=sd, **mbs)
    assert plain_model.ngram_lm is None and plain_model.ngram_lm_alpha == 0.0
    audio, lens = synthetic_batch(9, 2.0, seed=50, ragged=True, min_seconds=0.5)
    audios = [interface.AudioData(audio[b, :lens[b]], 16000) for b in range(9)]
    conf = interface.TranscribeConfig(verbose=False)
    base = k2tr.transcribe_batch(plain_model, audios, conf)
    waves = [np.pad(a.waveform, PAD) for a in audios]
    dec = plain_model.am.transcribe_waveforms(waves)
    # an LM file in the pieces of tokens.txt, cut from what the plain search says: it dislikes the most frequent token and likes the rest
    flat = [t for ids in dec.ids for t in ids]
    top = max(set(flat), key=flat.count)
    ent = {(t,): ((-4.0 if t == top else -0.5), -0.25) for t in range(cfg.vocab_size) if t not in (cfg.blank_id, cfg.unk_id)}
    ent[(BOS,)] = (-99.0, -0.125)
    for ids in dec.ids:
        for a, b in zip(ids, ids[1:]):
            if top not in (a, b):
                ent[(a, b)] = (-0.125, 0.0)
    tokens = synthetic_tokens(cfg.vocab_size, 3)
    path = NR.write_arpa(str(tmp_path / "lm.arpa"), ent, "pieces", pieces=tokens)
    model, _ = build(cfg, 3, sd=sd, ngram_lm_model=path, ngram_lm_alpha=0.6, **mbs)
    assert model.ngram_lm.key == NL.build(ent, cfg.vocab_size, cfg.blank_id).key and model.ngram_lm_alpha == 0.6
    assert list(model.am._lm_sets) == [model.ngram_lm.key]                # uploaded once, at load
    res = k2tr.transcribe_batch(model, audios, conf)
    text = lambda rs: [r.text for r in rs]                                 # noqa: E731
    assert text(res) != text(base), "the LM must change a transcript: re-choose the model"
    for b in (0, 4):                                                       # transcribe == the transcribe_batch row
        one = k2tr.transcribe(model, audios[b], conf)
        assert one.text == res[b].text and [s.seconds for s in one.subwords] == [s.seconds for s in res[b].subwords]
    # per call: alpha 0 = without the LM; another alpha = the runtime at that weight; the model's value is settable
    assert [k2tr.transcribe(model, audios[b], conf, ngram_lm_alpha=0).text for b in (0, 3, 4)] == [base[b].text for b in (0, 3, 4)]
    other = model.am.transcribe_waveforms(waves, ngram_lm=(model.ngram_lm, 1.5))
    assert k2tr.transcribe(model, audios[3], conf, ngram_lm_alpha=1.5).text == "".join(model.symbol(i) for i in other.ids[3])
    model.ngram_lm_alpha = 0.0
    assert text(k2tr.transcribe_batch(model, audios, conf)) == text(base)
    model.ngram_lm_alpha = 0.6
    assert list(model.am._lm_sets) == [model.ngram_lm.key]                # still the one upload
    with pytest.raises(ValueError, match="no n-gram LM"):
        k2tr.transcribe(plain_model, audios[0], conf, ngram_lm_alpha=0.3)
    with pytest.raises(ValueError, match="finite number"):
        model.ngram_lm_alpha = -1.0
    # the runtime's results are the checker's on the device's projection; token scores stay the model's own distribution
    am = model.am
    buf = am.stage(waves, buf=am.new_buffers(9, max(len(w) for w in waves)))
    am.token_scores = True
    am.run_device(buf)
    torch.cuda.synchronize()
    got = am.collect(buf)
    am.token_scores = False
    want = LR.mbs_lm_checker(cfg, sd, buf.joint_enc.cpu().numpy(), np.asarray(got.enc_lens, np.int32), lm=model.ngram_lm, alpha=0.6, K=4)
    assert got.ids == [w["ids"] for w in want] and got.frames == [w["frames"] for w in want]
    assert [np.float32(s) for s in got.scores] == [np.float32(w["score"]) for w in want]
    assert ["".join(model.symbol(i) for i in ids) for ids in got.ids] == text(res) and got.ids != dec.ids
    u_cap = max(1, max(len(y) for y in got.ids))
    ids_m, n_m = TS.pack(got.ids, u_cap)
    logp, _ = TS.scores_checker(cfg, sd, buf.joint_enc.cpu().numpy(), np.asarray(got.enc_lens, np.int32), ids_m, TS.pack(got.frames, u_cap)[0], n_m)
    fbits = lambda v: int(np.asarray([v], np.float32).view(np.int32)[0])   # noqa: E731
    assert [[fbits(v) for v in lp] for lp in got.token_logprobs] == [[fbits(v) for v in logp[b, :n_m[b]]] for b in range(9)]
    # hotwords and the LM in one call, through the host pipeline (max_batch < n): the same rows as one batch
    graphs = [kh.build_graph([((top,), 4.0)]) if b % 2 else None for b in range(9)]
    whole = am.transcribe_waveforms(waves, hotwords=graphs)
    parts = am.transcribe_waveforms(waves, max_batch=4, hotwords=graphs)
    assert (whole.ids, whole.frames, whole.scores) == (parts.ids, parts.frames, parts.scores) and whole.ids != got.ids
    no_graphs = am.transcribe_waveforms(waves, max_batch=4)
    assert (no_graphs.ids, no_graphs.frames) == (got.ids, got.frames)


def test_errors(tiny, toy):
    model, _ = tiny
    am = model.am
    f, lens, graphs, lm = toy
    ns = _NgramSet(lm, am.device)
    nemo = AsrModel(TINY, synthetic_state_dict(TINY, 0), SyntheticTokenizer(TINY.vocab_size), device="cuda:0")
    with pytest.raises(RuntimeError):
        nemo.ctx.mbs_workspace_bytes(2, 4, 10, 10, lm=True)
    dev = nemo.device
    z = lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)          # noqa: E731
    with pytest.raises(capi.RsError, match="Zipformer") as e:
        nemo.ctx.rnnt_mbs(torch.zeros((2, 10, TINY.joint_hidden), device=dev), z(2) + 10, 2, 10, 4, 0.0, True, z(2, 10), z(2, 10),
                          z(2), torch.zeros((2,), device=dev), torch.empty((1 << 20,), dtype=torch.uint8, device=dev), 0, lm=ns.struct, lm_alpha=0.5)
    assert e.value.code == capi.RS_EINVAL

    def broken(**fields):
        t = capi.RsNgram.from_buffer_copy(ns.struct)
        for k, v in fields.items():
            setattr(t, k, v)
        return types.SimpleNamespace(struct=t)
    # refused from the argument list, before anything is enqueued
    for bad, alpha, pattern in ((ns, float("nan"), "lm_alpha"), (ns, float("inf"), "lm_alpha"), (ns, -0.5, "lm_alpha"),
                                (broken(n_children=-1), 0.5, "negative count"), (broken(n_logits=ZIPFORMER_TINY.vocab_size + 1), 0.5, "logits"),
                                (broken(order=0), 0.5, "order"), (broken(order=9), 0.5, "order"), (broken(start=lm.n_nodes), 0.5, "start"),
                                (broken(logp=None), 0.5, "null array")):
        with pytest.raises(capi.RsError, match=pattern) as e:
            device_search(am, f, lens, 4, lm=bad, alpha=alpha)
        assert e.value.code == capi.RS_EINVAL
    with pytest.raises(capi.RsError, match="workspace") as e:
        device_search(am, f, lens, 4, lm=ns, alpha=0.5, short=1)
    assert e.value.code == RS_EWORKSPACE
    with pytest.raises(capi.RsError) as e:                                 # what rs_rnnt_mbs rejects
        device_search(am, f, lens, 8, lm=ns, alpha=0.5, blank_penalty=-1.0)
    assert e.value.code == capi.RS_EINVAL
    with pytest.raises(ValueError, match="modified_beam_search"):         # the greedy model refuses an LM at every entrance
        am.lm_plan((lm, 0.5))
    with pytest.raises(ValueError, match="modified_beam_search"):
        model.ngram_lm = lm
