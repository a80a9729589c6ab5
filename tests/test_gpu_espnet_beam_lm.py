"""-m gpu: hotwords and n-gram LM fusion in ESPnet's default beam search on the device (rs_rnnt_beam_lm, csrc/k_rnnt_beam.hip) against
its C checker (tests/espnet_beam_lm_checker.c): ids, frames, n_ids, scores, norm_scores, n_hyps and the pop count of every utterance
BIT FOR BIT, given the same joint-encoder projection.

  toy geometry               ESPNET_TINY, B = 7, ragged lengths 24, 17, 1, 9, 0, 20 and 13 frames (tests/espnet_beam_lm_ref.py toy: the
                             projection, graphs and LM the host tests search); graphs A, B, C and "none" mixed over the rows; beam 1, 2,
                             4, 8 x nbest 0, 1, 2, beam; score norm on and off; the LM alone, the graphs alone, both; frames = NULL
  beam 20, a large vocabulary  one case at beam 20 with max_pops 640 (extensions across two waves, the LDS bound), one with V = 1061 (the
                             record kernel's other variant feeds the step kernel)
  the hand-built edges       tests/espnet_beam_lm_ref.py EDGES on a joint that is its bias alone: device == checker, and the overflow
  no model                   rs_rnnt_beam_lm with NULL tables, an empty table, alpha = 0: rs_rnnt_beam / rs_rnnt_beam_nbest bit for bit,
                             pops included
  batch invariance           a row alone with its own graph == the row inside the ragged batch
  the public surface         EspnetModel(beam_size=6, ngram_lm_model=path, hotwords_file=path); model(speech, hotwords=);
                             recognize_batch(hotwords=[...], nbest=3); transcribe / transcribe_batch with segmentation="device";
                             ngram_lm_alpha=0 per call; the setter; token scores stay the model's own; the overflow ladder ending in
                             `degraded`
  errors                     every RS_EINVAL of include/rs_asr.h leaves the outputs untouched; RS_EWORKSPACE; RS_EOVERFLOW
Without the feature these fail at symbol lookup."""
import ctypes
import importlib
import types
import warnings

import numpy as np
import pytest
import torch

import espnet_beam_lm_ref as BL
import k2_mbs_lm_ref as LR
import ngram_lm_ref as NR
import token_scores_ref as TS
from ngram_lm_ref import BOS
from reazonspeech_amd.espnet.asr import interface
from reazonspeech_amd.espnet.asr.model import EspnetModel, synthetic_token_list
from reazonspeech_amd.k2.asr.model import K2Model, synthetic_tokens
from reazonspeech_amd.runtime import capi, k2_hotwords as kh, ngram_lm as NL
from reazonspeech_amd.runtime.config import ESPNET_TINY
from reazonspeech_amd.runtime.k2_config import ZIPFORMER_TINY
from reazonspeech_amd.runtime.k2_weights import synthetic_state_dict_k2
from reazonspeech_amd.runtime.model import _HotwordSet, _NgramSet
from reazonspeech_amd.runtime.synth import synthetic_batch
from reazonspeech_amd.runtime.weights_espnet import synthetic_state_dict_espnet

tr = importlib.import_module("reazonspeech_amd.espnet.asr.transcribe")

pytestmark = pytest.mark.gpu
RS_EWORKSPACE = -3
FILL = -7
GRAPH_OF = BL.TOY_GRAPH_OF
ALPHA = BL.TOY_ALPHA


def build(cfg, sd, seed=0, **kw):
    return EspnetModel(cfg, sd, synthetic_token_list(cfg.vocab_size, seed), device="cuda:0", **kw)


def device_search(am, f, lens, beam, nbest=0, score_norm=True, max_pops=0, out_cap=None, hw=None, graph_of=None, lm=None, alpha=0.0,
                  entry="lm", short=0, with_frames=True):
    """rs_rnnt_beam_lm (or, by `entry`, rs_rnnt_beam / rs_rnnt_beam_nbest through the wrapper) on a projection f [B][Tp][J] -> per
    utterance dict(entries=[(ids, frames, score bits, norm bits or None)], n_ids, pops); nbest = 0: the one result as a list of one.
    `short`: bytes withheld from the workspace.  `device_search.untouched`: the outputs still hold their fill."""
    dev = am.device
    f = torch.as_tensor(f)
    B, Tp, _ = f.shape
    out_cap = out_cap or (2 * Tp + 16)
    N = max(int(nbest), 1)
    f = f.to(dev).contiguous()
    lens = torch.as_tensor(np.asarray(lens), dtype=torch.int32).to(dev)
    shape = (B, N, out_cap) if nbest else (B, out_cap)
    ids = torch.zeros(shape, dtype=torch.int32, device=dev)
    frames = torch.zeros_like(ids)
    n_ids = torch.full((B, N), FILL, dtype=torch.int32, device=dev)
    n_hyps = torch.full((B,), FILL, dtype=torch.int32, device=dev)
    pops = torch.full((B,), FILL, dtype=torch.int32, device=dev)
    scores = torch.full((B, N), float("nan"), dtype=torch.float32, device=dev)
    norms = torch.full((B, N), float("nan"), dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    gof = None if graph_of is None else torch.as_tensor(np.asarray(graph_of), dtype=torch.int32).to(dev)
    try:
        if entry == "lm":
            # straight to rs_rnnt_beam_lm, also with NULL tables and alpha = 0 (Context.rnnt_beam would pick a narrower entry)
            ws = torch.empty((am.ctx.beam_workspace_bytes(B, max(beam, 1), Tp, max_pops, hotwords=True, lm=True, nbest=max(0, min(nbest, 8, beam))),),
                             dtype=torch.uint8, device=dev)
            am.ctx.check(am.ctx.lib.rs_rnnt_beam_lm(
                am.ctx._h, f.data_ptr(), lens.data_ptr(), B, Tp, int(beam), 1 if score_norm else 0, int(max_pops), int(nbest), out_cap,
                ids.data_ptr(), frames.data_ptr() if with_frames else None, n_ids.data_ptr(), scores.data_ptr(),
                norms.data_ptr() if nbest else None, n_hyps.data_ptr() if nbest else None, pops.data_ptr(),
                ctypes.byref(hw.struct) if hw is not None else None, gof.data_ptr() if gof is not None else None,
                ctypes.byref(lm.struct) if lm is not None else None, ctypes.c_float(alpha), ws.data_ptr(), ws.numel() - short, ctypes.c_void_p(stream)))
        elif nbest:
            ws = torch.empty((am.ctx.beam_nbest_workspace_bytes(B, beam, Tp, max_pops, nbest),), dtype=torch.uint8, device=dev)
            am.ctx.rnnt_beam_nbest(f, lens, B, Tp, beam, score_norm, max_pops, nbest, ids, n_ids, scores, norms, n_hyps, pops, ws, stream, frames=frames)
        else:
            ws = torch.empty((am.ctx.beam_workspace_bytes(B, beam, Tp, max_pops),), dtype=torch.uint8, device=dev)
            am.ctx.rnnt_beam(f, lens, B, Tp, beam, score_norm, max_pops, ids, n_ids.view(-1), scores.view(-1), pops, ws, stream, frames=frames)
    finally:
        torch.cuda.synchronize()
        device_search.untouched = bool((n_ids.cpu() == FILL).all() and (n_hyps.cpu() == FILL).all() and (pops.cpu() == FILL).all()
                                       and bool(torch.isnan(scores).all()) and int(ids.abs().sum()) == 0)
    n, hp = n_ids.cpu().numpy(), pops.cpu().numpy()
    nh = n_hyps.cpu().numpy() if nbest else np.ones((B,), np.int32)
    sb, nb = scores.cpu().numpy().view(np.int32), norms.cpu().numpy().view(np.int32)
    hi, hf = ids.cpu().numpy().reshape(B, N, out_cap), frames.cpu().numpy().reshape(B, N, out_cap)
    return [dict(entries=[(hi[b, r, :n[b, r]].tolist(), hf[b, r, :n[b, r]].tolist() if with_frames else None, int(sb[b, r]),
                           int(nb[b, r]) if nbest else None) for r in range(nh[b])],
                 n_ids=n[b].tolist(), pops=int(hp[b])) for b in range(B)]


def expect(want, nbest):
    """what the device must return for `nbest`, from the checker's rows at nbest = min(beam, 8): a shorter list is its prefix, and
    nbest = 0 is entry 0 without the norm (tests/test_espnet_beam_lm_host.py holds the checker to both)"""
    out = []
    for w in want:
        ent = w["entries"][:max(nbest, 1)]
        if not nbest:
            ent = [e[:3] + (None,) for e in ent]
        out.append(dict(entries=ent, n_ids=[len(e[0]) for e in ent] + [0] * (max(nbest, 1) - len(ent)), pops=w["pops"]))
    return out


def same(got, want, what):
    for b, (g, w) in enumerate(zip(got, want)):
        assert g["n_ids"] == w["n_ids"] and g["pops"] == w["pops"], (what, b, g["n_ids"], w["n_ids"], g["pops"], w["pops"])
        assert g["entries"] == w["entries"], (what, b, g["entries"], w["entries"])


@pytest.fixture(scope="module")
def toy(gpu_device):
    t = BL.toy()
    model = build(t["cfg"], t["sd"])
    am = model.am
    return dict(t, model=model, am=am, hw=_HotwordSet(t["graphs"], am.device), ns=_NgramSet(t["lm"], am.device), ft=torch.from_numpy(t["f"]))


def tables(toy, form):
    """-> (device keywords, checker keywords) of a form: "lm", "graphs", "both" """
    dev, chk = {}, {}
    if form != "graphs":
        dev.update(lm=toy["ns"], alpha=ALPHA)
        chk.update(lm=toy["lm"], alpha=ALPHA)
    if form != "lm":
        dev.update(hw=toy["hw"], graph_of=GRAPH_OF)
        chk.update(table=toy["table"], graph_of=GRAPH_OF)
    return dev, chk


@pytest.mark.parametrize("beam", [1, 2, 4, 8])
def test_device_equals_checker_toy_geometry(toy, beam):
    cfg, sd, f, lens, am = toy["cfg"], toy["sd"], toy["ft"], toy["lens"], toy["am"]
    mp = 64 * beam
    plain = BL.lm_checker(cfg, sd, toy["f"], lens, 0, beam=beam)
    for form in ("lm", "graphs", "both"):
        dev, chk = tables(toy, form)
        for score_norm in ((True, False) if form == "both" else (True,)):
            want = BL.lm_checker(cfg, sd, toy["f"], lens, beam, beam=beam, score_norm=score_norm, max_pops=mp, **chk)
            for nbest in sorted({0, 1, min(2, beam), beam}) if score_norm else (0, beam):
                got = device_search(am, f, lens, beam, nbest, score_norm=score_norm, max_pops=mp, **dev)
                same(got, expect(want, nbest), (beam, form, score_norm, nbest))
                assert got[4]["entries"] == [([], [], 0, 0 if nbest else None)] and got[4]["pops"] == 0      # no frames: the start hypothesis alone
        differ = [b for b in range(len(lens)) if want[b]["entries"][0][0] != plain[b]["entries"][0][0]]
        print(f"beam {beam} {form}: rows whose ids differ from the plain search {differ}; pops {[w['pops'] for w in want]}")
        if beam >= 2:
            assert differ, "re-choose the toy (tests/espnet_beam_lm_ref.py)"
    dev, _ = tables(toy, "both")
    no_frames = device_search(am, f, lens, beam, beam, max_pops=mp, with_frames=False, **dev)                # frames may be NULL
    with_frames = device_search(am, f, lens, beam, beam, max_pops=mp, **dev)
    assert [[(e[0], e[2], e[3]) for e in g["entries"]] for g in no_frames] == [[(e[0], e[2], e[3]) for e in g["entries"]] for g in with_frames]


def test_beam_20_extensions_across_two_waves(toy):
    cfg, sd, f, lens, am = toy["cfg"], toy["sd"], toy["ft"], toy["lens"], toy["am"]
    dev, chk = tables(toy, "both")
    want = BL.lm_checker(cfg, sd, toy["f"], lens, 8, beam=20, max_pops=640, **chk)
    assert max(w["pops"] for w in want) > 320                               # more pops than the plain search's default bound allows
    same(device_search(am, f, lens, 20, 8, max_pops=640, **dev), expect(want, 8), "beam 20, lists")
    same(device_search(am, f, lens, 20, 0, max_pops=640, **dev), expect(want, 0), "beam 20")


def test_a_vocabulary_above_64_x_16(gpu_device):
    cfg = ESPNET_TINY.with_(vocab_size=64 * 16 + 37).validate()              # the record kernel's <48> variant
    sd = synthetic_state_dict_espnet(cfg, 5, blank_bias=9.0, dec_gain=8.0)
    am = build(cfg, sd).am
    g = torch.Generator().manual_seed(2)
    f = torch.randn((3, 10, cfg.joint_hidden), generator=g) * 0.9
    lens = [10, 6, 8]
    plain = BL.as_plain(BL.lm_checker(cfg, sd, f.numpy(), lens, 4, beam=4, max_pops=256))
    seqs = [y for r in plain for y, _ in r["final"] if y]
    assert seqs, "the fixture must emit labels"
    lm = NL.build(LR.random_lm(BL.fixture_cfg(cfg), seqs, n_high=500, order=3, seed=9), cfg.n_logits, cfg.blank_id)
    graph = kh.build_graph([(tuple(y[:2]), 1.5) for y in seqs if len(y) >= 2][:20])
    want = BL.lm_checker(cfg, sd, f.numpy(), lens, 4, beam=4, max_pops=256, lm=lm, alpha=0.3, table=kh.concat([graph]), graph_of=[0, -1, 0])
    assert sum(w["walks"] for w in want) > 0 and sum(w["child_hits"] for w in want) > 0
    got = device_search(am, f, lens, 4, 4, max_pops=256, lm=_NgramSet(lm, am.device), alpha=0.3, hw=_HotwordSet([graph], am.device), graph_of=[0, -1, 0])
    same(got, expect(want, 4), "V = 1061")


def test_the_hand_built_edges_on_the_device(gpu_device):
    models = {}
    for name in sorted(BL.EDGES):
        case = BL.EDGES[name]
        key = tuple(sorted(case.get("probs", BL.EDGE_PROBS).items()))
        if key not in models:
            cfg, sd = BL.flat_sd(dict(key))
            models[key] = build(cfg, sd, seed=7).am
        am = models[key]
        cfg = ESPNET_TINY
        graphs, lm, alpha = BL.edge_tables(case, cfg)
        T, beam, nbest, mp = case["T"], case["beam"], case["nbest"], case.get("max_pops") or 16 * case["beam"]
        want = BL.run_edge(name)
        kw = dict(hw=_HotwordSet(graphs, am.device) if graphs else None, graph_of=[0] if graphs else None,
                  lm=_NgramSet(lm, am.device) if lm is not None else None, alpha=alpha)
        got = device_search(am, torch.zeros((1, T, cfg.joint_hidden)), [T], beam, nbest, max_pops=mp, **kw)
        same(got, expect([want], nbest), name)
        plain = device_search(am, torch.zeros((1, T, cfg.joint_hidden)), [T], beam, nbest, max_pops=mp, entry="nbest")
        if name == "phrase_open_at_the_end":                               # begun at the last frame, taken back by Finalize: the plain result
            assert [g["entries"] for g in got] == [p["entries"] for p in plain]
        else:
            assert got != plain, name                                      # every other edge moves the result or the pop count
        if name == "more_pops":                                            # ... and with a small max_pops the overflow
            assert got[0]["pops"] > 2 * plain[0]["pops"]
            assert device_search(am, torch.zeros((1, T, cfg.joint_hidden)), [T], beam, nbest, max_pops=8, entry="nbest") == plain
            with pytest.raises(capi.RsError, match="max_pops") as e:
                device_search(am, torch.zeros((1, T, cfg.joint_hidden)), [T], beam, nbest, max_pops=8, **kw)
            assert e.value.code == capi.RS_EOVERFLOW


def test_no_model_is_the_search_without_one(toy):
    f, lens, am, hw, ns = toy["ft"], toy["lens"], toy["am"], toy["hw"], toy["ns"]
    empty = types.SimpleNamespace(struct=capi.RsNgram())                   # n_nodes == 0
    no_graphs = types.SimpleNamespace(struct=capi.RsHotwords())            # n_graphs == 0
    for beam, nbest in ((2, 0), (4, 0), (4, 4), (8, 2)):
        for score_norm in (True, False):
            old = device_search(am, f, lens, beam, nbest, score_norm=score_norm, entry="old")
            for kw in (dict(), dict(lm=ns, alpha=0.0), dict(lm=empty, alpha=0.5), dict(lm=None, alpha=0.5), dict(hw=hw, graph_of=None),
                       dict(hw=no_graphs, graph_of=GRAPH_OF), dict(hw=None, graph_of=GRAPH_OF, lm=ns, alpha=0.0),
                       dict(hw=hw, graph_of=[-1] * 7)):                     # the last: the hotword form, no row has a graph
                got = device_search(am, f, lens, beam, nbest, score_norm=score_norm, **kw)
                assert got == old, (beam, nbest, score_norm, sorted(kw))
    with_lm = device_search(am, f, lens, 4, 4, max_pops=256, lm=ns, alpha=ALPHA)
    assert with_lm != device_search(am, f, lens, 4, 4, max_pops=256, entry="old")
    assert device_search(am, f, lens, 4, 4, max_pops=256, lm=ns, alpha=ALPHA, hw=hw, graph_of=[-1] * 7) == with_lm


def test_alone_equals_inside_the_ragged_batch(toy):
    f, lens, am, hw, ns = toy["ft"], toy["lens"], toy["am"], toy["hw"], toy["ns"]
    together = device_search(am, f, lens, 8, 8, max_pops=512, lm=ns, alpha=ALPHA, hw=hw, graph_of=GRAPH_OF)
    for b in (0, 1, 2, 3, 5):
        alone = device_search(am, f[b:b + 1, :lens[b]], lens[b:b + 1], 8, 8, max_pops=512, lm=ns, alpha=ALPHA, hw=hw, graph_of=[GRAPH_OF[b]])
        assert alone[0] == together[b], b


def test_through_espnetmodel_and_the_transcribe_functions(toy, tmp_path, monkeypatch):
    cfg, sd = toy["cfg"], toy["sd"]
    tokens = synthetic_token_list(cfg.vocab_size, 0)
    off = build(cfg, sd, beam_size=6)
    assert off.ngram_lm is None and off.ngram_lm_alpha == 0.0 and off.hotwords is None
    audio, lens = synthetic_batch(4, 1.5, seed=4)
    waves = [audio[b, :int(lens[b])] for b in range(4)]
    padded = [np.pad(w, (16000, 8000)) for w in waves]
    dec = off._search(padded)
    # an LM file in the symbols of token_list, cut from what the plain search says: it dislikes the most frequent label
    flat = [t for ids in dec.ids for t in ids]
    assert flat, "the plain search must emit labels: re-choose the model"
    top = max(set(flat), key=lambda t: (flat.count(t), -t))
    ent = {(t,): ((-4.0 if t == top else -0.5), -0.25) for t in range(2, cfg.vocab_size - 1)}
    ent[(BOS,)] = (-99.0, -0.125)
    for ids in dec.ids:
        for a, b in zip(ids, ids[1:]):
            if top not in (a, b):
                ent[(a, b)] = (-0.125, 0.0)
    path = NR.write_arpa(str(tmp_path / "lm.arpa"), ent, "pieces", pieces=tokens)
    others = sorted(set(flat) - {top}) or [top]
    hot = tmp_path / "hotwords.txt"
    hot.write_text(tokens[others[0]] + " :2.0\n", encoding="utf-8")
    model = build(cfg, sd, beam_size=6, ngram_lm_model=path, ngram_lm_alpha=0.6, hotwords_file=str(hot))
    assert model.ngram_lm.key == NL.build(ent, cfg.n_logits, cfg.blank_id).key and model.ngram_lm_alpha == 0.6
    assert model.hotwords.key == (((others[0],), 2.0),) and list(model.am._lm_sets) == [model.ngram_lm.key]      # uploaded once, at load
    # the model's own tables: the checker's result on the device's projection
    buf = model.am.stage(padded)
    with torch.cuda.device(model.am.device):
        model.am.run_encoder(buf, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    fe, le = buf.joint_enc.cpu().numpy(), buf.enc_lens.cpu().numpy()
    chk = lambda graphs, graph_of, alpha, nbest: BL.lm_checker(   # noqa: E731
        cfg, sd, fe, le, nbest, beam=6, max_pops=96 * 16, out_cap=2 * buf.tp_max + 16, table=kh.concat(graphs) if graphs else None,
        graph_of=graph_of if graphs else None, lm=model.ngram_lm, alpha=alpha)
    res = model._search(padded, hotwords=model.call_graphs(None, 4))
    want = chk([model.hotwords], [0] * 4, 0.6, 0)
    assert [(res.ids[b], res.frames[b], BL.bits(res.scores[b])) for b in range(4)] == [w["entries"][0][:3] for w in want]
    assert res.ids != dec.ids and res.degraded == [False] * 4, "the tables must change a result: re-choose the model"
    assert model(padded[0])[0][2] == res.ids[0]
    # a call's own hotwords instead of the model's; per window, with lists
    mine = [(top,), (others[-1],)]
    one = model(padded[1], hotwords=[(p, 1.5) for p in mine])
    g_mine = kh.build_graph([(p, 1.5) for p in mine])
    assert one[0][2] == chk([g_mine], [-1, 0, -1, -1], 0.6, 0)[1]["entries"][0][0]
    lists = model.recognize_batch(waves, hotwords=[None, [(p, 1.5) for p in mine], tokens[top], None], nbest=3)
    g_top = kh.build_graph([((top,), 1.5)])
    want = chk([model.hotwords, g_mine, g_top], [0, 1, 2, 0], 0.6, 3)
    for b in range(4):
        assert [(ids, BL.bits(h.score), BL.bits(h.norm_score)) for _, _, ids, h in lists[b]] == [(e[0], e[2], e[3]) for e in want[b]["entries"]], b
    # ngram_lm_alpha = 0 per call: without the LM (the model's graph stays); the setter
    no_lm = chk([model.hotwords], [0] * 4, 0.0, 0)
    assert model.recognize_batch(waves, ngram_lm_alpha=0) == [model.ids_to_text(w["entries"][0][0]) for w in no_lm]
    model.ngram_lm_alpha = 0.0
    assert model.recognize_batch(waves) == [model.ids_to_text(w["entries"][0][0]) for w in no_lm]
    model.ngram_lm_alpha = 0.6
    with pytest.raises(ValueError, match="finite number"):
        model.ngram_lm_alpha = -1.0
    with pytest.raises(ValueError, match="no n-gram LM"):
        off(padded[0], ngram_lm_alpha=0.3)
    # transcribe / transcribe_batch, segmentation on the device: a recording's hotwords reach its windows
    # (the segmenter is not what is under test, and synthetic weights emit punctuation its text preparation drops: one segment per window)
    model.segmentation = "device"
    model.align_batch = lambda waves, texts, max_batch=256: [None] * len(waves)
    monkeypatch.setattr(tr, "split_text", lambda model, samples, text: [(0, len(samples), text)])
    conf = interface.TranscribeConfig(verbose=False)
    audios = [interface.AudioData(w, 16000) for w in waves]
    specs = [None, [(p, 1.5) for p in mine], tokens[top], None]
    batch = tr.transcribe_batch(model, audios, conf, hotwords=specs)
    assert [r.text for r in batch] == [x[0][0] for x in lists]
    assert tr.transcribe(model, audios[1], conf, hotwords=specs[1]).text == batch[1].text
    assert tr.transcribe(model, audios[2], conf, hotwords=specs[2], ngram_lm_alpha=0.6).text == batch[2].text
    model.segmentation = "host"
    # token scores stay the model's own distribution
    model.token_scores = True
    scored = model._search(padded, hotwords=model.call_graphs(None, 4))
    model.token_scores = False
    assert scored.ids == res.ids
    u_cap = max(1, max(len(y) for y in scored.ids))
    ids_m, n_m = TS.pack(scored.ids, u_cap)
    logp, _ = TS.scores_checker(cfg, sd, fe, le.astype(np.int32), ids_m, TS.pack(scored.frames, u_cap)[0], n_m)
    assert [[BL.bits(v) for v in lp] for lp in scored.token_logprobs] == [[BL.bits(v) for v in logp[b, :n_m[b]]] for b in range(4)]
    # the overflow ladder: a bonus on EVERY label, above every label's log-probability, lets each extension outscore its parent, so
    # a frame never ends — x4, x16, then greedy, flagged
    tight = build(cfg, sd, beam_size=2, max_pops=2)
    endless = kh.build_graph([((t,), 40.0) for t in range(2, cfg.vocab_size - 1)])
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        res = tight._search(padded[:2], hotwords=[endless] * 2)
    assert res.degraded == [True, True] and any("greedy search instead" in str(x.message) for x in w)
    assert [len(y) <= e for y, e in zip(res.ids, res.enc_lens)] == [True, True]          # the greedy search: at most one label a frame


def test_errors(toy):
    f, lens, am, hw, ns, lm = toy["ft"], toy["lens"], toy["am"], toy["hw"], toy["ns"], toy["lm"]

    def broken(base, cls, **fields):
        t = cls.from_buffer_copy(base.struct)
        for k, v in fields.items():
            setattr(t, k, v)
        return types.SimpleNamespace(struct=t)
    bad_lm = lambda **kw: dict(lm=broken(ns, capi.RsNgram, **kw), alpha=0.5)                            # noqa: E731
    bad_hw = lambda **kw: dict(hw=broken(hw, capi.RsHotwords, **kw), graph_of=GRAPH_OF)                # noqa: E731
    # refused from the argument list, before anything is enqueued: the outputs keep their fill
    cases = [(dict(lm=ns, alpha=float("nan")), "lm_alpha"), (dict(lm=ns, alpha=float("inf")), "lm_alpha"), (dict(lm=ns, alpha=-0.5), "lm_alpha"),
             (bad_lm(n_logits=ESPNET_TINY.n_logits + 1), "logits"), (bad_lm(order=0), "order"), (bad_lm(order=9), "order"),
             (bad_lm(start=lm.n_nodes), "start"), (bad_lm(start=-1), "start"), (bad_lm(n_children=-1), "negative count"),
             (bad_lm(n_nodes=-1), "negative count"), (bad_lm(logp=None), "null array"), (bad_lm(suffix=None), "null array"),
             (bad_hw(n_nodes=-1), "negative count"), (bad_hw(max_level=-1), "negative count"), (bad_hw(fail=None), "null array"),
             (bad_hw(graph_root=None), "null array")]
    for kw, pattern in cases:
        with pytest.raises(capi.RsError, match=pattern) as e:
            device_search(am, f, lens, 4, 2, **kw)
        assert e.value.code == capi.RS_EINVAL and device_search.untouched, (pattern, sorted(kw))
    for beam, nbest, pattern in ((20, 9, "nbest must be 0..8"), (4, -1, "nbest must be 0..8"), (4, 5, "above the beam"), (2, 3, "above the beam"),
                                 (0, 0, "beam size must be >= 1")):
        with pytest.raises(capi.RsError, match=pattern) as e:
            device_search(am, f, lens, beam, nbest, lm=ns, alpha=0.5)
        assert e.value.code == capi.RS_EINVAL and device_search.untouched, (beam, nbest)
    for args in ((4, 5), (0, 1), (20, 9), (4, -1)):
        with pytest.raises(RuntimeError):
            am.ctx.beam_workspace_bytes(7, args[0], 24, 0, lm=True, nbest=args[1])
    with pytest.raises(capi.RsError, match="workspace") as e:
        device_search(am, f, lens, 4, 4, lm=ns, alpha=0.5, short=1)
    assert e.value.code == RS_EWORKSPACE
    with pytest.raises(capi.RsError, match="max_pops") as e:
        device_search(am, f, lens, 8, 8, max_pops=9, lm=ns, alpha=0.5, hw=hw, graph_of=GRAPH_OF)
    assert e.value.code == capi.RS_EOVERFLOW
    with pytest.raises(capi.RsError, match="out_cap") as e:               # a returned entry that does not fit
        device_search(am, f, lens, 4, 4, max_pops=256, out_cap=1, lm=ns, alpha=0.5)
    assert e.value.code == capi.RS_EOVERFLOW
    assert device_search(am, f, lens, 2, 2, max_pops=128, lm=ns, alpha=0.5)                              # and the context is usable afterwards
    # a Zipformer context
    k2 = K2Model(ZIPFORMER_TINY, synthetic_state_dict_k2(ZIPFORMER_TINY, 0), synthetic_tokens(ZIPFORMER_TINY.vocab_size, 0), device="cuda:0")
    with pytest.raises(RuntimeError):
        k2.am.ctx.beam_workspace_bytes(2, 4, 10, 0, lm=True)
    dev = k2.am.device
    z = lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)          # noqa: E731
    zf = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)       # noqa: E731
    with pytest.raises(capi.RsError, match="rs_rnnt_beam_lm: not defined for a Zipformer context") as e:
        k2.am.ctx.rnnt_beam(zf(2, 10, ZIPFORMER_TINY.joiner_dim), z(2) + 10, 2, 10, 4, True, 0, z(2, 10), z(2), zf(2), z(2),
                            torch.empty((1 << 20,), dtype=torch.uint8, device=dev), 0, lm=ns.struct, lm_alpha=0.5)
    assert e.value.code == capi.RS_EINVAL
    # the greedy model refuses both at every entrance
    greedy = toy["model"]
    with pytest.raises(ValueError, match="needs the beam search"):
        greedy.ngram_lm = lm
    with pytest.raises(ValueError, match="need the beam search"):
        greedy(np.zeros(16000, np.float32), hotwords=[(10,)])
