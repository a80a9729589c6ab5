"""-m gpu: n-gram LM shallow fusion in the ALSD beam search on the device (rs_rnnt_alsd_lm, csrc/k_rnnt_alsd.hip, k_rnnt_ngram.h)
against its C checker (tests/alsd_checker.c, itself held to its predecessor's recorded results and a float64 restatement in
tests/test_alsd_lm_host.py): labels, alignment steps and score BITS.

  toy geometry      7 ragged rows (one without frames, one of full length); beams 1 / 2 / 4 / 8, and once each: merge on, score
                    normalisation off, an absolute label budget; the LM alone, and with the three toy graphs plus "none"
  619M geometry     V + 1 = 3001 (the <48> form of the selection kernel), an order-4 LM with a unigram for every token and a few
                    thousand higher-order n-grams around what the search proposes: long child lists and root_child
  wide vocabulary   n_logits > 3072 (the <0> form) with an LM
  no model          a null table / alpha 0 is rs_rnnt_alsd_hotwords, bits; without graphs as well rs_rnnt_alsd, bits
  batch invariance; the nemo package's keywords; errors from the argument list (a table meant to misbehave is never uploaded: the
  corrupt-table cases live in tests/test_ngram_lm_host.py)"""
import types

import numpy as np
import pytest
import torch

import alsd_hotwords_ref as AR
import ngram_lm_ref as NR
import token_scores_ref as TS
from reazonspeech_amd.runtime import capi, k2_hotwords as kh, ngram_lm as NL
from reazonspeech_amd.runtime.config import TINY, WIDE2
from reazonspeech_amd.runtime.k2_config import ZIPFORMER_TINY
from reazonspeech_amd.runtime.model import AsrModel, _HotwordSet, _NgramSet
from reazonspeech_amd.runtime.synth import synthetic_batch
from reazonspeech_amd.runtime.tokenizer import SyntheticTokenizer
from reazonspeech_amd.runtime.weights import synthetic_state_dict

pytestmark = pytest.mark.gpu

TOY_SEED = 6            # tests/test_alsd_lm_host.py decides on the CPU that this batch exercises every counter
TOY_ALPHA = 0.5
GRAPH_OF = AR.TOY_GRAPH_OF
BOS = NL.BOS


def device_search(model, f, lens, beam, lm=None, alpha=0.0, hw=None, graph_of=None, max_target_len=2.0, score_norm=True, merge=False,
                  entry="lm"):
    """rs_rnnt_alsd_lm (or rs_rnnt_alsd_hotwords / rs_rnnt_alsd: `entry`) on a projection f [B][Tp][J] -> list of (ids, steps, score bits)"""
    dev = model.device
    f = torch.as_tensor(f)
    B, Tp, _ = f.shape
    budget = int(max_target_len * Tp) if isinstance(max_target_len, float) else int(max_target_len)
    out_cap = max(1, Tp + budget)
    f = f.to(dev).contiguous()
    lens = torch.as_tensor(np.asarray(lens), dtype=torch.int32).to(dev)
    ids = torch.zeros((B, out_cap), dtype=torch.int32, device=dev)
    steps = torch.zeros_like(ids)
    n_ids = torch.full((B,), -7, dtype=torch.int32, device=dev)
    scores = torch.full((B,), float("nan"), dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    gof = None if graph_of is None else torch.as_tensor(np.asarray(graph_of), dtype=torch.int32).to(dev)
    hws = hw.struct if hw is not None else None
    if entry == "plain":
        ws = torch.empty((model.ctx.alsd_workspace_bytes(B, beam, Tp, max_target_len),), dtype=torch.uint8, device=dev)
        model.ctx.rnnt_alsd(f, lens, B, Tp, beam, max_target_len, score_norm, merge, ids, steps, n_ids, scores, ws, stream)
    elif entry == "hotwords":
        ws = torch.empty((model.ctx.alsd_workspace_bytes(B, beam, Tp, max_target_len, hotwords=True),), dtype=torch.uint8, device=dev)
        model.ctx.rnnt_alsd(f, lens, B, Tp, beam, max_target_len, score_norm, merge, ids, steps, n_ids, scores, ws, stream, hotwords=hws, graph_of=gof)
    else:
        n = model.ctx.alsd_workspace_bytes(B, beam, Tp, max_target_len, hotwords=True, lm=True)
        assert n >= model.ctx.alsd_workspace_bytes(B, beam, Tp, max_target_len, hotwords=True) + 2 * 4 * B * min(beam, model.cfg.n_logits - 1)
        ws = torch.empty((n,), dtype=torch.uint8, device=dev)
        model.ctx.rnnt_alsd(f, lens, B, Tp, beam, max_target_len, score_norm, merge, ids, steps, n_ids, scores, ws, stream, hotwords=hws,
                            graph_of=gof, lm=lm.struct if lm is not None else None, lm_alpha=alpha)
    torch.cuda.synchronize()
    n = n_ids.cpu().numpy()
    bits = scores.cpu().numpy().view(np.int32)
    return [(ids[b, :n[b]].cpu().tolist(), steps[b, :n[b]].cpu().tolist(), int(bits[b])) for b in range(B)]


def check(model, sd, f, lens, lm, alpha, graphs=None, graph_of=None, **kw):
    """device == checker, bits; -> (device rows, checker rows)"""
    hw = _HotwordSet(graphs, model.device) if graphs else None
    got = device_search(model, f, lens, lm=_NgramSet(lm, model.device), alpha=alpha, hw=hw, graph_of=graph_of if graphs else None, **kw)
    want = AR.alsd_checker(model.cfg, sd, np.asarray(f), np.asarray(lens, np.int32), kh.concat(graphs) if graphs else None,
                           graph_of if graphs else None, lm, alpha, **kw)
    for b, (g, w) in enumerate(zip(got, want)):
        assert g[0] == w["ids"] and g[1] == w["steps"], (kw, b, g[:2], w["ids"], w["steps"])
        assert g[2] == w["score_bits"], (kw, b, g[2], w["score_bits"], w["score"])
    return got, want


@pytest.fixture(scope="module")
def tiny(gpu_device):
    sd = synthetic_state_dict(TINY, 0)
    return AsrModel(TINY, sd, SyntheticTokenizer(TINY.vocab_size), device="cuda:0"), sd


@pytest.fixture(scope="module")
def toy(tiny):
    """the ragged batch, and the graphs and the LM cut from the plain checker's results at beam 4"""
    _, sd = tiny
    f, lens = AR.toy_batch(TINY, seed=TOY_SEED)
    f, lens = f.numpy(), lens.numpy()
    assert len(lens) == 7 and f.shape[1] == 21 and lens[2] == 0 and lens[5] == 21
    plain = AR.alsd_checker(TINY, sd, f, lens, beam=4)
    graphs = [kh.build_graph(p) for p in AR.toy_graphs(plain)]
    return f, lens, graphs, NL.build(NR.toy_lm(plain, TINY), TINY.vocab_size, TINY.blank_id)


@pytest.mark.parametrize("beam,max_target_len,norm,merge", [(1, 2.0, True, False), (2, 2.0, True, False), (4, 2.0, True, False),
                                                            (8, 2.0, True, False), (4, 2.0, True, True), (4, 2.0, False, False),
                                                            (4, 9, True, False)])
def test_bit_exact_toy_geometry(tiny, toy, beam, max_target_len, norm, merge):
    model, sd = tiny
    f, lens, graphs, lm = toy
    kw = dict(beam=beam, max_target_len=max_target_len, score_norm=norm, merge=merge)
    plain = device_search(model, f, lens, entry="plain", **kw)
    for with_graphs in (False, True):                      # the LM alone; the LM together with the three graphs plus "none"
        got, want = check(model, sd, f, lens, lm, TOY_ALPHA, graphs if with_graphs else None, GRAPH_OF, **kw)
        assert got[2] == ([], [], 0)
        t = NR.totals(want, lm.order)
        print("toy geometry", kw, "graphs" if with_graphs else "no graphs", t, "rows changed:", sum(g[0] != p[0] for g, p in zip(got, plain)))
        if beam == 1:
            t["recombinations"] = 1                        # one hypothesis per utterance: nothing to recombine with
        assert NR.all_counted(t), f"the model must be exercised; re-choose the inputs: {t}"
        assert any(g[0] != p[0] for g, p in zip(got, plain)), "the LM must change a row's labels; re-choose the inputs"
        if with_graphs:
            assert sum(w["child_hits"] for w in want) > 0


def test_bit_exact_at_619m_geometry(gpu_device):
    """V + 1 = 3001: the <48> form; an order-4 LM with every unigram and a few thousand higher-order n-grams around the labels the
    plain search proposes: the bisection of long child lists, and root_child for the candidates that back off all the way"""
    cfg = WIDE2
    sd = synthetic_state_dict(cfg, 0, blank_bias=6.5)
    model = AsrModel(cfg, sd, SyntheticTokenizer(cfg.vocab_size), device="cuda:0")
    assert (cfg.pred_hidden, cfg.joint_hidden, cfg.n_logits) == (640, 640, 3001)
    g = torch.Generator().manual_seed(15)
    B, Tp = 5, 12
    f = (torch.randn((B, Tp, cfg.joint_hidden), generator=g) * (0.8 + 0.4 * torch.rand((B, 1, 1), generator=g))).numpy()
    lens = torch.randint(3, Tp + 1, (B,), generator=g, dtype=torch.int32).numpy()
    lens[2] = Tp
    plain = AR.alsd_checker(cfg, sd, f, lens, beam=4, max_target_len=1.0)                # the label sequences the search proposes
    seqs = [y for r in plain for y, *_ in r["beam"] + [(r["ids"], 0, 0)] if y]
    seen = sorted({t for y in seqs for t in y})
    assert len(seen) >= 2
    lm = NL.build(NR.random_lm(cfg, seqs, n_high=3000, order=4), cfg.vocab_size, cfg.blank_id)
    a = lm.arrays
    longest = int(np.diff(a["child_begin"])[1:].max())
    assert lm.order == 4 and lm.n_nodes > 3000 + cfg.vocab_size and (a["root_child"][:cfg.vocab_size] > 0).all() and longest >= 64
    got, want = check(model, sd, f, lens, lm, 0.4, beam=4, max_target_len=1.0)
    t = NR.totals(want, 4)
    print("619M decoder geometry:", lm.n_nodes, "nodes, the longest child list below the root has", longest, "entries;", t)
    assert all(h > 0 for h in t["hits"]) and t["backoffs"] > 0 and t["full_order_pops"] > 0
    assert any(g[0] != p["ids"] for g, p in zip(got, plain))
    graph = kh.build_graph([((int(seen[0]), int(seen[1])), 2.0), ((int(seen[1]),), 1.5)])
    check(model, sd, f, lens, lm, 0.4, [graph], [0, -1, 0, 0, -1], beam=4, max_target_len=1.0)


def test_bit_exact_wide_vocabulary_form(gpu_device):
    """n_logits > 3072: the <0> form of the selection kernel (two passes over memory) with an LM; TINY widened in vocabulary only"""
    cfg = TINY.with_(vocab_size=3100)
    assert cfg.n_logits > 64 * 48
    sd = synthetic_state_dict(cfg, 0)
    model = AsrModel(cfg, sd, SyntheticTokenizer(cfg.vocab_size), device="cuda:0")
    g = torch.Generator().manual_seed(33)
    B, Tp = 3, 8
    f = (torch.randn((B, Tp, cfg.joint_hidden), generator=g) * 0.9).numpy()
    lens = np.asarray([8, 5, 7], np.int32)
    plain = AR.alsd_checker(cfg, sd, f, lens, beam=2, max_target_len=1.0)
    seqs = [y for r in plain for y, *_ in r["beam"] + [(r["ids"], 0, 0)] if y]
    assert seqs, "the fixture must emit labels"
    lm = NL.build(NR.random_lm(cfg, seqs, n_high=500, order=3, seed=9), cfg.vocab_size, cfg.blank_id)
    got, want = check(model, sd, f, lens, lm, 0.6, beam=2, max_target_len=1.0)
    print("wide vocabulary:", NR.totals(want, 3))
    assert all(h > 0 for h in NR.totals(want, 3)["hits"])


def test_no_model_is_the_search_without_one(tiny, toy):
    model, _ = tiny
    f, lens, graphs, lm = toy
    hw, ns = _HotwordSet(graphs, model.device), _NgramSet(lm, model.device)
    empty = types.SimpleNamespace(struct=capi.RsNgram())                   # n_nodes == 0
    for beam in (2, 4):
        plain = device_search(model, f, lens, beam, entry="plain")
        hot = device_search(model, f, lens, beam, hw=hw, graph_of=GRAPH_OF, entry="hotwords")
        assert hot != plain
        assert device_search(model, f, lens, beam, lm=None, alpha=0.5) == plain                           # a null table, no graphs: rs_rnnt_alsd
        assert device_search(model, f, lens, beam, lm=ns, alpha=0.0) == plain                             # alpha 0
        assert device_search(model, f, lens, beam, lm=empty, alpha=0.5) == plain
        assert device_search(model, f, lens, beam, lm=None, alpha=0.5, hw=hw, graph_of=GRAPH_OF) == hot   # ... with graphs: rs_rnnt_alsd_hotwords
        assert device_search(model, f, lens, beam, lm=ns, alpha=0.0, hw=hw, graph_of=GRAPH_OF) == hot
        assert device_search(model, f, lens, beam, lm=ns, alpha=0.5, hw=hw, graph_of=[-1] * 7) == device_search(model, f, lens, beam, lm=ns, alpha=0.5)


def test_alone_equals_inside_a_ragged_batch(tiny, toy):
    model, _ = tiny
    f, lens, graphs, lm = toy
    hw, ns = _HotwordSet(graphs, model.device), _NgramSet(lm, model.device)
    together = device_search(model, f, lens, 4, lm=ns, alpha=TOY_ALPHA, hw=hw, graph_of=GRAPH_OF)
    for b in (0, 1, 4):
        gof = [GRAPH_OF[b]]
        alone = device_search(model, f[b:b + 1, :lens[b]], lens[b:b + 1], 4, lm=ns, alpha=TOY_ALPHA, hw=hw, graph_of=gof)
        assert alone[0] == together[b], b


def test_through_the_nemo_package(gpu_device, tmp_path):
    from reazonspeech_amd.nemo.asr import TranscribeConfig, audio_from_numpy, load_model, transcribe, transcribe_batch
    conf = TranscribeConfig(verbose=False)
    plain_model = load_model(device="cuda:0", config=TINY, decoding="alsd", beam_size=4)
    assert plain_model.ngram_lm is None and plain_model.ngram_lm_alpha == 0.0
    audio, lens = synthetic_batch(9, 2.0, seed=50, ragged=True, min_seconds=0.5)
    audios = [audio_from_numpy(audio[b, :lens[b]], 16000) for b in range(9)]
    waves = [np.ascontiguousarray(a.waveform, dtype=np.float32) for a in audios]
    base = transcribe_batch(plain_model, audios, conf)
    dec = plain_model.transcribe_waveforms(waves)
    # an LM file in NeMo's encoding, cut from what the plain search says: it dislikes the most frequent label and likes the rest
    flat = [t for ids in dec.ids for t in ids]
    top = max(set(flat), key=flat.count)
    ent = {(t,): ((-4.0 if t == top else -0.5), -0.25) for t in range(TINY.vocab_size)}
    ent[(BOS,)] = (-99.0, -0.125)
    for ids in dec.ids:
        for a, b in zip(ids, ids[1:]):
            if top not in (a, b):
                ent[(a, b)] = (-0.125, 0.0)
    path = NR.write_arpa(str(tmp_path / "lm.arpa"), ent, "nemo")
    model = load_model(device="cuda:0", config=TINY, decoding="alsd", beam_size=4, ngram_lm_model=path, ngram_lm_alpha=0.6)
    assert model.ngram_lm.key == NL.build(ent, TINY.vocab_size, TINY.blank_id).key and model.ngram_lm_alpha == 0.6
    res = transcribe_batch(model, audios, conf)
    text = lambda rs: [r.text for r in rs]                                 # noqa: E731
    assert text(res) != text(base), "the LM must change a transcript: re-choose the model"
    for b in (0, 4):                                                       # transcribe == the transcribe_batch row
        one = transcribe(model, audios[b], conf)
        assert one.text == res[b].text and [s.seconds for s in one.subwords] == [s.seconds for s in res[b].subwords]
    # per call: alpha 0 = without the LM; another alpha = the runtime at that weight; the model's value is settable
    assert [transcribe(model, audios[b], conf, ngram_lm_alpha=0).text for b in (0, 3, 4)] == [base[b].text for b in (0, 3, 4)]
    other = model.transcribe_waveforms(waves, ngram_lm=(model.ngram_lm, 1.5))
    assert transcribe(model, audios[3], conf, ngram_lm_alpha=1.5).text == model.tokenizer.ids_to_text(other.ids[3])
    model.ngram_lm_alpha = 0.0
    assert text(transcribe_batch(model, audios, conf)) == text(base)
    model.ngram_lm_alpha = 0.6
    with pytest.raises(ValueError, match="no n-gram LM"):
        transcribe(plain_model, audios[0], conf, ngram_lm_alpha=0.3)
    # the runtime's results are the checker's on the device's projection; token scores stay the model's own distribution
    sd = synthetic_state_dict(TINY, 0)
    buf = model.stage(waves, buf=model.new_buffers(9, max(len(w) for w in waves)))
    model.token_scores = True
    model.run_device(buf)
    torch.cuda.synchronize()
    got = model.collect(buf)
    model.token_scores = False
    want = AR.alsd_checker(TINY, sd, buf.joint_enc.cpu().numpy(), np.asarray(got.enc_lens, np.int32), lm=model.ngram_lm, alpha=0.6,
                           beam=4, max_target_len=TINY.alsd_max_target_len)
    assert got.ids == [w["ids"] for w in want] and got.frames == [[i - u for u, i in enumerate(w["steps"])] for w in want]
    assert [np.float32(s) for s in got.scores] == [np.float32(w["score"]) for w in want]
    assert [model.tokenizer.ids_to_text(ids) for ids in got.ids] == text(res) and got.ids != dec.ids
    u_cap = max(1, max(len(y) for y in got.ids))
    ids_m, n_m = TS.pack(got.ids, u_cap)
    logp, _ = TS.scores_checker(TINY, sd, buf.joint_enc.cpu().numpy(), np.asarray(got.enc_lens, np.int32), ids_m, TS.pack(got.frames, u_cap)[0], n_m)
    assert [[AR.bits(v) for v in lp] for lp in got.token_logprobs] == [[AR.bits(v) for v in logp[b, :n_m[b]]] for b in range(9)]
    # hotwords and the LM in one batch, through the host pipeline (max_batch < n): the same rows as one batch
    graphs = [kh.build_graph([((top,), 4.0)]) if b % 2 else None for b in range(9)]
    whole = model.transcribe_waveforms(waves, hotwords=graphs)
    parts = model.transcribe_waveforms(waves, max_batch=4, hotwords=graphs)
    assert (whole.ids, whole.frames, whole.scores) == (parts.ids, parts.frames, parts.scores) and whole.ids != got.ids


def test_errors(tiny, toy):
    model, _ = tiny
    f, lens, graphs, lm = toy
    dev = model.device
    ns = _NgramSet(lm, dev)
    z = lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)          # noqa: E731
    k2 = capi.Context(ZIPFORMER_TINY, 0)
    try:
        with pytest.raises(RuntimeError):
            k2.alsd_workspace_bytes(2, 4, 10, 1.0, lm=True)
        with pytest.raises(capi.RsError, match="not defined for a Zipformer context") as e:
            k2.rnnt_alsd(torch.zeros((2, 10, TINY.joint_hidden), device=dev), z(2) + 10, 2, 10, 4, 1.0, True, False, z(2, 20), z(2, 20),
                         z(2), torch.zeros((2,), device=dev), torch.empty((1 << 20,), dtype=torch.uint8, device=dev), 0, lm=ns.struct, lm_alpha=0.5)
        assert e.value.code == capi.RS_EINVAL
    finally:
        k2.close()

    def broken(**fields):
        t = capi.RsNgram.from_buffer_copy(ns.struct)
        for k, v in fields.items():
            setattr(t, k, v)
        return types.SimpleNamespace(struct=t)
    # refused from the argument list, before anything is enqueued: the outputs keep their fill
    for bad, alpha, pattern in ((ns, float("nan"), "lm_alpha"), (ns, float("inf"), "lm_alpha"), (ns, -0.5, "lm_alpha"),
                                (broken(n_children=-1), 0.5, "negative count"), (broken(n_logits=TINY.n_logits + 1), 0.5, "logits"),
                                (broken(order=0), 0.5, "order"), (broken(order=9), 0.5, "order"), (broken(start=lm.n_nodes), 0.5, "start"),
                                (broken(logp=None), 0.5, "null array"), (broken(unk_logp=float("nan")), 0.5, "unk_logp")):
        with pytest.raises(capi.RsError, match=pattern) as e:
            device_search(model, f, lens, 4, lm=bad, alpha=alpha)
        assert e.value.code == capi.RS_EINVAL
    with pytest.raises(capi.RsError) as e:                                 # what rs_rnnt_alsd rejects
        device_search(model, f, lens, 9, lm=ns, alpha=0.5)
    assert e.value.code == capi.RS_EINVAL
    with pytest.raises(ValueError, match="alsd"):                          # greedy refuses an LM
        AsrModel(TINY, synthetic_state_dict(TINY, 0), SyntheticTokenizer(TINY.vocab_size), device="cuda:0").lm_plan((lm, 0.5))
