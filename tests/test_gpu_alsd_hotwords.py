"""-m gpu: hotwords in the ALSD beam search on the device (rs_rnnt_alsd_hotwords, csrc/k_rnnt_alsd.hip) against its C checker
(tests/alsd_checker.c, itself held to oracle/rnnt_alsd.c and a float64 restatement in tests/test_alsd_hotwords_host.py):
labels, alignment steps and score BITS.

  toy geometry      7 ragged rows (one without frames, one of full length), three graphs plus "none" spread over them; beams
                    1 / 2 / 4 / 8, and once each: merge on, score normalisation off, an absolute label budget
  619M geometry     V + 1 = 3001 (the <48> form of the selection kernel), one graph of 3000 phrases: a long child list at the root
  wide vocabulary   n_logits > 3072 (the <0> form) with hotwords
  no graph          a null table / graph_of all -1 is rs_rnnt_alsd, bits;  batch invariance;  the nemo package's keywords;  errors"""
import types

import numpy as np
import pytest
import torch

import alsd_hotwords_ref as AR
import token_scores_ref as TS
from reazonspeech_amd.runtime import capi, k2_hotwords as kh
from reazonspeech_amd.runtime.config import TINY, WIDE2
from reazonspeech_amd.runtime.k2_config import ZIPFORMER_TINY
from reazonspeech_amd.runtime.model import AsrModel, _HotwordSet
from reazonspeech_amd.runtime.synth import synthetic_batch
from reazonspeech_amd.runtime.tokenizer import SyntheticTokenizer
from reazonspeech_amd.runtime.weights import synthetic_state_dict

pytestmark = pytest.mark.gpu

TOY_SEED = 6            # tests/test_alsd_hotwords_host.py decides on the CPU that this batch exercises every counter
GRAPH_OF = AR.TOY_GRAPH_OF


def device_search(model, f, lens, beam, hw=None, graph_of=None, max_target_len=2.0, score_norm=True, merge=False, plain=False):
    """rs_rnnt_alsd_hotwords (or, `plain`, rs_rnnt_alsd) on a projection f [B][Tp][J] -> list of (ids, steps, score bits)"""
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
    if plain:
        ws = torch.empty((model.ctx.alsd_workspace_bytes(B, beam, Tp, max_target_len),), dtype=torch.uint8, device=dev)
        model.ctx.rnnt_alsd(f, lens, B, Tp, beam, max_target_len, score_norm, merge, ids, steps, n_ids, scores, ws, stream)
    else:
        gof = None if graph_of is None else torch.as_tensor(np.asarray(graph_of), dtype=torch.int32).to(dev)
        n = model.ctx.alsd_workspace_bytes(B, beam, Tp, max_target_len, hotwords=True)
        assert n >= model.ctx.alsd_workspace_bytes(B, beam, Tp, max_target_len) + 2 * 4 * B * min(beam, model.cfg.n_logits - 1)
        ws = torch.empty((n,), dtype=torch.uint8, device=dev)
        model.ctx.rnnt_alsd(f, lens, B, Tp, beam, max_target_len, score_norm, merge, ids, steps, n_ids, scores, ws, stream,
                            hotwords=hw.struct if hw is not None else None, graph_of=gof)
    torch.cuda.synchronize()
    n = n_ids.cpu().numpy()
    bits = scores.cpu().numpy().view(np.int32)
    return [(ids[b, :n[b]].cpu().tolist(), steps[b, :n[b]].cpu().tolist(), int(bits[b])) for b in range(B)]


def check(model, sd, f, lens, graphs, graph_of, **kw):
    """device == checker, bits; -> (device rows, checker rows)"""
    hw = _HotwordSet(graphs, model.device)
    got = device_search(model, f, lens, hw=hw, graph_of=graph_of, **kw)
    want = AR.alsd_checker(model.cfg, sd, np.asarray(f), np.asarray(lens, np.int32), kh.concat(graphs), graph_of, **kw)
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
    """the ragged batch, and the graphs cut from the plain checker's results at beam 4"""
    _, sd = tiny
    f, lens = AR.toy_batch(TINY, seed=TOY_SEED)
    f, lens = f.numpy(), lens.numpy()
    assert len(lens) == 7 and f.shape[1] == 21 and lens[2] == 0 and lens[5] == 21
    graphs = [kh.build_graph(p) for p in AR.toy_graphs(AR.alsd_checker(TINY, sd, f, lens, beam=4))]
    return f, lens, graphs


@pytest.mark.parametrize("beam,max_target_len,norm,merge", [(1, 2.0, True, False), (2, 2.0, True, False), (4, 2.0, True, False),
                                                            (8, 2.0, True, False), (4, 2.0, True, True), (4, 2.0, False, False),
                                                            (4, 9, True, False)])
def test_bit_exact_toy_geometry(tiny, toy, beam, max_target_len, norm, merge):
    model, sd = tiny
    f, lens, graphs = toy
    kw = dict(beam=beam, max_target_len=max_target_len, score_norm=norm, merge=merge)
    got, want = check(model, sd, f, lens, graphs, GRAPH_OF, **kw)
    plain = device_search(model, f, lens, plain=True, **kw)
    assert got[2] == ([], [], 0)
    for b, g in enumerate(GRAPH_OF):
        if g < 0:
            assert got[b] == plain[b], b                   # a row without a graph inside a hotword call: the plain search's bits
    total = {k: sum(w[k] for w in want) for k in AR.COUNTERS}
    print("toy geometry", kw, total, "rows changed:", sum(g[0] != p[0] for g, p in zip(got, plain)))
    assert all(total[k] > 0 for k in AR.COUNTERS[:4]), f"the graphs must be exercised; re-choose the inputs: {total}"
    assert beam < 2 or any(g[0] != p[0] for g, p in zip(got, plain)), "the graphs must change a row's labels; re-choose the inputs"


def test_bit_exact_at_619m_geometry(gpu_device):
    """V + 1 = 3001: the <48> form; 3000 random phrases over 400 first tokens: the bisection of a long child list"""
    cfg = WIDE2
    sd = synthetic_state_dict(cfg, 0, blank_bias=6.5)
    model = AsrModel(cfg, sd, SyntheticTokenizer(cfg.vocab_size), device="cuda:0")
    assert (cfg.pred_hidden, cfg.joint_hidden, cfg.n_logits) == (640, 640, 3001)
    g = torch.Generator().manual_seed(15)
    B, Tp = 5, 12
    f = (torch.randn((B, Tp, cfg.joint_hidden), generator=g) * (0.8 + 0.4 * torch.rand((B, 1, 1), generator=g))).numpy()
    lens = torch.randint(3, Tp + 1, (B,), generator=g, dtype=torch.int32).numpy()
    lens[2] = Tp
    plain = AR.alsd_checker(cfg, sd, f[2:3], lens[2:3], beam=4, max_target_len=1.0)      # labels the search proposes: one row is enough
    seen = sorted({t for r in plain for y, *_ in r["beam"] + [(r["ids"], 0, 0)] for t in y})
    assert len(seen) >= 2
    rng = np.random.default_rng(4)
    firsts = np.unique(np.concatenate([rng.choice(cfg.vocab_size, size=400 - len(seen), replace=False), seen]))
    phrases = []
    for _ in range(3000):
        n = int(rng.integers(1, 5))
        tail = [int(rng.choice(seen)) if rng.random() < 0.5 else int(rng.integers(0, cfg.vocab_size)) for _ in range(n - 1)]
        phrases.append(((int(rng.choice(firsts)), *tail), float(rng.choice([1.0, 1.5, 2.0, 4.0]))))
    graph = kh.build_graph(phrases)
    root_children = graph.arrays["child_begin"][1] - graph.arrays["child_begin"][0]
    assert root_children >= 390 and graph.max_level == 4
    got, want = check(model, sd, f, lens, [graph], [0, 0, 0, -1, 0], beam=4, max_target_len=1.0)
    print("619M decoder geometry:", root_children, "children of the root;", {k: sum(w[k] for w in want) for k in AR.COUNTERS})
    assert sum(w["child_hits"] for w in want) > 0
    assert got[3] == device_search(model, f, lens, 4, max_target_len=1.0, plain=True)[3]


def test_bit_exact_wide_vocabulary_form(gpu_device):
    """n_logits > 3072: the <0> form of the selection kernel (two passes over memory) with hotwords; TINY widened in vocabulary only"""
    cfg = TINY.with_(vocab_size=3100)
    assert cfg.n_logits > 64 * 48
    sd = synthetic_state_dict(cfg, 0)
    model = AsrModel(cfg, sd, SyntheticTokenizer(cfg.vocab_size), device="cuda:0")
    g = torch.Generator().manual_seed(33)
    B, Tp = 3, 8
    f = (torch.randn((B, Tp, cfg.joint_hidden), generator=g) * 0.9).numpy()
    lens = np.asarray([8, 5, 7], np.int32)
    plain = AR.alsd_checker(cfg, sd, f, lens, beam=2, max_target_len=1.0)
    phrases = [(tuple(r["ids"][:2]), 2.0) for r in plain if len(r["ids"]) >= 2]
    phrases += [(tuple(y[-2:]) + (7,), 1.5) for r in plain for y, *_ in r["beam"] if len(y) >= 2]
    assert phrases, "the fixture must emit labels"
    got, want = check(model, sd, f, lens, [kh.build_graph(phrases)], [0, -1, 0], beam=2, max_target_len=1.0)
    print("wide vocabulary:", {k: sum(w[k] for w in want) for k in AR.COUNTERS})
    assert sum(w["child_hits"] for w in want) > 0
    assert got[1] == device_search(model, f, lens, 2, max_target_len=1.0, plain=True)[1]


def test_no_graph_is_the_plain_search(tiny, toy):
    model, _ = tiny
    f, lens, graphs = toy
    hw = _HotwordSet(graphs, model.device)
    for beam in (2, 4):
        plain = device_search(model, f, lens, beam, plain=True)
        assert device_search(model, f, lens, beam, hw=None, graph_of=None) == plain            # a null table
        assert device_search(model, f, lens, beam, hw=None, graph_of=GRAPH_OF) == plain
        assert device_search(model, f, lens, beam, hw=hw, graph_of=None) == plain              # no graph_of
        assert device_search(model, f, lens, beam, hw=hw, graph_of=[-1] * 7) == plain          # the hotword form, nobody has a graph


def test_alone_equals_inside_a_ragged_batch(tiny, toy):
    model, _ = tiny
    f, lens, graphs = toy
    hw = _HotwordSet(graphs, model.device)
    together = device_search(model, f, lens, 4, hw=hw, graph_of=GRAPH_OF)
    for b in (0, 1, 3):
        one = _HotwordSet([graphs[GRAPH_OF[b]]], model.device)
        alone = device_search(model, f[b:b + 1, :lens[b]], lens[b:b + 1], 4, hw=one, graph_of=[0])
        assert alone[0] == together[b], b


def test_through_the_nemo_package(gpu_device):
    from reazonspeech_amd.nemo.asr import TranscribeConfig, audio_from_numpy, load_model, transcribe, transcribe_batch
    conf = TranscribeConfig(verbose=False)
    plain_model = load_model(device="cuda:0", config=TINY, decoding="alsd", beam_size=4)
    audio, lens = synthetic_batch(9, 2.0, seed=50, ragged=True, min_seconds=0.5)
    audios = [audio_from_numpy(audio[b, :lens[b]], 16000) for b in range(9)]
    waves = [np.ascontiguousarray(a.waveform, dtype=np.float32) for a in audios]
    base = transcribe_batch(plain_model, audios, conf)
    dec = plain_model.transcribe_waveforms(waves)
    # hotwords as token ids, cut from what the plain search says: the first labels of some results and one frequent label
    spec_a = [(tuple(ids[:2]), 4.0) for ids in dec.ids if len(ids) >= 2][:4]
    flat = [t for ids in dec.ids for t in ids]
    spec_b = [((max(set(flat), key=flat.count),), 4.0)]
    model = load_model(device="cuda:0", config=TINY, decoding="alsd", beam_size=4, hotwords=spec_a)
    assert model.hotwords is not None and model.hotwords.n_phrases == len(spec_a) and plain_model.hotwords is None
    res = transcribe_batch(model, audios, conf)
    text = lambda rs: [r.text for r in rs]                                 # noqa: E731
    assert text(res) != text(base), "the model's hotwords must change a transcript: re-choose the phrases"
    for b in (0, 4):                                                       # transcribe == the transcribe_batch row
        one = transcribe(model, audios[b], conf)
        assert one.text == res[b].text and [s.seconds for s in one.subwords] == [s.seconds for s in res[b].subwords]
    # the runtime's results are the checker's on the device's projection, with the model's graph on every row
    sd = synthetic_state_dict(TINY, 0)
    plan = model.graph_plan([model.hotwords] * 9, 9)
    buf = model.stage(waves, buf=model.new_buffers(9, max(len(w) for w in waves)), hotwords=plan)
    model.token_scores = True
    model.run_device(buf)
    torch.cuda.synchronize()
    got = model.collect(buf)
    model.token_scores = False
    want = AR.alsd_checker(TINY, sd, buf.joint_enc.cpu().numpy(), np.asarray(got.enc_lens, np.int32), kh.concat([model.hotwords]), [0] * 9,
                         beam=4, max_target_len=TINY.alsd_max_target_len)
    assert got.ids == [w["ids"] for w in want] and got.frames == [[i - u for u, i in enumerate(w["steps"])] for w in want]
    assert [np.float32(s) for s in got.scores] == [np.float32(w["score"]) for w in want]
    assert [model.tokenizer.ids_to_text(ids) for ids in got.ids] == text(res)
    assert any(w["child_hits"] for w in want) and got.ids != dec.ids
    # token scores stay the model's own distribution, bonus or not: the token score checker's bits on the biased result
    u_cap = max(1, max(len(y) for y in got.ids))
    ids_m, n_m = TS.pack(got.ids, u_cap)
    logp, _ = TS.scores_checker(TINY, sd, buf.joint_enc.cpu().numpy(), np.asarray(got.enc_lens, np.int32), ids_m, TS.pack(got.frames, u_cap)[0], n_m)
    assert [[AR.bits(v) for v in lp] for lp in got.token_logprobs] == [[AR.bits(v) for v in logp[b, :n_m[b]]] for b in range(9)]
    # per-audio hotwords: None = the model's graph, a specification = that graph instead of it; a string applies to all
    per = [None, spec_b, None, spec_b, spec_a, None, spec_b, None, spec_b]
    mixed = transcribe_batch(model, audios, conf, hotwords=per)
    only_b = transcribe_batch(plain_model, audios, conf, hotwords=[spec_b] * 9)
    assert text(mixed) == [(only_b if per[b] is spec_b else res)[b].text for b in range(9)]
    assert transcribe(model, audios[3], conf, hotwords=spec_b).text == only_b[3].text
    piece = model.tokenizer.pieces[spec_b[0][0][0]]
    if model.tokenizer.text_to_ids(piece) == [spec_b[0][0]]:
        assert text(transcribe_batch(plain_model, audios, conf, hotwords=piece + " :4.0")) == text(only_b)
    # a list longer than max_batch goes through the host pipeline: the graph index follows its utterance through sorting and grouping
    graphs = [kh.build_graph(spec_b) if b % 2 else (model.hotwords if b % 3 else None) for b in range(9)]
    whole = model.transcribe_waveforms(waves, hotwords=graphs)
    parts = model.transcribe_waveforms(waves, max_batch=4, hotwords=graphs)
    assert (whole.ids, whole.frames, whole.scores) == (parts.ids, parts.frames, parts.scores)
    assert whole.ids != dec.ids
    # rows the hotwords did not change report what a run without hotwords reports
    first2 = tuple(next(ids for ids in dec.ids if len(ids) >= 2)[:2])
    spec_c = [(first2, 4.0)]
    plain_model.token_scores = True
    a = plain_model.transcribe_waveforms(waves)
    c = plain_model.transcribe_waveforms(waves, hotwords=[kh.build_graph(spec_c) if k % 2 == 0 else None for k in range(9)])
    kept = [k for k in range(9) if a.ids[k] == c.ids[k] and a.frames[k] == c.frames[k] and a.ids[k]]
    assert kept and a.ids != c.ids, "some rows must keep their labels and some must change: re-choose the phrase"
    for k in kept:
        assert [AR.bits(v) for v in a.token_logprobs[k]] == [AR.bits(v) for v in c.token_logprobs[k]], k
    # and through the package: a model loaded with hotwords and token_scores reports the same numbers as the runtime
    c = plain_model.transcribe_waveforms(waves, hotwords=[kh.build_graph(spec_c)] * 9)
    plain_model.token_scores = False
    scored = transcribe_batch(load_model(device="cuda:0", config=TINY, decoding="alsd", beam_size=4, hotwords=spec_c, token_scores=True), audios, conf)
    assert [[float(v) for v in r.token_logprobs] for r in scored] == [[float(v) for v in lp] for lp in c.token_logprobs]


def test_errors(tiny, toy):
    from reazonspeech_amd.nemo.asr import load_model
    model, _ = tiny
    f, lens, graphs = toy
    dev = model.device
    hw = _HotwordSet(graphs, dev)
    z = lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)          # noqa: E731
    k2 = capi.Context(ZIPFORMER_TINY, 0)
    try:
        with pytest.raises(RuntimeError):
            k2.alsd_workspace_bytes(2, 4, 10, 1.0, hotwords=True)
        with pytest.raises(capi.RsError, match="not defined for a Zipformer context") as e:
            k2.rnnt_alsd(torch.zeros((2, 10, TINY.joint_hidden), device=dev), z(2) + 10, 2, 10, 4, 1.0, True, False, z(2, 20), z(2, 20),
                         z(2), torch.zeros((2,), device=dev), torch.empty((1 << 20,), dtype=torch.uint8, device=dev), 0, hotwords=hw.struct, graph_of=z(2))
        assert e.value.code == capi.RS_EINVAL
    finally:
        k2.close()
    # the arguments rs_rnnt_alsd rejects, and a table with a negative count
    with pytest.raises(capi.RsError) as e:
        device_search(model, f, lens, 9, hw=hw, graph_of=GRAPH_OF)
    assert e.value.code == capi.RS_EINVAL
    broken = capi.RsHotwords.from_buffer_copy(hw.struct)
    broken.n_children = -1
    with pytest.raises(capi.RsError, match="hotwords") as e:
        device_search(model, f, lens, 4, hw=types.SimpleNamespace(struct=broken), graph_of=GRAPH_OF)
    assert e.value.code == capi.RS_EINVAL
    # a table that fails the check never reaches the device: _HotwordSet raises before it uploads anything
    bad = kh.build_graph([((5, 6, 7), 2.0), ((6, 7), 1.5)])
    bad.arrays["fail"][2] = 2                                              # a fail link that does not lower the level
    with pytest.raises(capi.RsError, match="does not lower the level") as e:
        _HotwordSet([bad], dev)
    assert e.value.code == capi.RS_EINVAL
    with pytest.raises(ValueError, match="alsd"):                          # greedy refuses hotwords at every entrance
        load_model(device="cuda:0", config=TINY, decoding="greedy_batch", hotwords=[(5, 6)])
    with pytest.raises(ValueError, match="alsd"):
        model.transcribe_waveforms([np.zeros(16000, np.float32)], hotwords=[graphs[0]])
