"""CPU: hotwords and n-gram LM fusion in ESPnet's default beam search (rs_rnnt_beam_lm, csrc/k_rnnt_beam.hip; the rule is stated in
include/rs_asr.h): the C checker that restates the search in all its forms (tests/espnet_beam_lm_checker.c)

  * without a graph and without an LM — and again with a table present at alpha = 0 — against the two existing checkers, bit for
    bit: oracle/espnet_beam.c for nbest = 0 and tests/espnet_beam_nbest_checker.c for nbest >= 1, on the toy geometry (ESPNET_TINY,
    24, 17, 1, 9 and 0 frames; beam 1, 2, 4, 8; score norm on and off);
  * against an independent float64 restatement of upstream's loop with the LM term (tests/espnet_beam_lm_ref.py beam_lm_float64, over
    a dictionary backoff and a pointer graph): the labels of every row, none skipped; seed, blank bias and alpha of the toy are
    chosen so that this holds;
  * that the comparison shows something: at every beam >= 2 the LM changes an utterance's ids, and so do the graphs;
  * hand-built edges on a joint that is its bias alone, each shown reached by the checker's counters or by the result;
  * the host plumbing: the ARPA "pieces" mapping onto an ESPnet token list, phrase encoding, keyword validation with the greedy
    search, and the fan-out of hotwords over windows and recordings (the pooled long-form plan included)."""
import ctypes
import os
import types
import warnings

import numpy as np
import importlib

import pytest

import espnet_beam_lm_ref as BL
import espnet_beam_nbest_ref as EB
import k2_hotwords_ref as H
import ngram_lm_ref as NR
from oracle import greedy as og
from reazonspeech_amd import build as rs_build
from reazonspeech_amd.espnet.asr import load_model
from reazonspeech_amd.espnet.asr import model as em
from reazonspeech_amd.espnet.asr.interface import AudioData
from reazonspeech_amd.espnet.asr.model import EspnetModel, synthetic_token_list
from reazonspeech_amd.runtime import capi, fusion, k2_hotwords as kh, ngram_lm as NL
from reazonspeech_amd.runtime.config import ESPNET_TINY

tr = importlib.import_module("reazonspeech_amd.espnet.asr.transcribe")       # (the package exports a function of the same name)
LINE = 1e-4                                   # |float32 - float64| <= LINE x max(1, |score|): the line of tests/test_oracle_espnet_beam.py
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BEAMS = (1, 2, 4, 8)
N_HOST = 5                                    # the host tests search rows 24, 17, 1, 9 and 0 frames of the toy


@pytest.fixture(scope="module")
def toy():
    return BL.toy()


def host_rows(toy):
    return toy["cfg"], toy["sd"], toy["f"][:N_HOST], toy["lens"][:N_HOST]


def test_without_terms_it_is_the_existing_checkers_bit_for_bit(toy):
    cfg, sd, f, lens = host_rows(toy)
    assert lens.tolist() == [24, 17, 1, 9, 0]
    for beam in BEAMS:
        for score_norm in (True, False):
            # "none": no table at all; "alpha 0": the LM and the graphs' table present, but alpha = 0 and no utterance has a graph
            forms = (dict(), dict(lm=toy["lm"], alpha=0.0, table=toy["table"], graph_of=[-1] * N_HOST), dict(lm=toy["lm"], alpha=0.0))
            want = og.espnet_beam(cfg, sd, f, lens, beam=beam, score_norm=score_norm, max_pops=16 * beam, with_frames=True)
            for kw in forms:
                got = BL.lm_checker(cfg, sd, f, lens, 0, beam=beam, score_norm=score_norm, **kw)
                for b, (g, w) in enumerate(zip(got, want)):
                    assert g["entries"][0][:3] == (w[0], w[1], EB.bits(w[2])) and g["pops"] == w[3], (beam, score_norm, b)
                    assert g["walks"] == 0 and g["child_hits"] + g["fail_transitions"] == 0
            for nbest in sorted({1, 2, beam} - {n for n in (2,) if n > beam}):
                lists = EB.nbest_checker(cfg, sd, f, lens, nbest, beam=beam, score_norm=score_norm, max_pops=16 * beam)
                for kw in forms:
                    got = BL.lm_checker(cfg, sd, f, lens, nbest, beam=beam, score_norm=score_norm, **kw)
                    for b, (g, w) in enumerate(zip(got, lists)):
                        assert g["entries"] == w["entries"] and g["n_ids"] == w["n_ids"] and g["pops"] == w["pops"], (beam, nbest, score_norm, b)
                        assert [g[k] for k in ("kept", "duplicates", "ties", "norm_reorders")] == [w[k] for k in ("kept", "duplicates", "ties", "norm_reorders")]
    assert got[4]["entries"] == [([], [], 0, 0)] and got[4]["kept"] == 1              # no frames: the start hypothesis alone


def test_labels_equal_the_float64_restatement_on_every_row(toy):
    cfg, sd, f, lens = host_rows(toy)
    deviation, rows, least_gap = 0.0, 0, np.inf
    for beam in BEAMS:
        N = min(beam, 8)
        for form in ("lm", "graphs", "both"):
            kw, kw64 = {}, {}
            if form != "graphs":
                kw.update(lm=toy["lm"], alpha=BL.TOY_ALPHA)
                kw64.update(arpa=toy["arpa"], alpha=BL.TOY_ALPHA)
            if form != "lm":
                kw.update(table=toy["table"], graph_of=BL.TOY_GRAPH_OF[:N_HOST])
            got = BL.lm_checker(cfg, sd, f, lens, N, beam=beam, max_pops=64 * beam, **kw)
            for b in range(N_HOST):
                gi = BL.TOY_GRAPH_OF[b] if form != "lm" else -1
                graph = H.ContextGraph(toy["phrases"][gi]) if gi >= 0 else None
                want, gap = BL.beam_lm_float64(EB.model_logp_fn(cfg, sd, f[b]), int(lens[b]), cfg.n_logits, cfg.blank_id, beam=beam, graph=graph,
                                               nbest=N, **kw64)
                ent = got[b]["entries"]
                assert [e[0] for e in ent] == [w[0] for w in want], (beam, form, b, gap)          # every row: none is skipped for a near-tie
                for e, w in zip(ent, want):
                    assert abs(EB.f32(e[2]) - w[1]) <= LINE * max(1.0, abs(w[1])) and abs(EB.f32(e[3]) - w[2]) <= LINE * max(1.0, abs(w[2])), (beam, form, b)
                    deviation = max(deviation, abs(EB.f32(e[2]) - w[1]))
                rows += 1
                least_gap = min(least_gap, gap)
    print(f"{rows} rows; largest |float32 - float64| score {deviation:.3e}; least distance between two compared float64 scores {least_gap:.3e}")
    assert rows == len(BEAMS) * 3 * N_HOST


def test_the_comparison_shows_something(toy):
    cfg, sd, f, lens = host_rows(toy)
    order = toy["lm"].order
    assert order == 3 and toy["lm"].start != 0
    open_at_the_end = 0
    for beam in BEAMS:
        plain = BL.lm_checker(cfg, sd, f, lens, 0, beam=beam)
        with_lm = BL.lm_checker(cfg, sd, f, lens, 0, beam=beam, max_pops=64 * beam, lm=toy["lm"], alpha=BL.TOY_ALPHA)
        with_hw = BL.lm_checker(cfg, sd, f, lens, 0, beam=beam, max_pops=64 * beam, table=toy["table"], graph_of=BL.TOY_GRAPH_OF[:N_HOST])
        differ_lm = [b for b in range(N_HOST) if with_lm[b]["entries"][0][0] != plain[b]["entries"][0][0]]
        differ_hw = [b for b in range(N_HOST) if with_hw[b]["entries"][0][0] != plain[b]["entries"][0][0]]
        print(f"beam {beam}: rows whose ids differ with the LM {differ_lm}, with the graphs {differ_hw}")
        if beam >= 2:
            assert differ_lm and differ_hw, "re-choose the toy (tests/espnet_beam_lm_ref.py TOY_SEED, TOY_BIAS, TOY_ALPHA)"
        # a row without a graph inside a hotword call is the plain search, bits and pops
        for b in range(N_HOST):
            if BL.TOY_GRAPH_OF[b] < 0:
                assert with_hw[b]["entries"] == plain[b]["entries"] and with_hw[b]["pops"] == plain[b]["pops"]
        # the LM is met at every level: hits at levels 1..3, backoffs, unknown labels, full-order pops; the graphs: hits, fail links, exits
        if beam >= 2:
            hits = [sum(r["hits"][k] for r in with_lm) for k in range(1, order + 1)]
            assert all(h > 0 for h in hits) and all(sum(r[k] for r in with_lm) > 0 for k in ("backoffs", "unk", "full_order_pops"))
            assert all(sum(r[k] for r in with_hw) > 0 for k in ("child_hits", "fail_transitions", "exits"))
        open_at_the_end += sum(r["finalize"] < 0 for r in with_hw)
    assert open_at_the_end > 0                                             # Finalize took a bonus back somewhere


def test_a_shorter_list_is_a_prefix_and_nbest_0_is_entry_0(toy):
    cfg, sd, f, lens = host_rows(toy)
    kw = dict(lm=toy["lm"], alpha=BL.TOY_ALPHA, table=toy["table"], graph_of=BL.TOY_GRAPH_OF[:N_HOST])
    for beam, score_norm in ((4, True), (8, False)):
        full = BL.lm_checker(cfg, sd, f, lens, beam, beam=beam, score_norm=score_norm, max_pops=64 * beam, **kw)
        for nbest in (0, 1, 2):
            part = BL.lm_checker(cfg, sd, f, lens, nbest, beam=beam, score_norm=score_norm, max_pops=64 * beam, **kw)
            for p, w in zip(part, full):
                assert p["entries"] == w["entries"][:max(nbest, 1)] and p["pops"] == w["pops"], (beam, nbest)


# ---- the hand-built edges ---------------------------------------------------------------------------------------------------------
def labels(r):
    return [e[0] for e in r["entries"]]


def float64_of(name):
    """the float64 restatement on a case of BL.EDGES -> its ranked list"""
    case = BL.EDGES[name]
    cfg = ESPNET_TINY
    lp = BL.flat_logp(case.get("probs", BL.EDGE_PROBS), cfg)
    arpa = None
    if case.get("lm"):
        lm = NL.build(case["lm"], cfg.n_logits, cfg.blank_id)
        arpa = NR.ArpaDict(case["lm"], lm.order, min(p for k, (p, _) in case["lm"].items() if len(k) == 1))
    graph = H.ContextGraph(case["phrases"]) if case.get("phrases") else None
    return BL.beam_lm_float64(lambda t, y: lp, case["T"], cfg.n_logits, cfg.blank_id, beam=case["beam"], arpa=arpa, alpha=case.get("alpha", 0.0),
                              bos=False, graph=graph, nbest=case["nbest"])[0]


@pytest.mark.parametrize("name", sorted(BL.EDGES))
def test_every_edge_equals_the_float64_restatement(name):
    got, want = BL.run_edge(name), float64_of(name)
    assert labels(got) == [w[0] for w in want], name
    for e, w in zip(got["entries"], want):
        assert abs(EB.f32(e[2]) - w[1]) <= 1e-5 and abs(EB.f32(e[3]) - w[2]) <= 1e-5, (name, e, w)


def test_an_lm_that_changes_the_winner():
    with_lm, plain = BL.run_edge("lm_changes_the_winner"), BL.run_edge("lm_changes_the_winner", with_terms=False)
    assert labels(plain)[0] == [BL.A] and labels(with_lm)[0] == [BL.B]
    assert with_lm["walks"] > 0 and plain["walks"] == 0


def test_an_lm_whose_backoff_path_and_unk_path_are_both_taken():
    r = BL.run_edge("lm_backoff_and_unk")
    assert r["backoffs"] > 0 and r["unk"] > 0 and r["hits"][2] > 0 and r["full_order_pops"] > 0      # the edges are reached
    assert r["hits"][1] + r["hits"][2] + r["unk"] == r["walks"]


def test_an_lm_of_order_1():
    r = BL.run_edge("lm_order_1")
    assert r["walks"] > 0 and r["hits"][1] == r["walks"] == r["full_order_pops"] and r["backoffs"] == 0   # every hit is a full-order pop to the root
    assert labels(r) != labels(BL.run_edge("lm_order_1", with_terms=False))


def test_a_phrase_completed_keeps_its_bonus():
    r = BL.run_edge("phrase_completed")
    cfg = ESPNET_TINY
    lp = BL.flat_logp(BL.EDGE_PROBS, cfg)
    assert r["exits"] > 0 and labels(r)[0] == [BL.A, BL.B] != labels(BL.run_edge("phrase_completed", with_terms=False))[0]
    want = lp[BL.A] + lp[BL.B] + 2 * lp[cfg.blank_id] + 2 * 1.2            # two frames' blanks, both tokens' bonuses, nothing taken back
    assert abs(EB.f32(r["entries"][0][2]) - want) <= 1e-5


def test_a_phrase_begun_and_abandoned_loses_its_bonus():
    r, plain = BL.run_edge("phrase_abandoned"), BL.run_edge("phrase_abandoned", with_terms=False)
    # the edge is reached: steps that leave a begun phrase over its fail link (the counter counts exactly those), and no phrase is
    # ever completed — so no bonus may be left anywhere: every entry of the list scores what the float64 search WITHOUT a graph gives
    # its label sequence (and test_every_edge_equals_the_float64_restatement holds the list to the search with the graph)
    assert r["fail_transitions"] > 0 and r["exits"] == 0 and r["child_hits"] > 0
    lp = BL.flat_logp(BL.EDGE_PROBS, ESPNET_TINY)
    for ids, _, sb, _ in r["entries"]:
        assert abs(EB.f32(sb) - (sum(lp[v] for v in ids) + 2 * lp[ESPNET_TINY.blank_id])) <= 1e-5, ids
    assert labels(r) != labels(plain)                                       # the bonus, while it lasted, moved the search


def test_a_phrase_left_open_at_the_last_frame_is_cancelled_by_finalize():
    r = BL.run_edge("phrase_open_at_the_end")
    assert r["finalize"] < 0 and r["finalize_reorders"] == 1               # the edge is reached: Finalize changes the n-best order
    assert labels(r) == [[], [BL.A]]
    e = r["entries"][1]
    assert e[3] == EB.bits(np.float32(EB.f32(e[2])) / np.float32(2))       # the norm is formed after Finalize


def test_overlapping_phrases():
    r = BL.run_edge("overlapping_phrases")
    assert r["exits"] > 0 and r["fail_transitions"] > 0 and r["child_hits"] > 0
    assert labels(r) != labels(BL.run_edge("overlapping_phrases", with_terms=False))


def test_a_bonus_makes_a_frame_take_more_pops_and_a_small_max_pops_overflows():
    r, plain = BL.run_edge("more_pops"), BL.run_edge("more_pops", with_terms=False)
    assert r["pops"] > 2 * plain["pops"]
    assert BL.run_edge("more_pops", with_terms=False, max_pops=8)["pops"] == plain["pops"]       # the plain search fits 8 pops a frame
    with pytest.raises(RuntimeError, match="-5"):
        BL.run_edge("more_pops", max_pops=8)


def test_a_tie_between_two_extensions_after_their_terms_is_resolved_by_position():
    r, plain = BL.run_edge("tie_after_the_terms"), BL.run_edge("tie_after_the_terms", with_terms=False)
    assert plain["pop_ties"] == 0 and r["pop_ties"] == 1                   # the edge is reached: the bonus lifts B onto A, bit for bit
    assert labels(r) == [[], [BL.A]] and r["pops"] == plain["pops"] + 1     # A, opened first, is popped first; B's pop ends the frame


# ---- host plumbing ----------------------------------------------------------------------------------------------------------------
TOKENS = ["<blank>", "<unk>", "あ", "い", "う", "<space>", "え", "<sos/eos>"]


def model_lm(cfg, token_list, *keywords):
    """(the shared function asks the configuration for its search first: the stand-ins below name the fusing one)"""
    return fusion.model_lm(fusion.ESPNET, cfg, token_list, *keywords)


def test_arpa_pieces_map_onto_an_espnet_token_list(tmp_path):
    cfg = types.SimpleNamespace(vocab_size=len(TOKENS), n_logits=len(TOKENS), blank_id=0, decoding="beam")
    ent = {("<s>",): (-99.0, -0.25), ("あ",): (-0.5, -0.125), ("い",): (-0.75, 0.0), ("<space>",): (-1.0, -0.125), ("<unk>",): (-2.0, None),
           ("<sos/eos>",): (-1.5, 0.0), ("</s>",): (-1.25, None), ("<s>", "あ"): (-0.25, 0.0), ("あ", "<space>"): (-0.125, 0.0),
           ("<space>", "い"): (-0.375, None)}
    path = NR.write_arpa(str(tmp_path / "toy.arpa"), ent, order=2)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        lm = model_lm(cfg, TOKENS, path)
    assert any("dropped" in str(x.message) for x in w)                     # </s> and <sos/eos> name no token
    assert lm.order == 2 and lm.n_logits == len(TOKENS) and lm.start != 0
    root = lm.arrays["root_child"]
    assert [int(root[i]) >= 0 for i in range(len(TOKENS))] == [False, False, True, True, False, True, False, False]
    assert abs(float(lm.unk_logp) - (-2.0 * np.log(10.0))) < 1e-5          # the file's <unk> is the unknown-word entry
    lp, state, _ = NR.step(lm, lm.start, 2)                                 # <s> あ
    assert abs(float(lp) - (-0.25 * np.log(10.0))) < 1e-5
    lp, state, _ = NR.step(lm, state, 5)                                    # あ <space>
    assert abs(float(lp) - (-0.125 * np.log(10.0))) < 1e-5
    lp, _, _ = NR.step(lm, state, 3)                                        # <space> い
    assert abs(float(lp) - (-0.375 * np.log(10.0))) < 1e-5
    gz = NR.write_arpa(str(tmp_path / "toy.arpa.gz"), ent, order=2, gz=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert model_lm(cfg, TOKENS, gz).key == lm.key
        ids = model_lm(cfg, TOKENS, NR.write_arpa(str(tmp_path / "ids.arpa"), {(2,): (-0.5, 0.0), (5,): (-1.0, 0.0)}), "ids")
    assert int(ids.arrays["root_child"][5]) >= 0
    assert model_lm(cfg, TOKENS, lm) is lm
    with pytest.raises(ValueError, match="built for"):
        model_lm(types.SimpleNamespace(vocab_size=9, n_logits=9, blank_id=0, decoding="beam"), TOKENS + ["x"], lm)
    with pytest.raises(ValueError, match="ngram_lm_tokens"):
        model_lm(cfg, TOKENS, path, "nemo")
    kenlm = tmp_path / "lm.bin"
    kenlm.write_bytes(NL.KENLM_MAGIC + b"\0" * 64)
    with pytest.raises(ValueError):
        model_lm(cfg, TOKENS, str(kenlm))


def test_phrases_are_encoded_per_character():
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        enc = em.encode_phrases(kh.parse_hotwords(["あい", "あ い :2.5", "あお", "  "]), TOKENS, 0, 1.5)
    assert enc == [((2, 3), 1.5), ((2, 5, 3), 2.5)]                        # whitespace is <space>; "あお" is skipped
    assert sum("skipped" in str(x.message) and "お" in str(x.message) for x in w) == 1
    no_space = [t for t in TOKENS if t != "<space>"]
    assert em.encode_phrases(kh.parse_hotwords("あ い/う"), no_space, 0, 1.0) == [((2, 3), 1.0), ((4,), 1.0)]     # ... dropped without one
    assert em.encode_phrases([((2, 3), 0.0)], TOKENS, 0, 1.5) == [((2, 3), 1.5)]
    with pytest.raises(ValueError, match="blank or <unk>"):
        em.encode_phrases([((1,), 0.0)], TOKENS, 0, 1.5)


def test_the_keywords_need_the_beam_search():
    toks = synthetic_token_list(ESPNET_TINY.vocab_size)
    lm = NL.build({(10,): (-0.5, 0.0)}, ESPNET_TINY.n_logits, ESPNET_TINY.blank_id)
    for call in (lambda **kw: load_model(device="cuda:0", config=ESPNET_TINY, **kw), lambda **kw: EspnetModel(ESPNET_TINY, {}, toks, **kw)):
        with pytest.raises(ValueError, match="an n-gram LM needs the beam search"):       # before anything is loaded
            call(ngram_lm_model=lm)
        with pytest.raises(ValueError, match="an n-gram LM needs the beam search"):
            call(ngram_lm_model="lm.arpa", beam_size=1)
        with pytest.raises(ValueError, match="hotwords need the beam search"):
            call(hotwords_file="hot.txt")
        with pytest.raises(ValueError, match="ngram_lm_alpha must be a finite number >= 0"):
            call(beam_size=4, ngram_lm_alpha=-1.0)
        with pytest.raises(ValueError, match="ngram_lm_tokens"):
            call(beam_size=4, ngram_lm_tokens="nemo")
        with pytest.raises(ValueError, match="hotwords_score"):
            call(beam_size=4, hotwords_score=float("nan"))
    em.check_fusion_keywords(4, lm, 0.3, "ids", "hot.txt", 2.0)
    em.check_fusion_keywords(1)                                            # nothing asked for: the greedy search is fine
    greedy = EspnetModel.__new__(EspnetModel)
    greedy.cfg, greedy.token_list = ESPNET_TINY, toks
    with pytest.raises(ValueError, match="hotwords need the beam search"):
        greedy.hotword_graph([(10, 11)])
    assert greedy.hotword_graph(None) is None and greedy.call_graphs(None, 3) is None


class _Recorder:
    """an EspnetModel whose search is replaced by a recorder: what reaches `_search` for every call"""

    def __init__(self):
        m = EspnetModel.__new__(EspnetModel)
        m.cfg = ESPNET_TINY.with_(decoding="beam", beam_size=4)
        m.token_list, m.beam_size = synthetic_token_list(ESPNET_TINY.vocab_size), 4
        m.am = types.SimpleNamespace(nbest=0, ngram_lm=NL.build({(10,): (-0.5, 0.0)}, ESPNET_TINY.n_logits, 0), ngram_lm_alpha=0.3, token_scores=False)
        self.calls = []

        def search(waves, **kw):
            from reazonspeech_amd.runtime.model import DecodedBatch
            self.calls.append((len(waves), kw.get("hotwords"), kw.get("ngram_lm")))
            return DecodedBatch([[10]] * len(waves), [[0]] * len(waves), [1] * len(waves), [0.0] * len(waves), [False] * len(waves))
        m._search = search
        self.model = m


def test_hotwords_fan_out_per_window():
    rec = _Recorder()
    m = rec.model
    wave = np.zeros(100, np.float32)
    m(wave)
    assert rec.calls[-1] == (1, None, None)                                 # nothing given: the model's own, and it has no graph
    m(wave, hotwords=[(10, 11)], ngram_lm_alpha=0)
    n, graphs, lm = rec.calls[-1]
    assert graphs[0].key == (((10, 11), 1.5),) and lm == (m.am.ngram_lm, 0.0)
    m.hotwords = m.hotword_graph([(12,)])
    m.recognize_batch([wave] * 3, hotwords=[None, [(10, 11), (13,)], None], ngram_lm_alpha=0.7)
    n, graphs, lm = rec.calls[-1]
    assert n == 3 and [g.n_phrases for g in graphs] == [1, 2, 1] and graphs[0] is m.hotwords and lm[1] == 0.7     # None = the model's own
    tok = m.token_list
    m.recognize_batch([wave] * 2, hotwords=tok[10] + tok[11] + "/" + tok[12] + " :3")       # a string: one spec for every window
    n, graphs, lm = rec.calls[-1]
    assert graphs[0] is graphs[1] and graphs[0].key == (((10, 11), 1.5), ((12,), 3.0)) and lm is None
    with pytest.raises(ValueError, match="2 entries for 3 windows"):
        m.recognize_batch([wave] * 3, hotwords=[None, None])
    m.am.ngram_lm = None
    with pytest.raises(ValueError, match="the model has no n-gram LM"):
        m(wave, ngram_lm_alpha=0.5)
    assert m.call_lm(0) == (None, 0.0)


def test_hotwords_fan_out_per_recording_also_on_the_pooled_path():
    import espnet_fake
    seen = []

    class Fake(espnet_fake.FakeEspnetModel):
        segmentation = "host"

        def __call__(self, speech, hotwords=None, ngram_lm_alpha=None):
            seen.append(("call", len(speech), hotwords, ngram_lm_alpha))
            return super().__call__(speech)

        def recognize_batch(self, waves, isolate_overflow=False, hotwords=None, ngram_lm_alpha=None):
            seen.append(("batch", [len(w) for w in waves], hotwords, ngram_lm_alpha))
            return [espnet_fake.text_of(np.asarray(w)) for w in waves]

    model = Fake()
    short = AudioData(espnet_fake.long_audio(3.0, seed=1), 16000)
    long_ = AudioData(espnet_fake.long_audio(45.0, seed=2), 16000)
    plain = tr.transcribe(model, long_)
    n_windows = len(seen)
    assert n_windows >= 3 and all(s[2] is None and s[3] is None for s in seen)            # nothing given: called as ever
    seen.clear()
    assert tr.transcribe(model, long_, hotwords="x/y", ngram_lm_alpha=0.0).text == plain.text
    assert len(seen) == n_windows and all(s[2:] == ("x/y", 0.0) for s in seen)            # every window of the recording
    # transcribe_batch, host segmentation: the short recordings as one batch with their own specs, the long one through transcribe
    seen.clear()
    tr.transcribe_batch(model, [short, long_, short], hotwords=["a", "b", None], ngram_lm_alpha=0.4)
    batch = [s for s in seen if s[0] == "batch"]
    assert len(batch) == 1 and batch[0][2] == ["a", None] and batch[0][3] == 0.4
    assert [s[2:] for s in seen if s[0] == "call"] == [("b", 0.4)] * n_windows
    with pytest.raises(ValueError, match="2 entries for 3 recordings"):
        tr.transcribe_batch(model, [short, long_, short], hotwords=["a", "b"])
    assert tr.per_recording("a/b", 2) == ["a/b", "a/b"] and tr.per_recording(None, 2) is None
    # the pooled long-form plan: every piece carries the spec of the recording it was cut from
    seen.clear()
    pooled = []

    class Pooled(Fake):
        segmentation = "device"

        def find_blank_batch(self, windows, threshold=0.98, max_batch=256):
            from reazonspeech_amd.espnet.asr.ctc import find_blank
            return [find_blank(self, w, threshold) for w in windows]

        def recognize_batch(self, waves, isolate_overflow=False, hotwords=None, ngram_lm_alpha=None):
            pooled.append(([len(w) for w in waves], hotwords, ngram_lm_alpha))
            return super().recognize_batch(waves, isolate_overflow, hotwords, ngram_lm_alpha)

        def blank_posteriors(self, samples):
            return self.ctc_posteriors(samples)[:, 0]

        def align_batch(self, waves, texts, max_batch=256):
            return [None] * len(waves)

    tr.transcribe_batch(Pooled(), [short, long_], hotwords=["a", "b"], ngram_lm_alpha=0.2)
    (sizes, specs, alpha), = pooled
    assert len(sizes) == 1 + n_windows and alpha == 0.2
    assert sorted(specs) == ["a"] + ["b"] * n_windows
    assert [spec for size, spec in zip(sizes, specs) if size == len(short.waveform)] == ["a"]


def test_the_entry_points_are_exported_declared_and_guarded():
    lib = ctypes.CDLL(rs_build.build())
    assert lib.rs_abi_version() == 7
    assert hasattr(lib, "rs_rnnt_beam_lm") and hasattr(lib, "rs_rnnt_beam_lm_workspace_bytes")          # fails without the feature
    assert {"rs_rnnt_beam_lm", "rs_rnnt_beam_lm_workspace_bytes"} <= set(capi.EXPORTS)
    loaded = capi.load()
    assert len(loaded.rs_rnnt_beam_lm.argtypes) == len(loaded.rs_rnnt_beam_nbest.argtypes) + 4           # hw, graph_of, lm, lm_alpha
    lib.rs_rnnt_beam_lm_workspace_bytes.restype = ctypes.c_size_t
    assert lib.rs_rnnt_beam_lm_workspace_bytes(None, 4, 4, 100, 0, 2) == 0                               # no context: invalid
    header = open(os.path.join(ROOT, "include", "rs_asr.h"), encoding="utf-8").read()
    assert "size_t rs_rnnt_beam_lm_workspace_bytes(const rs_ctx* ctx, int B, int beam, int tp_max, int max_pops, int nbest);" in header
    assert "int rs_rnnt_beam_lm(rs_ctx* ctx," in header and "[UPSTREAM, not vendored, UNVERIFIED] espnet2 BeamSearchTransducer.default_beam_search" in header
    family = open(os.path.join(ROOT, "reazonspeech_amd", "csrc", "rs_family.h"), encoding="utf-8").read()
    assert "X(rs_rnnt_beam_lm_workspace_bytes, C, FINAL, RS_HINT_LSTM_ONLY)" in family and "X(rs_rnnt_beam_lm, C, FINAL, RS_HINT_LSTM_ONLY)" in family
