"""CPU: hotwords (contextual biasing) of the NeMo family's ALSD beam search (rs_rnnt_alsd_hotwords, csrc/k_rnnt_alsd.hip; the
semantics are stated in include/rs_asr.h).  What needs no GPU:

  * the C checker (tests/alsd_checker.c) with an empty table, or with graph_of all -1, IS oracle/rnnt_alsd.c, bit for bit
  * the checker against a float64 Python restatement of the same rules on the toy geometry (the tolerance of
    tests/test_oracle_alsd.py for the plain pair)
  * hand-built cases on a five-entry vocabulary with injected logits: a boosted continuation overtakes in the ranking, an
    abandoned phrase gets its bonus taken back, Finalize changes the winner, recombined duplicates carry one state
  * the toy fixture of the GPU test exercises every counter and changes results (conditions on the inputs)
  * text_to_ids of both tokenizers, the phrase encoder, the keywords of the nemo package, the export list and the family rows"""
import ctypes
import math
import os
import re
import types
import warnings

import numpy as np
import pytest

import alsd_hotwords_ref as AR
import k2_hotwords_ref as KR
from oracle import greedy as og
from reazonspeech_amd.nemo.asr.transcribe import _call_graphs as per_audio
from reazonspeech_amd.runtime import capi, fusion, k2_hotwords, nemo_hotwords
from reazonspeech_amd.runtime.config import TINY
from reazonspeech_amd.runtime.tokenizer import SentencePieceTokenizer, SyntheticTokenizer
from reazonspeech_amd.runtime.weights import synthetic_state_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOY_SEED = 6


@pytest.fixture(scope="module")
def toy():
    """the GPU test's batch, the plain search at beam 4 and the three graphs cut from it"""
    sd = synthetic_state_dict(TINY, 0)
    f, lens = AR.toy_batch(TINY, seed=TOY_SEED)
    f, lens = f.numpy(), lens.numpy()
    plain = AR.alsd_checker(TINY, sd, f, lens, beam=4)
    graphs = AR.toy_graphs(plain)
    return sd, f, lens, graphs, AR.table_of(graphs)


# ---- without a graph the checker is the plain oracle ------------------------------------------------------------------------------
@pytest.mark.parametrize("beam,max_target_len,norm,merge", [(1, 1.0, False, False), (2, 1.0, True, True), (4, 2.0, True, False),
                                                            (4, 7, False, True), (8, 0.5, True, False), (8, 5, True, True)])
def test_checker_without_graph_is_the_plain_oracle(toy, beam, max_target_len, norm, merge):
    sd, f, lens, _, table = toy
    assert lens[2] == 0 and lens.max() == f.shape[1]
    ref = og.rnnt_alsd(TINY, sd, f, lens, beam=beam, max_target_len=max_target_len, score_norm=norm, recombine="merge" if merge else "upstream")
    kw = dict(beam=beam, max_target_len=max_target_len, score_norm=norm, merge=merge)
    for got in (AR.alsd_checker(TINY, sd, f, lens, **kw),                                           # an empty table
                AR.alsd_checker(TINY, sd, f, lens, table, [-1] * len(lens), **kw)):                 # a table nobody points at
        for b, (g, r) in enumerate(zip(got, ref)):
            assert g["ids"] == r[0] and g["steps"] == r[1], b
            assert AR.same_bits(g["score"], r[2]), (b, g["score"], r[2])
            assert all(g[k] == 0 for k in AR.COUNTERS[:4]) and g["finalize"] == 0.0
    assert ref[2] == ([], [], 0.0) and sum(len(r[0]) for r in ref) > 20


# ---- the checker against float64 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beam,mode,norm", [(1, "upstream", False), (2, "merge", True), (4, "upstream", True), (4, "merge", False)])
def test_checker_matches_float64_restatement(toy, beam, mode, norm):
    """same decisions as the float64 restatement (AR.hw_float64): labels, alignment steps and the score of the winner within the
    tolerance tests/test_oracle_alsd.py holds for the plain pair"""
    import torch
    sd, f, lens, graphs, table = toy
    rows, graph_of = [0, 1, 3, 6], [0, 1, 2, 0]
    got = AR.alsd_checker(TINY, sd, f[rows], lens[rows], table, graph_of, beam=beam, max_target_len=1.0, score_norm=norm, merge=mode == "merge")
    plain = AR.alsd_checker(TINY, sd, f[rows], lens[rows], beam=beam, max_target_len=1.0, score_norm=norm, merge=mode == "merge")
    n_tok = 0
    for k, b in enumerate(rows):
        graph = KR.ContextGraph(graphs[graph_of[k]])
        ids, steps, score = AR.hw_float64(TINY, sd, torch.from_numpy(f[b]), int(lens[b]), graph, beam=beam, max_target_len=1.0,
                                          score_norm=norm, recombine=mode)
        assert got[k]["ids"] == ids and got[k]["steps"] == steps, (b, got[k]["ids"], ids)
        assert abs(got[k]["score"] - score) < 1e-3 * max(1.0, abs(score)), (b, got[k]["score"], score)
        n_tok += len(ids)
    assert n_tok > 6, "degenerate fixture"
    assert sum(g["child_hits"] for g in got) > 0
    assert beam == 1 or any(g["score"] != p["score"] for g, p in zip(got, plain)), "the graphs changed nothing: re-choose the inputs"


# ---- hand-built cases: a vocabulary of four labels and the blank, injected logits -------------------------------------------------
V, BLANK = 5, 4
LOW = -30.0


def logits(T):
    """inject [T][V][V], every entry LOW; rows are filled in by the cases: inject[t][last label + 1][v]"""
    return np.full((T, V, V), LOW, np.float32)


def lsm(row):
    row = np.asarray(row, np.float64)
    return row - (row.max() + math.log(np.exp(row - row.max()).sum()))


def run(z, T, phrases, beam, budget, norm=False, merge=False):
    table = AR.table_of([phrases]) if phrases else None
    return AR.alsd_checker(None, None, None, [T], table, [0] if phrases else None, beam=beam, max_target_len=int(budget), score_norm=norm,
                         merge=merge, inject=z, dims=(V, BLANK))[0]


def test_a_boosted_continuation_overtakes_in_the_ranking():
    """beam 1: the blank has the better log-probability, label 0 is the hypothesis's best label.  The bonus is part of the ranking,
    so with the phrase (0,) the label is kept; sherpa-onnx's rule (select first, add the bonus afterwards) would keep the blank, as
    the plain search does"""
    z = logits(1)
    z[0, 0, BLANK], z[0, 0, 0] = 2.0, 1.0
    z[0, 1, BLANK], z[0, 1, 3] = 5.0, 0.0                  # after label 0: the blank (best label: 3, no part of a phrase)
    plain = run(z, 1, None, 1, 1)
    hot = run(z, 1, [((0,), 2.0)], 1, 1)
    assert plain["ids"] == [] and hot["ids"] == [0] and hot["steps"] == [0]
    want = lsm(z[0, 0])[0] + 2.0 + lsm(z[0, 1])[BLANK]
    assert abs(hot["score"] - want) < 1e-5 and hot["score"] > plain["score"]
    assert (hot["child_hits"], hot["exits"], hot["finalize"]) == (1, 1, 0.0)     # the phrase ended: the state is the root again


def test_an_abandoned_phrase_gets_its_bonus_taken_back():
    z = logits(1)
    z[0, 0, 0] = 10.0                                      # label 0, then label 2 (the phrase wants 1), then the blank
    z[0, 1, 2] = 10.0
    z[0, 3, BLANK], z[0, 3, 3] = 10.0, 0.0
    plain = run(z, 1, None, 1, 2)
    hot = run(z, 1, [((0, 1), 1.5)], 1, 2)
    assert plain["ids"] == hot["ids"] == [0, 2]
    assert (hot["child_hits"], hot["fail_transitions"], hot["exits"], hot["finalize"]) == (1, 1, 0, 0.0)
    assert abs(hot["score"] - plain["score"]) < 1e-5       # +1.5 at the first label, -1.5 at the second
    assert hot["beam"][0][2] == 0                          # back at the root


def test_finalize_changes_the_winner():
    """beam 2, no normalisation: [0] stands in the middle of the phrase (0, 1) with +2 when it finishes; Finalize takes the 2 back
    and the empty hypothesis, finished a step earlier, wins.  Without Finalize [0] would have won"""
    z = logits(1)
    z[0, 0, BLANK], z[0, 0, 0], z[0, 0, 2] = 1.0, 0.0, -1.0
    z[0, 1, BLANK] = 10.0
    hot = run(z, 1, [((0, 1), 2.0)], 2, 1)
    assert hot["ids"] == [] and hot["finalize"] == 0.0 and hot["finalized"] == 1
    pending = [e for e in hot["beam"] if e[0] == [0]]
    assert pending and pending[0][2] != 0 and pending[0][1] > hot["score"] > pending[0][1] - 2.0
    assert abs(hot["score"] - lsm(z[0, 0])[BLANK]) < 1e-5


@pytest.mark.parametrize("merge", [False, True])
def test_recombined_duplicates_carry_one_state(merge):
    """[0] is reached as (label, blank) and as (blank, label): equal labels, equal states by construction; the first stays"""
    z = logits(2)
    z[0, 0, BLANK], z[0, 0, 0] = 0.0, 0.0
    z[0, 1, BLANK] = 5.0
    z[1, 0, BLANK], z[1, 0, 0] = 0.0, 0.0
    z[1, 1, BLANK] = 5.0
    hot = run(z, 2, [((0, 1), 1.0)], 2, 1, merge=merge)
    assert hot["ids"] == [0] and hot["recombinations"] >= 1 and hot["state_mismatches"] == 0
    same = [e for e in hot["beam"] if e[0] == [0]]
    assert len(same) == (1 if merge else 2) and len({e[2] for e in same}) == 1 and same[0][2] != 0
    a = lsm(z[0, 0])[0] + 1.0 + lsm(z[0, 1])[BLANK]       # label at step 0, blank at step 1
    b = lsm(z[0, 0])[BLANK] + lsm(z[1, 0])[0] + 1.0       # blank at step 0, label at step 1
    last = lsm(z[1, 1])[BLANK]                             # the last blank; then Finalize takes the pending 1.0 back
    want = np.logaddexp(a, b) + last - 1.0                 # ("upstream" keeps the duplicate in the beam: it is added in once more)
    if not merge:
        want = np.logaddexp(np.logaddexp(a, b) + last, b + last) - 1.0
    assert abs(hot["score"] - want) < 1e-5 and hot["finalize"] == -1.0


# ---- the toy fixture: conditions on the inputs, decided by the checker alone ----------------------------------------------------------
TOY_CASES = [(1, 2.0, True, False), (2, 2.0, True, False), (4, 2.0, True, False), (8, 2.0, True, False),
             (4, 2.0, True, True), (4, 2.0, False, False), (4, 9, True, False)]


@pytest.mark.parametrize("beam,max_target_len,norm,merge", TOY_CASES)
def test_toy_fixture_exercises_the_graph(toy, beam, max_target_len, norm, merge):
    sd, f, lens, graphs, table = toy
    assert all(s * 2 == int(s * 2) for g in graphs for _, s in g)
    kw = dict(beam=beam, max_target_len=max_target_len, score_norm=norm, merge=merge)
    hot = AR.alsd_checker(TINY, sd, f, lens, table, AR.TOY_GRAPH_OF, **kw)
    plain = AR.alsd_checker(TINY, sd, f, lens, **kw)
    total = {k: sum(h[k] for h in hot) for k in AR.COUNTERS}
    assert all(total[k] > 0 for k in AR.COUNTERS[:4]) and total["state_mismatches"] == 0, f"re-choose the inputs: {total}"
    for b, g in enumerate(AR.TOY_GRAPH_OF):
        if g < 0:
            assert hot[b]["ids"] == plain[b]["ids"] and hot[b]["score_bits"] == plain[b]["score_bits"]
    assert beam < 2 or any(h["ids"] != p["ids"] for h, p in zip(hot, plain)), "re-choose the inputs: no row's labels changed"


# ---- tokenising phrases --------------------------------------------------------------------------------------------------------------
def _tiny_sentencepiece(tmp_path):
    import sentencepiece as spm
    corpus = tmp_path / "corpus.txt"
    words = ["こんにちは", "世界", "音声", "認識", "です", "ます", "。", "、", "東京", "大阪", "天気", "今日", "明日"]
    rng = np.random.default_rng(0)
    corpus.write_text("\n".join("".join(rng.choice(words, size=6)) for _ in range(400)), encoding="utf-8")
    prefix = str(tmp_path / "spm")
    spm.SentencePieceTrainer.train(input=str(corpus), model_prefix=prefix, vocab_size=63, model_type="unigram",
                                   character_coverage=1.0, minloglevel=2)
    return open(prefix + ".model", "rb").read()


def test_text_to_ids_sentencepiece(tmp_path):
    tok = SentencePieceTokenizer(_tiny_sentencepiece(tmp_path))
    sp = tok._sp
    readings = tok.text_to_ids("東京")
    assert readings[0] == tuple(sp.encode("東京")) and len(readings) == 2, readings
    first = sp.id_to_piece(readings[0][0])
    assert first.startswith("▁")
    # the second reading is the word as it stands in the middle of a sentence: the same text, no word-start mark
    assert "".join(sp.id_to_piece(i) for i in readings[1]) == "東京" and "▁" not in sp.id_to_piece(readings[1][0])
    inside = sp.encode("今日東京")
    assert any(tuple(inside[k:k + len(readings[1])]) == readings[1] for k in range(len(inside)))
    assert tok.text_to_ids("") == [] and tok.text_to_ids("zebra") == []           # nothing to spell / <unk>
    # both readings enter the graph with the phrase's score; an unencodable phrase is skipped with a warning naming it
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        enc = nemo_hotwords.encode(k2_hotwords.parse_hotwords("東京 :2.5/zebra/天気"), tok, tok.vocab_size, tok.vocab_size, 1.5)
    assert len([x for x in w if "hotwords" in str(x.message)]) == 1 and "'zebra'" in str(w[0].message)
    assert [e for e in enc if e[1] == 2.5] == [(readings[0], 2.5), (readings[1], 2.5)]
    assert {e[1] for e in enc} == {2.5, 1.5} and len(enc) == 4
    g = nemo_hotwords.make_graph(["東京 :2.5"], tok, tok.vocab_size, tok.vocab_size)
    assert g.n_phrases == 2 and g.key == tuple((r, 2.5) for r in readings)
    with pytest.warns(UserWarning, match="zebra"):
        assert nemo_hotwords.make_graph("zebra", tok, tok.vocab_size, tok.vocab_size) is None


def test_text_to_ids_synthetic():
    tok = SyntheticTokenizer(TINY.vocab_size, 0)
    ids = [7, 12, 9]
    text = "".join(tok.pieces[i] for i in ids)
    (got,) = tok.text_to_ids(text)
    assert "".join(tok.pieces[i] for i in got) == text
    k = 0
    for i in got:                                          # greedy longest match: no longer piece fits at any position
        assert not any(text.startswith(p, k) and len(p) > len(tok.pieces[i]) for p in tok.pieces)
        k += len(tok.pieces[i])
    assert tok.text_to_ids("q") == [] and tok.text_to_ids("") == []


def test_token_id_phrases_keep_their_checks():
    tok = SyntheticTokenizer(TINY.vocab_size, 0)
    V1 = TINY.vocab_size
    assert nemo_hotwords.encode([((3, 4), 0.0), ((5,), 2.0)], tok, V1, V1, 1.5) == [((3, 4), 1.5), ((5,), 2.0)]
    for bad in ([(V1,)], [(-1,)], [(1.5,)], [()]):
        with pytest.raises(ValueError):
            nemo_hotwords.encode([(bad[0], 0.0)], tok, V1, V1)
    with pytest.raises(ValueError):
        nemo_hotwords.encode([("x", float("inf"))], tok, V1, V1)


# ---- the keywords of the nemo package ------------------------------------------------------------------------------------------------
def _model(decoding="alsd", own=None):
    return types.SimpleNamespace(cfg=TINY.with_(decoding=decoding), tokenizer=SyntheticTokenizer(TINY.vocab_size, 0), hotwords=own, hotwords_score=1.5)


def test_keyword_errors():
    from reazonspeech_amd.nemo.asr import load_model
    import inspect
    from reazonspeech_amd.nemo.asr import transcribe, transcribe_batch
    sig = inspect.signature(load_model).parameters
    assert (sig["hotwords_file"].default, sig["hotwords_score"].default, sig["hotwords"].default) == ("", 1.5, None)
    assert inspect.signature(transcribe).parameters["hotwords"].default is None
    assert list(inspect.signature(transcribe_batch).parameters) == ["model", "audios", "config", "distributed", "hotwords"]
    for decoding in ("greedy_batch", "greedy", "beam"):    # before any device is touched
        with pytest.raises(ValueError, match="alsd"):
            load_model(device="cuda:0", config=TINY, decoding=decoding, hotwords=[(3, 4)])
    with pytest.raises(ValueError, match="alsd"):          # the configuration's own strategy (greedy_batch)
        load_model(device="cuda:0", config=TINY, hotwords="x")
    with pytest.raises(ValueError, match="hotwords_score"):
        load_model(device="cuda:0", config=TINY, decoding="alsd", hotwords=[(3,)], hotwords_score=float("nan"))
    with pytest.raises(FileNotFoundError):
        load_model(device="cuda:0", config=TINY, decoding="alsd", hotwords_file="/nonexistent/hotwords.txt")
    assert fusion.check_hotword_keywords(fusion.NEMO, "greedy_batch") is False and fusion.check_hotword_keywords(fusion.NEMO, "alsd", hotwords=[(1,)]) is True


def test_per_audio_meaning():
    m = _model()
    assert per_audio(m, None, 3) is None and per_audio(m, "", 3) is None
    one = per_audio(m, [[(3, 4), (5,)]], 1)            # transcribe: a list is ONE audio's phrases
    assert len(one) == 1 and one[0].n_phrases == 2
    tok = m.tokenizer
    text = tok.pieces[7] + tok.pieces[9]
    allg = per_audio(m, text, 3)
    assert len(allg) == 3 and allg[0] is allg[1] is allg[2] and allg[0].key == ((tok.text_to_ids(text)[0], 1.5),)
    mixed = per_audio(m, [None, text, [(3, 4)]], 3)
    assert mixed[0] is None and mixed[1].key == allg[0].key and mixed[2].key == (((3, 4), 1.5),)
    with pytest.raises(ValueError, match="3 entries for 2 audios"):
        per_audio(m, [None, None, None], 2)
    own = k2_hotwords.build_graph([((1, 2), 1.5)])
    m2 = _model(own=own)
    assert per_audio(m2, None, 2) == [own, own]
    assert [g.key for g in per_audio(m2, [None, [(3,)]], 2)] == [own.key, (((3,), 1.5),)]
    with pytest.raises(ValueError, match="alsd"):
        per_audio(_model("greedy_batch"), [[(3, 4)]], 1)
    with pytest.warns(UserWarning, match="skipped"):
        assert per_audio(m, "q", 1) is None


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_exports_and_family_rows():
    names = {"rs_rnnt_alsd_hotwords", "rs_rnnt_alsd_hotwords_workspace_bytes"}
    assert names <= set(capi.EXPORTS)
    lib = capi.load()
    lib.rs_rnnt_alsd_hotwords_workspace_bytes.restype = ctypes.c_size_t
    assert lib.rs_rnnt_alsd_hotwords_workspace_bytes(None, 4, 4, 100, ctypes.c_double(1.0), -1) == 0       # no context: invalid
    assert lib.rs_rnnt_alsd_hotwords(None, *([None] * 2), 0, 0, 0, ctypes.c_double(0.0), 0, 0, 0, *([None] * 7), 0, None) == capi.RS_EINVAL
    text = open(os.path.join(ROOT, "reazonspeech_amd", "csrc", "rs_family.h")).read()
    rows = dict(re.findall(r"^\s*X\((rs_rnnt_alsd_hotwords\w*), (\w+), ", text, flags=re.M))
    assert rows == {n: "C" for n in names}                 # the Conformer family only: Zipformer and AV-HuBERT contexts get RS_EINVAL
    header = open(os.path.join(ROOT, "include", "rs_asr.h")).read()
    assert all(re.search(r"\b" + n + r"\(", header) for n in names)
    # the walk is one text for both searches
    csrc = os.path.join(ROOT, "reazonspeech_amd", "csrc")
    for f in ("k_rnnt_mbs.hip", "k_rnnt_alsd.hip"):
        src = open(os.path.join(csrc, f)).read()
        assert '#include "k_rnnt_hotwords.h"' in src and "hw_step(const rs_hotwords" not in src
    assert open(os.path.join(csrc, "k_rnnt_hotwords.h")).read().count("float hw_step(const rs_hotwords") == 1
