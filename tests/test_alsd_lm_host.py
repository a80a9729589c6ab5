"""CPU: n-gram LM shallow fusion in the NeMo family's ALSD beam search (rs_rnnt_alsd_lm, csrc/k_rnnt_alsd.hip; the rule is stated in
include/rs_asr.h).  What needs no GPU:

  * the C checker (tests/alsd_checker.c) with no LM, or with alpha 0, returns what tests/alsd_hotwords_checker.c returned before
    this file absorbed it (tests/golden/alsd_hotwords_checker_pins.json), bit for bit, with and without graphs
  * the checker against a float64 Python restatement of the same rules on the toy geometry (labels, steps; scores with the tolerance
    tests/test_alsd_hotwords_host.py holds for its pair)
  * hand-built cases on a five-entry vocabulary with injected logits: an LM term overtakes inside a hypothesis's top `beam` (and
    only there), a tie, an unknown token, a full-order pop, LM plus hotword on one candidate (the order of the two additions)
  * the toy fixture of the GPU test exercises every counter and changes results (conditions on the inputs)
  * the keywords of the nemo package, the export list and the family rows"""
import ctypes
import inspect
import json
import math
import os
import re
import types

import numpy as np
import pytest

import alsd_hotwords_ref as AR
import k2_hotwords_ref as KR
import ngram_lm_ref as NR
from reazonspeech_amd.runtime import capi, fusion, ngram_lm as NL
from reazonspeech_amd.runtime.config import TINY
from reazonspeech_amd.runtime.tokenizer import SyntheticTokenizer
from reazonspeech_amd.runtime.weights import synthetic_state_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOY_SEED = 6
TOY_ALPHA = 0.5
F32 = np.float32
BOS = NL.BOS


@pytest.fixture(scope="module")
def toy():
    """the GPU test's batch, the plain search at beam 4, the three graphs and the LM cut from it"""
    sd = synthetic_state_dict(TINY, 0)
    f, lens = AR.toy_batch(TINY, seed=TOY_SEED)
    f, lens = f.numpy(), lens.numpy()
    plain = AR.alsd_checker(TINY, sd, f, lens, beam=4)
    graphs = AR.toy_graphs(plain)
    ent = NR.toy_lm(plain, TINY)
    return sd, f, lens, graphs, AR.table_of(graphs), ent, NL.build(ent, TINY.vocab_size, TINY.blank_id)


# ---- without an LM the checker is the hotword checker ----------------------------------------------------------------------------------
with open(os.path.join(ROOT, "tests", "golden", "alsd_hotwords_checker_pins.json")) as _fh:
    PINS = {(c["beam"], c["max_target_len"], c["score_norm"], c["merge"], c["graphs"]): c["rows"] for c in json.load(_fh)["cases"]}


@pytest.mark.parametrize("beam,max_target_len,norm,merge", [(1, 1.0, False, False), (2, 1.0, True, True), (4, 2.0, True, False),
                                                            (4, 7, False, True), (8, 0.5, True, False)])
def test_checker_without_lm_is_the_hotword_checker(toy, beam, max_target_len, norm, merge):
    """the hotword checker is the one deleted from the tree: its results on these inputs are the pins (floats as bit patterns)"""
    sd, f, lens, _, table, _, lm = toy
    kw = dict(beam=beam, max_target_len=max_target_len, score_norm=norm, merge=merge)
    for tab, gof in ((None, None), (table, AR.TOY_GRAPH_OF)):
        ref = PINS[(beam, max_target_len, norm, merge, tab is not None)]
        runs = [AR.alsd_checker(TINY, sd, f, lens, tab, gof, None, 0.7, **kw),                    # no model
                AR.alsd_checker(TINY, sd, f, lens, tab, gof, lm, 0.0, **kw)]                      # alpha 0
        if tab is None:
            runs.append(AR.alsd_checker(TINY, sd, f, lens, **kw))                                 # no graph or LM argument at all
        for got in runs:
            assert len(got) == len(ref)
            for b, (g, r) in enumerate(zip(got, ref)):
                assert g["ids"] == r["ids"] and g["steps"] == r["steps"] and g["score_bits"] == r["score_bits"], (b, g["score"])
                assert AR.bits(g["finalize"]) == r["finalize_bits"] and [[y, AR.bits(sc), st] for y, sc, st, _ in g["beam"]] == r["beam"]
                assert all(g[k] == r[k] for k in AR.COUNTERS)
                assert sum(g["hits"]) == g["backoffs"] == g["unk"] == g["full_order_pops"] == 0
        assert sum(len(r["ids"]) for r in ref) > 20


# ---- the checker against float64 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beam,mode,norm,hot", [(1, "upstream", False, False), (2, "merge", True, True), (4, "upstream", True, True),
                                                (4, "merge", False, False)])
def test_checker_matches_float64_restatement(toy, beam, mode, norm, hot):
    """same decisions as the float64 restatement (NR.lm_float64): labels, alignment steps and the score of the winner within the
    tolerance tests/test_alsd_hotwords_host.py holds for its pair"""
    import torch
    sd, f, lens, graphs, table, ent, lm = toy
    rows, graph_of = [0, 1, 3, 6], [0, 1, 2, 0]
    kw = dict(beam=beam, max_target_len=1.0, score_norm=norm, merge=mode == "merge")
    got = AR.alsd_checker(TINY, sd, f[rows], lens[rows], table if hot else None, graph_of if hot else None, lm, TOY_ALPHA, **kw)
    plain = AR.alsd_checker(TINY, sd, f[rows], lens[rows], table if hot else None, graph_of if hot else None, **kw)
    arpa = NR.ArpaDict(ent, 3, min(p for k, (p, _) in ent.items() if len(k) == 1 and k != (BOS,)))
    n_tok = 0
    for k, b in enumerate(rows):
        graph = KR.ContextGraph(graphs[graph_of[k]]) if hot else None
        ids, steps, score = NR.lm_float64(TINY, sd, torch.from_numpy(f[b]), int(lens[b]), graph, arpa, TOY_ALPHA, bos=True, beam=beam,
                                          max_target_len=1.0, score_norm=norm, recombine=mode)
        assert got[k]["ids"] == ids and got[k]["steps"] == steps, (b, got[k]["ids"], ids)
        assert abs(got[k]["score"] - score) < 1e-3 * max(1.0, abs(score)), (b, got[k]["score"], score)
        n_tok += len(ids)
    assert n_tok > 6, "degenerate fixture"
    assert sum(sum(g["hits"]) for g in got) > 0 and sum(g["backoffs"] for g in got) > 0
    assert any(g["score"] != p["score"] for g, p in zip(got, plain)), "the LM changed nothing: re-choose the inputs"


# ---- hand-built cases: a vocabulary of four labels and the blank, injected logits -------------------------------------------------
V, BLANK = 5, 4
LOW = -30.0
LN10 = math.log(10.0)


def logits(T):
    """inject [T][V][V], every entry LOW; rows are filled in by the cases: inject[t][last label + 1][v]"""
    return np.full((T, V, V), LOW, np.float32)


def lsm(row):
    row = np.asarray(row, np.float64)
    return row - (row.max() + math.log(np.exp(row - row.max()).sum()))


def model(ent, unk=None):
    return NL.build(NL.Ngrams(max(len(k) for k in ent), ent, unk), V - 1, BLANK)


def run(z, T, lm, alpha, beam, budget, phrases=None, norm=False, merge=False):
    table = AR.table_of([phrases]) if phrases else None
    return AR.alsd_checker(None, None, None, [T], table, [0] if phrases else None, lm, alpha, beam=beam, max_target_len=int(budget),
                           score_norm=norm, merge=merge, inject=z, dims=(V, BLANK))[0]


def test_an_lm_term_overtakes_inside_the_top_beam_and_only_there():
    """label 0 has the better logit, the LM prefers label 1.  Beam 2: both are among the hypothesis's two best labels, the LM term is
    part of the ranking and [1] wins.  Beam 1: only label 0 is expanded — the LM is applied AFTER the pick by raw logit, so label 1 is
    never seen, label 0 falls behind the blank and nothing is emitted"""
    z = logits(1)
    z[0, 0, BLANK], z[0, 0, 0], z[0, 0, 1] = -1.0, 1.0, 0.5
    z[0, 1, BLANK] = z[0, 2, BLANK] = 10.0
    lm = model({(0,): (-2.0, 0.0), (1,): (-0.125, 0.0)})
    plain = run(z, 1, None, 0.0, 2, 1)
    fused = run(z, 1, lm, 1.0, 2, 1)
    assert plain["ids"] == [0] and fused["ids"] == [1] and fused["steps"] == [0]
    want = lsm(z[0, 0])[1] + 1.0 * (-0.125 * LN10) + lsm(z[0, 2])[BLANK]
    assert abs(fused["score"] - want) < 1e-5
    assert abs(plain["score"] - (lsm(z[0, 0])[0] + lsm(z[0, 1])[BLANK])) < 1e-5
    one = run(z, 1, lm, 1.0, 1, 1)
    assert run(z, 1, None, 0.0, 1, 1)["ids"] == [0] and one["ids"] == []
    assert abs(one["score"] - lsm(z[0, 0])[BLANK]) < 1e-5 and one["hits"][1] >= 1


def test_a_tie_goes_to_the_lower_candidate():
    """logits 1.0 and 0.875, LM terms -1.0 and -0.875 (natural logarithms set directly, alpha 1): both subtractions z - lse are exact
    (lse lies within a factor two of both logits) and both sums are -lse exactly — a tie the LM made; the earlier expansion stays
    first, as in rs_rnnt_alsd"""
    z = logits(1)
    z[0, 0, BLANK], z[0, 0, 0], z[0, 0, 1] = -1.0, 0.875, 1.0
    z[0, 1, BLANK] = z[0, 2, BLANK] = 10.0
    lm = model({(0,): (-1.0, 0.0), (1,): (-1.0, 0.0)})
    a = lm.arrays
    a["logp"][a["root_child"][0]], a["logp"][a["root_child"][1]] = -0.875, -1.0
    lse = F32(-lsm(z[0, 0])[1] + 1.0)
    assert 0.5 * lse <= 0.875 and 1.0 <= 2 * lse                # Sterbenz: z - lse is exact for both
    r = run(z, 1, lm, 1.0, 2, 1)
    (y0, s0, _, _), (y1, s1, _, _) = r["beam"]
    assert AR.same_bits(s0, s1) and abs(s0 + float(lse)) < 1e-6
    assert (y0, y1) == ([1], [0]) and r["ids"] == [1]          # label 1 has the better logit: it is expanded first, and stays first
    a["logp"][a["root_child"][0]] = F32(-0.875) + F32(2.0 ** -20)           # a little more for label 0 (8 ulp of the sum): no tie any more
    r = run(z, 1, lm, 1.0, 2, 1)
    assert [e[0] for e in r["beam"]] == [[0], [1]] and r["ids"] == [0]


def test_an_unknown_token_costs_unk_and_resets_the_state():
    z = logits(1)
    z[0, 0, 2] = 10.0                                           # label 2 has no unigram
    z[0, 3, BLANK] = 10.0
    lm = model({(0,): (-1.0, -0.5), (1,): (-1.25, 0.0), (BOS,): (-99.0, -0.25)}, unk=-1.5)
    r = run(z, 1, lm, 0.5, 1, 1)
    assert r["ids"] == [2] and r["unk"] >= 1 and r["beam"][0][3] == 0
    unk, bo = F32(-1.5 * LN10), F32(-0.25 * LN10)
    assert lm.unk_logp == unk and lm.start != 0
    want = lsm(z[0, 0])[2] + 0.5 * float(F32(bo + unk)) + lsm(z[0, 3])[BLANK]        # from `<s>`: its backoff, then <unk>
    assert abs(r["score"] - want) < 1e-5 and r["backoffs"] >= 1


def test_a_full_order_match_pops_to_its_suffix():
    """order 2: after label 0 the state is the unigram (0); label 1 finds the bigram (0 1), a full-order node: the next state is its
    longest suffix, the unigram (1)"""
    z = logits(1)
    z[0, 0, 0] = 10.0
    z[0, 1, 1] = 10.0
    z[0, 2, BLANK] = 10.0
    lm = model({(0,): (-1.0, -0.5), (1,): (-1.5, -0.25), (0, 1): (-0.25, 0.0)})
    r = run(z, 1, lm, 2.0, 1, 2)
    assert r["ids"] == [0, 1] and r["full_order_pops"] >= 1 and r["hits"][2] >= 1
    assert r["beam"][0][3] == lm.arrays["root_child"][1]
    want = lsm(z[0, 0])[0] + 2.0 * (-1.0 * LN10) + lsm(z[0, 1])[1] + 2.0 * (-0.25 * LN10) + lsm(z[0, 2])[BLANK]
    assert abs(r["score"] - want) < 1e-4


def test_lm_and_hotword_on_one_candidate_add_in_the_stated_order():
    """cs = ((hs + (z[v] - lse)) + delta) + (alpha * lp): the hotword delta first, then the rounded product.  Beam 1, one frame: the
    winner's score is that candidate's score exactly (the closing blank adds 0.0: exp(-40) vanishes next to 1), so the four runs give
    base, base + delta, base + t and the sum in question as bits"""
    z = logits(1)
    z[0, 0, 0], z[0, 0, 1] = 3.0, 1.0
    z[0, 1, BLANK] = 10.0
    lm = model({(0,): (-0.75, 0.0), (1,): (-1.0, 0.0)})
    phrases = [((0,), 1.5)]
    alpha = 1.1                                                 # (with 0.3 the two orders round alike: the last assertion but two says so)
    base = F32(run(z, 1, None, 0.0, 1, 1)["score"])
    hot = run(z, 1, None, 0.0, 1, 1, phrases)
    fused = run(z, 1, lm, alpha, 1, 1)
    both = run(z, 1, lm, alpha, 1, 1, phrases)
    assert hot["ids"] == fused["ids"] == both["ids"] == [0]
    t = F32(F32(alpha) * F32(-0.75 * LN10))                     # the product, rounded first
    assert AR.same_bits(hot["score"], F32(base + F32(1.5))) and AR.same_bits(fused["score"], F32(base + t))
    first_delta, first_lm = F32(F32(base + F32(1.5)) + t), F32(F32(base + t) + F32(1.5))
    assert not AR.same_bits(first_delta, first_lm), "the two orders must differ in bits: re-choose the values"
    assert AR.same_bits(both["score"], first_delta)
    assert both["child_hits"] >= 1 and both["hits"][1] >= 1


# ---- the toy fixture: conditions on the inputs, decided by the checker alone ----------------------------------------------------------
TOY_CASES = [(1, 2.0, True, False), (2, 2.0, True, False), (4, 2.0, True, False), (8, 2.0, True, False),
             (4, 2.0, True, True), (4, 2.0, False, False), (4, 9, True, False)]


@pytest.mark.parametrize("beam,max_target_len,norm,merge", TOY_CASES)
def test_toy_fixture_exercises_the_model(toy, beam, max_target_len, norm, merge):
    sd, f, lens, graphs, table, ent, lm = toy
    assert lm.order == 3 and lm.start != 0 and any(lm.arrays["root_child"][:TINY.vocab_size] < 0)
    capi.ngram_check(lm.arrays, lm.start, lm.order, lm.unk_logp)
    kw = dict(beam=beam, max_target_len=max_target_len, score_norm=norm, merge=merge)
    plain = AR.alsd_checker(TINY, sd, f, lens, **kw)
    for tab, gof in ((None, None), (table, AR.TOY_GRAPH_OF)):
        got = AR.alsd_checker(TINY, sd, f, lens, tab, gof, lm, TOY_ALPHA, **kw)
        t = NR.totals(got, lm.order)
        if beam == 1:                                          # one hypothesis per utterance: nothing to recombine with
            t["recombinations"] = 1
        assert NR.all_counted(t) and sum(g["lm_mismatches"] for g in got) == 0, f"re-choose the inputs: {t}"
        assert got[2]["ids"] == [] and got[2]["score"] == 0.0
        assert any(g["ids"] != p["ids"] for g, p in zip(got, plain)), "re-choose the inputs: no row's labels changed"


# ---- the keywords of the nemo package ------------------------------------------------------------------------------------------------
def _model(decoding="alsd", lm=None, alpha=0.0):
    return types.SimpleNamespace(cfg=TINY.with_(decoding=decoding), tokenizer=SyntheticTokenizer(TINY.vocab_size, 0), hotwords=None,
                                 hotwords_score=1.5, ngram_lm=lm, ngram_lm_alpha=alpha)


def check_keywords(decoding, *keywords):
    return fusion.check_lm_keywords(fusion.NEMO, decoding, *keywords)


def model_lm(model, *keywords):
    return fusion.model_lm(fusion.NEMO, model.cfg, model.tokenizer, *keywords)


def call_alpha(model, ngram_lm_alpha):
    return fusion.call_alpha(fusion.NEMO, model, ngram_lm_alpha)


def test_keyword_errors(tmp_path):
    from reazonspeech_amd.nemo.asr import load_model, transcribe
    sig = inspect.signature(load_model).parameters
    assert (sig["ngram_lm_model"].default, sig["ngram_lm_alpha"].default, sig["ngram_lm_tokens"].default) == (None, 0.0, "nemo")
    assert inspect.signature(transcribe).parameters["ngram_lm_alpha"].default is None
    arpa = NR.TOY_ARPA
    for decoding in ("greedy_batch", "greedy", "beam"):        # before any device is touched
        with pytest.raises(ValueError, match="alsd"):
            load_model(device="cuda:0", config=TINY, decoding=decoding, ngram_lm_model=arpa, ngram_lm_alpha=0.3)
    with pytest.raises(ValueError, match="alsd"):              # the configuration's own strategy (greedy_batch)
        load_model(device="cuda:0", config=TINY, ngram_lm_model=arpa, ngram_lm_alpha=0.3)
    for bad in (float("nan"), float("inf"), -0.1, "0.3", True, None):
        with pytest.raises(ValueError, match="ngram_lm_alpha"):
            load_model(device="cuda:0", config=TINY, decoding="alsd", ngram_lm_model=arpa, ngram_lm_alpha=bad)
    with pytest.raises(ValueError, match="ngram_lm_tokens"):
        load_model(device="cuda:0", config=TINY, decoding="alsd", ngram_lm_model=arpa, ngram_lm_alpha=0.3, ngram_lm_tokens="words")
    with pytest.raises(FileNotFoundError, match="ngram_lm_model"):
        load_model(device="cuda:0", config=TINY, decoding="alsd", ngram_lm_model=str(tmp_path / "missing.arpa"), ngram_lm_alpha=0.3)
    assert check_keywords("greedy_batch") is False and check_keywords("alsd", arpa, 0.3) is True and check_keywords(None, arpa, 0.3) is True


def test_model_lm_and_per_call_alpha(tmp_path):
    m = _model()
    toks = m.tokenizer.ids_to_tokens(range(TINY.vocab_size))
    ent = {(3,): (-1.0, -0.5), (4,): (-1.25, 0.0), (3, 4): (-0.25, 0.0)}
    keys = set()
    for mode in NL.TOKEN_MODES:
        if mode == "pieces" and len(set(toks[i] for i in (3, 4))) < 2:
            continue
        path = NR.write_arpa(str(tmp_path / f"{mode}.arpa"), ent, mode, toks)
        lm = model_lm(m, path, mode)
        assert lm.n_logits == TINY.n_logits and lm.n_nodes == 4
        keys.add(lm.key)
    assert len(keys) == 1                                       # one model, three spellings
    assert model_lm(m, lm) is lm
    with pytest.raises(ValueError, match="logits"):
        model_lm(m, NL.build(ent, 10, 10))
    with pytest.raises(ValueError, match="alsd"):
        model_lm(_model("greedy_batch"), lm)
    # None = the model's value, 0 = this call without the LM, a value with no LM loaded raises
    assert call_alpha(_model(), None) == (None, 0.0) and call_alpha(_model(), 0) == (None, 0.0)
    assert call_alpha(_model(lm=lm, alpha=0.3), None) == (lm, 0.3) and call_alpha(_model(lm=lm, alpha=0.3), 0.0) == (None, 0.0)
    assert call_alpha(_model(lm=lm, alpha=0.3), 0.7) == (lm, 0.7) and call_alpha(_model(lm=lm, alpha=0.0), None) == (None, 0.0)
    with pytest.raises(ValueError, match="no n-gram LM"):
        call_alpha(_model(), 0.3)
    with pytest.raises(ValueError, match="ngram_lm_alpha"):
        call_alpha(_model(lm=lm, alpha=0.3), -1.0)
    with pytest.raises(ValueError, match="alsd"):
        call_alpha(_model("greedy_batch", lm=lm, alpha=0.3), None)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_exports_and_family_rows():
    names = {"rs_rnnt_alsd_lm", "rs_rnnt_alsd_lm_workspace_bytes"}
    assert names | {"rs_ngram_check"} <= set(capi.EXPORTS)
    lib = capi.load()
    lib.rs_rnnt_alsd_lm_workspace_bytes.restype = ctypes.c_size_t
    assert lib.rs_rnnt_alsd_lm_workspace_bytes(None, 4, 4, 100, ctypes.c_double(1.0), -1) == 0       # no context: invalid
    assert lib.rs_rnnt_alsd_lm(None, *([None] * 2), 0, 0, 0, ctypes.c_double(0.0), 0, 0, 0, *([None] * 7), ctypes.c_float(0.0), None, 0,
                               None) == capi.RS_EINVAL
    text = open(os.path.join(ROOT, "reazonspeech_amd", "csrc", "rs_family.h")).read()
    rows = dict(re.findall(r"^\s*X\((rs_rnnt_alsd_lm\w*), (\w+), ", text, flags=re.M))
    assert rows == {n: "C" for n in names}                     # the Conformer family only: Zipformer and AV-HuBERT contexts get RS_EINVAL
    header = open(os.path.join(ROOT, "include", "rs_asr.h")).read()
    assert all(re.search(r"\b" + n + r"\(", header) for n in names | {"rs_ngram_check"})
    assert ctypes.sizeof(capi.RsNgram) == 8 * ctypes.sizeof(ctypes.c_void_p) + 6 * 4
    src = open(os.path.join(ROOT, "reazonspeech_amd", "csrc", "k_rnnt_alsd.hip")).read()
    assert '#include "k_rnnt_ngram.h"' in src and "float lm_step(" not in src
    assert open(os.path.join(ROOT, "reazonspeech_amd", "csrc", "k_rnnt_ngram.h")).read().count("float lm_step(const rs_ngram") == 1
