"""CPU: n-best lists from the ALSD beam search of `reazonspeech.nemo.asr` (rs_rnnt_alsd_nbest, csrc/k_rnnt_alsd.hip; the ranking rule is
stated in include/rs_asr.h): the C checker that restates the search with its ranked list (tests/alsd_nbest_checker.c)

  * with nbest = 1 against the existing checker tests/alsd_checker.c through its loader, bit for bit, on the toy fixture of
    tests/test_alsd_lm_host.py: plain, hotwords, LM, LM + hotwords; merge on and off; norm on and off; a budget that ends the search;
  * with nbest = N: entry 0 is the nbest = 1 result, the list is ordered by norm_scores, no two entries hold the same labels, and the
    list for every n < N is a prefix of it;
  * hand-built cases on injected logits, each asserting by the checker's counters that it reaches its edge: more hypotheses finish
    than nbest (eviction from the tail), fewer finish than nbest, nothing finishes (the budget exit), two equal label sequences
    finish in one step with merge off, an exact tie of norms across two steps, a Finalize that reorders the list under hotwords.
    Of the two norm orders of equal sequences only one can occur: the first occurrence holds the recombined sum
    logaddexp(first, duplicate) > duplicate, both read the same logits from then on, and the beam keeps selection order — the
    earlier slot never has the smaller norm.  The case asserts that order and that the replacement branch was not taken;
  * against a float64 restatement that keeps the whole `final` list (tests/alsd_nbest_ref.py final_float64), scores only, entries
    matched by label sequence.  The deviation line is the one tests/test_alsd_lm_host.py carries: 1e-3 x max(1, |value|).  The
    fixtures are (row, depth) pairs of the toy batch whose adjacent float64 norms differ by more than ten times that line, asserted
    here, so that order is not what is compared;
  * the Python surface over fake models: result assembly, argument errors, off returns today's types, the exports."""
import ctypes
import inspect
import os
import types

import numpy as np
import pytest
import torch

import alsd_hotwords_ref as AR
import alsd_nbest_ref as AN
import ngram_lm_ref as NR
from reazonspeech_amd import build as rs_build
from reazonspeech_amd.nemo.asr import interface, load_model, transcribe as nemo_transcribe
from reazonspeech_amd.runtime import capi, ngram_lm as NL
from reazonspeech_amd.runtime.config import TINY
from reazonspeech_amd.runtime.model import AsrModel
from reazonspeech_amd.runtime.weights import synthetic_state_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALPHA = 0.5


@pytest.fixture(scope="module")
def toy():
    """the batch of tests/test_alsd_lm_host.py, the plain search at beam 4, the three graphs and the LM cut from it"""
    sd = synthetic_state_dict(TINY, 0)
    f, lens = AR.toy_batch(TINY, seed=6)
    f, lens = f.numpy(), lens.numpy()
    plain = AR.alsd_checker(TINY, sd, f, lens, beam=4)
    table = AR.table_of(AR.toy_graphs(plain))
    return sd, f, lens, table, NL.build(NR.toy_lm(plain, TINY), TINY.vocab_size, TINY.blank_id)


def forms(table, lm):
    hw = dict(table=table, graph_of=AR.TOY_GRAPH_OF)
    return dict(plain={}, hotwords=hw, lm=dict(lm=lm, alpha=ALPHA), lm_hotwords=dict(lm=lm, alpha=ALPHA, **hw))


SEARCHES = [(1, 1.0, False, False), (2, 1.0, True, True), (4, 2.0, True, False), (4, 7, False, True), (8, 0.5, True, False)]


@pytest.mark.parametrize("beam,max_target_len,norm,merge", SEARCHES)
def test_nbest_1_is_the_existing_checker_bit_for_bit(toy, beam, max_target_len, norm, merge):
    sd, f, lens, table, lm = toy
    kw = dict(beam=beam, max_target_len=max_target_len, score_norm=norm, merge=merge)
    for name, form in forms(table, lm).items():
        want = AR.alsd_checker(TINY, sd, f, lens, **form, **kw)
        got = AN.nbest_checker(TINY, sd, f, lens, 1, **form, **kw)
        for b, (g, w) in enumerate(zip(got, want)):
            assert g["entries"] and g["entries"][0][:3] == (w["ids"], w["steps"], w["score_bits"]), (name, b)
            assert g["beam"] == [(y, sc) for y, sc, *_ in w["beam"]] and g["recombinations"] == w["recombinations"], (name, b)


@pytest.mark.parametrize("beam,max_target_len,norm,merge", SEARCHES[1:])
def test_the_list_is_ranked_without_duplicates_and_every_shorter_list_is_its_prefix(toy, beam, max_target_len, norm, merge):
    sd, f, lens, table, lm = toy
    kw = dict(beam=beam, max_target_len=max_target_len, score_norm=norm, merge=merge)
    for name, form in forms(table, lm).items():
        full = AN.nbest_checker(TINY, sd, f, lens, beam, **form, **kw)
        for row in full:
            ent = row["entries"]
            assert 1 <= len(ent) <= beam and len({tuple(e[0]) for e in ent}) == len(ent)
            norms = [AN.f32(e[3]) for e in ent]
            assert all(a >= c for a, c in zip(norms, norms[1:])), norms
            for e in ent:
                s = np.float32(AN.f32(e[2]))
                assert e[3] == AN.bits(s / np.float32(len(e[0]) + 1) if norm else s) and len(e[1]) == len(e[0])
        for n in range(1, beam):
            part = AN.nbest_checker(TINY, sd, f, lens, n, **form, **kw)
            for p, w in zip(part, full):
                assert p["entries"] == w["entries"][:n], (name, n)
                assert p["n_ids"] == [len(e[0]) for e in p["entries"]] + [0] * (n - len(p["entries"]))


# ---- hand-built cases: a vocabulary of four labels and the blank, injected logits -------------------------------------------------
V, BLANK = 5, 4


def inject(fn, T):
    """fn(t, last label or -1) -> 5 probabilities (labels 0..3, then the blank); -> float32 logits [T][V][V] by (frame, last label + 1)"""
    z = np.zeros((T, V, V), np.float32)
    for t in range(T):
        for u in range(V):
            z[t, u] = np.log(np.asarray(fn(t, u - 1), np.float64)).astype(np.float32)
    return z


def run(fn, T, nbest, beam, budget, phrases=None, norm=True, merge=False):
    table = AR.table_of([phrases]) if phrases else None
    return AN.nbest_checker(None, None, None, [T], nbest, table, [0] if phrases else None, beam=beam, max_target_len=int(budget),
                            score_norm=norm, merge=merge, inject=inject(fn, T), dims=(V, BLANK))[0]


def labels(r):
    return [e[0] for e in r["entries"]]


def test_more_finish_than_nbest_and_the_tail_is_evicted():
    # one frame; label 0 is likely and the blank rare: with the norm every longer hypothesis that finishes beats the shorter ones
    fn = lambda t, u: [.8, .05, .03, .02, .1]                   # noqa: E731
    r = run(fn, 1, 2, beam=2, budget=3)
    assert r["offered"] > 2 and r["evicted"] >= 2 and r["budget_exit"] == 0          # the edge is reached
    assert labels(r) == [[0, 0, 0], [0, 0]] and len(r["entries"]) == 2
    assert labels(run(fn, 1, 1, beam=2, budget=3)) == [[0, 0, 0]]


def test_fewer_finish_than_nbest():
    fn = lambda t, u: [.2, .15, .1, .05, .5]                    # noqa: E731
    r = run(fn, 1, 3, beam=3, budget=0)                          # one alignment step: only the empty hypothesis can finish
    assert r["offered"] == 1 and r["budget_exit"] == 0 and len(r["entries"]) == 1 < 3          # the edge is reached
    assert labels(r) == [[]] and r["n_ids"] == [0, 0, 0]


def test_nothing_finishes_and_the_beam_is_ranked():
    fn = lambda t, u: [.9, .05, .02, .02, .01]                  # noqa: E731  two frames, no budget: nobody reaches the last frame's blank
    r = run(fn, 2, 2, beam=2, budget=0)
    assert r["budget_exit"] == 1 and r["offered"] == len(r["beam"]) == 2                # the edge is reached
    assert labels(r) == [y for y, _ in r["beam"]] == [[0, 0], [0, 1]]
    one = run(fn, 2, 1, beam=2, budget=0)
    assert one["entries"] == r["entries"][:1]


def test_equal_sequences_finishing_in_one_step_are_kept_once():
    # two frames: [0] is reached as (0, blank) and as (blank, 0); with merge off both stay in the beam and finish in the same step
    fn = lambda t, u: [.45, .02, .02, .01, .5]                  # noqa: E731
    r = run(fn, 2, 4, beam=4, budget=2, merge=False)
    assert r["equal_met"] >= 1 and r["equal_replaced"] == 0                             # the edge is reached; the first held the sum
    assert len({tuple(y) for y in labels(r)}) == len(r["entries"]) and [0] in labels(r)
    merged = run(fn, 2, 4, beam=4, budget=2, merge=True)                                # merge on: the duplicate never existed
    assert merged["equal_met"] == 0
    assert [0] in labels(merged)


def test_an_exact_tie_of_norms_across_two_steps_goes_to_the_earlier():
    # every row is the same and label 0 is as likely as the blank: [] finishes at step 0 with x, [0] at step 1 with 2x / 2 = x
    fn = lambda t, u: [.4, .1, .05, .05, .4]                    # noqa: E731
    r = run(fn, 1, 3, beam=3, budget=2)
    assert r["cross_step_ties"] >= 1                                                    # the edge is reached
    assert labels(r)[:2] == [[], [0]] and r["entries"][0][3] == r["entries"][1][3]


def test_finalize_reorders_the_list_under_hotwords():
    # the phrase 0 2 gives [0] a pending + 1.0: before Finalize [0] would rank above [1], after it below
    fn = lambda t, u: [.25, .3, .02, .03, .4]                   # noqa: E731
    plain = run(fn, 1, 3, beam=3, budget=1, norm=False)
    r = run(fn, 1, 3, beam=3, budget=1, norm=False, phrases=[((0, 2), 1.0)])
    assert r["finalize_reorders"] == 1 and plain["finalize_reorders"] == 0              # the edge is reached
    assert labels(r) == [[], [1], [0]] and labels(plain) == [[], [1], [0]]
    assert abs(AN.f32(r["entries"][2][2]) - np.log(.25 * .4)) < 1e-5                    # + 1.0 at the step, - 1.0 at Finalize


# ---- the float64 restatement: scores only ------------------------------------------------------------------------------------------
FIXTURES = [(4, 4), (0, 1)]                             # (row of the toy batch, depth of the list compared)


def test_scores_equal_the_float64_restatement(toy):
    sd, f, lens, _, _ = toy
    chk = AN.nbest_checker(TINY, sd, f, lens, 4, beam=4)
    line = lambda x: 1e-3 * max(1.0, abs(x))                    # noqa: E731
    for b, depth in FIXTURES:
        want = AN.final_float64(TINY, sd, torch.from_numpy(f[b]), int(lens[b]), beam=4)
        for a, c in zip(want[:depth], want[1:depth + 1]):
            assert a[2] - c[2] > 10 * line(a[2]), (b, a[2], c[2])                       # the fixture keeps its gaps: order is not compared
        got = chk[b]["entries"][:depth]
        assert [e[0] for e in got] == [w[0] for w in want[:depth]], b
        for e, w in zip(got, want):
            assert abs(AN.f32(e[2]) - w[1]) <= line(w[1]) and abs(AN.f32(e[3]) - w[2]) <= line(w[2]), (b, e, w)


# ---- the Python surface over fake models -----------------------------------------------------------------------------------------
def test_argument_errors_and_result_assembly():
    plan = lambda cfg, n, own=0: AsrModel.nbest_plan(types.SimpleNamespace(cfg=cfg, nbest=own), n)        # noqa: E731
    alsd = TINY.with_(decoding="alsd", beam_size=4)
    assert [plan(alsd, n) for n in (None, 0, 1, 4)] == [0, 0, 1, 4] and plan(alsd, None, own=2) == 2
    with pytest.raises(ValueError, match=r"nbest=5 is above the beam \(4\)"):
        plan(alsd, 5)
    with pytest.raises(ValueError, match="nbest=2 needs a beam search"):
        plan(TINY, 2)
    for bad, pattern in ((dict(nbest=2), "needs a beam search"), (dict(decoding="alsd", beam_size=2, nbest=3), "above the beam"),
                         (dict(decoding="alsd", nbest=9), "integer in 1..8")):
        with pytest.raises(ValueError, match=pattern):          # before any device is touched
            load_model(device="cuda:0", config=TINY, **bad)
    assert inspect.signature(load_model).parameters["nbest"].default == 0
    assert inspect.signature(nemo_transcribe).parameters["nbest"].default is None
    # alignment steps become frames, as `collect` does for the one hypothesis
    nb = dict(ids=np.array([[[5, 6, 0], [5, 0, 0]]], np.int32), frames=np.array([[[1, 4, 0], [2, 0, 0]]], np.int32),
              n_ids=np.array([[2, 1]], np.int32), scores=np.array([[-1.5, -2.5]], np.float32),
              norm_scores=np.array([[-0.5, -1.25]], np.float32), n_hyps=np.array([2], np.int32))
    assert AsrModel.nbest_lists(nb, 1, "alsd") == [[([5, 6], [1, 3], -1.5, -0.5), ([5], [2], -2.5, -1.25)]]
    assert issubclass(interface.NBestTranscribeResult, interface.TranscribeResult)


def test_the_entry_points_are_exported_declared_and_guarded():
    lib = ctypes.CDLL(rs_build.build())
    assert lib.rs_abi_version() == 7
    assert hasattr(lib, "rs_rnnt_alsd_nbest") and hasattr(lib, "rs_rnnt_alsd_nbest_workspace_bytes")    # fails without the feature
    assert {"rs_rnnt_alsd_nbest", "rs_rnnt_alsd_nbest_workspace_bytes"} <= set(capi.EXPORTS)
    loaded = capi.load()
    assert len(loaded.rs_rnnt_alsd_nbest.argtypes) == len(loaded.rs_rnnt_alsd_lm.argtypes) + 3           # nbest, norm_scores, n_hyps
    lib.rs_rnnt_alsd_nbest_workspace_bytes.restype = ctypes.c_size_t
    lib.rs_rnnt_alsd_nbest_workspace_bytes.argtypes = loaded.rs_rnnt_alsd_nbest_workspace_bytes.argtypes
    assert lib.rs_rnnt_alsd_nbest_workspace_bytes(None, 4, 4, 100, 2.0, -1, 2) == 0                       # no context: invalid
    header = open(os.path.join(ROOT, "include", "rs_asr.h"), encoding="utf-8").read()
    assert "int rs_rnnt_alsd_nbest(rs_ctx* ctx," in header and "ENTERS BELOW EVERY" in header
    assert "THE LIST HOLDS EACH LABEL SEQUENCE AT MOST ONCE" in header and "a slot table with an order array" in header
    family = open(os.path.join(ROOT, "reazonspeech_amd", "csrc", "rs_family.h"), encoding="utf-8").read()
    assert "X(rs_rnnt_alsd_nbest_workspace_bytes, C, FINAL, RS_HINT_LSTM_ONLY)" in family and "X(rs_rnnt_alsd_nbest, C, FINAL, RS_HINT_LSTM_ONLY)" in family
