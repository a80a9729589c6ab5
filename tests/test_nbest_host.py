"""CPU: n-best lists from the modified beam search of `reazonspeech.k2.asr` (rs_rnnt_mbs_nbest, csrc/k_rnnt_mbs.hip; the ranking rule
is stated in include/rs_asr.h) — the C checker that restates the search with its ranked list (tests/k2_mbs_nbest_checker.c)

  * with nbest = 1 against the existing checkers of the search, bit for bit: tests/k2_mbs_checker.c (plain, hotwords) and
    tests/k2_mbs_lm_checker.c (n-gram LM, LM + hotwords), on the toy projections of tests/test_k2_mbs_host.py;
  * with nbest = N: entry 0 is the nbest = 1 result, the list is ordered by norm_scores under the tie rule (equal norms: the one
    that entered the last set first), no two entries hold the same tokens, and the list for every n < N is a prefix of it;
  * hand-built cases on injected logits, each asserting by the checker's counters that it reaches its edge: a last set smaller than
    nbest, an exact tie, a merge in the last frame, an utterance without frames, a hotword Finalize that reorders the list;
  * against the float64 restatement (tests/k2_mbs_lm_ref.py lm_float64), scores only, entries matched by token sequence.  The
    deviation line is that of tests/test_k2_mbs_host.py and tests/test_k2_mbs_lm_host.py: LINE = 2e-4, scores within LINE / 2.
    The fixtures are the rows listed in FLOAT64_FIXTURES: their float64 search has every candidate gap, and their ranked list every
    adjacent norm gap, above 10 x LINE (so neither the sets nor the order are what is compared); both are asserted for every one;
  * the Python surface over fake models: result assembly, argument errors, off returns today's types, the exports.

The ESPnet beam search's lists are tested in tests/test_nbest_espnet_host.py, the ALSD's in tests/test_nbest_alsd_host.py."""
import ctypes
import importlib
import inspect
import os
import types

import numpy as np
import pytest

import k2_hotwords_ref as H
import k2_mbs_lm_ref as LR
import k2_mbs_nbest_ref as NB
import k2_mbs_ref as R
from ngram_lm_ref import ArpaDict
from reazonspeech_amd import build as rs_build
from reazonspeech_amd.k2.asr import huggingface as hfm, interface
from reazonspeech_amd.k2.asr.model import K2Model, _Stream, search_config, synthetic_tokens
from reazonspeech_amd.runtime import capi, k2_hotwords as kh, ngram_lm as NL
from reazonspeech_amd.runtime.config import TINY
from reazonspeech_amd.runtime.k2_config import ZIPFORMER_TINY
from reazonspeech_amd.runtime.k2_weights import synthetic_state_dict_k2
from reazonspeech_amd.runtime.model import AsrModel, DecodedBatch
from test_k2_mbs_host import projection

k2tr = importlib.import_module("reazonspeech_amd.k2.asr.transcribe")

LINE = 2e-4
ALPHA = 0.5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRAPH_OF = [(b % 4) - 1 for b in range(12)]


@pytest.fixture(scope="module")
def runs():
    """the two projections of tests/test_k2_mbs_host.py, the plain search on them, the toy graphs and the toy LM cut from each"""
    cfg = ZIPFORMER_TINY
    out = {}
    for seed in (3, 4):
        sd = synthetic_state_dict_k2(cfg, seed)
        f, el = projection(cfg, sd, seed)
        plain = R.mbs_checker(cfg, sd, f, el, K=4)
        out[seed] = (sd, f, el, plain, NL.build(LR.toy_lm(plain, cfg), cfg.vocab_size, cfg.blank_id), LR.toy_lm(plain, cfg))
    graphs = [kh.build_graph(p) for p in H.toy_graphs(out[3][3])]          # (cut from seed 3: seed 4's results are too short to cut from)
    return out, kh.concat(graphs)


def forms(lm, table):
    """the four forms of the search as keyword sets: plain, hotwords, LM, LM + hotwords"""
    hw = dict(table=table, graph_of=GRAPH_OF)
    return dict(plain={}, hotwords=hw, lm=dict(lm=lm, alpha=ALPHA), lm_hotwords=dict(lm=lm, alpha=ALPHA, **hw))


def test_nbest_1_is_the_existing_checker_bit_for_bit(runs):
    cfg = ZIPFORMER_TINY
    out, table = runs
    for seed, (sd, f, el, plain, lm, _) in out.items():
        for name, kw in forms(lm, table).items():
            for extra in (dict(), dict(blank_penalty=1.5), dict(length_norm=False)):
                if "lm" in kw:
                    want = LR.mbs_lm_checker(cfg, sd, f, el, K=4, **kw, **extra)
                else:
                    want = R.mbs_checker(cfg, sd, f, el, K=4, **kw, **extra)
                got = NB.nbest_checker(cfg, sd, f, el, 1, K=4, **kw, **extra)
                for b, (g, w) in enumerate(zip(got, want)):
                    where = (seed, name, extra, b)
                    assert len(g["entries"]) == 1 and g["n_ids"] == [len(w["ids"])], where
                    assert g["entries"][0][:3] == (w["ids"], w["frames"], w["score_bits"]), where
                    assert g["final"] == w["final"] and g["merges"] == w["merges"] and g["last_set"] == len(w["final"]), where


def check_list(full, K, length_norm=True):
    """the properties of one utterance's list `full` (a checker row at nbest = K): order, tie rule, no duplicates, consistency with
    the last set"""
    ent = full["entries"]
    assert len(ent) == min(K, full["last_set"]) == min(K, len(full["final"]))
    norms = [NB.f32(e[3]) for e in ent]
    assert all(a >= b for a, b in zip(norms, norms[1:])), norms
    order = [y for y, _ in full["final"]]                                  # the order of entry into the last set
    assert len({tuple(e[0]) for e in ent}) == len(ent)                      # the set merged equal sequences
    pos = [order.index(e[0]) for e in ent]
    for k in range(len(ent) - 1):
        if norms[k] == norms[k + 1]:
            assert pos[k] < pos[k + 1], "equal norms: the one that entered the last set first"
    for e, p in zip(ent, pos):                                             # score and norm are the last set's
        lp = np.float32(full["final"][p][1])
        assert e[2] == NB.bits(lp)
        assert e[3] == NB.bits(lp / np.float32(len(e[0]) + 2) if length_norm else lp)
        assert len(e[1]) == len(e[0]) and all(a < b for a, b in zip(e[1], e[1][1:]))      # at most one token per frame


def test_the_list_is_ranked_and_every_shorter_list_is_its_prefix(runs):
    cfg = ZIPFORMER_TINY
    out, table = runs
    sizes = set()
    for seed, (sd, f, el, plain, lm, _) in out.items():
        for name, kw in forms(lm, table).items():
            for K, extra in ((4, {}), (8, {}), (2, {}), (4, dict(length_norm=False))):
                full = NB.nbest_checker(cfg, sd, f, el, K, K=K, **kw, **extra)
                for row in full:
                    check_list(row, K, extra.get("length_norm", True))
                    sizes.add(len(row["entries"]))
                for n in range(1, K):
                    part = NB.nbest_checker(cfg, sd, f, el, n, K=K, **kw, **extra)
                    for b, (p, w) in enumerate(zip(part, full)):
                        assert p["entries"] == w["entries"][:n], (seed, name, K, n, b)
                        assert p["n_ids"] == [len(e[0]) for e in p["entries"]] + [0] * (n - len(p["entries"]))
    assert {2, 4, 8} <= sizes, sizes


# ---- hand-built cases: a 6-symbol vocabulary (0 blank, 2 <unk>), decoder and joiner replaced by a table of logits --------------------
TOY = types.SimpleNamespace(context_size=2, blank_id=0, unk_id=2, vocab_size=6, decoder_dim=0)


def inject(fn, T):
    a = np.zeros((T, 6, 6), np.float32)
    for t in range(T):
        for u in range(6):
            a[t, u] = np.log(np.asarray(fn(t, u), np.float64)).astype(np.float32)
    return a


def run(fn, T, nbest, **kw):
    return NB.nbest_checker(TOY, None, np.zeros((1, T, 1), np.float32), [T], nbest, inject=inject(fn, T), **kw)[0]


def test_a_last_set_smaller_than_nbest_and_a_merge_in_the_last_frame():
    fn = lambda t, u: [.5, .02, .3, .15, .02, .01]              # noqa: E731  blank, <unk> (merges into the blank's entry), then token 3
    r = run(fn, 1, 3, K=3)
    assert r["last_set"] == 2 and r["last_merges"] == 1                    # the edge is reached: 2 entries for 3 places, one merge
    assert [e[0] for e in r["entries"]] == [[], [3]] and r["n_ids"] == [0, 1, 0]
    assert abs(NB.f32(r["entries"][0][2]) - np.log(.8)) < 1e-6             # the merged probability is what the list carries
    assert run(fn, 1, 1, K=3)["entries"] == r["entries"][:1]


def test_an_exact_tie_goes_to_the_entry_that_came_first():
    fn = lambda t, u: [.02, .4, .02, .4, .14, .02]              # noqa: E731  tokens 1 and 3: equal values, 1 has the lower flat index
    for length_norm in (True, False):
        r = run(fn, 1, 3, K=3, length_norm=length_norm)
        assert r["ties"] >= 1                                              # the edge is reached
        assert [e[0] for e in r["entries"]] == [[1], [3], [4]] and r["entries"][0][3] == r["entries"][1][3]


def test_an_utterance_without_frames_has_no_entry():
    r = NB.nbest_checker(TOY, None, np.zeros((2, 1, 1), np.float32), [0, 1], 2, K=2,
                         inject=inject(lambda t, u: [.02, .5, .02, .3, .14, .02], 1))
    assert r[0]["entries"] == [] and r[0]["n_ids"] == [0, 0] and r[0]["last_set"] == 0
    assert [e[0] for e in r[1]["entries"]] == [[1], [3]]
    alone = NB.nbest_checker(TOY, None, np.zeros((1, 0, 1), np.float32), [0], 1, K=2, inject=np.zeros((0, 6, 6), np.float32))
    assert alone[0]["entries"] == []


def test_finalize_reorders_the_list():
    # one frame: 1 (.53) or 3 (.43).  The phrase 3 4 gives [3] a pending +1.0: before Finalize [3] leads, after it [1] does
    fn = lambda t, u: [.01, .53, .01, .43, .01, .01]            # noqa: E731
    table = kh.concat([kh.build_graph([((3, 4), 1.0)])])
    plain = run(fn, 1, 2, K=2, length_norm=False)
    r = run(fn, 1, 2, K=2, length_norm=False, table=table, graph_of=[0])
    assert r["finalize_reorders"] == 1 and plain["finalize_reorders"] == 0 and r["finalize"] == -1.0     # the edge is reached
    assert [e[0] for e in r["entries"]] == [[1], [3]]
    lp3 = np.float32(NB.f32(plain["entries"][1][2]))                      # [3]: + 1.0 at the step, - 1.0 at Finalize, in that order
    assert [e[2] for e in r["entries"]] == [plain["entries"][0][2], NB.bits(np.float32(np.float32(lp3 + np.float32(1.0)) + np.float32(-1.0)))]
    # with the one-token phrase the bonus is earned and stays: [3] leads the list
    r = run(fn, 1, 2, K=2, length_norm=False, table=kh.concat([kh.build_graph([((3,), 1.0)])]), graph_of=[0])
    assert [e[0] for e in r["entries"]] == [[3], [1]] and r["finalize_reorders"] == 0


# ---- the float64 restatement: scores only ------------------------------------------------------------------------------------------
# (seed, with the LM, row) of the toy projections whose float64 search keeps every candidate gap, and whose ranked list keeps every
# adjacent norm gap, above 10 x LINE — asserted for each of them below, so that order is never what is compared
FLOAT64_FIXTURES = [(3, False, 11), (3, True, 6), (3, True, 7), (4, False, 1), (4, False, 3), (4, False, 4), (4, False, 6), (4, False, 8),
                    (4, True, 0), (4, True, 1), (4, True, 2), (4, True, 4), (4, True, 5), (4, True, 6), (4, True, 7), (4, True, 10), (4, True, 11)]
def test_scores_equal_the_float64_restatement(runs):
    cfg = ZIPFORMER_TINY
    out, _ = runs
    compared, deviation, took = 0, 0.0, []
    for seed, (sd, f, el, plain, lm, ent) in out.items():
        for with_lm in (False, True):
            kw = dict(lm=lm, alpha=ALPHA) if with_lm else {}
            chk = NB.nbest_checker(cfg, sd, f, el, 4, K=4, **kw)
            arpa = ArpaDict(ent, 3, LR.unk_log10(ent)) if with_lm else None
            for b in range(len(el)):
                ref = LR.lm_float64(cfg, sd, f[b, :el[b]], arpa=arpa, alpha=ALPHA if with_lm else 0.0, bos=True, K=4)
                want = NB.ranked_float64(ref)
                gaps = [a[2] - c[2] for a, c in zip(want, want[1:])]
                if (seed, with_lm, b) not in FLOAT64_FIXTURES:
                    continue
                took.append((seed, with_lm, b))
                assert all(g > 10 * LINE for g in gaps) and ref["min_gap"] > 10 * LINE, (seed, with_lm, b, gaps, ref["min_gap"])     # the fixture keeps its gaps
                got = chk[b]["entries"]
                assert [e[0] for e in got] == [w[0] for w in want[:4]], (seed, with_lm, b)      # matched by token sequence: the same, in order
                for e, w in zip(got, want):
                    deviation = max(deviation, abs(NB.f32(e[2]) - w[1]), abs(NB.f32(e[3]) - w[2]))
                compared += 1
    print(f"{compared} fixture rows; largest |float32 - float64| over their scores and norms {deviation:.3e}")
    assert sorted(took) == sorted(FLOAT64_FIXTURES)
    assert deviation < LINE / 2, deviation


# ---- the Python surface over fake models -----------------------------------------------------------------------------------------
MBS = dict(decoding_method="modified_beam_search")


def fake_am(cfg, nbest=0):
    return types.SimpleNamespace(cfg=cfg, nbest=nbest)


def test_argument_errors_name_the_reason():
    cfg = ZIPFORMER_TINY
    for call in (lambda **kw: hfm.load_model(**kw), lambda **kw: search_config(cfg, **kw),
                 lambda **kw: K2Model(cfg, {}, synthetic_tokens(cfg.vocab_size), **kw)):
        with pytest.raises(ValueError, match="nbest=2 needs decoding_method='modified_beam_search'"):
            call(nbest=2)
        with pytest.raises(ValueError, match="nbest=5 is above max_active_paths=4"):
            call(nbest=5, **MBS)
        with pytest.raises(ValueError, match="nbest=3 is above max_active_paths=2"):
            call(nbest=3, max_active_paths=2, **MBS)
        for bad in (-1, 9, 2.0, "2", True):
            with pytest.raises(ValueError, match="nbest must be an integer in 0..8"):
                call(nbest=bad, **MBS)
    assert search_config(cfg, nbest=4, **MBS) == search_config(cfg, **MBS) and search_config(cfg, nbest=1) == search_config(cfg)
    # the runtime model's own check, for every search
    mbs = fake_am(search_config(cfg, **MBS))
    plan = lambda am, n: AsrModel.nbest_plan(am, n)             # noqa: E731
    assert [plan(mbs, n) for n in (None, 0, 1, 4)] == [0, 0, 1, 4] and plan(fake_am(mbs.cfg, nbest=3), None) == 3
    with pytest.raises(ValueError, match=r"nbest=5 is above the beam \(4\)"):
        plan(mbs, 5)
    with pytest.raises(ValueError, match="nbest must be an integer in 1..8"):
        plan(mbs, 9)
    greedy = fake_am(cfg)
    assert plan(greedy, 1) == 0
    with pytest.raises(ValueError, match="nbest=2 needs a beam search: the greedy search"):
        plan(greedy, 2)
    for decoding in ("alsd", "beam"):                                      # every beam search has its n-best form
        assert plan(fake_am(TINY.with_(decoding=decoding, beam_size=4)), 2) == 2
    # the keyword's place: before the LM keywords, whose position tests/test_k2_mbs_lm_host.py pins
    params = list(inspect.signature(hfm.load_model).parameters)
    assert "nbest" in params and inspect.signature(hfm.load_model).parameters["nbest"].default == 0
    assert inspect.signature(AsrModel.decode).parameters["nbest"].default is None
    assert inspect.signature(AsrModel.transcribe_waveforms).parameters["nbest"].default is None


def test_result_assembly():
    nb = dict(ids=np.array([[[5, 6, 0], [5, 0, 0]], [[0, 0, 0], [0, 0, 0]]], np.int32),
              frames=np.array([[[1, 4, 0], [2, 0, 0]], [[0, 0, 0], [0, 0, 0]]], np.int32), n_ids=np.array([[2, 1], [0, 0]], np.int32),
              scores=np.array([[-1.5, -2.5], [0, 0]], np.float32), norm_scores=np.array([[-0.375, -0.8125], [0, 0]], np.float32),
              n_hyps=np.array([2, 0], np.int32))
    lists = AsrModel.nbest_lists(nb, 2, "modified_beam_search")
    assert lists == [[([5, 6], [1, 4], -1.5, -0.375), ([5], [2], -2.5, -0.8125)], []]
    assert AsrModel.nbest_lists(nb, 1, "alsd")[0][0][1] == [1, 3]          # alignment steps become frames, as `collect` does
    assert DecodedBatch([], [], []).nbest is None and list(DecodedBatch.__dataclass_fields__)[-2:] == ["nbest", "token_logprobs"]
    # K2Model.decode_streams over a fake runtime model: the list becomes results, entry 0 is the result itself
    cfg = search_config(ZIPFORMER_TINY, **MBS)
    model = K2Model.__new__(K2Model)
    model.cfg, model.tokens, model.hotwords = cfg, synthetic_tokens(cfg.vocab_size, 3), None
    for with_scores in (False, True):
        decoded = DecodedBatch([[5, 6], []], [[1, 4], []], [9, 0], [-1.5, 0.0], nbest=lists,
                               token_logprobs=[[-0.25, -0.5], []] if with_scores else None)
        model.am = types.SimpleNamespace(transcribe_waveforms=lambda waves, **kw: decoded)
        streams = [_Stream(), _Stream()]
        model.decode_streams(streams)
        r = streams[0].result
        assert r.nbest[0] is r and len(r.nbest) == 2 and (r.log_prob, r.norm_log_prob) == (-1.5, -0.375)
        assert r.tokens == [model.symbol(5), model.symbol(6)] and r.nbest[1].tokens == [model.symbol(5)]
        assert r.nbest[1].timestamps == [float(np.float32(cfg.seconds_per_frame() * 2))] and r.nbest[1].log_prob == -2.5
        assert r.nbest[1].token_log_probs is None and (r.token_log_probs == [-0.25, -0.5]) == with_scores
        assert streams[1].result.nbest == [] and streams[1].result.text == ""
        res = k2tr._result(streams[0])
        assert type(res) is interface.NBestTranscribeResult and isinstance(res, interface.TranscribeResult)
        assert [e.text for e in res.nbest] == [r.text, r.nbest[1].text] and res.text == r.text and res.nbest[0].subwords == res.subwords
        assert (res.log_prob, res.nbest[1].norm_log_prob) == (-1.5, -0.8125) and res.nbest[1].token_logprobs is None
        assert res.token_logprobs == ([-0.25, -0.5] if with_scores else None) and res.nbest[0].token_logprobs == res.token_logprobs
        assert type(k2tr._result(streams[1])) is interface.NBestTranscribeResult and k2tr._result(streams[1]).nbest == []
    # off: today's objects
    model.am = types.SimpleNamespace(transcribe_waveforms=lambda waves, **kw: DecodedBatch([[5]], [[1]], [9], [-1.0]))
    st = _Stream()
    model.decode_streams([st])
    assert st.result.nbest is None and st.result.log_prob is None and type(k2tr._result(st)) is interface.TranscribeResult


def test_the_entry_points_are_exported_declared_and_guarded():
    lib = ctypes.CDLL(rs_build.build())
    assert lib.rs_abi_version() == 7
    assert hasattr(lib, "rs_rnnt_mbs_nbest") and hasattr(lib, "rs_rnnt_mbs_nbest_workspace_bytes")      # fails without the feature
    assert {"rs_rnnt_mbs_nbest", "rs_rnnt_mbs_nbest_workspace_bytes"} <= set(capi.EXPORTS)
    loaded = capi.load()
    assert len(loaded.rs_rnnt_mbs_nbest.argtypes) == len(loaded.rs_rnnt_mbs_lm.argtypes) + 3           # nbest, norm_scores, n_hyps
    assert loaded.rs_rnnt_mbs_nbest_workspace_bytes.restype is ctypes.c_size_t
    lib.rs_rnnt_mbs_nbest_workspace_bytes.restype = ctypes.c_size_t
    assert lib.rs_rnnt_mbs_nbest_workspace_bytes(None, 4, 4, 100, 100, 2) == 0                            # no context: invalid
    header = open(os.path.join(ROOT, "include", "rs_asr.h"), encoding="utf-8").read()
    assert "size_t rs_rnnt_mbs_nbest_workspace_bytes(const rs_ctx* ctx, int B, int max_active_paths, int tp_max, int out_cap, int nbest);" in header
    assert "int rs_rnnt_mbs_nbest(rs_ctx* ctx," in header and "RANKING RULE" in header
    assert "EQUAL NORMS: THE ONE THAT ENTERED THE LAST SET FIRST" in header
    family = open(os.path.join(ROOT, "reazonspeech_amd", "csrc", "rs_family.h"), encoding="utf-8").read()
    assert "X(rs_rnnt_mbs_nbest_workspace_bytes, Z, FINAL, RS_HINT_MBS)" in family and "X(rs_rnnt_mbs_nbest, Z, FINAL, RS_HINT_MBS)" in family
