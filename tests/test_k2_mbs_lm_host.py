"""CPU: n-gram LM shallow fusion in the modified beam search of `reazonspeech.k2.asr` (rs_rnnt_mbs_lm, csrc/k_rnnt_mbs.hip;
the rule is stated in include/rs_asr.h) — the C checker that restates all three forms of the search in the device's float32 order
(tests/k2_mbs_lm_checker.c) against the one checker of the search without an LM (tests/k2_mbs_checker.c), against a float64
restatement over the textbook dictionary backoff (tests/k2_mbs_lm_ref.py: lm_float64), hand-built cases for every statement of the
rule, and the keywords of `load_model` / `K2Model` / `transcribe`.

The agreement rule of the float64 test is that of tests/test_k2_mbs_host.py: a row whose candidate gaps (adjacent values among the
K + 1 best of a frame) and final gap all exceed LINE must agree in ids and frames; a row below LINE may differ only from the first
such frame on; at most 3 of the 24 rows may use that excuse.  LINE = 2e-4, re-measured WITH the LM terms in the scores (the toy
order-3 LM at alpha 0.5, |score| up to about 70): a torch-float32 run of the float64 restatement agrees with it on 24 / 24 rows and
its hypothesis scores deviate by at most 2.4e-5, under LINE / 8 = 2.5e-5, so the line stays.  One row lies below it in the float64
reference (seed 3 row 4, gap 1.997e-4; 1 of the 3 allowed); the next gaps above it are 3.3e-4, 4.4e-4, 4.5e-4.  Measured with the C
checker: 24 / 24 rows identical, no excuse used; the largest |float32 score - float64 score| over the final sets is 1.6e-5 (printed
by the test, bounded by LINE / 2).  With the LM the ids of 11 of the 12 seed-3 rows differ from the search without it (seed 4: none,
its results have one token)."""
import ctypes
import importlib
import inspect
import math
import os
import types

import numpy as np
import pytest

import k2_hotwords_ref as H
import k2_mbs_lm_ref as LR
import k2_mbs_ref as R
import ngram_lm_ref as NR
from ngram_lm_ref import ArpaDict, BOS
from reazonspeech_amd import build as rs_build
from reazonspeech_amd.k2.asr import huggingface as hfm
from reazonspeech_amd.k2.asr.model import K2Model, search_config, synthetic_tokens
from reazonspeech_amd.runtime import capi, fusion, k2_hotwords as kh, ngram_lm as NL
from reazonspeech_amd.runtime.k2_config import ZIPFORMER_TINY
from reazonspeech_amd.runtime.k2_weights import synthetic_state_dict_k2
from reazonspeech_amd.runtime.model import _NgramSet
from test_k2_mbs_host import projection

k2tr = importlib.import_module("reazonspeech_amd.k2.asr.transcribe")

LINE = 2e-4
MAX_EXCUSED = 3
ALPHA = 0.5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAME = ("ids", "frames", "score_bits", "merges", "final", "child_hits", "fail_transitions", "exits", "finalize")


@pytest.fixture(scope="module")
def runs():
    """the two projections of tests/test_k2_mbs_host.py, the plain search on them, and the toy LM cut from each"""
    cfg = ZIPFORMER_TINY
    out = {}
    for seed in (3, 4):
        sd = synthetic_state_dict_k2(cfg, seed)
        f, el = projection(cfg, sd, seed)
        plain = R.mbs_checker(cfg, sd, f, el, K=4)
        out[seed] = (sd, f, el, plain, LR.toy_lm(plain, cfg))
    return out


def test_without_an_lm_the_checker_is_the_one_checker_of_the_search(runs):
    cfg = ZIPFORMER_TINY
    graphs = [kh.build_graph(p) for p in H.toy_graphs(runs[3][3])]       # (cut from seed 3: seed 4's results are too short to cut from)
    table, graph_of = kh.concat(graphs), [(b % 4) - 1 for b in range(12)]
    for seed, (sd, f, el, plain, ent) in runs.items():
        lm = NL.build(ent, cfg.vocab_size, cfg.blank_id)
        for kw in (dict(), dict(table=table, graph_of=graph_of)):
            want = plain if not kw else R.mbs_checker(cfg, sd, f, el, K=4, **kw)
            for extra in (dict(), dict(lm=None, alpha=0.7), dict(lm=lm, alpha=0.0)):
                got = LR.mbs_lm_checker(cfg, sd, f, el, K=4, **kw, **extra)
                for b, (g, w) in enumerate(zip(got, want)):
                    assert all(g[k] == w[k] for k in SAME), (seed, b, list(kw), list(extra))
                    assert g["walks"] == 0
        if seed == 3:
            assert sum(w["child_hits"] for w in want) > 0                 # the graphs are met


def test_checker_equals_the_float64_restatement_with_the_lm(runs):
    cfg = ZIPFORMER_TINY
    excused, below_ref, deviation, rows = [], [], 0.0, 0
    for seed, (sd, f, el, plain, ent) in runs.items():
        lm = NL.build(ent, cfg.vocab_size, cfg.blank_id)
        arpa = ArpaDict(ent, 3, LR.unk_log10(ent))
        chk = LR.mbs_lm_checker(cfg, sd, f, el, lm=lm, alpha=ALPHA, K=4)
        differs = sum(c["ids"] != p["ids"] for c, p in zip(chk, plain))
        for b in range(len(el)):
            ref = LR.lm_float64(cfg, sd, f[b, :el[b]], arpa=arpa, alpha=ALPHA, bos=True, K=4)
            got = chk[b]
            rows += 1
            by_tokens = {tuple(y): lp for y, lp in ref["final"]}
            for y, lp in got["final"]:
                if tuple(y) in by_tokens:
                    deviation = max(deviation, abs(lp - by_tokens[tuple(y)]))
            same = (got["ids"], got["frames"]) == (ref["ids"], ref["frames"])
            below = min(ref["min_gap"], ref["final_gap"]) <= LINE
            below_ref += [(seed, b)] if below else []
            print(f"seed {seed} row {b}: T {el[b]} gap {ref['min_gap']:.2e} @ {ref['min_gap_frame']} final gap {ref['final_gap']:.2e} "
                  f"merges {got['merges']} / {ref['merges']} tokens {len(got['ids'])} same {same}")
            if same:
                assert got["merges"] == ref["merges"], (seed, b)
                continue
            assert below, f"seed {seed} row {b} differs although every gap exceeds {LINE}: {ref['min_gap']:.3e}, {ref['final_gap']:.3e}"
            first = next((t for t, g in enumerate(ref["frame_gaps"]) if g <= LINE), el[b])
            cut = lambda r: [(i, t) for i, t in zip(r["ids"], r["frames"]) if t < first]     # noqa: E731
            assert cut(got) == cut(ref), f"seed {seed} row {b} differs before frame {first}, the first with a gap <= {LINE}"
            excused.append((seed, b))
        print(f"seed {seed}: {differs} of {len(el)} rows differ from the search without the LM; {LR.totals(chk, 3)}")
        if seed == 3:
            assert differs >= 1, "the LM must change a result: " + LR.RECHOOSE
    print(f"largest |float32 score - float64 score| over the final sets: {deviation:.3e}; rows below the line in the float64 reference: "
          f"{below_ref}; rows excused: {excused}")
    assert rows == 24 and len(below_ref) <= MAX_EXCUSED, f"the float64 reference alone leaves {below_ref} below the line: " + LR.RECHOOSE
    assert len(excused) <= MAX_EXCUSED, excused
    assert deviation < LINE / 2, deviation


def test_the_toy_lm_is_met_at_every_level(runs):
    cfg = ZIPFORMER_TINY
    sd, f, el, plain, ent = runs[3]
    lm = NL.build(ent, cfg.vocab_size, cfg.blank_id)
    t = LR.totals(LR.mbs_lm_checker(cfg, sd, f, el, lm=lm, alpha=ALPHA, K=4), lm.order)
    print(t)
    assert sum(t["hits"][1:]) > 0 and t["backoffs"] > 0 and t["unk"] > 0 and t["full_order_pops"] > 0, LR.RECHOOSE
    assert LR.all_counted(t) and t["state_mismatches"] == 0, LR.RECHOOSE


# ---- hand-built cases: a 6-symbol vocabulary (0 blank, 2 <unk>), decoder and joiner replaced by a table of logits --------------------
TOY = types.SimpleNamespace(context_size=2, blank_id=0, unk_id=2, vocab_size=6, decoder_dim=0)
F = np.float32


def inject(fn, T):
    """fn(t, last token) -> 6 probabilities; -> float32 logits [T][6][6]"""
    a = np.zeros((T, 6, 6), np.float32)
    for t in range(T):
        for u in range(6):
            a[t, u] = np.log(np.asarray(fn(t, u), np.float64)).astype(np.float32)
    return a


def run(fn, T, **kw):
    return LR.mbs_lm_checker(TOY, None, np.zeros((1, T, 1), np.float32), [T], inject=inject(fn, T), **kw)[0]


def toy_model(ent):
    return NL.build(ent, TOY.vocab_size, TOY.blank_id)


def bits(x):
    return int(np.asarray([x], np.float32).view(np.int32)[0])


TWO = lambda t, u: [.02, .48, .02, .42, .04, .02]            # noqa: E731  tokens 1 and 3 survive at K = 2; token 4 is ranked third


def test_the_lm_flips_the_winner_among_two_survivors():
    lm = toy_model({(1,): (-3.0, 0.0), (3,): (-0.125, 0.0), (4,): (-0.125, 0.0)})
    assert run(TWO, 1, K=2)["ids"] == [1]
    r = run(TWO, 1, K=2, lm=lm, alpha=1.0)
    assert r["ids"] == [3] and [y for y, _ in r["final"]] == [[1], [3]] and r["walks"] == 2     # the order of entry is the selection's


def test_a_candidate_that_was_not_selected_is_not_rescued():
    lm = toy_model({(1,): (-3.0, 0.0), (3,): (-3.0, 0.0), (4,): (0.0, 0.0)})                  # the LM wants token 4, ranked K + 1
    r = run(TWO, 1, K=2, lm=lm, alpha=5.0)
    assert [y for y, _ in r["final"]] == [[1], [3]] and r["ids"] == [1]                         # the selection is LM-free
    assert run(TWO, 1, K=3, lm=lm, alpha=5.0)["ids"] == [4]                                     # selected, it wins


def test_blank_and_unk_make_no_walk_and_keep_their_state():
    lm = toy_model({(BOS,): (-99.0, -0.25), (3,): (-1.0, 0.0), (3, 3): (-0.5, 0.0)})
    assert lm.start != 0 and lm.order == 2
    fn = lambda t, u: [.5, .02, .3, .15, .02, .01]              # noqa: E731
    plain, r = run(fn, 1, K=3), run(fn, 1, K=3, lm=lm, alpha=0.7)
    assert [y for y, _ in r["final"]] == [[], [3]] and r["merges"] == 1 and r["walks"] == 1
    assert r["final_bits"][0] == plain["final_bits"][0]                                        # blank + <unk>: their score, no term
    assert r["final_lm"][0] == lm.start and r["final_lm"][1] == lm.arrays["root_child"][3]


def test_a_token_missing_from_the_model_takes_unk_logp_and_returns_to_the_root():
    lm = toy_model({(BOS,): (-99.0, -0.25), (3,): (-1.0, 0.0)})                             # no unigram for token 4
    fn = lambda t, u: [.02, .02, .02, .02, .9, .02]             # noqa: E731
    plain, r = run(fn, 1, K=1), run(fn, 1, K=1, lm=lm, alpha=0.7)
    assert r["ids"] == [4] and r["unk"] == 1 and r["backoffs"] == 1 and r["final_lm"] == [0]
    l = F(lm.arrays["backoff"][lm.start] + lm.unk_logp)
    assert r["score_bits"] == bits(F(F(plain["score"]) + F(F(0.7) * l)))
    assert NR.step(lm, lm.start, 4)[:2] == (l, 0)


def test_a_full_order_hit_moves_to_the_suffix_node():
    lm = toy_model({(BOS,): (-99.0, -0.25), (3,): (-1.0, -0.5), (BOS, 3): (-0.25, 0.0)})
    assert lm.order == 2
    fn = lambda t, u: [.02, .02, .02, .9, .02, .02]             # noqa: E731
    r = run(fn, 1, K=1, lm=lm, alpha=0.7)
    assert r["full_order_pops"] == 1 and r["hits"][2] == 1 and r["backoffs"] == 0
    assert r["final_lm"] == [int(lm.arrays["root_child"][3])]                                   # the unigram node of 3, not the bigram's


# values chosen so that every other evaluation order gives other bits (asserted below: a change of the inputs that loses this fails)
ORDER_LM = {(BOS,): (-99.0, -0.375), (3,): (-1.0, -0.25)}
ORDER_FN = lambda t, u: [.02, .02, .02, .9, .02, .02]           # noqa: E731


def test_with_a_hotword_the_lm_term_is_added_to_the_biased_score():
    lm = toy_model(ORDER_LM)
    graph = kh.build_graph([((3,), 1.7)])
    lp = F(run(ORDER_FN, 1, K=1)["score"])
    hw = run(ORDER_FN, 1, K=1, table=kh.concat([graph]), graph_of=[0])
    delta = F(1.7)
    assert hw["score_bits"] == bits(F(lp + delta))                                             # (the non-strict exit returns the phrase's score)
    l = NR.step(lm, lm.start, 3)[0]
    term = F(F(0.7) * l)
    r = run(ORDER_FN, 1, K=1, table=kh.concat([graph]), graph_of=[0], lm=lm, alpha=0.7)
    assert r["score_bits"] == bits(F(F(lp + delta) + term))
    assert bits(F(F(lp + delta) + term)) != bits(F(lp + F(delta + term))), "re-choose the values: both associations give the same bits"


def test_the_product_with_alpha_is_rounded_before_the_add():
    lm = toy_model(ORDER_LM)
    lp = F(run(ORDER_FN, 1, K=1)["score"])
    l = NR.step(lm, lm.start, 3)[0]
    r = run(ORDER_FN, 1, K=1, lm=lm, alpha=0.7)
    assert r["score_bits"] == bits(F(lp + F(F(0.7) * l)))
    fused = F(np.float64(F(0.7)) * np.float64(l) + np.float64(lp))
    assert bits(fused) != r["score_bits"], "re-choose the values: a fused multiply-add gives the same bits"


def test_merged_candidates_carry_their_lm_terms_into_logaddexp():
    # frame 0: [3] (.6) and [] (.4); frame 1: [3] + blank (.9) enters first, [] + 3 (.9) merges into it — both hold one LM term
    def fn(t, u):
        if t == 0:
            return [.4, .0001, .0001, .5996, .0001, .0001]
        return [.9, .02, .02, .02, .02, .02] if u == 3 else [.02, .02, .02, .9, .02, .02]
    lm = toy_model(ORDER_LM)
    plain, r = run(fn, 2, K=2), run(fn, 2, K=2, lm=lm, alpha=0.7)
    l = float(NR.step(lm, lm.start, 3)[0])
    for x in (plain, r):
        assert x["merges"] == 1 and x["final"][0][0] == [3] and x["ids"] == [3]
    # the term [3] took at frame 0 is inside its log_prob at frame 1: [] + 3 now ranks first, enters first and its timestamp stays
    assert plain["frames"] == [0] and r["frames"] == [1]
    assert r["walks"] >= 2 and r["state_mismatches"] == 0
    assert abs(plain["final"][0][1] - math.log(.5996 * .9 + .4 * .9)) < 1e-5
    assert abs(r["final"][0][1] - (math.log(.5996 * .9 + .4 * .9) + 0.7 * l)) < 1e-5       # logaddexp(a + x, b + x) = logaddexp(a, b) + x
    ref = LR.lm_float64(TOY, None, None, arpa=ArpaDict(ORDER_LM, 2, -1.0), alpha=0.7, bos=True, K=2, n_frames=2,
                        logits_fn=lambda t, ys: np.log(np.asarray(fn(t, ys[-1]), np.float64)))
    assert ref["merges"] == 1 and abs(ref["final"][0][1] - r["final"][0][1]) < 1e-5


# ---- keywords and exports --------------------------------------------------------------------------------------------------------
MBS = dict(decoding_method="modified_beam_search")


def k2_call_alpha(model, ngram_lm_alpha):
    return fusion.call_alpha(fusion.K2, model, ngram_lm_alpha)


def k2_model_lm(cfg, tokens, *keywords):
    return fusion.model_lm(fusion.K2, cfg, tokens, *keywords)


def test_the_lm_keywords_are_checked_before_anything_is_loaded(tmp_path):
    cfg = ZIPFORMER_TINY
    for call in (lambda **kw: hfm.load_model(**kw), lambda **kw: search_config(cfg, **kw),
                 lambda **kw: K2Model(cfg, {}, synthetic_tokens(cfg.vocab_size), **kw)):
        with pytest.raises(ValueError, match="an n-gram LM needs decoding_method='modified_beam_search'"):
            call(ngram_lm_model="lm.arpa")
        with pytest.raises(ValueError, match="an n-gram LM needs decoding_method='modified_beam_search'"):
            call(decoding_method="greedy_search", ngram_lm_model="lm.arpa", ngram_lm_alpha=0.3)
        for bad in (-0.1, float("nan"), float("inf"), "0.3", True):
            with pytest.raises(ValueError, match="ngram_lm_alpha must be a finite number >= 0"):
                call(ngram_lm_model="lm.arpa", ngram_lm_alpha=bad, **MBS)
        with pytest.raises(ValueError, match="'nemo' is the NeMo package's"):
            call(ngram_lm_model="lm.arpa", ngram_lm_tokens="nemo", **MBS)
        with pytest.raises(ValueError, match="ngram_lm_tokens must be one of"):
            call(ngram_lm_model="lm.arpa", ngram_lm_tokens="words", **MBS)
    with pytest.raises(FileNotFoundError, match="ngram_lm_model"):
        hfm.load_model(ngram_lm_model=str(tmp_path / "missing.arpa"), **MBS)
    assert search_config(cfg) == cfg and search_config(cfg, ngram_lm_alpha=0.3) == cfg        # no model: today's configuration
    # the per-call weight
    no_lm = types.SimpleNamespace(ngram_lm=None, ngram_lm_alpha=0.0, cfg=search_config(cfg, **MBS))
    assert k2_call_alpha(no_lm, None) == (None, 0.0) and k2_call_alpha(no_lm, 0) == (None, 0.0)
    with pytest.raises(ValueError, match="the model has no n-gram LM"):
        k2_call_alpha(no_lm, 0.3)
    lm = NL.build({(5,): (-1.0, 0.0)}, cfg.vocab_size, cfg.blank_id)
    has = types.SimpleNamespace(ngram_lm=lm, ngram_lm_alpha=0.25, cfg=no_lm.cfg)
    assert k2_call_alpha(has, None) == (lm, 0.25) and k2_call_alpha(has, 0) == (None, 0.0) and k2_call_alpha(has, 2) == (lm, 2.0)
    # the signatures: transcribe gains the keyword last, transcribe_batch and create_stream keep theirs
    assert list(inspect.signature(k2tr.transcribe).parameters) == ["model", "audio", "config", "hotwords", "ngram_lm_alpha"]
    assert list(inspect.signature(k2tr.transcribe_batch).parameters) == ["model", "audios", "config", "hotwords"]
    assert list(inspect.signature(K2Model.create_stream).parameters) == ["self", "hotwords"]
    assert list(inspect.signature(hfm.load_model).parameters)[-3:] == ["ngram_lm_model", "ngram_lm_alpha", "ngram_lm_tokens"]
    assert inspect.signature(hfm.load_model).parameters["ngram_lm_tokens"].default == "pieces"


def test_a_table_for_other_logits_or_one_that_fails_the_check_is_refused():
    cfg = search_config(ZIPFORMER_TINY, **MBS)
    tokens = synthetic_tokens(cfg.vocab_size, 3)
    wrong = NL.build({(5,): (-1.0, 0.0)}, cfg.vocab_size + 3, cfg.blank_id)
    with pytest.raises(ValueError, match=f"built for {cfg.vocab_size + 3} logits, the model has {cfg.vocab_size}"):
        k2_model_lm(cfg, tokens, wrong)
    with pytest.raises(ValueError, match="an n-gram LM needs decoding_method='modified_beam_search'"):
        k2_model_lm(ZIPFORMER_TINY, tokens, NL.build({(5,): (-1.0, 0.0)}, cfg.vocab_size, cfg.blank_id))
    bad = NL.build({(5,): (-1.0, 0.0), (6,): (-1.0, 0.0), (5, 6): (-0.5, 0.0)}, cfg.vocab_size, cfg.blank_id)
    bad.arrays["suffix"][3] = 3                                           # a suffix link that does not lower the level
    with pytest.raises(capi.RsError, match="does not lower the level") as e:
        _NgramSet(bad, "cuda:0")                                          # rs_ngram_check runs first: nothing is uploaded, no GPU is touched
    assert e.value.code == capi.RS_EINVAL


def test_an_arpa_file_in_the_pieces_of_tokens_txt_reads_back(tmp_path):
    cfg = search_config(ZIPFORMER_TINY, **MBS)
    tokens = synthetic_tokens(97, 3)
    ent = {(BOS,): (-99.0, -0.25), (5,): (-1.0, -0.125), (9,): (-1.5, -0.25), (40,): (-2.0, 0.0), (7,): (-1.25, 0.0),
           (BOS, 5): (-0.25, -0.125), (5, 9): (-0.5, -0.125), (9, 40): (-0.375, 0.0), (5, 9, 40): (-0.125, None), (BOS, 5, 9): (-0.25, None)}
    want = NL.build({k: (p, b if b is not None else 0.0) for k, (p, b) in ent.items()}, cfg.vocab_size, cfg.blank_id)
    path = NR.write_arpa(str(tmp_path / "lm.arpa"), ent, mode="pieces", pieces=tokens)
    text = open(path, encoding="utf-8").read()
    assert tokens[5] in text and tokens[40] in text and "<s>" in text
    got = k2_model_lm(cfg, tokens, path)                               # "pieces" is the default
    assert got.key == want.key and got.order == 3 and got.n_logits == cfg.vocab_size and got.start == want.start != 0
    for k in NL.ARRAYS:
        assert np.array_equal(got.arrays[k], want.arrays[k]), k
    ids = k2_model_lm(cfg, tokens, NR.write_arpa(str(tmp_path / "ids.arpa"), ent, mode="ids"), "ids")
    assert ids.key == want.key
    with pytest.raises(ValueError, match="NeMo package"):
        k2_model_lm(cfg, tokens, path, "nemo")
    # `<unk>` of the file is the unknown-word entry, not tokens.txt's <unk> symbol
    unk = k2_model_lm(cfg, tokens, NR.write_arpa(str(tmp_path / "unk.arpa"), {**ent, ("<unk>",): (-4.0, None)}, mode="pieces", pieces=tokens))
    assert unk.unk_logp == np.float32(-4.0 * math.log(10.0)) and np.array_equal(unk.arrays["logp"], want.arrays["logp"])


def test_the_entry_points_are_exported_declared_and_guarded():
    lib = ctypes.CDLL(rs_build.build())
    assert lib.rs_abi_version() == 7
    assert hasattr(lib, "rs_rnnt_mbs_lm") and hasattr(lib, "rs_rnnt_mbs_lm_workspace_bytes")
    assert {"rs_rnnt_mbs_lm", "rs_rnnt_mbs_lm_workspace_bytes"} <= set(capi.EXPORTS)
    loaded = capi.load()
    assert loaded.rs_rnnt_mbs_lm.argtypes is not None and loaded.rs_rnnt_mbs_lm_workspace_bytes.restype is ctypes.c_size_t
    assert len(loaded.rs_rnnt_mbs_lm.argtypes) == len(loaded.rs_rnnt_mbs_hotwords.argtypes) + 2
    lib.rs_rnnt_mbs_lm_workspace_bytes.restype = ctypes.c_size_t
    assert lib.rs_rnnt_mbs_lm_workspace_bytes(None, 4, 4, 100, 100) == 0   # no context: invalid
    header = open(os.path.join(ROOT, "include", "rs_asr.h"), encoding="utf-8").read()
    assert "size_t rs_rnnt_mbs_lm_workspace_bytes(const rs_ctx* ctx, int B, int max_active_paths, int tp_max, int out_cap);" in header
    assert "int rs_rnnt_mbs_lm(rs_ctx* ctx," in header and "[UPSTREAM, not vendored, UNVERIFIED] icefall" in header
    assert header.index("int rs_rnnt_mbs_hotwords(") < header.index("int rs_rnnt_mbs_lm(") < header.index("int rs_rnnt_alsd_hotwords(")
    family = open(os.path.join(ROOT, "reazonspeech_amd", "csrc", "rs_family.h"), encoding="utf-8").read()
    assert "X(rs_rnnt_mbs_lm_workspace_bytes, Z, FINAL, RS_HINT_MBS)" in family and "X(rs_rnnt_mbs_lm, Z, FINAL, RS_HINT_MBS)" in family


def test_the_nemo_packages_helpers_keep_their_messages():
    with pytest.raises(ValueError, match=r"^an n-gram LM needs decoding='alsd', not 'greedy_batch'$"):
        fusion.check_lm_keywords(fusion.NEMO, "greedy_batch", "lm.arpa", 0.3)
    with pytest.raises(ValueError, match=r"^ngram_lm_tokens must be one of \('nemo', 'pieces', 'ids'\), not 'words'$"):
        fusion.check_lm_keywords(fusion.NEMO, "alsd", "lm.arpa", 0.3, "words")
    with pytest.raises(ValueError, match=r"^ngram_lm_alpha must be a finite number >= 0, not -1$"):
        fusion.check_lm_keywords(fusion.NEMO, "alsd", "lm.arpa", -1)
    assert fusion.check_lm_keywords(fusion.NEMO, "alsd", "lm.arpa", 0.3) is True and fusion.check_lm_keywords(fusion.NEMO, "greedy_batch", None, 0.0) is False
    nemo = types.SimpleNamespace(ngram_lm=None, ngram_lm_alpha=0.0, cfg=types.SimpleNamespace(decoding="alsd"))
    with pytest.raises(ValueError, match=r"^ngram_lm_alpha given, but the model has no n-gram LM \(load_model\(ngram_lm_model=...\)\)$"):
        fusion.call_alpha(fusion.NEMO, nemo, 0.3)
    assert NL.TOKEN_MODES == ("nemo", "pieces", "ids")
