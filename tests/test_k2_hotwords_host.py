"""CPU: hotwords (contextual biasing) of the Zipformer family's modified beam search (rs_rnnt_mbs_hotwords, csrc/k_rnnt_mbs.hip;
runtime/k2_hotwords.py) — the graph against upstream's own unit-test tables, the product's flat builder against an independent
pointer restatement, rs_hotwords_check, the C checker (tests/k2_mbs_checker.c) without graphs against what the plain checker returned
before the hotword one absorbed it (tests/golden/k2_mbs_checker_pins.json) and with graphs against a float64 restatement, hand-built cases for every context rule of the search, and parsing / argument checking.

The agreement rule of the checker test is the one of tests/test_k2_mbs_host.py (LINE = 2e-4 on the gaps the float64 run reports;
a row below it may differ from the first such frame on).  The bonuses do not move it: with scores that are multiples of 0.5 every
graph quantity is exact in float32 and float64 alike, so the two searches still part only at near-ties of the log-softmax values.
At most 1 row in 8 may use the excuse (there: 3 of 24)."""
import ctypes
import json
import math
import os
import types
import warnings

import numpy as np
import pytest
import torch

import k2_hotwords_ref as H
import k2_mbs_ref as R
from reazonspeech_amd import build as rs_build
from reazonspeech_amd.k2.asr import huggingface as hfm
from reazonspeech_amd.k2.asr import model as k2model
from reazonspeech_amd.k2.asr.model import K2Model, search_config, synthetic_tokens
from reazonspeech_amd.runtime import capi, k2_hotwords as kh
from reazonspeech_amd.runtime.k2_config import ZIPFORMER_TINY
from reazonspeech_amd.runtime.k2_weights import synthetic_state_dict_k2
from reazonspeech_amd.runtime.synth import synthetic_batch
from oracle import zipformer as oz

PAD = int(0.9 * 16000)
LINE = 2e-4

NINE = [(tuple(ord(c) for c in w), 1.0) for w in "S HE SHE SHELL HIS HERS HELLO THIS THEM".split()]
UPSTREAM = {"HEHERSHE": (14, 7), "HERSHE": (12, 5), "HISHE": (9, 5), "SHED": (6, 3), "SHELF": (6, 3), "HELL": (2, 2), "HELLO": (7, 2),
            "DHRHISQ": (4, 3), "THEN": (2, 2)}          # query -> (strict, non-strict): the two tables of upstream's unit test


# ---- the graph -------------------------------------------------------------------------------------------------------------------
def test_graph_reproduces_upstreams_unit_test_tables():
    ptr = H.ContextGraph(NINE)
    table = kh.concat([kh.build_graph(NINE)])
    flat = H.FlatView(table)
    for query, want in UPSTREAM.items():
        for strict, total in zip((True, False), want):
            st, fs, a, b = ptr.root, 0, 0.0, 0.0
            for c in query:
                d, st = ptr.step(st, ord(c), strict)
                a += d
                d, fs = flat.step(0, fs, ord(c), strict)
                b += d
            a += ptr.finalize(st)[0]
            b += flat.finalize(0, fs)[0]
            assert (a, b) == (total, total), (query, strict, a, b, total)


def random_phrases(rng):
    n = int(rng.integers(1, 51))
    return [(tuple(int(t) for t in rng.integers(3, 8, size=int(rng.integers(1, 7)))), float(rng.choice([1.0, 1.5, 2.0, 4.0]))) for _ in range(n)]


def test_flat_builder_equals_the_pointer_restatement_and_passes_the_check():
    rng = np.random.default_rng(0)
    steps = 0
    for case in range(200):
        phrases = random_phrases(rng)
        ptr = H.ContextGraph(phrases)
        graph = kh.build_graph(phrases)
        table = kh.concat([graph])
        capi.hotwords_check(table)
        flat = H.FlatView(table)
        streams = rng.integers(3, 8, size=(50, 12))
        for stream in streams:
            st, fs = ptr.root, 0
            for tok in stream.tolist():
                d0, st = ptr.step(st, tok)
                d1, fs = flat.step(0, fs, tok)
                assert d0 == d1 and st.path() == flat.path(fs), (case, phrases, stream, tok)
                steps += 1
            assert ptr.finalize(st)[0] == flat.finalize(0, fs)[0]
    assert steps == 200 * 50 * 12


def test_concatenated_graphs_walk_like_each_graph_alone():
    rng = np.random.default_rng(1)
    sets = [random_phrases(rng) for _ in range(4)]
    graphs = [kh.build_graph(p) for p in sets]
    table = kh.concat(graphs)
    capi.hotwords_check(table)
    assert len(table["graph_root"]) == 4 and table["max_level"] == max(g.max_level for g in graphs)
    flat = H.FlatView(table)
    for g, phrases in enumerate(sets):
        ptr, root = H.ContextGraph(phrases), int(table["graph_root"][g])
        st, fs = ptr.root, root
        for tok in rng.integers(3, 8, size=200).tolist():
            d0, st = ptr.step(st, tok)
            d1, fs = flat.step(root, fs, tok)
            assert d0 == d1 and st.path() == flat.path(fs)


def test_hotwords_check_rejects_bad_tables():
    good = kh.concat([kh.build_graph(NINE), kh.build_graph([((5, 6, 7), 2.0), ((6, 7), 1.5)])])
    capi.hotwords_check(good)
    capi.hotwords_check(H.EMPTY_TABLE)                                     # no graph at all is a valid table

    def broken(**edit):
        t = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in good.items()}
        for k, (i, v) in edit.items():
            t[k][i] = v
        return t

    root_kids = slice(good["child_begin"][0], good["child_begin"][1])
    assert len(good["child_tok"][root_kids]) >= 3
    unsorted = broken()
    unsorted["child_tok"][root_kids] = good["child_tok"][root_kids][::-1]
    deep = int(np.argmax(good["level"]))
    n = len(good["fail"])
    cases = {
        "sorted": unsorted,
        "outside": broken(child_node=(0, n)),
        "fail.*outside": broken(fail=(deep, -1)),
        "output.*outside": broken(output=(deep, n + 5)),
        "graph_root.*outside": broken(graph_root=(1, n)),
        "does not lower the level": broken(fail=(deep, deep)),
        "fail to itself": broken(fail=(0, 1)),
        "child_begin": broken(child_begin=(1, len(good["child_tok"]) + 1)),
    }
    for word, table in cases.items():
        with pytest.raises(capi.RsError, match=word) as e:
            capi.hotwords_check(table)
        assert e.value.code == capi.RS_EINVAL
    bad_level = broken()
    bad_level["max_level"] = 1
    with pytest.raises(capi.RsError, match="max_level"):
        capi.hotwords_check(bad_level)
    short = broken()
    short["level"] = short["level"][:-1]
    with pytest.raises(capi.RsError, match="length"):
        capi.hotwords_check(short)


# ---- the C checker with hotwords ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def toy():
    """six ragged utterances of the toy model (seed 3) with the reference's padding -> the float32 oracle projection, lengths (one
    row without frames), the plain search's results at K = 4 and the three graphs tests/k2_hotwords_ref.py cuts from them"""
    cfg = ZIPFORMER_TINY
    sd = synthetic_state_dict_k2(cfg, 3)
    audio, lens = synthetic_batch(6, 3.0, seed=5, ragged=True, min_seconds=0.7)
    fs = [oz.forward(cfg, sd, np.pad(audio[b, :lens[b]], PAD), "fp32")["joint_enc"].numpy() for b in range(6)]
    f = np.zeros((6, max(len(x) for x in fs), cfg.joiner_dim), np.float32)
    for b, x in enumerate(fs):
        f[b, :len(x)] = x
    el = [len(x) for x in fs]
    el[2] = 0
    plain = R.mbs_checker(cfg, sd, f, el, K=4)
    phrases = H.toy_graphs(plain)
    return types.SimpleNamespace(cfg=cfg, sd=sd, f=f, el=el, plain=plain, phrases=phrases,
                                 table=kh.concat([kh.build_graph(p) for p in phrases]), graph_of=[0, 1, -1, 2, -1, 0])


def bits(rows):
    return [(r["ids"], r["frames"], r["score_bits"]) for r in rows]


# The plain checker is the one the hotword checker replaced: its results on the toy batch (floats as bit patterns), by keywords.
# The checker is deterministic, its input here is not: the toy batch is the float32 oracle's encoder projection, and torch's CPU
# kernels differ by a few ulp from one machine to another (seen: the same tokens and frames, scores 2 - 8 ulp apart).  So tokens,
# frames and merge counts are held exactly and scores within LINE / 2, the tolerance of the float64 test below.
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "k2_mbs_checker_pins.json")) as _fh:
    PINS = {tuple(sorted(c["kw"].items())): c["rows"] for c in json.load(_fh)["cases"]}


def pinned(**kw):
    return PINS[tuple(sorted(kw.items()))]


def f32(pattern):
    return float(np.asarray([pattern], np.int32).view(np.float32)[0])


def assert_equals_pins(rows, want):
    assert len(rows) == len(want)
    for b, (r, w) in enumerate(zip(rows, want)):
        assert (r["ids"], r["frames"], r["merges"]) == (w["ids"], w["frames"], w["merges"]), b
        assert abs(r["score"] - f32(w["score_bits"])) < LINE / 2, (b, r["score"], f32(w["score_bits"]))
        assert [y for y, _ in r["final"]] == [y for y, _ in w["final"]], b
        assert all(abs(lp - f32(p)) < LINE / 2 for (_, lp), (_, p) in zip(r["final"], w["final"])), b


@pytest.mark.parametrize("K", [1, 2, 4, 8])
def test_checker_without_a_graph_is_the_plain_checker(toy, K):
    want = R.mbs_checker(toy.cfg, toy.sd, toy.f, toy.el, K=K)                          # no graph argument at all
    assert_equals_pins(want, pinned(K=K))
    assert bits(R.mbs_checker(toy.cfg, toy.sd, toy.f, toy.el, None, None, K=K)) == bits(want)
    got = R.mbs_checker(toy.cfg, toy.sd, toy.f, toy.el, toy.table, [-1] * 6, K=K)      # graphs in the call, none used
    assert bits(got) == bits(want)
    assert all(r["child_hits"] == r["fail_transitions"] == r["exits"] == 0 and r["finalize"] == 0.0 for r in got)
    assert [r["final"] for r in got] == [r["final"] for r in want] and [r["merges"] for r in got] == [r["merges"] for r in want]


def test_checker_with_graphs_equals_the_float64_restatement(toy):
    graphs = [H.ContextGraph(p) for p in toy.phrases]
    rows = excused = 0
    totals = dict(child_hits=0, fail_transitions=0, exits=0)
    finalized = differs = 0
    for kw in (dict(K=4), dict(K=2, blank_penalty=1.5), dict(K=8, length_norm=False)):
        chk = R.mbs_checker(toy.cfg, toy.sd, toy.f, toy.el, toy.table, toy.graph_of, **kw)
        plain = R.mbs_checker(toy.cfg, toy.sd, toy.f, toy.el, **kw)
        assert_equals_pins(plain, pinned(**kw))
        for b, g in enumerate(toy.graph_of):
            ref = H.hw_float64(toy.cfg, toy.sd, toy.f[b, :toy.el[b]], graphs[g] if g >= 0 else None, **kw)
            got = chk[b]
            rows += 1
            if g < 0:
                assert bits([got]) == bits([plain[b]])
            for k in totals:
                totals[k] += got[k]
            finalized += got["finalize"] != 0.0
            differs += got["ids"] != plain[b]["ids"]
            same = (got["ids"], got["frames"]) == (ref["ids"], ref["frames"])
            print(f"{kw} row {b} graph {g}: gap {ref['min_gap']:.2e} final gap {ref['final_gap']:.2e} same {same} hits {got['child_hits']} "
                  f"fails {got['fail_transitions']} exits {got['exits']} finalize {got['finalize']}")
            if same:
                assert got["merges"] == ref["merges"] and abs(got["score"] - ref["score"]) < LINE / 2, (kw, b)
                continue
            assert min(ref["min_gap"], ref["final_gap"]) <= LINE, f"{kw} row {b} differs although every gap exceeds {LINE}"
            first = next((t for t, gap in enumerate(ref["frame_gaps"]) if gap <= LINE), toy.el[b])
            cut = lambda r: [(i, t) for i, t in zip(r["ids"], r["frames"]) if t < first]     # noqa: E731
            assert cut(got) == cut(ref), f"{kw} row {b} differs before frame {first}"
            excused += 1
    print(f"rows {rows}, excused {excused}, counters {totals}, rows with a non-zero Finalize {finalized}, rows that differ from the plain search {differs}")
    assert excused * 8 <= rows, excused
    assert min(totals.values()) > 0 and finalized > 0 and differs > 0, "the graphs must be met: re-choose the inputs (toy_graphs)"


# ---- hand-built cases: a 6-symbol vocabulary, decoder and joiner replaced by tables (float64 restatement) ------------------------
TOY = types.SimpleNamespace(context_size=2, blank_id=0, unk_id=2)


def table(fn):
    return lambda t, ys: torch.log(torch.tensor(fn(t, ys[2:]), dtype=torch.float64))


def test_a_boosted_runner_up_overtakes():
    fn = table(lambda t, y: [.05, .5, 0.0, .4, .05, 0.0])
    plain = H.hw_float64(TOY, None, None, None, K=2, logits_fn=fn, n_frames=1, length_norm=False)
    assert plain["ids"] == [1]
    r = H.hw_float64(TOY, None, None, H.ContextGraph([((3,), 1.0)]), K=2, logits_fn=fn, n_frames=1, length_norm=False)
    assert r["ids"] == [3] and abs(r["score"] - (math.log(.4) + 1.0)) < 1e-12           # the phrase is complete: Finalize takes nothing
    # the selection itself sees no bonus: at K = 1 the runner-up is never expanded
    assert H.hw_float64(TOY, None, None, H.ContextGraph([((3,), 1.0)]), K=1, logits_fn=fn, n_frames=1)["ids"] == [1]


def test_a_partial_match_is_taken_back_at_a_mismatch():
    seq = [3, 4, 1]                                                         # the phrase is 3 4 5: the third token breaks it
    fn = table(lambda t, y: [(.9 if i == seq[t] else .02) if i != 2 else 0.0 for i in range(6)])
    g = H.ContextGraph([((3, 4, 5), 2.0)])
    plain = H.hw_float64(TOY, None, None, None, K=1, logits_fn=fn, n_frames=3)
    for n, bonus in ((1, 0.0), (2, 0.0), (3, 0.0)):                         # pending bonuses are taken back by Finalize, then by the mismatch
        r = H.hw_float64(TOY, None, None, g, K=1, logits_fn=fn, n_frames=n)
        assert r["ids"] == seq[:n] and r["bonus"] == [bonus]
    r = H.hw_float64(TOY, None, None, g, K=1, logits_fn=fn, n_frames=3)
    assert r["states"] == [()] and abs(r["score"] - plain["score"]) < 1e-12   # net 0, and back at the root before Finalize
    step = []
    st = g.root
    for tok in seq:
        d, st = g.step(st, tok)
        step.append(d)
    assert step == [2.0, 2.0, -4.0]


def test_a_match_pending_at_the_last_frame_is_taken_back_and_the_winner_changes():
    # frame 0: 3 (.45) or 1 (.55).  The phrase 3 4 gives [3] a pending +1.0: before Finalize [3] leads, after it [1] wins again
    fn = table(lambda t, y: [0.0, .55, 0.0, .45, 0.0, 0.0])
    g = H.ContextGraph([((3, 4), 1.0)])
    r = H.hw_float64(TOY, None, None, g, K=2, logits_fn=fn, n_frames=1, length_norm=False)
    assert r["states"] == [(), (3,)] and r["bonus"] == [0.0, 0.0]
    assert r["ids"] == [1] and abs(r["score"] - math.log(.55)) < 1e-12
    lp = dict((tuple(y), s) for y, s in r["final"])
    assert abs(lp[(3,)] - math.log(.45)) < 1e-12                              # +1.0 at the step, -1.0 at Finalize
    # with the one-token phrase the bonus is earned, stays, and [3] wins
    r = H.hw_float64(TOY, None, None, H.ContextGraph([((3,), 1.0)]), K=2, logits_fn=fn, n_frames=1, length_norm=False)
    assert r["ids"] == [3]


def test_merged_candidates_keep_the_first_ones_state():
    # frame 0: [3] (.6) and [] (.4).  frame 1: [3] + blank (.6 x .9) enters first, [] + 3 (.4 x .9, bonus +1 for the phrase 3 4,
    # state (3,)) merges into it.  The first one's state — also (3,), reached at frame 0 — stays; so do its timestamps.
    def fn(t, y):
        if t == 0:
            return [.4, 0.0, 0.0, .6, 0.0, 0.0]
        return [.9, .025, 0.0, .025, .025, .025] if y == [3] else [.025, .025, 0.0, .9, .025, .025]
    g = H.ContextGraph([((3, 4), 1.0)])
    r = H.hw_float64(TOY, None, None, g, K=2, logits_fn=table(fn), n_frames=2)
    assert r["merges"] == 1 and r["final"][0][0] == [3] and r["frames"] == [0] and r["states"][0] == (3,)
    want = np.logaddexp(math.log(.6) + 1.0 + math.log(.9), math.log(.4) + math.log(.9) + 1.0) - 1.0
    assert abs(r["final"][0][1] - want) < 1e-12
    # states that differ: the phrase 1 3 — [] + 3 stands at the root, [3]@0 + blank too; with the first token 1 instead
    def fn2(t, y):
        if t == 0:
            return [.4, .6, 0.0, 0.0, 0.0, 0.0]
        return [.05, .05, 0.0, .8, .05, .05]
    r = H.hw_float64(TOY, None, None, H.ContextGraph([((1, 3, 4), 1.0)]), K=2, logits_fn=table(fn2), n_frames=2)
    by = dict((tuple(y), st) for (y, _), st in zip(r["final"], r["states"]))
    assert by[(1, 3)] == (1, 3) and by[(3,)] == ()


def test_a_blank_extension_keeps_its_state():
    seq = [3, 0, 0, 4]
    fn = table(lambda t, y: [(.9 if i == seq[t] else .025) if i != 2 else 0.0 for i in range(6)])
    g = H.ContextGraph([((3, 4), 1.5)])
    r = H.hw_float64(TOY, None, None, g, K=1, logits_fn=fn, n_frames=3)
    assert r["ids"] == [3] and r["states"] == [(3,)] and r["bonus"] == [0.0]          # pending through two blanks, then Finalize
    r = H.hw_float64(TOY, None, None, g, K=1, logits_fn=fn, n_frames=4)
    assert r["ids"] == [3, 4] and r["frames"] == [0, 3] and r["bonus"] == [3.0] and r["states"] == [()]
    assert abs(r["score"] - (4 * math.log(.9) + 3.0)) < 1e-12


# ---- parsing and the public surface, without a GPU ---------------------------------------------------------------------------------
TOKENS = ["<blk>", "<sos/eos>", "<unk>", "東", "京", "都", "大", "阪", "a", "b"]


def test_phrases_scores_and_separators():
    assert kh.parse_hotwords("東京 :2.0/大阪/ 京都 :1") == [("東京", 2.0), ("大阪", 0.0), ("京都", 1.0)]
    assert kh.parse_hotwords(None) == [] and kh.parse_hotwords("") == [] and kh.parse_hotwords("/") == []
    assert kh.parse_hotwords(["東京 :4", (3, 4), ((5, 6), 2.0), ("大阪", 1.5), np.array([7, 8])]) == \
        [("東京", 4.0), ((3, 4), 0.0), ((5, 6), 2.0), ("大阪", 1.5), ((7, 8), 0.0)]
    with pytest.raises(ValueError, match="not a number"):
        kh.parse_hotwords("東京 :abc")
    enc = kh.encode(kh.parse_hotwords("東京 :2.0/大阪/a b"), TOKENS, 0, 2, hotwords_score=1.5)
    assert enc == [((3, 4), 2.0), ((6, 7), 1.5), ((8, 9), 1.5)]                       # own score, else hotwords_score; white space dropped
    assert kh.encode([("東京", 0.0)], TOKENS, 0, 2) == [((3, 4), kh.DEFAULT_SCORE)] and kh.DEFAULT_SCORE == 1.5


def test_hotwords_file(tmp_path):
    path = tmp_path / "hotwords.txt"
    path.write_text("東京 :2.0\n\n大阪\n   \n京都 :4\n", encoding="utf-8")
    assert kh.read_hotwords_file(str(path)) == [("東京", 2.0), ("大阪", 0.0), ("京都", 4.0)]
    g = kh.make_graph(["大阪 :1"], TOKENS, 0, 2, hotwords_score=1.0, hotwords_file=str(path))
    assert g.n_phrases == 4 and g.key[0] == ((3, 4), 2.0) and g.key[-1] == ((6, 7), 1.0)
    assert kh.make_graph(None, TOKENS, 0, 2) is None and kh.make_graph("", TOKENS, 0, 2) is None


def test_an_unknown_character_skips_the_phrase_with_a_warning():
    with pytest.warns(UserWarning, match="名.*not in tokens.txt"):
        enc = kh.encode(kh.parse_hotwords("東京/名古屋/大阪"), TOKENS, 0, 2)
    assert [ids for ids, _ in enc] == [(3, 4), (6, 7)]
    with pytest.warns(UserWarning):
        assert kh.make_graph("名古屋", TOKENS, 0, 2) is None                         # nothing left: no graph


def test_blank_and_unk_ids_raise():
    for bad in ([(3, 0)], [(2,)], [((4, 2), 1.0)]):
        with pytest.raises(ValueError, match="blank or <unk>"):
            kh.encode(kh.parse_hotwords(bad), TOKENS, 0, 2)
    with pytest.raises(ValueError, match="outside the vocabulary"):
        kh.encode(kh.parse_hotwords([(3, 99)]), TOKENS, 0, 2)
    with pytest.raises(ValueError, match="integers"):
        kh.encode(kh.parse_hotwords([(3, 4.5)]), TOKENS, 0, 2)


def test_hotwords_with_greedy_search_raise(tmp_path):
    cfg = ZIPFORMER_TINY
    path = tmp_path / "h.txt"
    path.write_text("あ\n", encoding="utf-8")
    for kw in (dict(hotwords=["あ"]), dict(hotwords="あ/い"), dict(hotwords_file=str(path))):
        with pytest.raises(ValueError, match="modified_beam_search"):
            search_config(cfg, **kw)
        with pytest.raises(ValueError, match="modified_beam_search"):
            K2Model(cfg, {}, synthetic_tokens(cfg.vocab_size), **kw)
        with pytest.raises(ValueError, match="modified_beam_search"):
            hfm.load_model(**kw)
        assert search_config(cfg, "modified_beam_search", **kw) == search_config(cfg, "modified_beam_search")
    assert search_config(cfg, hotwords=[], hotwords_file="") == cfg                   # empty hotwords are no hotwords
    with pytest.raises(ValueError, match="hotwords_score"):
        search_config(cfg, "modified_beam_search", hotwords_score=float("nan"))
    with pytest.raises(FileNotFoundError):
        hfm.load_model(decoding_method="modified_beam_search", hotwords_file=str(tmp_path / "missing.txt"))


def test_a_stream_level_graph_replaces_the_model_level_one():
    model_graph = kh.make_graph("東京", TOKENS, 0, 2)
    own = kh.make_graph("大阪 :2", TOKENS, 0, 2)
    streams = [k2model._Stream(), k2model._Stream(own), k2model._Stream()]
    assert k2model.stream_graphs(model_graph, streams) == [model_graph, own, model_graph]
    assert k2model.stream_graphs(None, streams) == [None, own, None]
    assert k2model.stream_graphs(None, [k2model._Stream()]) is None                   # nothing to bias: the plain search
    assert own.key == (((6, 7), 2.0),) and model_graph.key != own.key


def test_the_new_entry_points_are_exported_within_abi_7():
    lib = ctypes.CDLL(rs_build.build())
    assert lib.rs_abi_version() == 7
    names = {"rs_rnnt_mbs_hotwords", "rs_rnnt_mbs_hotwords_workspace_bytes", "rs_hotwords_check"}
    assert all(hasattr(lib, n) for n in names) and names <= set(capi.EXPORTS)
    lib.rs_rnnt_mbs_hotwords_workspace_bytes.restype = ctypes.c_size_t
    assert lib.rs_rnnt_mbs_hotwords_workspace_bytes(None, 4, 4, 100, 100) == 0       # no context: invalid
    assert [f[0] for f in capi.RsHotwords._fields_][:11] == list(capi.HOTWORD_ARRAYS)
