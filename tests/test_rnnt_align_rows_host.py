"""CPU: several texts per utterance on one lattice (rs_rnnt_align_rows, rs_rnnt_token_scores_rows) — what needs no GPU.

  * the sharing rule: tests/rnnt_align_rows_ref.py (the rule of include/rs_asr.h restated in plain Python) against
    reazonspeech_amd/csrc/rs_align_rows_plan.h, the header the plan kernel itself calls, through a stand-alone program built with
    g++ -Wall -Werror, once plain and once under AddressSanitizer + UBSan.  Hand-built groups: a duplicate text, a text that is a
    prefix of an earlier one, a first-label mismatch, a donor chain of depth 2, an infeasible and a bad row placed first, a skipped
    row inside a group, a group of 64 and a group of 65; row_utt out of range and decreasing
  * the entry points are exported, declared, bound and guarded, and the ABI is still 7
  * `AsrModel.align_candidates` / `score_texts`: argument errors before anything touches a GPU
"""
import ctypes
import os
import re
import subprocess

import pytest

import rnnt_align_rows_ref as RR
from reazonspeech_amd import build as rs_build
from reazonspeech_amd.runtime import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = os.path.join(ROOT, "tests", "align_rows_host_main.cpp")
HEADER = os.path.join(ROOT, "reazonspeech_amd", "csrc", "rs_align_rows_plan.h")
V, BLANK = 50, 49
a, b, c, d, x, y, z, f = 1, 2, 3, 4, 11, 12, 13, 20


def groups():
    """name -> dict(T [B], row_utt [R], texts [R], one, counts or None)"""
    issue = [[a, b, c, d], [a, b, x, y], [a, b, x, z], [a, b, c, d], [a, b], [f]]
    g = {
        # the scene of the GPU test: a chain through two donors, a duplicate, a prefix, nothing shared; the empty text alone; an
        # infeasible first row (5 labels on 1 frame, one label per frame) that must not become a donor; a skipped row
        "issue-one": dict(T=[9, 5, 1], row_utt=[0] * 6 + [1] + [2, -1, 2, 2], one=1,
                          texts=issue + [[]] + [[a, b, c, d, x], [a, a, a], [a], [a]]),
        "issue-standard": dict(T=[9, 5, 1], row_utt=[0] * 6 + [1] + [2, -1, 2, 2], one=0,
                               texts=issue + [[]] + [[a, b, c, d, x], [a, a, a], [a, b], [a, b, c]]),
        "duplicate": dict(T=[4], row_utt=[0, 0], one=0, texts=[[a, b, c], [a, b, c]]),
        "prefix": dict(T=[4], row_utt=[0, 0, 0], one=0, texts=[[a, b, c], [a, b], []]),
        "first-label": dict(T=[4], row_utt=[0, 0], one=0, texts=[[a, b, c], [x, b, c]]),
        "chain-2": dict(T=[6], row_utt=[0, 0, 0], one=1, texts=[[a, b, c, d], [a, b, x, y], [a, b, x, z]]),
        "first-attains": dict(T=[6], row_utt=[0, 0, 0, 0], one=0, texts=[[a, b, c], [a, b, d], [a, x], [a, b, y]]),
        "bad-first": dict(T=[6], row_utt=[0, 0, 0], one=0, texts=[[a, BLANK, c], [a, b], [a, b, c]]),
        "bad-count-first": dict(T=[6], row_utt=[0, 0, 0], one=0, texts=[[a, b, c], [a, b], [a, b, c]], counts=[4, 2, 3]),
        "negative-count": dict(T=[6], row_utt=[0, 0], one=0, texts=[[a, b, c], [a, b]], counts=[-1, 2]),
        "no-frames": dict(T=[0, 3], row_utt=[0, 0, 1, 1], one=0, texts=[[], [a], [a], [a]]),
        "skipped-inside": dict(T=[5, 5], row_utt=[0, -1, 0, -1, -1, 1, 1], one=0, texts=[[a, b], [a, b], [a, b, c], [], [a], [a, b], [a]]),
        "all-skipped": dict(T=[5], row_utt=[-1, -1], one=0, texts=[[a], [a]]),
        "group-64": dict(T=[3], row_utt=[0] * 64, one=0, texts=[[a] * (k % 5) + [b] * (k % 3) for k in range(64)]),
        "group-64-chain": dict(T=[70], row_utt=[0] * 64, one=1, texts=[[a] * (k + 1) + [b] for k in range(64)]),
        "group-65": dict(T=[3], row_utt=[0] * 65, one=0, texts=[[a]] * 65),
        "group-65-with-skips": dict(T=[3, 3], row_utt=[0] * 30 + [-1] * 4 + [0] * 35 + [1], one=0, texts=[[a]] * 70),
        "utt-too-large": dict(T=[3, 3], row_utt=[0, 2], one=0, texts=[[a], [a]]),
        "utt-below-minus-one": dict(T=[3, 3], row_utt=[-2, 1], one=0, texts=[[a], [a]]),
        "decrease": dict(T=[3, 3], row_utt=[0, 1, -1, 0], one=0, texts=[[a]] * 4),
    }
    return g


def block(case):
    texts, counts = case["texts"], case.get("counts")
    u_cap = max([len(t) for t in texts] + [1])
    n = counts if counts is not None else [len(t) for t in texts]
    ids = [t + [0] * (u_cap - len(t)) for t in texts]
    lines = [f"{len(case['T'])} {len(texts)} {u_cap} {V} {BLANK} {case['one']}", " ".join(map(str, case["T"])),
             " ".join(map(str, case["row_utt"])), " ".join(map(str, n))] + [" ".join(map(str, row)) for row in ids]
    return "\n".join(lines) + "\n"


@pytest.fixture(scope="module", params=["plain", "asan"])
def exe(request, tmp_path_factory):
    extra = [] if request.param == "plain" else ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    out = os.path.join(str(tmp_path_factory.mktemp("align_rows")), "align_rows_" + request.param)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-g", "-O1"] + extra + [MAIN, "-o", out], check=True, capture_output=True, text=True)
    return out


def test_the_restatement_on_the_hand_built_groups():
    g = groups()
    p = RR.plan(g["chain-2"]["row_utt"], g["chain-2"]["T"], g["chain-2"]["texts"], V, BLANK, 1)
    assert (p["m"], p["donor"]) == ([0, 2, 3], [-1, 0, 1]) and p["stats"] == (6 * 5 + 6 * 3 + 6 * 2, 3 * 6 * 5)
    p = RR.plan(g["duplicate"]["row_utt"], [4], g["duplicate"]["texts"], V, BLANK, 0)
    assert (p["m"], p["donor"], p["owned"]) == ([0, 3], [-1, 0], [16, 4])        # a duplicate computes its last column alone
    p = RR.plan(g["prefix"]["row_utt"], [4], g["prefix"]["texts"], V, BLANK, 0)
    assert (p["m"], p["donor"], p["owned"]) == ([0, 2, 0], [-1, 0, -1], [16, 4, 4])
    p = RR.plan(g["first-label"]["row_utt"], [4], g["first-label"]["texts"], V, BLANK, 0)
    assert (p["m"], p["donor"]) == ([0, 0], [-1, -1]) and p["stats"] == (32, 32)
    p = RR.plan(g["first-attains"]["row_utt"], [6], g["first-attains"]["texts"], V, BLANK, 0)
    assert p["donor"] == [-1, 0, 0, 0] and p["m"] == [0, 2, 1, 2]                # rows 0 and 1 both share two labels: row 0 gives
    p = RR.plan(g["bad-first"]["row_utt"], [6], g["bad-first"]["texts"], V, BLANK, 0)
    assert (p["lat_u"], p["m"], p["donor"]) == ([-1, 2, 3], [0, 0, 2], [-1, -1, 1])
    p = RR.plan(g["issue-one"]["row_utt"], g["issue-one"]["T"], g["issue-one"]["texts"], V, BLANK, 1)
    assert p["lat_u"] == [4, 4, 4, 4, 2, 1, 0, -1, -1, 1, 1] and p["donor"] == [-1, 0, 1, 0, 0, -1, -1, -1, -1, -1, 9]
    assert p["m"] == [0, 2, 3, 4, 2, 0, 0, 0, 0, 0, 1]
    assert RR.plan(g["group-64"]["row_utt"], [3], g["group-64"]["texts"], V, BLANK, 0)["err"] == 0
    deep = RR.plan(g["group-64-chain"]["row_utt"], [70], g["group-64-chain"]["texts"], V, BLANK, 1)
    assert deep["donor"] == [-1] + list(range(63)) and deep["m"] == list(range(64))      # a chain 63 deep
    assert RR.plan(g["group-65"]["row_utt"], [3], g["group-65"]["texts"], V, BLANK, 0)["err"] == RR.GROUP
    assert RR.plan(g["group-65-with-skips"]["row_utt"], [3, 3], g["group-65-with-skips"]["texts"], V, BLANK, 0)["err"] == RR.GROUP
    assert RR.plan(g["utt-too-large"]["row_utt"], [3, 3], [[a], [a]], V, BLANK, 0)["err"] == RR.BAD_UTT
    assert RR.plan(g["utt-below-minus-one"]["row_utt"], [3, 3], [[a], [a]], V, BLANK, 0)["err"] == RR.BAD_UTT
    assert RR.plan(g["decrease"]["row_utt"], [3, 3], [[a]] * 4, V, BLANK, 0)["err"] == RR.DECREASE


def test_the_header_equals_the_restatement(exe, tmp_path):
    cases = list(groups().items())
    path = tmp_path / "groups.txt"
    path.write_text("".join(block(c) for _, c in cases))
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stdout[-400:], r.stderr[-2000:])
    lines = iter(r.stdout.splitlines())
    for name, case in cases:
        want = RR.plan(case["row_utt"], case["T"], case["texts"], V, BLANK, case["one"], counts=case.get("counts"))
        assert next(lines) == f"err {want['err']}", name
        if want["err"]:
            continue
        for r_ in range(len(case["texts"])):
            assert next(lines) == f"row {r_} {want['lat_u'][r_]} {want['m'][r_]} {want['donor'][r_]} {want['owned'][r_]}", name
        assert next(lines) == f"stats {want['stats'][0]} {want['stats'][1]}", name
    assert next(lines, None) is None


def test_the_header_is_hip_free_and_is_the_one_the_kernels_call():
    text = open(HEADER).read()
    code = re.sub(r"//.*", "", text)
    assert "hip/" not in code and "#include <hip" not in code
    assert re.findall(r'#include "([^"]+)"', open(MAIN).read()) == ["../reazonspeech_amd/csrc/rs_align_rows_plan.h"]
    for src in ("k_rnnt_align.hip", "k_rnnt_scores.hip"):
        body = open(os.path.join(ROOT, "reazonspeech_amd", "csrc", src)).read()
        assert '#include "rs_align_rows_plan.h"' in body and "rs_align_rows_check_row(" in body
    assert "rs_align_rows_share(" in open(os.path.join(ROOT, "reazonspeech_amd", "csrc", "k_rnnt_align.hip")).read()


def test_the_entry_points_are_exported_declared_and_guarded():
    names = {"rs_rnnt_align_rows", "rs_rnnt_align_rows_workspace_bytes", "rs_rnnt_token_scores_rows", "rs_rnnt_token_scores_rows_workspace_bytes"}
    lib = ctypes.CDLL(rs_build.build())
    assert lib.rs_abi_version() == 7
    assert all(hasattr(lib, n) for n in names)              # fails without the feature
    assert names <= set(capi.EXPORTS)
    loaded = capi.load()
    assert len(loaded.rs_rnnt_align_rows.argtypes) == len(loaded.rs_rnnt_align.argtypes) + 3               # row_utt, R, stats
    assert len(loaded.rs_rnnt_token_scores_rows.argtypes) == len(loaded.rs_rnnt_token_scores.argtypes) + 2  # row_utt, R
    for n in ("rs_rnnt_align_rows_workspace_bytes", "rs_rnnt_token_scores_rows_workspace_bytes"):
        assert getattr(loaded, n).restype is ctypes.c_size_t
    lib.rs_rnnt_align_rows_workspace_bytes.restype = ctypes.c_size_t
    assert lib.rs_rnnt_align_rows_workspace_bytes(None, 2, 4, 10, 10) == 0                                  # no context: invalid
    header = open(os.path.join(ROOT, "include", "rs_asr.h"), encoding="utf-8").read()
    assert all(re.search(r"\b" + n + r"\(", header) for n in names)
    assert re.search(r"#define RS_ALIGN_ROWS_PER_UTT_MAX 64\b", header) and capi.ALIGN_ROWS_PER_UTT_MAX == 64 == RR.MAX_ROWS_PER_UTT
    assert re.search(r"RS_ALIGN_NO_SHARING = 2\b", header) and capi.ALIGN_NO_SHARING == 2
    family = open(os.path.join(ROOT, "reazonspeech_amd", "csrc", "rs_family.h"), encoding="utf-8").read()
    for n in names:
        assert re.search(r"X\(" + n + r", CZ, ", family), n  # Conformer and Zipformer contexts, refused for AV-HuBERT


# ---- the keywords, the re-ranking and the result types: no GPU ------------------------------------------------------------------
import importlib  # noqa: E402
import inspect  # noqa: E402
import types  # noqa: E402

import numpy as np  # noqa: E402

from reazonspeech_amd.espnet.asr import model as em  # noqa: E402
from reazonspeech_amd.k2.asr import huggingface as hfm, interface as ki  # noqa: E402
from reazonspeech_amd.k2.asr.model import K2Model, _Stream, search_config, synthetic_tokens  # noqa: E402
from reazonspeech_amd.nemo.asr import interface as ni  # noqa: E402
from reazonspeech_amd.runtime import rescore as rescoring  # noqa: E402
from reazonspeech_amd.runtime.config import ESPNET_TINY, TINY  # noqa: E402
from reazonspeech_amd.runtime.k2_config import ZIPFORMER_TINY  # noqa: E402
from reazonspeech_amd.runtime.model import AlignedBatch, AsrModel, DecodedBatch, RescoredBatch  # noqa: E402

k2tr = importlib.import_module("reazonspeech_amd.k2.asr.transcribe")
ntr = importlib.import_module("reazonspeech_amd.nemo.asr.transcribe")
etr = importlib.import_module("reazonspeech_amd.espnet.asr.transcribe")
MBS = dict(decoding_method="modified_beam_search")


class FakeAm:
    RESCORE_KEYS, nbest_plan, rescore_plan = AsrModel.RESCORE_KEYS, AsrModel.nbest_plan, AsrModel.rescore_plan

    def __init__(self, cfg, nbest=0, rescore=None):
        self.cfg, self.nbest, self.rescore = cfg, nbest, rescore


def test_argument_errors_of_the_new_keywords_come_before_anything_is_loaded():
    need = "needs a beam search and nbest >= 2"
    cfg = ZIPFORMER_TINY
    for call in (lambda **kw: hfm.load_model(**kw), lambda **kw: K2Model(cfg, {}, synthetic_tokens(cfg.vocab_size), **kw)):
        with pytest.raises(ValueError, match="must be None, 'likelihood' or 'norm_likelihood'"):
            call(nbest=2, rescore="best", **MBS)
        with pytest.raises(ValueError, match=need):
            call(nbest=1, rescore="likelihood", **MBS)
        with pytest.raises(ValueError, match=need):
            call(rescore="norm_likelihood", **MBS)
    with pytest.raises(ValueError, match=need):
        ntr.load_model(config=TINY, decoding="greedy_batch", rescore="likelihood", nbest=1)
    with pytest.raises(ValueError, match=need):
        ntr.load_model(config=TINY, decoding="alsd", beam_size=4, rescore="likelihood")
    with pytest.raises(ValueError, match="must be None"):
        ntr.load_model(config=TINY, decoding="alsd", beam_size=4, nbest=2, rescore=1)
    with pytest.raises(ValueError, match=need):
        etr.load_model(config=ESPNET_TINY, beam_size=1, nbest=1, rescore="likelihood")
    with pytest.raises(ValueError, match=need):
        etr.load_model(config=ESPNET_TINY, beam_size=4, rescore="likelihood")
    with pytest.raises(ValueError, match="must be None"):
        etr.load_model(config=ESPNET_TINY, beam_size=4, nbest=2, rescore="likelyhood")
    # the runtime model's own plan, for every search
    beam = FakeAm(TINY.with_(decoding="alsd", beam_size=4), nbest=3)
    assert beam.rescore_plan() is None and beam.rescore_plan("likelihood") == "likelihood" and beam.rescore_plan("norm_likelihood", 2) == "norm_likelihood"
    assert FakeAm(beam.cfg, 3, "likelihood").rescore_plan() == "likelihood" and beam.rescore_plan(False) is None
    for am, n in ((beam, 1), (beam, 0), (FakeAm(TINY, 0), 1), (FakeAm(beam.cfg, 0), None)):
        with pytest.raises(ValueError, match=need):
            am.rescore_plan("likelihood", n)
    with pytest.raises(ValueError, match="must be None"):
        beam.rescore_plan("loglik")
    for fn in (hfm.load_model, ntr.load_model, etr.load_model, AsrModel.__init__, K2Model.__init__, em.EspnetModel.__init__):
        assert inspect.signature(fn).parameters["rescore"].default is None
    assert inspect.signature(ntr.transcribe).parameters["rescore"].default is None
    assert inspect.signature(em.EspnetModel.recognize_batch).parameters["rescore"].default is None
    sig = inspect.signature(AsrModel.align_candidates).parameters
    assert (sig["max_batch"].default, sig["one_per_frame"].default, sig["share"].default) == (256, None, True)
    am = AsrModel.__new__(AsrModel)
    am.cfg = TINY
    with pytest.raises(ValueError, match="2 waveforms but 1 candidate lists"):
        am.align_candidates([np.zeros(8), np.zeros(8)], [[[1]]])
    with pytest.raises(ValueError, match="a text of 2048 tokens"):
        am.align_candidates([np.zeros(8)], [[[1] * 2048]])
    am.rescore, am.token_scores, am.nbest = "likelihood", False, 2
    with pytest.raises(ValueError, match="rescore is on: transcribe_waveforms_sharded"):
        am.transcribe_waveforms_sharded([np.zeros(8)])
    for pkg in ("nemo", "k2", "espnet"):
        mod = importlib.import_module(f"reazonspeech_amd.{pkg}.asr")
        with pytest.raises(ValueError, match="1 audios but 2 lists of texts"):
            mod.score_texts_batch(None, [None], [[], []])


def test_the_existing_types_keep_their_fields():
    assert list(DecodedBatch.__dataclass_fields__)[-2:] == ["nbest", "token_logprobs"]
    assert list(RescoredBatch.__dataclass_fields__) == list(DecodedBatch.__dataclass_fields__) + ["rescored"]
    assert list(AlignedBatch.__dataclass_fields__) == ["frames", "token_logprobs", "log_likelihood", "alignment_log_prob", "enc_lens", "feasible"]
    new = ["log_likelihood", "alignment_log_prob", "norm_log_likelihood", "search_rank"]
    for iface in (ni, ki):
        assert list(iface.RescoredTranscribeResult.__dataclass_fields__) == list(iface.NBestTranscribeResult.__dataclass_fields__) + new
        assert issubclass(iface.RescoredTranscribeResult, iface.NBestTranscribeResult)
    assert issubclass(em._RescoredHypothesis, em._NBestHypothesis)


def test_reranking_and_ties():
    assert rescoring.order([-3.0, -1.0, -2.0], [1, 1, 1], "likelihood") == [1, 2, 0]
    assert rescoring.order([-3.0, -3.0, -2.0, -3.0], [1, 2, 1, 1], "likelihood") == [2, 0, 1, 3]             # ties keep the search's order
    assert rescoring.order([-3.0, -4.0], [1, 2], "norm_likelihood") == [1, 0] and rescoring.order([-3.0, -4.0], [1, 2], "likelihood") == [0, 1]
    assert rescoring.order([-2.0, -1.0], [0, 1], "norm_likelihood") == [1, 0]                                 # / max(len, 1)
    assert rescoring.order([float("-inf"), -5.0, float("nan")], [1, 1, 1], "likelihood") == [1, 0, 2]
    assert rescoring.order([], [], "likelihood") == []
    with pytest.raises(ValueError):
        rescoring.order([-1.0], [1], "score")
    # K2Model.decode_streams over a faked runtime model: every entry scored, the list re-ranked, the result its entry 0
    cfg = search_config(ZIPFORMER_TINY, **MBS)
    model = K2Model.__new__(K2Model)
    model.cfg, model.tokens, model.hotwords = cfg, synthetic_tokens(cfg.vocab_size, 3), None
    lists = [[([5, 6], [1, 4], -1.5, -0.375), ([5], [2], -2.5, -0.8125), ([5, 6, 7], [1, 4, 5], -2.75, -0.7)], []]
    for key, want in (("likelihood", [1, 0, 2]), ("norm_likelihood", [2, 0, 1])):      # -4 / 2, -3 / 1, -4 / 3
        for with_scores in (False, True):
            lp = [[-0.25, -0.5], [-0.75], [-0.1, -0.2, -0.3]]
            scored = [[(-4.0, -4.5, lp[0] if with_scores else None), (-3.0, -3.25, lp[1] if with_scores else None),
                       (-4.0, -4.75, lp[2] if with_scores else None)], []]
            decoded = RescoredBatch([[5, 6], []], [[1, 4], []], [9, 0], [-1.5, 0.0], nbest=lists, rescored=scored,
                                    token_logprobs=[lp[0], []] if with_scores else None)
            model.am = types.SimpleNamespace(transcribe_waveforms=lambda waves, **kw: decoded, rescore=key)
            streams = [_Stream(), _Stream()]
            model.decode_streams(streams)
            r = streams[0].result
            assert r.nbest[0] is r and [e.search_rank for e in r.nbest] == want
            assert [e.log_likelihood for e in r.nbest] == [scored[0][k][0] for k in want]
            assert [e.alignment_log_prob for e in r.nbest] == [scored[0][k][1] for k in want]
            assert [e.norm_log_likelihood for e in r.nbest] == [scored[0][k][0] / len(lists[0][k][0]) for k in want]
            assert [e.log_prob for e in r.nbest] == [lists[0][k][2] for k in want]
            assert [e.token_log_probs for e in r.nbest] == [lp[k] if with_scores else None for k in want]
            assert streams[1].result.nbest == [] and streams[1].result.log_likelihood is None
            res = k2tr._result(streams[0])
            assert type(res) is ki.RescoredTranscribeResult and all(type(e) is ki.RescoredTranscribeResult for e in res.nbest)
            assert [e.search_rank for e in res.nbest] == want and res.text == r.text == res.nbest[0].text
            assert (res.log_likelihood, res.search_rank) == (r.log_likelihood, want[0])
            assert [e.token_logprobs for e in res.nbest] == [lp[k] if with_scores else None for k in want]
    # EspnetModel._nbest_entries on a faked batch
    m = em.EspnetModel.__new__(em.EspnetModel)
    m.token_list = em.synthetic_token_list(ESPNET_TINY.vocab_size, 11)
    m.am = types.SimpleNamespace(rescore="likelihood")
    batch = RescoredBatch([[5, 6]], [[1, 4]], [9], [-1.5], nbest=lists[:1], rescored=[[(-4.0, -4.5, None), (-3.0, -3.25, None), (-4.0, -4.75, None)]])
    entries = m._nbest_entries(batch, 0)
    assert [e[2] for e in entries] == [[5], [5, 6], [5, 6, 7]] and [e[3].search_rank for e in entries] == [1, 0, 2]
    assert [type(e[3]) for e in entries] == [em._RescoredHypothesis] * 3 and entries[0][3].log_likelihood == -3.0
    assert entries[2][3].norm_log_likelihood == -4.0 / 3 and entries[0][3].score == -2.5


def test_rescore_off_returns_todays_objects():
    cfg = search_config(ZIPFORMER_TINY, **MBS)
    model = K2Model.__new__(K2Model)
    model.cfg, model.tokens, model.hotwords = cfg, synthetic_tokens(cfg.vocab_size, 3), None
    lists = [[([5, 6], [1, 4], -1.5, -0.375), ([5], [2], -2.5, -0.8125)]]
    decoded = DecodedBatch([[5, 6]], [[1, 4]], [9], [-1.5], nbest=lists, token_logprobs=[[-0.25, -0.5]])
    model.am = types.SimpleNamespace(transcribe_waveforms=lambda waves, **kw: decoded, rescore=None)
    st = _Stream()
    model.decode_streams([st])
    res = k2tr._result(st)
    assert type(res) is ki.NBestTranscribeResult and type(res.nbest[1]) is ki.NBestTranscribeResult
    assert st.result.nbest[0] is st.result and st.result.log_likelihood is None and st.result.search_rank is None
    assert res.nbest[1].token_logprobs is None and res.token_logprobs == [-0.25, -0.5]        # the runners-up carry none, as before
    m = em.EspnetModel.__new__(em.EspnetModel)
    m.token_list = em.synthetic_token_list(ESPNET_TINY.vocab_size, 11)
    entries = m._nbest_entries(decoded, 0)
    assert [type(e[3]) for e in entries] == [em._NBestHypothesis] * 2 and entries[1][3].token_logprobs is None
    assert entries[0][3].token_logprobs == [-0.25, -0.5] and not hasattr(entries[0][3], "log_likelihood")
    assert FakeAm(TINY.with_(decoding="alsd", beam_size=4), nbest=3).rescore_plan() is None


def test_a_refused_value_leaves_the_option_and_an_empty_list_keeps_the_type():
    cfg = search_config(ZIPFORMER_TINY, **MBS)
    model = K2Model.__new__(K2Model)
    model.cfg, model.tokens, model.hotwords = cfg, synthetic_tokens(cfg.vocab_size, 3), None
    model.am = FakeAm(cfg, nbest=3, rescore="likelihood")
    for bad in ("best", 1):
        with pytest.raises(ValueError, match="must be None"):
            model.rescore = bad
        assert model.rescore == "likelihood"               # one bad assignment does not turn the model's rescoring off
    model.am.nbest = 1
    with pytest.raises(ValueError, match="nbest >= 2"):
        model.rescore = "norm_likelihood"
    assert model.rescore == "likelihood"
    model.am.nbest = 3
    model.rescore = "norm_likelihood"
    assert model.rescore == "norm_likelihood"
    model.rescore = None
    assert model.rescore is None
    # nemo's per-call keyword: the plan is made before the model is touched
    am = FakeAm(TINY.with_(decoding="alsd", beam_size=4), nbest=3, rescore="likelihood")
    for kw in (dict(rescore="best"), dict(rescore="likelihood", nbest=1)):
        with pytest.raises(ValueError):
            ntr.transcribe(am, None, None, **kw)
        assert am.rescore == "likelihood"
    # a stream without a hypothesis: the same result type as its neighbours, with an empty list
    decoded = RescoredBatch([[5], []], [[1], []], [9, 0], [-1.0, 0.0], nbest=[[([5], [1], -1.0, -0.5)], []], rescored=[[(-2.0, -2.5, None)], []])
    model.am = types.SimpleNamespace(transcribe_waveforms=lambda waves, **kw: decoded, rescore="likelihood")
    streams = [_Stream(), _Stream()]
    model.decode_streams(streams)
    got = [k2tr._result(st) for st in streams]
    assert [type(r) for r in got] == [ki.RescoredTranscribeResult] * 2 and got[1].nbest == [] and got[1].log_likelihood is None
    assert got[0].log_likelihood == -2.0 and streams[1].result.rescore_key == "likelihood"
