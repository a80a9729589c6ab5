"""CPU: n-best lists from ESPnet's default beam search (rs_rnnt_beam_nbest, csrc/k_rnnt_beam.hip; the ranking rule — upstream's
`sort_nbest(kept_hyps)[:nbest]` — is stated in include/rs_asr.h): the C checker that restates the search with its ranked list
(tests/espnet_beam_nbest_checker.c)

  * with nbest = 1 against the existing checker oracle/espnet_beam.c through its loader, bit for bit, on the toy fixtures of
    tests/test_oracle_espnet_beam.py (the ESPnet decoder at three beams and the NeMo-shaped one: two LSTM layers, blank last);
  * with nbest = N: entry 0 is the nbest = 1 result, the list is ordered by norm_scores, and the list for every n < N is a prefix
    of it (equal label sequences may appear twice: upstream keeps them);
  * hand-built cases on injected logits, each asserting by the checker's counters that it reaches its edge: a kept list longer than
    nbest, duplicates kept, a tie resolved by list position, score norm on and off (the norm changes the order);
  * against a float64 restatement that exposes the kept list (tests/espnet_beam_nbest_ref.py beam_float64; oracle/espnet.py's returns
    the best hypothesis only), scores only, entries matched by label sequence and frame-free.  The deviation line is the one
    tests/test_oracle_espnet_beam.py carries: |float32 - float64| <= 1e-4 x max(1, |score|).  Every utterance of the three
    ESPnet toys takes part; that its adjacent float64 norms differ by more than ten times that line is asserted for each, so that
    order is not what is compared;
  * the Python surface over fake models: result assembly, argument errors, off returns today's types, the exports."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

import espnet_beam_nbest_ref as EB
from oracle import greedy as og
from reazonspeech_amd import build as rs_build
from reazonspeech_amd.espnet.asr import load_model
from reazonspeech_amd.espnet.asr.model import EspnetModel, _NBestHypothesis, check_nbest, synthetic_token_list
from reazonspeech_amd.runtime import capi
from reazonspeech_amd.runtime.config import ESPNET_TINY, TINY
from reazonspeech_amd.runtime.model import DecodedBatch
from reazonspeech_amd.runtime.weights import synthetic_state_dict
from test_oracle_espnet_beam import _inputs

LINE = 1e-4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def toys():
    """(cfg, sd, f, lens, beam) of the toy fixtures: the ESPnet decoder on the oracle's projection of two 1 s utterances, the second
    cut to one frame in one of them; the NeMo-shaped decoder on random projections with an empty row"""
    out = []
    for beam, bias, seed in ((4, 12.0, 0), (20, 12.0, 1), (3, 12.0, 2)):
        sd, f, lens = _inputs(ESPNET_TINY, seed, 2, 1.0, bias)
        lens = lens.numpy().copy()
        if seed == 2:
            lens[1] = 1
        out.append((ESPNET_TINY, sd, f.numpy(), lens, beam))
    g = torch.Generator().manual_seed(3)
    f = (torch.randn((3, 14, TINY.joint_hidden), generator=g) * 1.2).numpy()
    out.append((TINY, synthetic_state_dict(TINY, 11, blank_bias=6.0), f, np.asarray([14, 9, 0], np.int32), 5))
    return out


def test_nbest_1_is_the_existing_checker_bit_for_bit(toys):
    for cfg, sd, f, lens, beam in toys:
        for score_norm in (True, False):
            want = og.espnet_beam(cfg, sd, f, lens, beam=beam, score_norm=score_norm, max_pops=64 * beam, with_frames=True)
            got = EB.nbest_checker(cfg, sd, f, lens, 1, beam=beam, score_norm=score_norm, max_pops=64 * beam)
            for b, (g, w) in enumerate(zip(got, want)):
                assert len(g["entries"]) == 1 and g["pops"] == w[3], (beam, score_norm, b)
                assert g["entries"][0][:3] == (w[0], w[1], EB.bits(w[2])), (beam, score_norm, b)
    assert got[2]["entries"] == [([], [], 0, 0)] and got[2]["kept"] == 1            # no frames: the start hypothesis alone


def test_the_list_is_ranked_and_every_shorter_list_is_its_prefix(toys):
    kept_longer = 0
    for cfg, sd, f, lens, beam in toys:
        N = min(beam, 8)
        for score_norm in (True, False):
            full = EB.nbest_checker(cfg, sd, f, lens, N, beam=beam, score_norm=score_norm, max_pops=64 * beam)
            for b, row in enumerate(full):
                ent = row["entries"]
                assert len(ent) == min(N, row["kept"]) and (row["kept"] >= beam or lens[b] == 0)
                kept_longer += row["kept"] > N
                norms = [EB.f32(e[3]) for e in ent]
                assert all(a >= c for a, c in zip(norms, norms[1:])), norms
                for e in ent:                                              # norm = score / len(yseq), one float32 division
                    s = np.float32(EB.f32(e[2]))
                    assert e[3] == EB.bits(s / np.float32(len(e[0]) + 1) if score_norm else s)
                    assert len(e[1]) == len(e[0]) and all(a <= c for a, c in zip(e[1], e[1][1:]))
            for n in range(1, N):
                part = EB.nbest_checker(cfg, sd, f, lens, n, beam=beam, score_norm=score_norm, max_pops=64 * beam)
                for p, w in zip(part, full):
                    assert p["entries"] == w["entries"][:n] and p["pops"] == w["pops"]
                    assert p["n_ids"] == [len(e[0]) for e in p["entries"]] + [0] * (n - len(p["entries"]))
    assert kept_longer > 0


# ---- hand-built cases: a 6-symbol vocabulary (0 blank), prediction network and joint replaced by a table of logits ------------------
TOY = types.SimpleNamespace(n_logits=6, blank_id=0, pred_hidden=1, pred_layers=1, espnet=True)
# the blank-led row opens label 1 (.4); once a label is out, the blank takes .9: the search settles, and [1] is reached at either frame
HIST = lambda t, u: [.5, .4, .05, .05, 1e-9, 1e-9] if u == 0 else [.9, .03, .03, .04, 1e-9, 1e-9]     # noqa: E731
FLAT = lambda t, u: [.5, .2, .2, .05, .03, .02]                                                        # noqa: E731  labels 1 and 2: equal


def inject(fn, T):
    a = np.zeros((T, 6, 6), np.float32)
    for t in range(T):
        for u in range(6):
            a[t, u] = np.log(np.asarray(fn(t, u), np.float64)).astype(np.float32)
    return a


def run(fn, T, nbest, **kw):
    return EB.nbest_checker(TOY, None, np.zeros((1, T, 1), np.float32), [T], nbest, inject=inject(fn, T), **kw)[0]


def labels(r):
    return [(e[0], e[1]) for e in r["entries"]]


def test_a_kept_list_longer_than_nbest():
    r = run(HIST, 1, 3, beam=3)
    assert r["kept"] == 4 > 3                                              # the edge is reached: the frame ended with 4 above the rest
    assert labels(r) == [([1], [0]), ([], []), ([2], [0])]                 # [3], equal to [2] and after it in the kept list, is cut
    assert run(HIST, 1, 2, beam=3)["entries"] == r["entries"][:2]


def test_duplicates_are_kept():
    r = run(HIST, 2, 3, beam=3)
    assert r["kept"] == 3 and r["duplicates"] == 1                         # the edge is reached: [1] emitted at frame 0 and at frame 1
    assert labels(r) == [([1], [0]), ([1], [1]), ([], [])]
    assert r["entries"][0][2] != r["entries"][1][2]                        # two hypotheses, two scores: upstream removes neither
    assert run(HIST, 2, 2, beam=3)["duplicates"] == 1


def test_a_tie_is_resolved_by_the_position_in_the_kept_list():
    r = run(FLAT, 1, 2, beam=2)
    assert r["kept"] == 3 and r["ties"] == 1                               # the edge is reached: [1] and [2] score the same, bits
    assert labels(r) == [([], []), ([1], [0])]                             # [1] was kept before [2]
    r = run(FLAT, 2, 3, beam=3, score_norm=False)
    assert r["ties"] >= 1 and labels(r)[1:] == [([1], [0]), ([2], [0])] and r["entries"][1][2:] == r["entries"][2][2:]


def test_score_norm_on_and_off():
    on, off = run(HIST, 2, 3, beam=3, score_norm=True), run(HIST, 2, 3, beam=3, score_norm=False)
    assert on["norm_reorders"] == 1 and off["norm_reorders"] == 0          # the edge is reached: the norm changes the order
    assert labels(on) == [([1], [0]), ([1], [1]), ([], [])] and labels(off) == [([1], [0]), ([], []), ([1], [1])]
    assert sorted(e[2] for e in on["entries"]) == sorted(e[2] for e in off["entries"])          # the same hypotheses, the same scores
    assert [e[3] for e in off["entries"]] == [e[2] for e in off["entries"]]
    for e in on["entries"]:
        assert e[3] == EB.bits(np.float32(EB.f32(e[2])) / np.float32(len(e[0]) + 1))


# ---- the float64 restatement: scores only ------------------------------------------------------------------------------------------
# (beam, utterance) of the toy fixtures whose ranked float64 list keeps every adjacent norm gap, down to the first entry left out,
# above ten times the line — asserted for each of them below, so that order is never what is compared
FLOAT64_FIXTURES = [(4, 0), (4, 1), (20, 0), (20, 1), (3, 0), (3, 1)]                 # every utterance of the three ESPnet toys
def test_scores_equal_the_float64_restatement(toys):
    deviation, took = 0.0, []
    for cfg, sd, f, lens, beam in toys[:3]:
        N = min(beam, 8)
        chk = EB.nbest_checker(cfg, sd, f, lens, N, beam=beam, max_pops=64 * beam)
        for b in range(len(lens)):
            want, _ = EB.beam_float64(EB.model_logp_fn(cfg, sd, f[b]), int(lens[b]), cfg.n_logits, cfg.blank_id, beam=beam)
            line = lambda x: LINE * max(1.0, abs(x))                      # noqa: E731
            if (beam, b) not in FLOAT64_FIXTURES:
                continue
            took.append((beam, b))
            assert all(a[2] - c[2] > 10 * line(a[2]) for a, c in zip(want, want[1:N + 1])), (beam, b)     # the fixture keeps its gaps
            got = chk[b]["entries"]
            assert [e[0] for e in got] == [w[0] for w in want[:N]], (beam, b)     # matched by label sequence: the same, in order
            for e, w in zip(got, want):
                assert abs(EB.f32(e[2]) - w[1]) <= line(w[1]) and abs(EB.f32(e[3]) - w[2]) <= line(w[2]), (beam, b, e, w)
                deviation = max(deviation, abs(EB.f32(e[2]) - w[1]))
    print(f"{len(took)} fixture utterances; largest |float32 - float64| score {deviation:.3e}")
    assert sorted(took) == sorted(FLOAT64_FIXTURES)


# ---- the Python surface over fake models -----------------------------------------------------------------------------------------
def test_argument_errors_name_the_reason():
    assert check_nbest(None, 20) == 0 and check_nbest(1, 1) == 0 and check_nbest(1, None) == 0 and check_nbest(3, 20) == 3
    with pytest.raises(ValueError, match=r"nbest=2 needs the beam search \(beam_size > 1\)"):
        check_nbest(2, 1)
    with pytest.raises(ValueError, match="nbest=5 is above beam_size=4"):
        check_nbest(5, 4)
    for bad in (0, 9, 2.0, "2", True):
        with pytest.raises(ValueError, match="nbest must be an integer in 1..8"):
            check_nbest(bad, 20)
    for call in (lambda **kw: load_model(device="cuda:0", config=ESPNET_TINY, **kw),
                 lambda **kw: EspnetModel(ESPNET_TINY, {}, synthetic_token_list(ESPNET_TINY.vocab_size), **kw)):
        with pytest.raises(ValueError, match="needs the beam search"):     # before anything is loaded
            call(nbest=2)
        with pytest.raises(ValueError, match="is above beam_size=4"):
            call(nbest=5, beam_size=4)


def test_result_assembly():
    cfg = ESPNET_TINY
    model = EspnetModel.__new__(EspnetModel)
    model.cfg, model.token_list, model.beam_size = cfg, synthetic_token_list(cfg.vocab_size, 0), 6
    lists = [[([7, 8], [1, 4], -1.5, -0.5), ([7], [2], -2.5, -1.25)], [([], [], 0.0, 0.0)]]
    for with_scores in (False, True):
        res = DecodedBatch([[7, 8], []], [[1, 4], []], [9, 0], [-1.5, 0.0], [False, False], nbest=lists,
                           token_logprobs=[[-0.25, -0.5], []] if with_scores else None)
        got = model._nbest_entries(res, 0)
        assert [(t, toks, ids) for t, toks, ids, _ in got] == [(model.ids_to_text([7, 8]), [model.token_list[7], model.token_list[8]], [7, 8]),
                                                               (model.ids_to_text([7]), [model.token_list[7]], [7])]
        assert all(isinstance(h, _NBestHypothesis) for *_, h in got)
        assert [(h.yseq, h.score, h.norm_score) for *_, h in got] == [([7, 8], -1.5, -0.5), ([7], -2.5, -1.25)]
        assert got[0][3].token_logprobs == ([-0.25, -0.5] if with_scores else None) and got[1][3].token_logprobs is None
        assert [e[:3] for e in model._nbest_entries(res, 1)] == [("", [], [])]
    # __call__ and recognize_batch over a fake search: N tuples with lists on, one tuple as ever with them off
    model._search = lambda waves, **kw: DecodedBatch([[7, 8]], [[1, 4]], [9], [-1.5], [False], nbest=lists[:1] if kw.get("nbest", 2) else None)
    model.am = types.SimpleNamespace(nbest=2)
    assert len(model(np.zeros(100, np.float32))) == 2 and model(np.zeros(100, np.float32))[0][3].score == -1.5
    assert [len(x) for x in model.recognize_batch([np.zeros(100, np.float32)], nbest=2)] == [2]
    with pytest.raises(ValueError, match="above beam_size=6"):
        model.recognize_batch([np.zeros(100, np.float32)], nbest=7)
    model._search = lambda waves, **kw: DecodedBatch([[7, 8]], [[1, 4]], [9], [-1.5], [False])
    out = model(np.zeros(100, np.float32))
    assert len(out) == 1 and out[0][2] == [7, 8] and out[0][3] is None     # off: today's one tuple
    assert model.recognize_batch([np.zeros(100, np.float32)]) == [model.ids_to_text([7, 8])]


def test_the_entry_points_are_exported_declared_and_guarded():
    lib = ctypes.CDLL(rs_build.build())
    assert lib.rs_abi_version() == 7
    assert hasattr(lib, "rs_rnnt_beam_nbest") and hasattr(lib, "rs_rnnt_beam_nbest_workspace_bytes")    # fails without the feature
    assert {"rs_rnnt_beam_nbest", "rs_rnnt_beam_nbest_workspace_bytes"} <= set(capi.EXPORTS)
    loaded = capi.load()
    assert len(loaded.rs_rnnt_beam_nbest.argtypes) == len(loaded.rs_rnnt_beam.argtypes) + 3             # nbest, norm_scores, n_hyps
    assert loaded.rs_rnnt_beam_nbest_workspace_bytes.restype is ctypes.c_size_t
    lib.rs_rnnt_beam_nbest_workspace_bytes.restype = ctypes.c_size_t
    assert lib.rs_rnnt_beam_nbest_workspace_bytes(None, 4, 4, 100, 0, 2) == 0                             # no context: invalid
    header = open(os.path.join(ROOT, "include", "rs_asr.h"), encoding="utf-8").read()
    assert "size_t rs_rnnt_beam_nbest_workspace_bytes(const rs_ctx* ctx, int B, int beam, int tp_max, int max_pops, int nbest);" in header
    assert "int rs_rnnt_beam_nbest(rs_ctx* ctx," in header and "sort_nbest(kept_hyps)[:nbest]" in header
    assert "DESCENDING AND STABLE IN THE ORDER OF THE KEPT LIST" in header and "EQUAL LABEL SEQUENCES ARE NOT REMOVED" in header
    family = open(os.path.join(ROOT, "reazonspeech_amd", "csrc", "rs_family.h"), encoding="utf-8").read()
    assert "X(rs_rnnt_beam_nbest_workspace_bytes, C, FINAL, RS_HINT_LSTM_ONLY)" in family and "X(rs_rnnt_beam_nbest, C, FINAL, RS_HINT_LSTM_ONLY)" in family
