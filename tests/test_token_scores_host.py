"""CPU: token log-probabilities (rs_rnnt_token_scores) — the checker, the float64 definition and the result assembly.

The checker (tests/token_scores_checker.c: the device pass restated on the oracle library, float32 in the device's order) is
compared with the torch-float64 restatement of the definition (tests/token_scores_ref.py: scores_float64) on the three toy
models with synthetic weights, on 6 ragged utterances of random projection frames (B = 6, T' = 14, lengths 14 9 0 1 5 12, torch
seed 0); ids and frames are the CPU oracle's greedy search.

Bound of |checker - float64| per log-probability: 4 x the largest difference measured on exactly these inputs (gcc -O2 -mfma
-ffp-contract=off, x86-64):

    family   model            V     J     tokens   measured max |d|   bound (4 x)
    nemo     TINY             64    128   81       6.306e-07          2.522e-06
    espnet   ESPNET_TINY      96    128   15       1.082e-06          4.328e-06
    k2       ZIPFORMER_TINY   97    128   38       1.322e-06          5.288e-06

The float32 error grows with V and J (sums of V exponentials, J-term dot products), so the figures hold for these models and
these seeds only; a change of either needs a new measurement.  Also: top1 == ids on every greedy token, every log-probability
<= 1e-6, the result assembly of the three packages over fake models, argument errors that need no device, and the two exports.
"""
import ctypes
import importlib
import math
import types

import numpy as np
import pytest
import torch

import espnet_fake as efk
import k2_fake as kfk
import token_scores_ref as R
from reazonspeech_amd import build as rs_build
from reazonspeech_amd.espnet.asr import interface as ei
from reazonspeech_amd.espnet.asr.model import _ScoredHypothesis
from reazonspeech_amd.k2.asr import interface as ki
from reazonspeech_amd.k2.asr.model import K2Model, _Result
from reazonspeech_amd.nemo.asr import interface as ni
from reazonspeech_amd.nemo.asr.decode import decode_hypothesis
from reazonspeech_amd.runtime import capi
from reazonspeech_amd.runtime.config import ESPNET_TINY, TINY
from reazonspeech_amd.runtime.k2_config import ZIPFORMER_TINY
from reazonspeech_amd.runtime.k2_weights import synthetic_state_dict_k2
from reazonspeech_amd.runtime.model import AsrModel, DecodedBatch
from reazonspeech_amd.runtime.weights import synthetic_state_dict
from reazonspeech_amd.runtime.weights_espnet import synthetic_state_dict_espnet

etr = importlib.import_module("reazonspeech_amd.espnet.asr.transcribe")
ktr = importlib.import_module("reazonspeech_amd.k2.asr.transcribe")

FAMILIES = {"nemo": (TINY, synthetic_state_dict), "espnet": (ESPNET_TINY, synthetic_state_dict_espnet),
            "k2": (ZIPFORMER_TINY, synthetic_state_dict_k2)}
MEASURED = {"nemo": 6.306e-07, "espnet": 1.082e-06, "k2": 1.322e-06}       # max |checker - float64| on the inputs below
LENS = [14, 9, 0, 1, 5, 12]


def inputs(cfg):
    J = cfg.joiner_dim if R.is_k2(cfg) else cfg.joint_hidden
    g = torch.Generator().manual_seed(0)
    B, Tp = len(LENS), max(LENS)
    f = (torch.randn((B, Tp, J), generator=g) * (0.7 + 0.6 * torch.rand((B, 1, 1), generator=g))).numpy()
    return f, np.asarray(LENS, np.int32)


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_checker_equals_the_float64_definition(family):
    cfg, make = FAMILIES[family]
    sd = make(cfg, 0)
    f, lens = inputs(cfg)
    greedy = R.oracle_greedy(cfg, sd, f, lens)
    u_cap = max(len(g[0]) for g in greedy)
    ids, n = R.pack([g[0] for g in greedy], u_cap)
    frames, _ = R.pack([g[1] for g in greedy], u_cap)
    logp, top1 = R.scores_checker(cfg, sd, f, lens, ids, frames, n)
    worst, n_tok = 0.0, 0
    for b, (gi, gf) in enumerate(greedy):
        assert np.isnan(logp[b, n[b]:]).all() and (top1[b, n[b]:] == -2).all()      # slots past the count are left alone
        if not gi:
            continue
        want, best = R.scores_float64(cfg, sd, f[b], gi, gf)
        got = logp[b, :n[b]]
        assert top1[b, :n[b]].tolist() == gi == best, (family, b)                      # greedy: every token is its row's argmax
        assert (got <= 1e-6).all(), (family, b, got.max())
        worst = max(worst, float(np.abs(got.astype(np.float64) - want).max()))
        n_tok += len(gi)
    print(f"{family}: {n_tok} tokens, max |checker - float64| = {worst:.3e}, bound {4 * MEASURED[family]:.3e}")
    assert n_tok >= 10, "the inputs must emit tokens"
    assert worst <= 4 * MEASURED[family], (family, worst)


def test_alignment_steps_are_converted_and_bad_entries_are_flagged():
    cfg, make = FAMILIES["nemo"]
    sd = make(cfg, 0)
    f, lens = inputs(cfg)
    greedy = R.oracle_greedy(cfg, sd, f, lens)
    u_cap = max(len(g[0]) for g in greedy) + 2
    ids, n = R.pack([g[0] for g in greedy], u_cap)
    frames, _ = R.pack([g[1] for g in greedy], u_cap)
    steps, _ = R.pack([[t + u for u, t in enumerate(g[1])] for g in greedy], u_cap)
    a = R.scores_checker(cfg, sd, f, lens, ids, frames, n)
    b = R.scores_checker(cfg, sd, f, lens, ids, steps, n, frames_are_steps=True)
    assert a[0].tobytes() == b[0].tobytes() and (a[1] == b[1]).all()
    # a frame at enc_len, a negative frame and an id outside the vocabulary: NaN / -1 in exactly those slots, return value -1
    bad_f, bad_i = frames.copy(), ids.copy()
    bad_f[0, 1] = lens[0]
    bad_f[5, 0] = -1
    bad_i[4, 2] = cfg.n_logits
    lp, t1 = R.scores_checker(cfg, sd, f, lens, bad_i, bad_f, n, want_rc=-1)
    bad = np.zeros_like(ids, bool)
    bad[0, 1] = bad[5, 0] = bad[4, 2] = True
    valid = np.arange(u_cap)[None, :] < n[:, None]
    assert np.isnan(lp[bad]).all() and (t1[bad] == -1).all()
    assert not np.isnan(lp[valid & ~bad]).any()
    ok_rows = [1, 3]                                        # untouched utterances keep their bits
    assert lp[ok_rows].tobytes() == a[0][ok_rows].tobytes()


# ---- result assembly --------------------------------------------------------------------------------------------------------
class _Tok:
    """ids 0..9 -> 'a'..'j'; id 3 is a bare word boundary that decodes to ''"""

    def ids_to_text(self, ids):
        return "".join("" if i == 3 else "。" if i == 9 else chr(ord("a") + i) for i in ids)


def test_nemo_assembly_keeps_the_alignment_across_dropped_pieces():
    model = types.SimpleNamespace(tokenizer=_Tok())
    ids = [1, 3, 2, 9, 3, 4, 5]
    frames = [0, 2, 2, 5, 9, 9, 30]
    lps = [-0.1, -0.2, -0.3, -0.4, -0.5, -0.6, -0.7]
    hyp = ni.Hypothesis.from_greedy(ids, frames, 63)
    plain = decode_hypothesis(model, hyp)
    assert type(plain) is ni.TranscribeResult                                          # off: the reference's type, nothing else
    res = decode_hypothesis(model, hyp, lps)
    assert isinstance(res, ni.ScoredTranscribeResult) and isinstance(res, ni.TranscribeResult)
    assert (res.text, res.subwords, res.segments) == (plain.text, plain.subwords, plain.segments)
    assert res.token_ids == ids and res.token_logprobs == lps
    assert [s.token_id for s in res.subwords] == [1, 2, 9, 4, 5]                       # the '' pieces are gone ...
    assert res.subword_logprobs == [-0.1, -0.3, -0.4, -0.6, -0.7]                      # ... and the log-probabilities follow the ids
    assert len(res.subword_logprobs) < len(res.token_logprobs)
    assert [s.text for s in res.segments] == ["bc。", "ef"]
    assert res.segment_confidence == pytest.approx([math.exp((-0.1 - 0.3 - 0.4) / 3), math.exp((-0.6 - 0.7) / 2)])
    assert res.confidence == pytest.approx(math.exp(sum(lps) / len(lps)))
    empty = decode_hypothesis(model, ni.Hypothesis.from_greedy([], [], 63), [])
    assert empty.confidence is None and empty.token_logprobs == [] and empty.segment_confidence == []
    assert [f.name for f in ni.TranscribeResult.__dataclass_fields__.values()] == ["text", "subwords", "segments", "hypothesis"]
    assert ni.Hypothesis.from_greedy([1], [0], 63).token_confidence is None


def test_k2_assembly():
    st = kfk.FakeRecognizer().create_stream()
    st.accept_waveform(16000, kfk.audio(1.0))
    kfk.FakeRecognizer().decode_stream(st)
    assert type(ktr._result(st)) is ki.TranscribeResult                                # a recogniser without scores: the plain type
    toks = kfk.TOKENS
    model = type("M", (), {"tokens": toks, "cfg": ZIPFORMER_TINY, "symbol": lambda self, i: toks[i]})()
    conv = K2Model.convert.__get__(model)
    plain = conv([5, 6], [1, 4])
    assert plain.token_log_probs is None and plain.token_ids is None
    st.result = conv([5, 6, 7], [1, 4, 9], [-0.5, -1.5, -0.25])
    assert st.result.token_log_probs == [-0.5, -1.5, -0.25] and st.result.token_ids == [5, 6, 7]
    res = ktr._result(st)
    assert isinstance(res, ki.ScoredTranscribeResult) and res.text == "".join(toks[i] for i in (5, 6, 7))
    assert res.token_ids == [5, 6, 7] and res.token_logprobs == res.subword_logprobs == [-0.5, -1.5, -0.25]
    assert len(res.subword_logprobs) == len(res.subwords) and res.confidence == pytest.approx(math.exp(-2.25 / 3))
    st.result = _Result([], [], "", token_ids=[], token_log_probs=[])
    assert ktr._result(st).confidence is None
    assert [f.name for f in ki.TranscribeResult.__dataclass_fields__.values()] == ["text", "subwords"]


class _ScoredFake(efk.FakeEspnetModel):
    """the fake ESPnet model with `token_scores` on: token k of a piece gets log-probability -(k + 1) / 100"""
    token_scores = True

    def __call__(self, speech):
        text, tokens, _, _ = super().__call__(speech)[0]
        ids = [efk.TOKENS.index(t) for t in tokens]
        self.pieces = getattr(self, "pieces", []) + [ids]
        return [(text, tokens, ids, _ScoredHypothesis(ids, [-(k + 1) / 100 for k in range(len(ids))]))]


def test_espnet_assembly_concatenates_the_pieces_of_a_long_recording():
    wav = efk.long_audio(47.0, 5)
    cfg = ei.TranscribeConfig(verbose=False)
    plain = etr.transcribe(efk.FakeEspnetModel(), ei.AudioData(wav, 16000), cfg)
    assert type(plain) is ei.TranscribeResult
    model = _ScoredFake()
    res = etr.transcribe(model, ei.AudioData(wav, 16000), cfg)
    assert isinstance(res, ei.ScoredTranscribeResult) and (res.text, res.segments) == (plain.text, plain.segments)
    assert len(model.calls) >= 3                                                       # several pieces
    assert "".join(efk.TOKENS[i] for i in res.token_ids) == res.text                   # ids of all pieces, in order
    assert res.token_ids == [i for piece in model.pieces for i in piece]
    assert res.token_logprobs == [-(k + 1) / 100 for piece in model.pieces for k in range(len(piece))]
    assert res.confidence == pytest.approx(math.exp(float(np.mean(res.token_logprobs))))
    none = ei.make_result("", [], [([], [])])
    assert none.confidence is None and none.token_ids == []
    assert [f.name for f in ei.TranscribeResult.__dataclass_fields__.values()] == ["text", "segments"]


# ---- arguments and exports ---------------------------------------------------------------------------------------------------
def test_exports_and_arguments_that_need_no_device():
    lib = ctypes.CDLL(rs_build.build())
    assert lib.rs_abi_version() == 7
    assert hasattr(lib, "rs_rnnt_token_scores") and hasattr(lib, "rs_rnnt_token_scores_workspace_bytes")
    assert {"rs_rnnt_token_scores", "rs_rnnt_token_scores_workspace_bytes"} <= set(capi.EXPORTS)
    lib.rs_rnnt_token_scores_workspace_bytes.restype = ctypes.c_size_t
    lib.rs_rnnt_token_scores_workspace_bytes.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    assert lib.rs_rnnt_token_scores_workspace_bytes(None, 4, 8) == 0
    lib.rs_rnnt_token_scores.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int] * 2 + [ctypes.c_void_p] * 3 + [ctypes.c_int] * 2 + \
        [ctypes.c_void_p] * 3 + [ctypes.c_size_t, ctypes.c_void_p]
    assert lib.rs_rnnt_token_scores(None, None, None, 1, 1, None, None, None, 1, 0, None, None, None, 0, None) == capi.RS_EINVAL
    assert capi.SCORES_FRAMES_ARE_STEPS == 1
    # the runtime: the last field, off by default, and no sharded gather
    assert list(DecodedBatch.__dataclass_fields__)[-1] == "token_logprobs" and DecodedBatch([], [], []).token_logprobs is None
    with pytest.raises(ValueError, match="token_scores"):
        AsrModel.transcribe_waveforms_sharded(types.SimpleNamespace(token_scores=True), [])
    with pytest.raises(ValueError, match="token_scores"):
        from reazonspeech_amd.nemo.asr import transcribe_batch
        transcribe_batch(types.SimpleNamespace(token_scores=True, resample="host", device="cpu"), [], ni.TranscribeConfig(verbose=False),
                         distributed=True)
