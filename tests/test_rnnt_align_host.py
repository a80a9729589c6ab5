"""CPU: transducer forced alignment and transcript likelihood (rs_rnnt_align) — the definition, the checker and the result assembly.

1. The torch/float64 restatement of the definition (tests/rnnt_align_ref.py: forward_float64, viterbi_float64) against brute force:
   on lattices small enough to list (T <= 4, U <= 3, both topologies) the log-sum over every enumerated alignment is the forward
   sum and the best enumerated alignment is Viterbi.  No DP takes part in the enumeration.
2. The checker (tests/rnnt_align_checker.c: the device entry restated serially on the oracle library, float32 in the device's
   order) against that float64 restatement on the three toy models with synthetic weights, on 6 ragged utterances of random
   projection frames (B = 6, T' = 14, lengths 14 9 0 1 5 12, torch seed 0, as tests/test_token_scores_host.py); the transcripts
   are the CPU oracle's greedy ids.  Bound per quantity: 4 x the largest difference measured on exactly these inputs (gcc -O2
   -mfma -ffp-contract=off, x86-64); `frames` must be identical:

    family   topology        feasible rows   max |d loglik|   max |d best|   max |d logp|
    espnet   standard        5               2.270e-06        4.099e-06      1.083e-06
    espnet   one per frame   5               1.497e-06        1.653e-06      1.083e-06
    k2       standard        5               8.960e-06        1.018e-05      2.140e-06
    k2       one per frame   5               1.425e-06        1.558e-06      1.323e-06
    nemo     standard        5               1.355e-05        1.204e-05      5.258e-07
    nemo     one per frame   5               3.217e-06        2.722e-06      5.465e-07

   (the sixth row has no frames and no text).  For the one-per-frame topology the transcripts are cut to max(T - 1, 1) labels: an
   LSTM family's greedy search emits several labels on a frame, and its full text has no such alignment.

   The float32 error grows with V, J and the path length, so the figures hold for these models and these seeds only.
3. Properties on the same inputs: loglik >= best; best is the float32 sum of the lattice entries along `frames`; logp equals
   scores_checker (tests/token_scores_checker.c) on (ids, frames) bit for bit; frames are monotone as the topology demands.
4. Argument errors that need no device, the two exports, and the result assembly of the three packages over fake models.
"""
import ctypes
import itertools
import math
import types

import numpy as np
import pytest
import torch

import rnnt_align_ref as A
import token_scores_ref as R
from reazonspeech_amd import build as rs_build
from reazonspeech_amd.runtime import capi
from reazonspeech_amd.runtime.config import ESPNET_TINY, TINY
from reazonspeech_amd.runtime.k2_config import ZIPFORMER_TINY
from reazonspeech_amd.runtime.k2_weights import synthetic_state_dict_k2
from reazonspeech_amd.runtime.weights import synthetic_state_dict
from reazonspeech_amd.runtime.weights_espnet import synthetic_state_dict_espnet

FAMILIES = {"nemo": (TINY, synthetic_state_dict), "espnet": (ESPNET_TINY, synthetic_state_dict_espnet),
            "k2": (ZIPFORMER_TINY, synthetic_state_dict_k2)}
LENS = [14, 9, 0, 1, 5, 12]
# (family, one label per frame) -> max |checker - float64| of (loglik, best, logp) on the inputs below
MEASURED = {
    ("espnet", False): (2.270e-06, 4.099e-06, 1.083e-06),
    ("espnet", True): (1.497e-06, 1.653e-06, 1.083e-06),
    ("k2", False): (8.960e-06, 1.018e-05, 2.140e-06),
    ("k2", True): (1.425e-06, 1.558e-06, 1.323e-06),
    ("nemo", False): (1.355e-05, 1.204e-05, 5.258e-07),
    ("nemo", True): (3.217e-06, 2.722e-06, 5.465e-07),
}
CASES = sorted(MEASURED)


# ---- 1. the definition against brute force -----------------------------------------------------------------------------------
@pytest.mark.parametrize("one", [False, True])
def test_float64_restatement_equals_brute_force(one):
    rng = np.random.default_rng(7)
    n = 0
    for T, U in itertools.product(range(1, 5), range(0, 4)):
        lb = np.log(rng.uniform(0.05, 0.9, (T, U + 1)))
        ly = np.log(rng.uniform(0.05, 0.9, (T, U)))
        if one and U > T:
            assert A.forward_float64(lb, ly, True) == -math.inf and A.viterbi_float64(lb, ly, True) == (-math.inf, [-1] * U)
            continue
        paths = A.enumerate_paths(lb, ly, one)
        assert len(paths) == (math.comb(T, U) if one else math.comb(T + U - 1, U))
        total = math.log(sum(math.exp(s) for s, _ in paths))
        top, top_frames = max(paths, key=lambda p: p[0])
        assert A.forward_float64(lb, ly, one) == pytest.approx(total, abs=1e-12)
        got, frames = A.viterbi_float64(lb, ly, one)
        assert got == pytest.approx(top, abs=1e-12) and frames == top_frames, (T, U)
        n += 1
    assert n >= (13 if one else 16)
    assert A.forward_float64(np.zeros((0, 1)), np.zeros((0, 0)), one) == 0.0              # no frames, no text
    assert A.forward_float64(np.zeros((0, 3)), np.zeros((0, 2)), one) == -math.inf        # no frames, a text


# ---- 2. / 3. the checker -----------------------------------------------------------------------------------------------------
def inputs(cfg):
    J = cfg.joiner_dim if R.is_k2(cfg) else cfg.joint_hidden
    g = torch.Generator().manual_seed(0)
    B, Tp = len(LENS), max(LENS)
    f = (torch.randn((B, Tp, J), generator=g) * (0.7 + 0.6 * torch.rand((B, 1, 1), generator=g))).numpy()
    return f, np.asarray(LENS, np.int32)


_cache = {}


def scene(family, one):
    """the checker's results on the family's inputs, computed once"""
    if (family, one) not in _cache:
        cfg, make = FAMILIES[family]
        sd = make(cfg, 0)
        f, lens = inputs(cfg)
        greedy = R.oracle_greedy(cfg, sd, f, lens)
        if one:                                              # an LSTM family's greedy search emits several labels on a frame: cut
            greedy = [(g[0][:max(int(T) - 1, 1)], None) for g, T in zip(greedy, lens)]
        u_cap = max(len(g[0]) for g in greedy) + 1
        ids, n = R.pack([g[0] for g in greedy], u_cap)
        got = A.align_checker(cfg, sd, f, lens, ids, n, one_per_frame=one, want_lattice=True)
        _cache[(family, one)] = (cfg, sd, f, lens, greedy, ids, n, got)
    return _cache[(family, one)]


def measure(family, one):
    """max |checker - float64| of (loglik, best, logp) over the feasible rows; asserts what must be identical"""
    cfg, sd, f, lens, greedy, ids, n, got = scene(family, one)
    worst, feasible = [0.0, 0.0, 0.0], 0
    for b, (gi, _) in enumerate(greedy):
        T, U = int(lens[b]), len(gi)
        assert (got["frames"][b, U:] == -2).all() and np.isnan(got["logp"][b, U:]).all()      # slots past the count are left alone
        lb, ly = A.lattice_float64(cfg, sd, f[b, :T], gi)
        want_ll = A.forward_float64(lb, ly, one)
        want_best, want_frames = A.viterbi_float64(lb, ly, one)
        if want_ll == -math.inf or (T == 0 and U == 0):
            assert got["loglik"][b] == want_ll and got["best"][b] == want_best, (family, one, b)
            assert got["frames"][b, :U].tolist() == [-1] * U and np.isnan(got["logp"][b, :U]).all()
            continue
        feasible += 1
        assert got["frames"][b, :U].tolist() == want_frames, (family, one, b)
        worst[0] = max(worst[0], abs(float(got["loglik"][b]) - want_ll))
        worst[1] = max(worst[1], abs(float(got["best"][b]) - want_best))
        if U:
            want_lp = np.asarray([ly[t][u] for u, t in enumerate(want_frames)])
            worst[2] = max(worst[2], float(np.abs(got["logp"][b, :U].astype(np.float64) - want_lp).max()))
    return tuple(worst), feasible


@pytest.mark.parametrize("family,one", CASES)
def test_checker_equals_the_float64_definition(family, one):
    worst, feasible = measure(family, one)
    bound = tuple(4 * m for m in MEASURED[(family, one)])
    print(f"{family} one_per_frame={one}: {feasible} feasible rows, max |checker - float64| (loglik, best, logp) = "
          f"({worst[0]:.3e}, {worst[1]:.3e}, {worst[2]:.3e}), bounds ({bound[0]:.3e}, {bound[1]:.3e}, {bound[2]:.3e})")
    assert feasible >= 3, "the inputs must hold feasible rows"
    assert all(w <= b for w, b in zip(worst, bound)), (family, one, worst, bound)


@pytest.mark.parametrize("family,one", CASES)
def test_properties_of_the_checker(family, one):
    cfg, sd, f, lens, greedy, ids, n, got = scene(family, one)
    frames, seen = got["frames"], 0
    for b, (gi, _) in enumerate(greedy):
        T, U = int(lens[b]), len(gi)
        if not np.isfinite(got["loglik"][b]) or T == 0:
            continue
        seen += 1
        assert got["loglik"][b] >= got["best"][b]
        fr = frames[b, :U].tolist()
        assert all(0 <= t < T for t in fr)
        assert all(y > x for x, y in zip(fr, fr[1:])) if one else all(y >= x for x, y in zip(fr, fr[1:]))
        path = A.path_sum_f32(got["lattice"][b, :T, :U + 1], fr, one)
        assert path.tobytes() == got["best"][b].tobytes(), (family, one, b, path, got["best"][b])
    assert seen >= 3
    # logp is what token scores give for (ids, frames), bit for bit (rows without an alignment hold -1 frames: left out)
    ok = np.asarray([np.isfinite(got["loglik"][b]) for b in range(len(LENS))])
    n_ok = np.where(ok, n, 0).astype(np.int32)
    lp, _ = R.scores_checker(cfg, sd, f, lens, ids, np.where(frames < 0, 0, frames), n_ok)
    for b in range(len(LENS)):
        assert lp[b, :n_ok[b]].tobytes() == got["logp"][b, :n_ok[b]].tobytes(), (family, one, b)


def test_bad_rows_are_flagged_and_the_others_keep_their_bits():
    cfg, sd, f, lens, greedy, ids, n, got = scene("nemo", False)
    bad_ids, bad_n = ids.copy(), n.copy()
    bad_ids[0, 1] = cfg.n_logits                           # an id outside the vocabulary
    bad_ids[5, 0] = cfg.blank_id                           # the blank is no label
    bad_n[4] = ids.shape[1] + 1                            # a count above u_cap
    out = A.align_checker(cfg, sd, f, lens, bad_ids, bad_n, want_rc=-1)
    for b in (0, 4, 5):
        k = min(int(bad_n[b]), ids.shape[1])
        assert np.isnan(out["loglik"][b]) and np.isnan(out["best"][b])
        assert (out["frames"][b, :k] == -1).all() and np.isnan(out["logp"][b, :k]).all()
    for b in (1, 2, 3):
        for key in ("loglik", "best", "frames", "logp"):
            assert out[key][b].tobytes() == got[key][b].tobytes(), (key, b)


# ---- 4. arguments and exports ---------------------------------------------------------------------------------------------------
def test_exports_and_arguments_that_need_no_device():
    lib = ctypes.CDLL(rs_build.build())
    assert lib.rs_abi_version() == 7
    assert hasattr(lib, "rs_rnnt_align") and hasattr(lib, "rs_rnnt_align_workspace_bytes")
    assert {"rs_rnnt_align", "rs_rnnt_align_workspace_bytes"} <= set(capi.EXPORTS)
    lib.rs_rnnt_align_workspace_bytes.restype = ctypes.c_size_t
    lib.rs_rnnt_align_workspace_bytes.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    assert lib.rs_rnnt_align_workspace_bytes(None, 4, 10, 8) == 0
    lib.rs_rnnt_align.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int] * 2 + [ctypes.c_void_p] * 2 + [ctypes.c_int] * 2 + \
        [ctypes.c_void_p] * 5 + [ctypes.c_size_t, ctypes.c_void_p]
    assert lib.rs_rnnt_align(None, None, None, 1, 1, None, None, 1, 0, None, None, None, None, None, 0, None) == capi.RS_EINVAL
    assert capi.ALIGN_ONE_PER_FRAME == 1 and capi.ALIGN_U_CAP_MAX >= 2047
    header = open(rs_build.HERE + "/../include/rs_asr.h").read()
    assert f"#define RS_ALIGN_U_CAP_MAX {capi.ALIGN_U_CAP_MAX}" in header and "RS_ALIGN_ONE_PER_FRAME = 1" in header


# ---- 4. result assembly over fake models -------------------------------------------------------------------------------------
class _Tok:
    """ids 0..9 -> 'a'..'j'; id 3 is a bare word boundary that decodes to ''; texts are read back one character per id"""

    def ids_to_text(self, ids):
        return "".join("" if i == 3 else "。" if i == 9 else chr(ord("a") + i) for i in ids)

    def text_to_ids(self, text):
        return [tuple(9 if c == "。" else ord(c) - ord("a") for c in text)] if all(c == "。" or "a" <= c <= "j" for c in text) else []


def test_nemo_assembly():
    from reazonspeech_amd.nemo.asr import align as na, interface as ni
    from reazonspeech_amd.nemo.asr.decode import decode_hypothesis
    model = types.SimpleNamespace(tokenizer=_Tok(), cfg=types.SimpleNamespace(blank_id=63))
    ids, frames, lps = [1, 3, 2, 9, 4], [0, 2, 2, 5, 30], [-0.1, -0.2, -0.3, -0.4, -0.5]
    res = na.aligned_result(model, ids, frames, lps, -1.0, -1.5, True)
    plain = decode_hypothesis(model, ni.Hypothesis.from_greedy(ids, frames, 63))
    assert isinstance(res, ni.AlignedTranscribeResult) and isinstance(res, ni.ScoredTranscribeResult)
    assert (res.text, res.subwords, res.segments) == (plain.text, plain.subwords, plain.segments)      # the package's own assembly
    assert res.token_ids == ids and res.token_logprobs == lps and res.subword_logprobs == [-0.1, -0.3, -0.4, -0.5]
    assert (res.log_likelihood, res.alignment_log_prob, res.norm_log_likelihood, res.feasible) == (-1.0, -1.5, -0.2, True)
    bad = na.aligned_result(model, ids, [-1] * 5, [math.nan] * 5, -math.inf, -math.inf, False)
    assert bad.feasible is False and bad.log_likelihood == bad.alignment_log_prob == bad.norm_log_likelihood == -math.inf
    assert bad.text == plain.text and bad.token_ids == ids and bad.subwords == [] and bad.segments == [] and bad.confidence is None
    empty = na.aligned_result(model, [], [], [], 0.0, 0.0, True)
    assert empty.norm_log_likelihood == 0.0 and empty.feasible and empty.text == ""
    assert na.text_ids(model, "bc。") == [1, 2, 9] and na.text_ids(model, [4, 5]) == [4, 5] and na.text_ids(model, " ") == []
    with pytest.raises(ValueError, match="cannot spell"):
        na.text_ids(model, "xyz")


def test_k2_assembly():
    import k2_fake as kfk
    from reazonspeech_amd.k2.asr import align as ka, interface as ki
    from reazonspeech_amd.k2.asr.model import K2Model
    toks = kfk.TOKENS
    model = type("M", (), {"tokens": toks, "cfg": ZIPFORMER_TINY, "symbol": lambda self, i: toks[i]})()
    model.convert = K2Model.convert.__get__(model)
    res = ka.aligned_result(model, [5, 6, 7], [1, 4, 9], [-0.5, -1.5, -0.25], -2.0, -2.25, True)
    want = model.convert([5, 6, 7], [1, 4, 9])
    assert isinstance(res, ki.AlignedTranscribeResult) and res.text == want.text
    assert [s.token for s in res.subwords] == want.tokens and [s.seconds for s in res.subwords] == want.timestamps
    assert res.token_ids == [5, 6, 7] and res.token_logprobs == res.subword_logprobs == [-0.5, -1.5, -0.25]
    assert res.norm_log_likelihood == pytest.approx(-2.0 / 3) and res.feasible
    bad = ka.aligned_result(model, [5, 6], [-1, -1], [math.nan, math.nan], -math.inf, -math.inf, False)
    assert not bad.feasible and bad.subwords == [] and bad.text == want.text[:len(bad.text)] and bad.log_likelihood == -math.inf
    text = "".join(toks[i] for i in (5, 6, 7))
    assert ka.text_ids(model, text) == [5, 6, 7] and ka.text_ids(model, " " + text[0] + " ") == [5] and ka.text_ids(model, (7, 5)) == [7, 5]
    with pytest.raises(ValueError, match="tokens.txt"):
        ka.text_ids(model, text + "\u0001")
    with pytest.raises(ValueError, match="tokens.txt"):
        ka.text_ids(model, toks[ZIPFORMER_TINY.blank_id])


def test_espnet_assembly():
    import espnet_fake as efk
    from reazonspeech_amd.espnet.asr import align as ea, interface as ei
    from reazonspeech_amd.espnet.asr.model import EspnetModel
    model = types.SimpleNamespace(token_list=efk.TOKENS, cfg=ESPNET_TINY, tokens2text=EspnetModel.tokens2text)
    ids = [i for i, t in enumerate(efk.TOKENS) if i != ESPNET_TINY.blank_id and len(t) == 1][:3]
    step = ESPNET_TINY.hop_length * ESPNET_TINY.sub_factor / ESPNET_TINY.sample_rate
    assert ea.frame_seconds(ESPNET_TINY) == step
    res = ea.aligned_result(model, ids, [10, 40, 400], [-0.1, -0.2, -0.3], -1.0, -1.25, True, duration=2.0)
    assert isinstance(res, ei.AlignedTranscribeResult) and res.text == "".join(efk.TOKENS[i] for i in ids)
    assert res.token_seconds == [0.0, pytest.approx(40 * step - 1.0), 2.0]              # the left padding is 1 s; inside the audio
    assert [s.text for s in res.segments] == [efk.TOKENS[i] for i in ids]
    assert [s.start_seconds for s in res.segments] == res.token_seconds and res.segments[-1].end_seconds == 2.0
    assert res.segments[0].end_seconds == res.segments[1].start_seconds
    assert res.norm_log_likelihood == pytest.approx(-1.0 / 3) and res.feasible and res.token_ids == ids
    bad = ea.aligned_result(model, ids, [-1] * 3, [math.nan] * 3, -math.inf, -math.inf, False, duration=2.0)
    assert not bad.feasible and bad.segments == [] and bad.token_seconds == [] and bad.text == res.text
    assert ea.text_ids(model, res.text) == ids and ea.text_ids(model, ids[::-1]) == ids[::-1]
    with pytest.raises(ValueError, match="token list"):
        ea.text_ids(model, "\u0001")


def test_align_waveforms_checks_its_arguments_before_any_device_work():
    from reazonspeech_amd.runtime.model import AlignedBatch, AsrModel
    fake = types.SimpleNamespace(cfg=types.SimpleNamespace(max_symbols=1))
    with pytest.raises(ValueError, match="2 waveforms but 1 texts"):
        AsrModel.align_waveforms(fake, [np.zeros(8), np.zeros(8)], [[1]])
    with pytest.raises(ValueError, match="at most 2047"):
        AsrModel.align_waveforms(fake, [np.zeros(8)], [[1] * 2048])
    assert list(AlignedBatch.__dataclass_fields__) == ["frames", "token_logprobs", "log_likelihood", "alignment_log_prob", "enc_lens", "feasible"]
    for pkg in ("nemo", "k2", "espnet"):
        mod = __import__(f"reazonspeech_amd.{pkg}.asr", fromlist=["x"])
        assert callable(mod.align_text) and callable(mod.align_text_batch)
