"""CPU: the checker of the avsr device search (tests/avsr_search_checker.c: csrc/k_avsr_search.hip's greedy / beam step restated in
the device's float32 order) and the host plumbing of `search=`.

    reference's generate() on weights that emit eos  --make_avsr_eos_golden.py-->  tests/golden/avsr_ref_eos.npz
    checker over oracle.avsr.decode_logits  ==  that golden, avsr_ref_tiny.npz and avsr_ref_fresh.npz (ids identical, scores 1e-3)
    checker  ==  oracle.avsr.beam_generate on seeded random logit streams with a raised eos (finishing and the early stop both occur)
    crafted exact ties follow the documented rule: lower flat index, then earlier position
    HIP search  ==  the checker, bit for bit                                        (tests/test_gpu_avsr_search.py, -m gpu)
"""
import ctypes
import hashlib
import os
import types
import zlib

import numpy as np
import pytest
import torch

from reazonspeech_amd import build as rs_build
from reazonspeech_amd.runtime import capi
from reazonspeech_amd.runtime.avsr_config import AVSR_TINY
from reazonspeech_amd.runtime.avsr_synth import synthetic_clips
from reazonspeech_amd.runtime.avsr_weights import synthetic_state_dict_avsr
from oracle import avsr as oa

import avsr_search_ref as sr

HERE = os.path.dirname(os.path.abspath(__file__))
TOL_SCORE = 1e-3


def checker_generate(cfg, sd, a, v, mask, K, max_new_tokens, greedy):
    with torch.no_grad():
        enc = oa.encode(cfg, sd, torch.from_numpy(a), torch.from_numpy(v), torch.from_numpy(mask))
    ck = sr.run_checker(sr.model_logits_fn(cfg, sd, enc, mask, K), a.shape[0], K, cfg.vocab_size, max_new_tokens, cfg.bos_token_id,
                        cfg.eos_token_id, cfg.pad_token_id, greedy=greedy)
    return ck.trimmed()


def eos_inputs():
    g = np.load(os.path.join(HERE, "golden", "avsr_ref_eos.npz"))
    r = sr.EOS_RECIPE
    a, v, mask, _ = synthetic_clips(r["clips"], r["frames"], seed=r["seed"], ragged=True, min_frames=r["min_frames"])
    assert hashlib.sha256(a.tobytes() + v.tobytes() + mask.tobytes()).digest() == bytes(g["input_sha256"].tolist()), "inputs drifted from the golden's"
    assert tuple(g["alphas"].tolist()) == sr.EOS_ALPHAS and int(g["beams"]) == r["num_beams"] and int(g["new_tokens"]) == r["max_new_tokens"]
    return g, a, v, mask


@pytest.mark.parametrize("alpha", sr.EOS_ALPHAS)
def test_checker_equals_the_reference_on_weights_that_emit_eos(alpha):
    g, a, v, mask = eos_inputs()
    cfg, r, s = AVSR_TINY, sr.EOS_RECIPE, f"_a{int(round(alpha * 10))}"
    sd = sr.eos_recipe(cfg, alpha, r["weights_seed"])
    N = r["max_new_tokens"]
    # what the golden exercises (the generator asserts the same of the reference)
    want = g["beam" + s]
    assert (want == cfg.eos_token_id).any() and (g["greedy" + s] == cfg.eos_token_id).any()
    if alpha == sr.EOS_ALPHAS[0]:
        assert want.shape[1] == 1 + N and ((want == cfg.eos_token_id).sum(axis=1) > 0).sum() >= 4
    else:
        assert want.shape[1] < 1 + N
    seq, scores = checker_generate(cfg, sd, a, v, mask, r["num_beams"], N, greedy=False)
    assert np.array_equal(seq, want), "beam ids differ from the reference's generate()"
    err = float(np.abs(scores - g["beam_scores" + s]).max())
    print(f"alpha {alpha}: beam score error {err:.2e}")
    assert err <= TOL_SCORE
    seq, _ = checker_generate(cfg, sd, a, v, mask, 1, N, greedy=True)
    assert np.array_equal(seq, g["greedy" + s]), "greedy ids differ from the reference's generate()"


def test_checker_equals_the_oracle_when_the_search_stops_early():
    """alpha 7.5: no clip can improve after nine steps, so the beam search stops long before the length limit (at alpha 6.5 the
    results are short but the search still runs to the limit); greedy stops after one token"""
    cfg, r = AVSR_TINY, sr.EOS_RECIPE
    a, v, mask, _ = synthetic_clips(r["clips"], r["frames"], seed=r["seed"], ragged=True, min_frames=r["min_frames"])
    sd = sr.eos_recipe(cfg, sr.EARLY_STOP_ALPHA, r["weights_seed"])
    N, K = r["max_new_tokens"], r["num_beams"]
    with torch.no_grad():
        enc = oa.encode(cfg, sd, torch.from_numpy(a), torch.from_numpy(v), torch.from_numpy(mask))
        want_seq, want_sc = oa.beam_generate(cfg, sd, enc, torch.from_numpy(mask), K, N)
        want_greedy = oa.greedy_generate(cfg, sd, enc, torch.from_numpy(mask), N)
    ck = sr.run_checker(sr.model_logits_fn(cfg, sd, enc, mask, K), a.shape[0], K, cfg.vocab_size, N, cfg.bos_token_id, cfg.eos_token_id, cfg.pad_token_id)
    assert 1 < ck.steps < N and not ck.can.any()
    seq, sc = ck.trimmed()
    assert np.array_equal(seq, want_seq.numpy()) and float(np.abs(sc - want_sc.numpy()).max()) <= 1e-4
    ck = sr.run_checker(sr.model_logits_fn(cfg, sd, enc, mask, 1), a.shape[0], 1, cfg.vocab_size, N, cfg.bos_token_id, cfg.eos_token_id, cfg.pad_token_id,
                        greedy=True)
    assert ck.steps < N and np.array_equal(ck.trimmed()[0], want_greedy.numpy())


def test_checker_equals_the_reference_goldens_without_eos():
    g = np.load(os.path.join(HERE, "golden", "avsr_ref_tiny.npz"))
    cfg = AVSR_TINY
    B, T = int(g["clips"]), int(g["frames"])
    a, v, mask, _ = synthetic_clips(B, T, seed=int(g["input_seed"]), ragged=True, min_frames=max(8, T // 3))
    sd = synthetic_state_dict_avsr(cfg, int(g["weight_seed"]))
    n_new, K, kb = int(g["new_tokens"]), int(g["beams"]), int(g["beam_clips"])
    seq, _ = checker_generate(cfg, sd, a, v, mask, 1, n_new, greedy=True)
    assert np.array_equal(seq, g["greedy"])
    seq, scores = checker_generate(cfg, sd, a[:kb], v[:kb], mask[:kb], K, n_new, greedy=False)
    assert np.array_equal(seq, g["beam"]) and float(np.abs(scores - g["beam_scores"]).max()) <= TOL_SCORE
    # the second geometry (3 encoder layers, 1 decoder layer, 40 tokens: V = 40 < 256 lanes)
    g = np.load(os.path.join(HERE, "golden", "avsr_ref_fresh.npz"))
    cfg = AVSR_TINY.with_(encoder_layers=3, decoder_layers=1, vocab_size=40)
    sd = synthetic_state_dict_avsr(cfg, 17)
    a, v, mask, _ = synthetic_clips(3, 17, seed=99, ragged=True)
    assert hashlib.sha256(a.tobytes() + v.tobytes() + mask.tobytes()).digest() == bytes(g["input_sha256"].tolist())
    assert np.array_equal(checker_generate(cfg, sd, a, v, mask, 1, 7, greedy=True)[0], g["generate_beams1"])
    assert np.array_equal(checker_generate(cfg, sd, a, v, mask, 4, 7, greedy=False)[0], g["generate_beams4"])


# ---- seeded random logit streams: the checker against oracle.avsr.beam_generate, no model ----------------------------------------
BOS, PAD, EOS = 0, 1, 2


def stream_logits(seed, V, eos_bias, prefix):
    """logits of a hypothesis as a function of its token prefix (so both searches see the same stream whatever their row order)"""
    rng = np.random.default_rng([seed, zlib.crc32(np.asarray(prefix, np.int64).tobytes())])
    x = (2.0 * rng.standard_normal(V)).astype(np.float32)
    x[EOS] += np.float32(eos_bias)
    return x


def stream_case(monkeypatch, seed, V, K, B=3, N=10, eos_bias=2.5):
    cfg = types.SimpleNamespace(vocab_size=V, bos_token_id=BOS, pad_token_id=PAD, eos_token_id=EOS)

    def fake_decode(cfg_, sd_, enc_k, mask_k, ids):
        rows = [stream_logits(seed + 1000 * int(enc_k[r, 0, 0]), V, eos_bias, ids[r].tolist()) for r in range(ids.shape[0])]
        return torch.from_numpy(np.stack(rows))[:, None, :]

    monkeypatch.setattr(oa, "decode_logits", fake_decode)
    enc = torch.arange(B, dtype=torch.float32).view(B, 1, 1)          # the clip index, so that clips have streams of their own
    want_seq, want_sc = oa.beam_generate(cfg, None, enc, torch.zeros((B, 1)), K, N)
    gaps = []

    def fn(ck, step):
        rows = [stream_logits(seed + 1000 * (r // K), V, eos_bias, ck.run_seq.reshape(B * K, -1)[r, :step + 1].tolist()) for r in range(B * K)]
        out = np.zeros((B * K, sr.pad4(V)), np.float32)
        out[:, :V] = np.stack(rows)
        return out

    def on_step(ck, step):
        lp = ck.top_lp
        live = lp[:, 1:] > -1.0e8                                     # ties among the -1e9 rows of dead beams decide nothing
        tol = 16 * np.finfo(np.float32).eps * np.maximum(1.0, np.abs(lp[:, :-1]))
        gaps.append(bool((live & (lp[:, :-1] - lp[:, 1:] <= tol)).any()))

    ck = sr.run_checker(fn, B, K, V, N, BOS, EOS, PAD, on_step=on_step)
    seq, sc = ck.trimmed()
    same = seq.shape == tuple(want_seq.shape) and np.array_equal(seq, want_seq.numpy())
    if same:
        assert float(np.abs(sc - want_sc.numpy()).max()) <= 1e-4
    finished = bool((seq[:, 1:] == EOS).any())
    early = ck.steps < N
    return same, any(gaps), finished, early


def test_checker_equals_the_oracle_on_random_logit_streams(monkeypatch):
    cases = excluded = n_finished = n_early = 0
    for V in (5, 61, 1000):
        for K in (1, 2, 5, 8):
            for seed in range(6):
                same, near_tie, finished, early = stream_case(monkeypatch, 100 * seed + K, V, K)
                cases += 1
                n_finished += finished
                n_early += early
                if not same:
                    assert near_tie, f"V={V} K={K} seed={seed}: ids differ from the oracle's without a near-tie among the candidates"
                    excluded += 1
    print(f"random logit streams: {cases} cases, {excluded} excluded for a near-tie, {n_finished} with eos in the result, {n_early} stopped early")
    assert n_finished > 0 and n_early > 0
    assert excluded <= 0.02 * cases


# ---- crafted exact ties --------------------------------------------------------------------------------------------------------------
def tie_logits(step):
    """V = 5, K = 2, eos = 2 at step 2 only (the eos id is moved out of the way before).  Step 0: tokens 3 and 4 tie.  Step 1: both
    rows see the same logits, so token 1 is reached from both parents with equal values.  Step 2: both rows end in eos with equal
    scores."""
    x = np.zeros((2, 8), np.float32)
    if step == 0:
        x[:, :5] = [0, 1, 0, 3, 3]
    elif step == 1:
        x[:, :5] = [0, 6, 0, 0, 0]
    else:
        x[:, :5] = [0, 0, 9, 0, 0]
    return x


def drive_ties(search_factory):
    """search_factory(eos) -> object with .step(logits, step) and the checker's state attributes"""
    ck = search_factory()
    ck.step(tie_logits(0), 0)
    first = (ck.tokens.tolist(), ck.src_rows.tolist(), ck.run_score.copy())
    ck.step(tie_logits(1), 1)
    second = (ck.tokens.tolist(), ck.src_rows.tolist(), ck.run_score.copy())
    ck.step(tie_logits(2), 2)
    return ck, first, second


def test_crafted_exact_ties_follow_the_documented_rule():
    ck, first, second = drive_ties(lambda: sr.Checker(1, 2, 5, 6, BOS, EOS, PAD))
    # two equal logits in one row: the lower index first
    assert first[0] == [3, 4] and first[1] == [0, 0] and first[2][0, 0].tobytes() == first[2][0, 1].tobytes()
    # the same value reached from two parents: the lower flat index (parent 0) first
    assert second[0] == [1, 1] and second[1] == [0, 1] and second[2][0, 0].tobytes() == second[2][0, 1].tobytes()
    # equal finished scores: the earlier position keeps the better slot
    assert ck.fin_seq[0, 0, :4].tolist() == [BOS, 3, 1, EOS] and ck.fin_seq[0, 1, :4].tolist() == [BOS, 4, 1, EOS]
    assert ck.fin_score[0, 0].tobytes() == ck.fin_score[0, 1].tobytes() and ck.is_fin.tolist() == [[1, 1]] and ck.fin_len.tolist() == [[4, 4]]
    # greedy: equal values take the lower index; a row of equal values takes index 0
    g = sr.Checker(2, 1, 5, 3, BOS, EOS, PAD, greedy=True)
    x = np.full((2, 8), -1.0e9, np.float32)
    x[0, :5] = [1, 7, 7, 2, 7]
    g.step(x, 0)
    assert g.tokens.tolist() == [1, 0]


# ---- host plumbing ----------------------------------------------------------------------------------------------------------------------
def test_search_keyword_and_environment(monkeypatch):
    from reazonspeech_amd.avsr import AVHubertForConditionalGeneration
    from reazonspeech_amd.avsr.modeling import synthetic_model
    from reazonspeech_amd.runtime.avsr_model import AvsrDevice, resolve_search
    monkeypatch.delenv("REAZONSPEECH_AVSR_SEARCH", raising=False)
    assert resolve_search(None) == "host"                                   # the default
    monkeypatch.setenv("REAZONSPEECH_AVSR_SEARCH", "device")
    assert resolve_search(None) == "device" and resolve_search("host") == "host"
    monkeypatch.setenv("REAZONSPEECH_AVSR_SEARCH", "gpu")
    with pytest.raises(ValueError, match="search="):
        resolve_search(None)
    with pytest.raises(ValueError, match="bogus"):
        AVHubertForConditionalGeneration(AVSR_TINY, {}, search="bogus")
    with pytest.raises(ValueError, match="bogus"):
        synthetic_model(AVSR_TINY, search="bogus")
    # more beams than the device search has: refused before anything runs, never a silent fall-back to the host path
    m = object.__new__(AVHubertForConditionalGeneration)
    m.search, m.config = "device", AVSR_TINY
    with pytest.raises(ValueError, match=f"limit of {AvsrDevice.MAX_DEVICE_BEAMS}"):
        m.generate(input_values=np.zeros((1, 8, 104), np.float32), num_beams=9, max_new_tokens=4)
    assert AvsrDevice.MAX_DEVICE_BEAMS == 8


def test_abi_7_exports_the_search_entry_points():
    lib = ctypes.CDLL(rs_build.build())
    assert lib.rs_abi_version() == 7
    names = {"rs_avsr_search_state_bytes", "rs_avsr_search_begin", "rs_avsr_search_step", "rs_avsr_search_rows", "rs_avsr_search_peek",
             "rs_avsr_search_finish", "rs_avsr_generate_state_bytes", "rs_avsr_generate"}
    assert names <= set(capi.EXPORTS)
    for n in names:
        assert hasattr(lib, n), n
    lib.rs_avsr_search_state_bytes.restype = ctypes.c_size_t
    lib.rs_avsr_generate_state_bytes.restype = ctypes.c_size_t
    assert lib.rs_avsr_search_state_bytes(None, 4, 5, 33) == 0               # no context: invalid
    assert lib.rs_avsr_generate_state_bytes(None, 4, 100, 5, 33) == 0
    assert lib.rs_avsr_generate(None, None, None, 1, 1, None, None, None, None, None, 0, None) == -1        # RS_EINVAL
    # the struct mirror has the header's fields in the header's order
    import re
    src = open(os.path.join(os.path.dirname(HERE), "include", "rs_asr.h")).read()
    body = src[src.index("typedef struct rs_avsr_search {"):src.index("} rs_avsr_search;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"\b(?:int32_t|float)\s+([a-z_0-9]+)\s*;", body) == [f[0] for f in capi.RsAvsrSearch._fields_]
