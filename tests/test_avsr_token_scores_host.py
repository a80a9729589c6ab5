"""CPU: what generate()'s device search records per token (the _scored entry points of csrc/k_avsr_search.hip: transformers'
`scores`, `beam_indices` and compute_transition_scores) — the C checker with recording (tests/avsr_token_scores_checker.c) and the
host plumbing.

    reference's generate(output_scores=True)  --make_avsr_token_scores_golden.py-->  tests/golden/avsr_ref_token_scores.npz
    checker with recording  ==  the options checker in every decision, bit for bit at every step
    checker over oracle.avsr.decode_logits  ==  that golden: sequences and beam_indices identical, transition scores and scores rows 1e-3
    checker fed the golden's own `scores` as logits  ==  the golden's sequences, beam_indices, transition scores
    HIP search  ==  the checker, bit for bit                          (tests/test_gpu_avsr_token_scores.py, -m gpu)
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from reazonspeech_amd import build as rs_build
from reazonspeech_amd.runtime import capi
from reazonspeech_amd.runtime.avsr_config import AVSR_TINY
from oracle import avsr as oa

import avsr_search_ref as sr
import avsr_search_opts_ref as so
import avsr_token_scores_ref as ts
from test_avsr_search_opts_host import RANDOM_OPTS, random_logits, same_state, bare_model, bits, BOS, PAD, EOS

HERE = os.path.dirname(os.path.abspath(__file__))
TOL_SCORE = 1e-3                     # tests/test_gpu_avsr_search_opts.py's, for the reference's sequences_scores
NEG = np.float32(-1.0e9)
SCORED = ("rs_avsr_search_state_bytes_scored", "rs_avsr_search_begin_scored", "rs_avsr_search_step_scored", "rs_avsr_search_peek_scored",
          "rs_avsr_search_finish_scored", "rs_avsr_generate_state_bytes_scored", "rs_avsr_generate_scored")


def test_abi_7_declares_and_exports_the_scored_entry_points():
    lib = ctypes.CDLL(rs_build.build())
    assert lib.rs_abi_version() == 7
    src = open(os.path.join(os.path.dirname(HERE), "include", "rs_asr.h")).read()
    assert "#define RS_ABI_VERSION 7" in src
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for n in SCORED:
        assert re.search(r"\b" + n + r"\s*\(", code), f"{n} is not declared in rs_asr.h"
        assert hasattr(lib, n), f"{n} is not exported"
        assert n in capi.EXPORTS
    lib.rs_avsr_search_state_bytes_scored.restype = ctypes.c_size_t
    lib.rs_avsr_generate_state_bytes_scored.restype = ctypes.c_size_t
    o = capi.RsAvsrSearchOpts.neutral()
    assert lib.rs_avsr_search_state_bytes_scored(None, 4, 5, 33, 1000, ctypes.byref(o)) == 0           # no context: invalid
    assert lib.rs_avsr_generate_state_bytes_scored(None, 4, 100, 5, 33, ctypes.byref(o)) == 0
    assert lib.rs_avsr_generate_scored(None, *([None] * 2), 1, 1, *([None] * 10), None, 0, None) == -1   # RS_EINVAL
    assert lib.rs_avsr_search_finish_scored(None, None, None, 1, None, 0, *([None] * 7), None) == -1


# ---- recording changes no decision; the identities of the recorded values ---------------------------------------------------------------
def check_identities(ck, what):
    """sum of a hypothesis' token scores, formed as the search forms its running score, == that score bit for bit; past the end 0 / 0 / -1"""
    N, K = ck.max_len - 1, ck.K
    tsc, tl, bi = ck.recorded()
    _, lens, scores = ck.result()
    live = np.arange(1, N + 1)[None, :] < lens[:, None]
    assert (tsc[~live] == 0).all() and (tl[~live] == 0).all() and (bi[~live] == -1).all(), (what, "past the end")
    if ck.greedy:
        assert (bi == -1).all()
        return 0
    assert ((bi[live] >= 0) & (bi[live] < ck.B * K)).all(), (what, "beam_indices outside the rows")
    n, checked = ck.n_ret, 0
    for r in range(ck.B * n):
        g = int(lens[r]) - 1
        if g < 1 or not scores[r] > -1.0e8:            # a slot that never finished, or finished under a NEG term of the bookkeeping
            continue
        b = r // n
        assert (bi[r, :g] // K == b).all(), (what, "a token taken from another clip's row")
        acc = np.float32(0.0 if bi[r, 0] == b * K else NEG)                # the row the hypothesis grew from at step 0
        for p in range(g):
            acc = np.float32(tsc[r, p] + acc)
            if p < g - 1:                                                  # a token that ends (eos / the last position) never runs on
                assert ck.fin_seq[b, r % n, p + 1] != ck.eos
        den = np.float32(float(g) ** ck.length_penalty)
        want = np.float32(np.float32(np.float32(acc / den) + np.float32(0.0) * NEG) + np.float32(0.0) * NEG)
        assert bits(want) == bits(scores[r]), (what, "row", r, "sum of token scores / length", want, "sequences_scores", scores[r])
        checked += 1
    return checked


@pytest.mark.parametrize("V", [4, 61, 300])
@pytest.mark.parametrize("K", [1, 3, 8])
def test_recording_changes_no_decision_and_sums_to_the_running_score(V, K):
    B, N = 2, 32
    checked = 0
    for i, opts in enumerate([{}] + RANDOM_OPTS):
        opts = dict(opts)
        lp = opts.pop("length_penalty", 1.0)
        if opts.get("num_return_sequences", 1) > K:
            opts["num_return_sequences"] = K
        for greedy in (False, True):
            o = {k: v for k, v in opts.items() if not (greedy and k in ("early_stopping", "num_return_sequences"))}
            k = 1 if greedy else K
            rng = np.random.default_rng([V, K, i, int(greedy)])
            ck = so.OptsChecker(B, k, V, N, BOS, EOS, PAD, greedy, lp, **o)
            rc = ts.ScoredChecker(B, k, V, N, BOS, EOS, PAD, greedy, lp, dump=True, **o)
            for step in range(N):
                x = random_logits(rng, B * k, V, step, eos_bias=-1.0 if V > 4 else 0.5)
                ck.step(x, step), rc.step(x, step)
                same_state(ck, rc, f"V={V} K={K} opts={opts} greedy={greedy} step {step}")
                row = rc.step_scores[step]
                assert (row[:, V:] == 0).all() and not np.isnan(row[:, :V]).any(), "dump: every column v < V written, the padding columns 0"
                if not greedy:                                             # the running scores are the sums of the recorded token scores
                    for b in range(B):
                        for j in range(k):
                            acc = np.float32(0.0 if rc.run_bi[b, j, 1] == b * k else NEG)
                            for pos in range(1, step + 2):
                                acc = np.float32(rc.run_ts[b, j, pos] + acc)
                                ends = rc.run_seq[b, j, pos] == EOS or pos + 1 >= rc.max_len
                                acc = np.float32(acc + np.float32(1.0 if ends else 0.0) * NEG)
                            assert bits(acc) == bits(rc.run_score[b, j]), (V, K, opts, step, b, j, acc, rc.run_score[b, j])
                            assert rc.run_bi[b, j, step + 1] == rc.src_rows[b * k + j]
                if not ck.goes_on:
                    break
            for got, want in zip(rc.result(), ck.result()):
                assert np.array_equal(bits(got) if got.dtype == np.float32 else got, bits(want) if want.dtype == np.float32 else want)
            checked += check_identities(rc, f"V={V} K={K} opts={opts} greedy={greedy}")
    assert checked > 0, "no finished hypothesis was checked"


def test_token_scores_are_the_processed_scores_and_lse_normalises_them():
    """V = 6, one greedy row, repetition_penalty 1.5 and no_repeat_ngram_size 2 by hand: the recorded score is the processed logit of
    the chosen token, exp(scores - lse) sums to 1 over the unbanned tokens, a banned token adds nothing"""
    V = 6
    x = np.zeros((1, 8), np.float32)
    x[0, :V] = [0.0, 0.0, 1.0, 5.0, 4.0, 3.0]
    ck = ts.ScoredChecker(1, 1, V, 4, BOS, EOS, PAD, True, dump=True, repetition_penalty=1.5, no_repeat_ngram_size=2)
    for step in range(3):
        ck.step(x, step)
    assert ck.run_seq[0, 0, :4].tolist() == [BOS, 3, 4, 3]
    tsc, tl, _ = ck.recorded()
    assert tsc[0, :3].tolist() == [5.0, 4.0, np.float32(5.0) / np.float32(1.5)]
    for step in range(3):
        row = ck.step_scores[step, 0, :V].astype(np.float64)
        assert row[BOS] == 0.0                                            # bos is in the prefix: 0 / 1.5
        assert abs(np.log(np.exp(row[np.isfinite(row)]).sum()) - float(tl[0, step])) < 1e-5
    # min_new_tokens bans eos: the -inf column is in the dump and not in the sum
    z = np.zeros((1, 8), np.float32)
    z[0, :V] = [0.0, 0.0, 9.0, 5.0, 4.0, 3.0]
    ck = ts.ScoredChecker(1, 1, V, 4, BOS, EOS, PAD, True, dump=True, min_new_tokens=2)
    ck.step(z, 0)
    assert np.isneginf(ck.step_scores[0, 0, EOS]) and ck.recorded()[0][0, 0] == 5.0
    assert abs(float(ck.recorded()[1][0, 0]) - np.log(np.exp([0.0, 0.0, 5.0, 4.0, 3.0]).sum())) < 1e-5
    # every column of a row banned (V = 4, K = 8, no_repeat_ngram_size 1: the rows run out of tokens): lse is -inf, nothing is NaN
    ck = ts.ScoredChecker(1, 8, 4, 6, BOS, EOS, PAD, False, dump=True, no_repeat_ngram_size=1)
    rng = np.random.default_rng(5)
    for step in range(6):
        ck.step(random_logits(rng, 8, 4, step, 0.0), step)
    assert ck.steps >= 4 and not np.isnan(ck.run_ts).any() and not np.isnan(ck.run_tl).any() and not np.isnan(ck.step_scores[:ck.steps]).any()
    assert np.isneginf(ck.step_scores[:ck.steps, :, :4]).all(axis=2).any() and np.isneginf(ck.run_tl).any()


# ---- against the reference's own output ----------------------------------------------------------------------------------------------------
def compare_with_golden(g, name, seq, scores, rec_ts, rec_tl, rec_bi, lens, step_scores, greedy):
    """sequences / beam_indices identical, transition scores (both normalisations) and, for the baselines, every scores row within TOL_SCORE"""
    want_seq = g[name + "_sequences"]
    assert seq.shape == want_seq.shape and np.array_equal(seq, want_seq), (name, "sequences differ from the reference's generate()")
    W = want_seq.shape[1] - 1
    live = np.arange(1, W + 1)[None, :] < np.asarray(lens)[:, None]
    if not greedy:
        want_bi = g[name + "_beam_indices"]
        assert want_bi.shape == (seq.shape[0], W) and np.array_equal(rec_bi[:, :W], want_bi), (name, "beam_indices differ from the reference's")
        assert np.array_equal(live, want_bi >= 0)
        err = float(np.abs(scores - g[name + "_sequences_scores"]).max())
        assert err <= TOL_SCORE, (name, "sequences_scores", err)
    logp = np.where(live, rec_ts[:, :W] - np.where(live, rec_tl[:, :W], 0), 0)
    # past a greedy row's eos transformers gathers the pad token's logit of a row fed with pad; here those positions are 0 (documented)
    for key, got in (("transition", rec_ts[:, :W]), ("transition_norm", logp)):
        want = g[f"{name}_{key}"]
        assert want.shape == got.shape
        err = float(np.abs(np.where(live, got - want, 0)).max())
        print(f"{name}: {key} error {err:.2e}")
        assert err <= TOL_SCORE, (name, key, err)
        if not greedy:
            assert (want[~live] == 0).all() and (got[~live] == 0).all()
    if step_scores is not None:
        want = g[name + "_scores"]
        assert step_scores.shape == want.shape, (name, "steps run / rows / vocabulary", step_scores.shape, want.shape)
        assert np.array_equal(np.isneginf(step_scores), np.isneginf(want)), (name, "-inf masks of the scores rows")
        fin = np.isfinite(want)
        err = float(np.abs(step_scores[fin] - want[fin]).max())
        print(f"{name}: scores rows error {err:.2e}")
        assert err <= TOL_SCORE, (name, "scores", err)


@pytest.mark.parametrize("name", list(ts.GOLDEN_CASES))
def test_scored_checker_equals_the_reference_golden(name):
    g, a, v, mask = ts.golden()
    cfg, r = AVSR_TINY, sr.EOS_RECIPE
    search, opts = ts.GOLDEN_CASES[name]
    greedy = search == "greedy"
    sd = sr.eos_recipe(cfg, float(g["alpha"]), r["weights_seed"])
    N, B, K = r["max_new_tokens"], a.shape[0], 1 if greedy else r["num_beams"]
    with torch.no_grad():
        enc = oa.encode(cfg, sd, torch.from_numpy(a), torch.from_numpy(v), torch.from_numpy(mask))
    ck = ts.run_search(sr.model_logits_fn(cfg, sd, enc, mask, K), B, K, cfg.vocab_size, N, cfg.bos_token_id, cfg.eos_token_id, cfg.pad_token_id,
                       greedy=greedy, dump=not opts, **opts)
    seq, scores = ck.trimmed()
    _, lens, _ = ck.result()
    tsc, tl, bi = ck.recorded()
    dump = None if opts else ck.step_scores[:ck.steps, :, :cfg.vocab_size]
    compare_with_golden(g, name, seq, scores, tsc, tl, bi, lens, dump, greedy)
    check_identities(ck, name)


@pytest.mark.parametrize("name", ["beam", "greedy"])
def test_checker_fed_the_golden_scores_reproduces_the_golden(name):
    """each step's golden `scores` given to the checker as that step's logits: for beam search they are log-probabilities, so their
    log-softmax is themselves up to rounding; for greedy search they are the logits themselves and the recorded score is exact"""
    g, _, _, _ = ts.golden()
    cfg, r = AVSR_TINY, sr.EOS_RECIPE
    greedy = name == "greedy"
    N, B, K, V = r["max_new_tokens"], r["clips"], 1 if greedy else r["num_beams"], cfg.vocab_size
    steps = g[name + "_scores"]
    assert steps.shape[1:] == (B * K, V)

    def fed(ck, step):
        x = np.zeros((B * K, sr.pad4(V)), np.float32)
        x[:, :V] = steps[step]
        return x
    ck = ts.run_search(fed, B, K, V, min(N, steps.shape[0]), cfg.bos_token_id, cfg.eos_token_id, cfg.pad_token_id, greedy=greedy, dump=True)
    assert ck.steps == steps.shape[0], "the search stops where the reference's did"
    seq, scores = ck.trimmed()
    _, lens, _ = ck.result()
    tsc, tl, bi = ck.recorded()
    compare_with_golden(g, name, seq, scores, tsc, tl, bi, lens, ck.step_scores[:ck.steps, :, :V], greedy)
    if greedy:
        W = seq.shape[1] - 1
        live = np.arange(1, W + 1)[None, :] < lens[:, None]
        assert np.array_equal(bits(tsc[:, :W][live]), bits(g["greedy_transition"][live])), "a greedy token's score is its logit, bit for bit"


# ---- argument handling and the Python fields -----------------------------------------------------------------------------------------------
def test_generate_keyword_checks_finish_before_the_device_is_touched():
    m = bare_model("device")
    x = dict(input_values=np.zeros((1, 8, 104), np.float32), max_new_tokens=4)
    with pytest.raises(TypeError, match="beam_indices"):
        m.generate(**x, num_beams=3, output_scores=True, beam_indices=True)
    with pytest.raises(TypeError):
        m.generate(**x, num_beams=3, return_dict_in_generate=True, output_scores=True, output_logits=True)
    with pytest.raises(ValueError):
        m.generate(**x, num_beams=3, return_dict_in_generate=True, output_scores=True, num_return_sequences=4)
    with pytest.raises(ValueError, match="no recorded generate"):
        m.compute_transition_scores(torch.zeros((1, 3), dtype=torch.int64))
    doc = type(m).generate.__doc__
    assert "per-step scores" not in doc and "beam_indices" in doc and "compute_transition_scores" in doc


def test_recorded_arrays_become_the_output_fields():
    m = bare_model("device")
    seq = np.array([[0, 5, 2], [0, 7, 1]], np.int64)
    rec = {"token_scores": np.array([[-0.5, -0.25], [-1.0, 0.0]], np.float32), "token_lse": np.array([[0.5, 0.0], [-0.5, 0.0]], np.float32),
           "beam_indices": np.array([[0, 1], [3, -1]], np.int32), "lengths": np.array([3, 2], np.int32), "steps": 2,
           "step_scores": np.zeros((2, 6, 61), np.float32)}
    out = m._scored_output(seq, np.array([-0.375, -1.0], np.float32), rec)
    assert out.beam_indices.dtype == torch.int64 and out.beam_indices.tolist() == [[0, 1], [3, -1]]
    assert out.token_logprobs.tolist() == [[-1.0, -0.25], [-0.5, 0.0]]
    assert np.allclose(out.confidence.numpy(), np.exp([-0.625, -0.5]))
    assert len(out.scores) == 2 and out.scores[0].shape == (6, 61)
    assert torch.equal(m.compute_transition_scores(out.sequences, out.scores, out.beam_indices), out.token_scores)
    assert torch.equal(m.compute_transition_scores(out.sequences, normalize_logits=True), out.token_logprobs)
    with pytest.raises(ValueError, match="not those of the last"):
        m.compute_transition_scores(torch.zeros((2, 3), dtype=torch.int64))
