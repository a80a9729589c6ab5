"""CPU: sherpa-onnx's modified_beam_search for `reazonspeech.k2.asr` (rs_rnnt_mbs, csrc/k_rnnt_mbs.hip) — the C checker that
restates the device's float32 order (tests/k2_mbs_checker.c) against a readable float64 restatement of the algorithm
(tests/k2_mbs_ref.py: mbs_float64, Python-float log_prob like upstream), hand-built cases for every rule of the algorithm, and
the argument checking of `load_model` / `K2Model`.

The agreement rule of test (a).  Float32 and float64 searches can only part where two candidates are nearly tied, so the float64
run reports, per utterance, the smallest gap between adjacent values among the K + 1 best candidates of any frame and the gap
between its two best final scores.  LINE = 2e-4: a row whose gaps all exceed it must agree in ids and frames; a row below it
may differ, but only from the first frame with such a gap on, and at most 3 of the 24 rows may use that excuse.  Where the
line comes from: a torch-float32 run of the float64 restatement agrees with it on 24 / 24 rows and its hypothesis scores
(|score| <= 36) deviate by at most 2.6e-5, an eighth of the line.  Three rows lie below it (gaps 1.3e-4, 1.5e-4, 2.0e-4), the
next ones are at 2.2e-4, 2.8e-4, 3.6e-4; 16 of 24 fall below 1e-3, so the project's usual 1e-3 would excuse most of the set.
Measured with the C checker's polynomial exp / log: 24 / 24 rows identical, no excuse used; the largest |float32 score - float64
score| over the hypotheses of the final sets is 1.3e-5 (printed by the test).  Seed 3: 222 merges, differs from greedy on
12 / 12 rows; seed 4: length normalisation picks one-token results."""
import ctypes
import math
import types

import numpy as np
import pytest
import torch

import k2_mbs_ref as R
from reazonspeech_amd import build as rs_build
from reazonspeech_amd.k2.asr import huggingface as hfm
from reazonspeech_amd.k2.asr.model import K2Model, search_config, synthetic_tokens
from reazonspeech_amd.runtime import capi
from reazonspeech_amd.runtime.k2_config import ZIPFORMER_TINY, ZIPFORMER_159M
from reazonspeech_amd.runtime.k2_weights import synthetic_state_dict_k2
from reazonspeech_amd.runtime.synth import synthetic_batch
from oracle import zipformer as oz, greedy as og

PAD = int(0.9 * 16000)
LINE = 2e-4
MAX_EXCUSED = 3


def projection(cfg, sd, seed):
    """twelve ragged utterances with the reference's 0.9 s padding -> float32 oracle projection [12][Tp][J], lengths"""
    audio, lens = synthetic_batch(12, 3.0, seed=5 + seed, ragged=True, min_seconds=0.7)
    fs = [oz.forward(cfg, sd, np.pad(audio[b, :lens[b]], PAD), "fp32")["joint_enc"].numpy() for b in range(12)]
    f = np.zeros((12, max(len(x) for x in fs), cfg.joiner_dim), np.float32)
    for b, x in enumerate(fs):
        f[b, :len(x)] = x
    return f, [len(x) for x in fs]


@pytest.fixture(scope="module")
def runs():
    cfg = ZIPFORMER_TINY
    out = {}
    for seed in (3, 4):
        sd = synthetic_state_dict_k2(cfg, seed)
        f, el = projection(cfg, sd, seed)
        out[seed] = (sd, f, el)
    return out


def test_checker_equals_the_float64_restatement(runs):
    cfg = ZIPFORMER_TINY
    excused, deviation, rows = [], 0.0, 0
    for seed, (sd, f, el) in runs.items():
        chk = R.mbs_checker(cfg, sd, f, el, K=4)
        greedy = og.k2_greedy(cfg, sd, f, el)
        merges = differs = 0
        for b in range(len(el)):
            ref = R.mbs_float64(cfg, sd, f[b, :el[b]], K=4)
            got = chk[b]
            rows += 1
            merges += got["merges"]
            differs += got["ids"] != greedy[b][0]
            by_tokens = {tuple(y): lp for y, lp in ref["final"]}
            for y, lp in got["final"]:
                if tuple(y) in by_tokens:
                    deviation = max(deviation, abs(lp - by_tokens[tuple(y)]))
            same = (got["ids"], got["frames"]) == (ref["ids"], ref["frames"])
            below = min(ref["min_gap"], ref["final_gap"]) <= LINE
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
        print(f"seed {seed}: {merges} merges, {differs} of {len(el)} rows differ from the greedy search")
        assert merges > 0 or seed != 3, "the merge path must be exercised"
        if seed == 3:
            assert differs >= 1, "the search must not degenerate to the greedy one"
        if seed == 4:
            assert all(len(r["ids"]) <= 1 for r in chk), "length normalisation picks the short results here"
    print(f"largest |float32 score - float64 score| over the final sets: {deviation:.3e}; rows excused: {excused}")
    assert rows == 24 and len(excused) <= MAX_EXCUSED, excused
    assert deviation < LINE / 2, deviation


def test_one_active_path_is_the_greedy_search(runs):
    cfg = ZIPFORMER_TINY
    for seed, (sd, f, el) in runs.items():
        k1 = R.mbs_checker(cfg, sd, f, el, K=1)
        greedy = og.k2_greedy(cfg, sd, f, el)
        for b in range(len(el)):
            assert (k1[b]["ids"], k1[b]["frames"]) == greedy[b], (seed, b)
            assert k1[b]["merges"] >= 0 and len(k1[b]["final"]) == 1
        assert sum(len(r["ids"]) for r in k1) > 10


def test_checker_options(runs):
    """blank penalty and the length-norm flag reach the C checker as they reach the float64 restatement; a zero-frame row"""
    cfg = ZIPFORMER_TINY
    sd, f, el = runs[3]
    f, el = f[:4], [el[0], 0, el[2], el[3]]
    for kw in (dict(K=2, blank_penalty=1.5), dict(K=8, length_norm=False), dict(K=3)):
        chk = R.mbs_checker(cfg, sd, f, el, **kw)
        assert (chk[1]["ids"], chk[1]["score"], chk[1]["final"]) == ([], 0.0, [([], 0.0)])
        for b in (0, 2, 3):
            ref = R.mbs_float64(cfg, sd, f[b, :el[b]], **kw)
            if min(ref["min_gap"], ref["final_gap"]) > LINE:
                assert (chk[b]["ids"], chk[b]["frames"]) == (ref["ids"], ref["frames"]), (kw, b)
                assert abs(chk[b]["score"] - ref["score"]) < LINE / 2
    with pytest.raises(RuntimeError, match="-5"):
        R.mbs_checker(cfg, sd, f, el, K=4, out_cap=1)


# ---- hand-built cases: a 5-symbol vocabulary, decoder and joiner replaced by tables (float64 restatement only) ----------------
TOY = types.SimpleNamespace(context_size=2, blank_id=0, unk_id=2)


def table(fn):
    """logits_fn from fn(t, tokens after the context) -> 5 probabilities"""
    return lambda t, ys: torch.log(torch.tensor(fn(t, ys[2:]), dtype=torch.float64))


def test_blank_and_unk_of_one_parent_merge():
    r = R.mbs_float64(TOY, None, None, K=2, logits_fn=table(lambda t, y: [.5, .05, .3, .1, .05]), n_frames=1)
    assert r["merges"] == 1 and r["final"][0][0] == [] and len(r["final"]) == 1
    assert abs(r["final"][0][1] - math.log(.8)) < 1e-12
    r = R.mbs_float64(TOY, None, None, K=3, logits_fn=table(lambda t, y: [.5, .05, .3, .1, .05]), n_frames=1)
    assert [y for y, _ in r["final"]] == [[], [3]] and r["merges"] == 1                 # <unk> is never appended


def test_label_extension_merges_with_blank_extension_and_the_first_timestamps_stay():
    def probs(blank_after_3, three_after_nothing):
        def fn(t, y):
            if t == 0:
                return [.4, 0.0, 0.0, .6, 0.0]
            if y == [3]:
                rest = (1 - blank_after_3) / 4
                return [blank_after_3, rest, rest, rest, rest]
            rest = (1 - three_after_nothing) / 4
            return [rest, rest, rest, three_after_nothing, rest]
        return fn
    # [3]@0 + blank (.6 x .9) enters first; [] + 3@1 (.4 x .9) merges into it: the timestamp stays 0
    r = R.mbs_float64(TOY, None, None, K=2, logits_fn=table(probs(.9, .9)), n_frames=2)
    assert r["final"][0][0] == [3] and r["ids"] == [3] and r["frames"] == [0] and r["merges"] == 1
    assert abs(r["final"][0][1] - math.log(.6 * .9 + .4 * .9)) < 1e-12
    # the other order: [] + 3@1 (.4 x .95) enters first, [3]@0 + blank (.6 x .5) merges into it: the timestamp stays 1
    r = R.mbs_float64(TOY, None, None, K=2, logits_fn=table(probs(.5, .95)), n_frames=2)
    assert r["ids"] == [3] and r["frames"] == [1] and r["merges"] == 1
    assert abs(r["final"][0][1] - math.log(.4 * .95 + .6 * .5)) < 1e-12


def test_an_exact_tie_goes_to_the_lower_flat_index():
    r = R.mbs_float64(TOY, None, None, K=1, logits_fn=table(lambda t, y: [.1, .35, .1, .35, .1]), n_frames=1)
    assert r["ids"] == [1] and r["min_gap"] == 0.0
    # across hypotheses: after frame 0 the set is [1], [3] with equal log_prob; at frame 1 both put .6 on the blank
    fn = lambda t, y: [.1, .35, .1, .35, .1] if t == 0 else [.6, .1, .1, .1, .1]         # noqa: E731
    r = R.mbs_float64(TOY, None, None, K=2, logits_fn=table(fn), n_frames=2)
    assert [y for y, _ in r["final"]] == [[1], [3]] and r["ids"] == [1]                # equal final scores: first entered


def test_length_normalisation_flips_the_winner():
    fn = table(lambda t, y: [.55, 0.0, 0.0, .45, 0.0])
    assert R.mbs_float64(TOY, None, None, K=2, logits_fn=fn, n_frames=1)["ids"] == [3]             # -0.799 / 3 > -0.598 / 2
    assert R.mbs_float64(TOY, None, None, K=2, logits_fn=fn, n_frames=1, length_norm=False)["ids"] == []


def test_blank_penalty_is_subtracted_from_the_blank_logit():
    fn = lambda t, ys: torch.tensor([1.0, -9.0, -9.0, 0.5, -9.0], dtype=torch.float64)            # noqa: E731
    assert R.mbs_float64(TOY, None, None, K=1, logits_fn=fn, n_frames=1)["ids"] == []
    r = R.mbs_float64(TOY, None, None, K=1, logits_fn=fn, n_frames=1, blank_penalty=1.0)
    assert r["ids"] == [3]
    want = torch.log_softmax(torch.tensor([0.0, -9.0, -9.0, 0.5, -9.0], dtype=torch.float64), 0)[3]
    assert abs(r["score"] - float(want)) < 1e-12


# ---- the public surface, without a GPU ---------------------------------------------------------------------------------------
def test_load_model_and_k2model_check_the_search_arguments():
    for kw in (dict(decoding_method="beam_search"), dict(decoding_method="greedy"), dict(decoding_method=None)):
        with pytest.raises(ValueError, match="greedy_search.*modified_beam_search"):
            hfm.load_model(**kw)
    for bad in (0, 9, -1, 2.5):
        with pytest.raises(ValueError, match="max_active_paths"):
            hfm.load_model(decoding_method="modified_beam_search", max_active_paths=bad)
    with pytest.raises(ValueError, match="blank_penalty"):
        hfm.load_model(decoding_method="modified_beam_search", blank_penalty=-0.5)
    with pytest.raises(ValueError, match="blank_penalty"):
        hfm.load_model(blank_penalty=1.0)                                 # the greedy search has no such knob
    with pytest.raises(ValueError, match="Unknown precision"):             # the reference's own checks still come first
        hfm.load_model(precision="fp16", decoding_method="nonsense")
    cfg = ZIPFORMER_TINY
    with pytest.raises(ValueError, match="greedy_search.*modified_beam_search"):
        K2Model(cfg, {}, synthetic_tokens(cfg.vocab_size), decoding_method="alsd")
    with pytest.raises(ValueError, match="max_active_paths"):
        K2Model(cfg, {}, synthetic_tokens(cfg.vocab_size), decoding_method="modified_beam_search", max_active_paths=16)


def test_search_config_keeps_sherpa_onnx_defaults():
    assert (ZIPFORMER_159M.decoding, ZIPFORMER_159M.beam_size, ZIPFORMER_159M.has_scores) == ("greedy_batch", 1, False)
    assert search_config(ZIPFORMER_159M) == ZIPFORMER_159M                # the default stays the reference's greedy search
    c = search_config(ZIPFORMER_159M, "modified_beam_search")
    assert (c.decoding, c.beam_size, c.blank_penalty, c.has_scores) == ("modified_beam_search", 4, 0.0, True)
    assert c.validate() is c
    c = search_config(ZIPFORMER_TINY, "modified_beam_search", max_active_paths=8, blank_penalty=1.5)
    assert (c.beam_size, c.blank_penalty) == (8, 1.5)
    with pytest.raises(AssertionError):
        ZIPFORMER_TINY.with_(decoding="alsd").validate()


def test_abi_7_exports_the_entry_point():
    lib = ctypes.CDLL(rs_build.build())
    assert lib.rs_abi_version() == 7
    assert hasattr(lib, "rs_rnnt_mbs") and hasattr(lib, "rs_rnnt_mbs_workspace_bytes")
    assert {"rs_rnnt_mbs", "rs_rnnt_mbs_workspace_bytes"} <= set(capi.EXPORTS) and capi.MBS_LENGTH_NORM == 1
    lib.rs_rnnt_mbs_workspace_bytes.restype = ctypes.c_size_t
    assert lib.rs_rnnt_mbs_workspace_bytes(None, 4, 4, 100, 100) == 0      # no context: invalid
