"""CPU: the options of the avsr device search (rs_avsr_search_opts: repetition_penalty, no_repeat_ngram_size, min_new_tokens,
early_stopping, num_return_sequences) — the C checker with options (tests/avsr_search_opts_checker.c) and the host plumbing.

    reference's generate(**case)  --make_avsr_search_opts_golden.py-->  tests/golden/avsr_ref_search_opts.npz
    checker over oracle.avsr.decode_logits  ==  that golden: ids identical for every case and clip, sequences_scores 1e-3
    checker  ==  the restatement over transformers' own processor classes (avsr_search_opts_ref.TorchSearch), bit for bit at every step
    HIP search  ==  the checker, bit for bit                              (tests/test_gpu_avsr_search_opts.py, -m gpu)
"""
import ctypes
import hashlib
import os
import re

import numpy as np
import pytest
import torch

from reazonspeech_amd import build as rs_build
from reazonspeech_amd.runtime import capi
from reazonspeech_amd.runtime.avsr_config import AVSR_TINY
from reazonspeech_amd.runtime.avsr_synth import synthetic_clips
from oracle import avsr as oa

import avsr_search_ref as sr
import avsr_search_opts_ref as so

HERE = os.path.dirname(os.path.abspath(__file__))
TOL_SCORE = 1e-3                     # tests/test_avsr_search_host.py's, for the reference's sequences_scores
BOS, PAD, EOS = 0, 1, 2


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.int32)


def golden():
    g = np.load(os.path.join(HERE, "golden", "avsr_ref_search_opts.npz"))
    r = sr.EOS_RECIPE
    a, v, mask, _ = synthetic_clips(r["clips"], r["frames"], seed=r["seed"], ragged=True, min_frames=r["min_frames"])
    assert hashlib.sha256(a.tobytes() + v.tobytes() + mask.tobytes()).digest() == bytes(g["input_sha256"].tolist()), "inputs drifted from the golden's"
    assert int(g["beams"]) == r["num_beams"] and int(g["new_tokens"]) == r["max_new_tokens"] and int(g["clips"]) == r["clips"]
    return g, a, v, mask


def test_golden_holds_every_case_and_names_its_transformers():
    g, _, _, _ = golden()
    assert str(g["transformers_version"])
    for name, (alpha, lp, opts, searches) in so.CASES.items():
        assert float(g[name + "_alpha"]) == alpha and float(g[name + "_length_penalty"]) == lp
        for search in searches:
            assert g[f"{name}_{search}"].shape[0] == sr.EOS_RECIPE["clips"] * opts.get("num_return_sequences", 1)


@pytest.mark.parametrize("name", list(so.CASES))
def test_opts_checker_equals_the_reference_golden(name):
    """every case, every clip: no row is left out"""
    g, a, v, mask = golden()
    cfg, r = AVSR_TINY, sr.EOS_RECIPE
    alpha, lp, opts, searches = so.CASES[name]
    sd = sr.eos_recipe(cfg, alpha, r["weights_seed"])
    N, B = r["max_new_tokens"], a.shape[0]
    with torch.no_grad():
        enc = oa.encode(cfg, sd, torch.from_numpy(a), torch.from_numpy(v), torch.from_numpy(mask))
    for search in searches:
        greedy = search == "greedy"
        K = 1 if greedy else r["num_beams"]
        o = {k: v_ for k, v_ in opts.items() if not (greedy and k in ("early_stopping", "num_return_sequences"))}
        ck = so.run_search(so.OptsChecker, sr.model_logits_fn(cfg, sd, enc, mask, K), B, K, cfg.vocab_size, N, cfg.bos_token_id, cfg.eos_token_id,
                           cfg.pad_token_id, greedy=greedy, length_penalty=1.0 if greedy else lp, **o)
        seq, scores = ck.trimmed()
        want = g[f"{name}_{search}"]
        print(f"{name} {search}: steps {ck.steps}, shape {seq.shape} (reference {want.shape})")
        assert seq.shape == want.shape and np.array_equal(seq, want), f"{name} / {search}: ids differ from the reference's generate()"
        if not greedy:
            err = float(np.abs(scores - g[name + "_beam_scores"]).max())
            print(f"{name}: beam score error {err:.2e}")
            assert err <= TOL_SCORE


# ---- the checker against the restatement over transformers' processors ---------------------------------------------------------------
def same_state(a, b, what):
    assert np.array_equal(a.tokens, b.tokens), (what, "tokens", a.tokens, b.tokens)
    assert np.array_equal(a.run_seq, b.run_seq), (what, "running prefixes")
    assert np.array_equal(a.can, b.can), (what, "can_improve / unfinished")
    if not a.greedy:
        assert np.array_equal(a.src_rows, b.src_rows), (what, "src_rows")
        assert np.array_equal(a.top_idx, b.top_idx) and np.array_equal(bits(a.top_lp), bits(b.top_lp)), (what, "the 2K candidates")
        assert np.array_equal(bits(a.run_score), bits(b.run_score)), (what, "running scores")
        assert np.array_equal(bits(a.fin_score), bits(b.fin_score)), (what, "finished scores")
        assert np.array_equal(a.fin_seq, b.fin_seq) and np.array_equal(a.fin_len, b.fin_len) and np.array_equal(a.is_fin, b.is_fin), (what, "finished slots")
    assert a.goes_on == b.goes_on, (what, "stop")


def random_logits(rng, rows, V, step, eos_bias):
    x = np.full((rows, sr.pad4(V)), 7.0e8, np.float32)                # the padding columns hold a value that would win if it were read
    x[:, :V] = np.round(2.0 * rng.standard_normal((rows, V)) * 4) / 4    # quarter steps: exact ties are common
    x[:, EOS] += np.float32(eos_bias)
    return x


RANDOM_OPTS = [
    dict(repetition_penalty=1.3, no_repeat_ngram_size=2),
    dict(no_repeat_ngram_size=1),                                      # bans every token seen: V = 4 runs out of finite candidates
    dict(no_repeat_ngram_size=3, min_new_tokens=5, early_stopping=True, num_return_sequences=2),
    dict(repetition_penalty=0.8, early_stopping="never", length_penalty=2.0),
    dict(repetition_penalty=1.2, min_new_tokens=70),
]


@pytest.mark.parametrize("V", [4, 61, 1000, 2050])
@pytest.mark.parametrize("K", [1, 3, 8])
def test_opts_checker_equals_transformers_processors_on_random_logits(V, K):
    B, N = 2, 64
    ran = 0
    for i, opts in enumerate(RANDOM_OPTS):
        opts = dict(opts)
        lp = opts.pop("length_penalty", 1.0)
        if opts.get("num_return_sequences", 1) > K:
            opts["num_return_sequences"] = K
        for greedy in (False, True):
            o = {k: v for k, v in opts.items() if not (greedy and k in ("early_stopping", "num_return_sequences"))}
            k = 1 if greedy else K
            rng = np.random.default_rng([V, K, i, int(greedy)])
            ck = so.OptsChecker(B, k, V, N, BOS, EOS, PAD, greedy, lp, **o)
            ts = so.TorchSearch(B, k, V, N, BOS, EOS, PAD, greedy, lp, **o)
            for step in range(N):
                x = random_logits(rng, B * k, V, step, eos_bias=-1.0 if V > 4 else 0.5)
                ck.step(x, step)
                ts.step(x, step)
                same_state(ck, ts, f"V={V} K={K} opts={opts} greedy={greedy} step {step}")
                if not ck.goes_on:
                    break
            ran = max(ran, ck.steps)
            for got, want in zip(ck.result(), ts.result()):
                assert np.array_equal(bits(got) if got.dtype == np.float32 else got, bits(want) if want.dtype == np.float32 else want)
    assert ran == N, "at least one option set must run all 64 steps"


def test_crafted_ban_and_penalty_hit_the_argmax():
    """V = 6; token 3 has the largest logit at every step.  Greedy: an n-gram ban removes it, a penalty pushes it under token 4;
    min_new_tokens keeps eos out while it would win.  Both searches, checker == restatement, and the expected tokens by hand."""
    V = 6
    x = np.zeros((1, 8), np.float32)
    x[0, :V] = [0.0, 0.0, 1.0, 5.0, 4.0, 3.0]
    # no_repeat_ngram_size=1: 3, then 4 (3 banned), then 5, then eos (index 2), the last unbanned one above bos / pad
    ck = so.OptsChecker(1, 1, V, 6, BOS, EOS, PAD, True, no_repeat_ngram_size=1)
    ts = so.TorchSearch(1, 1, V, 6, BOS, EOS, PAD, True, no_repeat_ngram_size=1)
    for step in range(4):
        ck.step(x, step), ts.step(x, step)
        same_state(ck, ts, f"ngram 1 step {step}")
    assert ck.run_seq[0, 0, :5].tolist() == [BOS, 3, 4, 5, EOS] and not ck.goes_on
    # no_repeat_ngram_size=2: 3, 3 (nothing banned yet: the prefix [bos, 3] has no bigram starting with 3), then (3, 3) exists -> 4,
    # then 3 again ((4, 3) is new), then (3, 3) and (3, 4) are banned -> 5
    ck = so.OptsChecker(1, 1, V, 8, BOS, EOS, PAD, True, no_repeat_ngram_size=2)
    ts = so.TorchSearch(1, 1, V, 8, BOS, EOS, PAD, True, no_repeat_ngram_size=2)
    for step in range(5):
        ck.step(x, step), ts.step(x, step)
        same_state(ck, ts, f"ngram 2 step {step}")
    assert ck.run_seq[0, 0, :6].tolist() == [BOS, 3, 3, 4, 3, 5]
    # repetition_penalty=1.5: 5 / 1.5 < 4, so 3, 4, then 3 (3.33 > 4 / 1.5 > 3 = token 5's)
    ck = so.OptsChecker(1, 1, V, 8, BOS, EOS, PAD, True, repetition_penalty=1.5)
    ts = so.TorchSearch(1, 1, V, 8, BOS, EOS, PAD, True, repetition_penalty=1.5)
    for step in range(3):
        ck.step(x, step), ts.step(x, step)
        same_state(ck, ts, f"penalty step {step}")
    assert ck.run_seq[0, 0, :4].tolist() == [BOS, 3, 4, 3]
    # a negative logit is multiplied: -1 * 1.5 < -1.2
    y = np.zeros((1, 8), np.float32)
    y[0, :V] = [-9.0, -9.0, -9.0, -1.0, -1.2, -9.0]
    ck = so.OptsChecker(1, 1, V, 8, BOS, EOS, PAD, True, repetition_penalty=1.5)
    ck.step(y, 0), ck.step(y, 1)
    assert ck.run_seq[0, 0, :3].tolist() == [BOS, 3, 4]
    # min_new_tokens=2: eos has the largest logit and is taken at step 2 only
    z = np.zeros((1, 8), np.float32)
    z[0, :V] = [0.0, 0.0, 9.0, 5.0, 4.0, 3.0]
    ck = so.OptsChecker(1, 1, V, 8, BOS, EOS, PAD, True, min_new_tokens=2)
    for step in range(3):
        ck.step(z, step)
    assert ck.run_seq[0, 0, :4].tolist() == [BOS, 3, 3, EOS] and ck.fin_len.tolist() == [[4]]
    # beam, K = 2: the ban acts on the log-probabilities per hypothesis row, so the two rows lose different tokens
    xb = np.repeat(x, 2, axis=0)
    ck = so.OptsChecker(1, 2, V, 8, BOS, EOS, PAD, False, no_repeat_ngram_size=1)
    ts = so.TorchSearch(1, 2, V, 8, BOS, EOS, PAD, False, no_repeat_ngram_size=1)
    ck.step(xb, 0), ts.step(xb, 0)
    assert ck.tokens.tolist() == [3, 4]
    ck.step(xb, 1), ts.step(xb, 1)
    same_state(ck, ts, "beam ban")
    assert ck.run_seq[0, :, :3].tolist() == [[BOS, 3, 4], [BOS, 4, 3]]


def test_fewer_than_2k_finite_candidates_keep_the_total_order():
    """V = 4, K = 3, no_repeat_ngram_size=1: after two steps every row has at most one unbanned token, then none: the 2 K = 6
    candidates are filled up with -inf ones in flat-index order and nothing is NaN"""
    V, K = 4, 3
    rng = np.random.default_rng(5)
    ck = so.OptsChecker(1, K, V, 6, BOS, EOS, PAD, False, no_repeat_ngram_size=1)
    ts = so.TorchSearch(1, K, V, 6, BOS, EOS, PAD, False, no_repeat_ngram_size=1)
    seen_inf = False
    for step in range(6):
        x = random_logits(rng, K, V, step, 0.0)
        ck.step(x, step), ts.step(x, step)
        same_state(ck, ts, f"step {step}")
        assert not np.isnan(ck.top_lp).any() and not np.isnan(ck.run_score).any() and not np.isnan(ck.fin_score).any()
        inf = np.isneginf(ck.top_lp[0])
        if inf.any():
            seen_inf = True
            first = int(np.argmax(inf))
            assert inf[first:].all() and (np.diff(ck.top_idx[0, first:]) > 0).all(), "-inf candidates: flat index ascending, after the finite ones"
        if not ck.goes_on:
            break
    assert seen_inf


# ---- argument handling ------------------------------------------------------------------------------------------------------------------
def bare_model(search):
    from reazonspeech_amd.avsr import AVHubertForConditionalGeneration
    m = object.__new__(AVHubertForConditionalGeneration)
    m.search, m.config = search, AVSR_TINY
    return m


def test_device_generate_validates_with_transformers_error_types():
    m = bare_model("device")
    x = dict(input_values=np.zeros((1, 8, 104), np.float32), max_new_tokens=4)
    for kw in (dict(num_beams=3, num_return_sequences=4), dict(num_beams=1, num_return_sequences=2), dict(num_beams=3, repetition_penalty=0.0),
               dict(num_beams=3, repetition_penalty=-1.0), dict(num_beams=3, no_repeat_ngram_size=-1), dict(num_beams=3, min_new_tokens=-2),
               dict(num_beams=3, early_stopping="sometimes"), dict(num_beams=3, num_return_sequences=0)):
        with pytest.raises(ValueError):
            m.generate(**x, **kw)
    for kw in (dict(bad_words_ids=[[3]]), dict(logits_processor=[]), dict(output_scores=True, beam_indices=True)):
        with pytest.raises(TypeError):
            m.generate(**x, num_beams=3, **kw)
    with pytest.raises(NotImplementedError):
        m.generate(**x, num_beams=3, do_sample=True)
    # min_length counts the bos token; the larger of the two wins
    opts = type(m)._device_options(dict(min_length=5, min_new_tokens=2), 3)
    assert opts["min_new_tokens"] == 4 and opts["num_return_sequences"] == 1 and opts["early_stopping"] is False
    assert type(m)._device_options(dict(early_stopping=True), 1)["early_stopping"] is False       # greedy search never reads it


def test_host_search_still_refuses_and_names_the_device_search():
    m = bare_model("host")
    x = dict(input_values=np.zeros((1, 8, 104), np.float32), max_new_tokens=4, num_beams=3)
    for kw in (dict(repetition_penalty=1.2), dict(no_repeat_ngram_size=2), dict(early_stopping=True), dict(num_return_sequences=2)):
        with pytest.raises(NotImplementedError, match='search="device"'):
            m.generate(**x, **kw)
    with pytest.raises(TypeError, match='search="device"'):
        m.generate(**x, min_new_tokens=3)
    with pytest.raises(TypeError) as e:
        m.generate(**x, logits_processor=[])
    assert 'search="device"' not in str(e.value)


def test_abi_7_exports_the_opts_entry_points():
    lib = ctypes.CDLL(rs_build.build())
    assert lib.rs_abi_version() == 7
    names = {"rs_avsr_search_state_bytes_opts", "rs_avsr_search_begin_opts", "rs_avsr_search_step_opts", "rs_avsr_search_peek_opts",
             "rs_avsr_search_finish_opts", "rs_avsr_generate_state_bytes_opts", "rs_avsr_generate_opts"}
    assert names <= set(capi.EXPORTS)
    for n in names:
        assert hasattr(lib, n), n
    lib.rs_avsr_search_state_bytes_opts.restype = ctypes.c_size_t
    lib.rs_avsr_generate_state_bytes_opts.restype = ctypes.c_size_t
    o = capi.RsAvsrSearchOpts.neutral()
    assert (o.repetition_penalty, o.no_repeat_ngram_size, o.min_new_tokens, o.early_stopping, o.num_return_sequences) == (1.0, 0, 0, 0, 1)
    assert lib.rs_avsr_search_state_bytes_opts(None, 4, 5, 33, 1000, ctypes.byref(o)) == 0              # no context: invalid
    assert lib.rs_avsr_generate_state_bytes_opts(None, 4, 100, 5, 33, ctypes.byref(o)) == 0
    assert lib.rs_avsr_generate_opts(None, None, None, 1, 1, None, None, None, None, None, None, 0, None) == -1        # RS_EINVAL
    assert capi.RsAvsrSearchOpts.EARLY_STOPPING == {False: 0, True: 1, "never": 2}
    # the struct mirror has the header's fields in the header's order, and the first struct is untouched
    src = open(os.path.join(os.path.dirname(HERE), "include", "rs_asr.h")).read()
    body = src[src.index("typedef struct rs_avsr_search_opts {"):src.index("} rs_avsr_search_opts;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"\b(?:int32_t|float)\s+([a-z_0-9]+)\s*;", body) == [f[0] for f in capi.RsAvsrSearchOpts._fields_]
    assert ctypes.sizeof(capi.RsAvsrSearchOpts) == 20 and ctypes.sizeof(capi.RsAvsrSearch) == 28
