"""-m gpu: the options of generate()'s device search (rs_avsr_search_opts; the <true> kernels of csrc/k_avsr_search.hip).

  stepwise      rs_avsr_decoder_step + rs_avsr_search_step_opts, each step's logits copied out and given to the CPU checker with
                options (tests/avsr_search_opts_checker.c): tokens, src_rows, running and finished scores (raw bits) and the stop
                identical at every step; the final n-best sequences, lengths and scores identical; rs_avsr_generate_opts == that
  reference     generate(search="device", **case) on tests/golden/avsr_ref_search_opts.npz: ids identical for every case and clip
  neutral       the _opts entry points with neutral options == the plain entry points, bit for bit
  crafted       random logits with ties, V = 4 .. 5000 (the marks in LDS and in the search state), K = 1 .. 8, -inf candidates
"""
import ctypes
import hashlib
import os

import numpy as np
import pytest
import torch

from reazonspeech_amd.runtime import capi
from reazonspeech_amd.runtime.avsr_config import AVSR_TINY, AVSR_BASE
from reazonspeech_amd.runtime.avsr_synth import synthetic_clips
from reazonspeech_amd.runtime.avsr_weights import synthetic_state_dict_avsr
from reazonspeech_amd.avsr import AVHubertForConditionalGeneration

import avsr_search_ref as sr
import avsr_search_opts_ref as so
from test_avsr_search_opts_host import RANDOM_OPTS, random_logits, BOS, PAD, EOS

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
TOL_SCORE = 1e-3
BASE_EOS_ALPHA = 14.0          # tests/test_gpu_avsr_search.py's: AVSR_BASE's eos logit sits 10.7 .. 24 below the best one


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.int32)


def c_opts(opts):
    o = so.with_neutral(opts)
    return capi.RsAvsrSearchOpts(float(o["repetition_penalty"]), int(o["no_repeat_ngram_size"]), int(o["min_new_tokens"]), so.es_code(o["early_stopping"]),
                                 int(o["num_return_sequences"]))


class DeviceSearchOpts:
    """the stepwise _opts ABI with the checker's attribute names; opts None: the plain entry points"""

    def __init__(self, dev, B, K, V, max_new_tokens, bos, eos, pad, greedy=False, length_penalty=1.0, opts=None, plain=False):
        self.dev, self.B, self.K, self.V, self.N, self.plain = dev, B, K, V, max_new_tokens, plain
        self.lib, self.h = dev.ctx.lib, dev.ctx._h
        self.sp = capi.RsAvsrSearch(K, max_new_tokens, bos, eos, pad, int(greedy), float(length_penalty))
        self.so = c_opts(opts or {})
        self.n_ret = 1 if plain else self.so.num_return_sequences
        self.o = ctypes.byref(self.so)
        if plain:
            need = int(self.lib.rs_avsr_search_state_bytes(self.h, B, K, 1 + max_new_tokens))
        else:
            need = int(self.lib.rs_avsr_search_state_bytes_opts(self.h, B, K, 1 + max_new_tokens, V, self.o))
        assert need > 0
        self.state = torch.empty((need,), dtype=torch.uint8, device=dev.device)
        self.stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        st = (capi._ptr(self.state), self.state.numel(), self.stream)
        if plain:
            dev.ctx.check(self.lib.rs_avsr_search_begin(self.h, ctypes.byref(self.sp), B, V, *st))
        else:
            dev.ctx.check(self.lib.rs_avsr_search_begin_opts(self.h, ctypes.byref(self.sp), self.o, B, V, *st))
        self.peek(0)

    def rows(self):
        tok, src = ctypes.c_void_p(), ctypes.c_void_p()
        self.dev.ctx.check(self.lib.rs_avsr_search_rows(self.h, ctypes.byref(self.sp), self.B, capi._ptr(self.state), self.state.numel(),
                                                        ctypes.byref(tok), ctypes.byref(src)))
        return tok, src

    def launch(self, logits_dev, step):
        st = (capi._ptr(self.state), self.state.numel(), self.stream)
        if self.plain:
            self.dev.ctx.check(self.lib.rs_avsr_search_step(self.h, capi._ptr(logits_dev), int(step), ctypes.byref(self.sp), self.B, self.V, *st))
        else:
            self.dev.ctx.check(self.lib.rs_avsr_search_step_opts(self.h, capi._ptr(logits_dev), int(step), ctypes.byref(self.sp), self.o, self.B, self.V, *st))

    def peek(self, step):
        R = self.B * self.K
        self.tokens, self.src_rows = np.zeros((R,), np.int32), np.zeros((R,), np.int32)
        self.run_score, self.fin_score = np.zeros((self.B, self.K), np.float32), np.zeros((self.B, self.K), np.float32)
        go = ctypes.c_int32(-1)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)                  # noqa: E731
        out = (int(step), p(self.tokens), p(self.src_rows), p(self.run_score), p(self.fin_score), ctypes.byref(go), self.stream)
        if self.plain:
            self.dev.ctx.check(self.lib.rs_avsr_search_peek(self.h, ctypes.byref(self.sp), self.B, capi._ptr(self.state), self.state.numel(), *out))
        else:
            self.dev.ctx.check(self.lib.rs_avsr_search_peek_opts(self.h, ctypes.byref(self.sp), self.o, self.B, capi._ptr(self.state), self.state.numel(), *out))
        self.goes_on = bool(go.value)
        return self.goes_on

    def step(self, logits, step):
        lg = torch.from_numpy(np.ascontiguousarray(logits, dtype=np.float32)).to(self.dev.device)
        assert lg.shape == (self.B * self.K, sr.pad4(self.V))
        self.launch(lg, step)
        return self.peek(step + 1)

    def finish(self):
        n = self.n_ret
        seq = torch.empty((self.B * n, 1 + self.N), dtype=torch.int32, device=self.dev.device)
        lens = torch.empty((self.B * n,), dtype=torch.int32, device=self.dev.device)
        scores = torch.empty((self.B * n,), dtype=torch.float32, device=self.dev.device)
        st = (capi._ptr(self.state), self.state.numel(), capi._ptr(seq), capi._ptr(lens), capi._ptr(scores), self.stream)
        if self.plain:
            self.dev.ctx.check(self.lib.rs_avsr_search_finish(self.h, ctypes.byref(self.sp), self.B, *st))
        else:
            self.dev.ctx.check(self.lib.rs_avsr_search_finish_opts(self.h, ctypes.byref(self.sp), self.o, self.B, *st))
        return seq.cpu().numpy(), lens.cpu().numpy(), scores.cpu().numpy()


def same_state(ds, ck, what):
    assert np.array_equal(ds.tokens, ck.tokens), (what, "tokens", ds.tokens, ck.tokens)
    if not ck.greedy:
        assert np.array_equal(ds.src_rows, ck.src_rows), (what, "src_rows")
        assert np.array_equal(bits(ds.run_score), bits(ck.run_score)), (what, "running scores", ds.run_score, ck.run_score)
        assert np.array_equal(bits(ds.fin_score), bits(ck.fin_score)), (what, "finished scores", ds.fin_score, ck.fin_score)
    assert ds.goes_on == ck.goes_on, (what, "stop word")


def same_result(ds, ck, what):
    seq, lens, scores = ds.finish()
    want_seq, want_lens, want_scores = ck.result()
    assert np.array_equal(seq, want_seq), (what, "sequences")
    assert np.array_equal(lens, want_lens), (what, "lengths")
    assert np.array_equal(bits(scores), bits(want_scores)), (what, "scores")
    return seq, lens, scores


def split(opts, greedy):
    """(length_penalty, the options a search of this kind takes)"""
    o = dict(opts)
    lp = o.pop("length_penalty", 1.0)
    if greedy:
        o.pop("early_stopping", None), o.pop("num_return_sequences", None)
    return lp, o


def stepwise(model, a, v, mask, K, N, greedy, opts, length_penalty=1.0):
    """decoder step + device search step by step, the checker on each step's logits -> (sequences, lengths, scores, steps)"""
    dev, cfg = model.dev, model.config
    lib, h = dev.ctx.lib, dev.ctx._h
    enc = model.avhubert(input_values=a, pixel_values=v, padding_mask=mask).last_hidden_state
    B, T = enc.shape[:2]
    dec = dev.decoding(enc, mask, K, 1 + N)
    ids = (cfg.vocab_size, N, cfg.bos_token_id, cfg.eos_token_id, cfg.pad_token_id, greedy, length_penalty)
    ds = DeviceSearchOpts(dev, B, K, *ids, opts=opts)
    ck = so.OptsChecker(B, K, *ids, **opts)
    same_state(ds, ck, "begin")
    tok, src = ds.rows()
    steps = 0
    for step in range(N):
        dev.ctx.check(lib.rs_avsr_decoder_step(h, tok, None if greedy else src, step, capi._ptr(dec.mask), B, T, K, 1 + N, capi._ptr(dec.logits),
                                               capi._ptr(dec.state), dec.state.numel(), ds.stream))
        ds.launch(dec.logits, step)
        ck.step(dec.logits.cpu().numpy(), step)
        ds.peek(step + 1)
        same_state(ds, ck, f"step {step}")
        steps = step + 1
        if not ck.goes_on:
            break
    before = same_result(ds, ck, "finish")
    if steps < N:                                                       # a step issued after the stop leaves the result untouched
        ds.launch(dec.logits, steps)
        ds.peek(steps + 1)
        assert not ds.goes_on
        after = same_result(ds, ck, "finish after an extra step")
        assert all(np.array_equal(x, y) for x, y in zip(before, after))
    return before + (steps,)


def device_generate_raw(model, a, v, mask, K, N, greedy, opts, length_penalty=1.0):
    enc = model.avhubert(input_values=a, pixel_values=v, padding_mask=mask).last_hidden_state
    return model.dev.generate(enc, mask, K, N, greedy, length_penalty, **opts)


def recipe_inputs():
    r = sr.EOS_RECIPE
    a, v, mask, _ = synthetic_clips(r["clips"], r["frames"], seed=r["seed"], ragged=True, min_frames=r["min_frames"])
    return a, v, mask


@pytest.mark.parametrize("name", list(so.CASES))
def test_stepwise_bit_exact_generate_equals_it_and_the_reference_ids(gpu_device, name):
    g = np.load(os.path.join(HERE, "golden", "avsr_ref_search_opts.npz"))
    cfg, r = AVSR_TINY, sr.EOS_RECIPE
    alpha, lp, opts, searches = so.CASES[name]
    a, v, mask = recipe_inputs()
    assert hashlib.sha256(a.tobytes() + v.tobytes() + mask.tobytes()).digest() == bytes(g["input_sha256"].tolist())
    model = AVHubertForConditionalGeneration(cfg, sr.eos_recipe(cfg, alpha, r["weights_seed"]), device=str(gpu_device), search="device")
    N = r["max_new_tokens"]
    for search in searches:
        greedy = search == "greedy"
        K = 1 if greedy else r["num_beams"]
        _, o = split(opts, greedy)
        seq, lens, scores, steps = stepwise(model, a, v, mask, K, N, greedy, o, 1.0 if greedy else lp)
        print(f"{name} {search}: {steps} steps, lengths {lens.tolist()}")
        got_seq, got_scores = device_generate_raw(model, a, v, mask, K, N, greedy, o, 1.0 if greedy else lp)
        assert np.array_equal(got_seq, seq[:, :int(lens.max())]), ("rs_avsr_generate_opts != stepwise", name, search)
        assert np.array_equal(bits(got_scores), bits(scores))
        # the public call against the reference's own generate(**case)
        kw = dict(input_values=a, pixel_values=v, padding_mask=mask, max_new_tokens=N, num_beams=K)
        want = g[f"{name}_{search}"]
        if greedy:
            out = model.generate(**kw, **o)
            assert np.array_equal(out.numpy(), want), (name, "greedy ids differ from the reference's generate()")
        else:
            out = model.generate(**kw, length_penalty=lp, return_dict_in_generate=True, **opts)
            assert out.sequences.shape == want.shape and np.array_equal(out.sequences.numpy(), want), (name, "beam ids differ from the reference's generate()")
            assert out.sequences_scores.shape == (a.shape[0] * opts.get("num_return_sequences", 1),)
            err = float(np.abs(out.sequences_scores.numpy() - g[name + "_beam_scores"]).max())
            print(f"{name}: beam score error {err:.2e}")
            assert err <= TOL_SCORE


def test_stepwise_bit_exact_base_geometry(gpu_device):
    """AVSR_BASE (161M, vocabulary 1000), beams 5, 16 clips x 100 frames: every option at once, then the two sets of the measurements"""
    cfg = AVSR_BASE
    sd = sr.eos_recipe(cfg, BASE_EOS_ALPHA, 0)
    a, v, mask, _ = synthetic_clips(16, 100, seed=4242, ragged=True, min_frames=33)
    model = AVHubertForConditionalGeneration(cfg, sd, device=str(gpu_device), search="device")
    N = 24
    for opts in (dict(repetition_penalty=1.2, no_repeat_ngram_size=2, min_new_tokens=6, num_return_sequences=3, early_stopping=True),
                 dict(no_repeat_ngram_size=3, repetition_penalty=1.2), dict(num_return_sequences=5, early_stopping="never")):
        seq, lens, scores, steps = stepwise(model, a, v, mask, 5, N, False, opts)
        print("base", opts, "lengths", lens.tolist(), "steps", steps)
        got_seq, got_scores = device_generate_raw(model, a, v, mask, 5, N, False, opts)
        assert np.array_equal(got_seq, seq[:, :int(lens.max())]) and np.array_equal(bits(got_scores), bits(scores))
    o = dict(no_repeat_ngram_size=3, repetition_penalty=1.2, min_new_tokens=4)
    gseq, glens, _, _ = stepwise(model, a, v, mask, 1, N, True, o)
    got_seq, _ = device_generate_raw(model, a, v, mask, 1, N, True, o)
    assert np.array_equal(got_seq, gseq[:, :int(glens.max())])


def test_neutral_options_equal_the_plain_entry_points(gpu_device):
    cfg, r = AVSR_TINY, sr.EOS_RECIPE
    a, v, mask = recipe_inputs()
    model = AVHubertForConditionalGeneration(cfg, sr.eos_recipe(cfg, 5.5, r["weights_seed"]), device=str(gpu_device), search="device")
    dev = model.dev
    # generate: rs_avsr_generate_opts with neutral options, spelled out and defaulted, against rs_avsr_generate through ctypes
    enc = model.avhubert(input_values=a, pixel_values=v, padding_mask=mask).last_hidden_state.contiguous()
    B, T = enc.shape[:2]
    N = r["max_new_tokens"]
    for greedy, K in ((False, r["num_beams"]), (True, 1)):
        sp = dev.search_params(K, N, greedy, 1.0)
        need = int(dev.ctx.lib.rs_avsr_generate_state_bytes(dev.ctx._h, B, T, K, 1 + N))
        assert need == int(dev.ctx.lib.rs_avsr_generate_state_bytes_opts(dev.ctx._h, B, T, K, 1 + N, ctypes.byref(capi.RsAvsrSearchOpts.neutral())))
        assert need == int(dev.ctx.lib.rs_avsr_generate_state_bytes_opts(dev.ctx._h, B, T, K, 1 + N, None))
        st = torch.empty((need,), dtype=torch.uint8, device=dev.device)
        seq = torch.empty((B, 1 + N), dtype=torch.int32, device=dev.device)
        lens = torch.empty((B,), dtype=torch.int32, device=dev.device)
        sc = torch.empty((B,), dtype=torch.float32, device=dev.device)
        dev.ctx.check(dev.ctx.lib.rs_avsr_generate(dev.ctx._h, capi._ptr(enc), capi._ptr(dev._dev(mask)), B, T, ctypes.byref(sp), capi._ptr(seq),
                                                   capi._ptr(lens), capi._ptr(sc), capi._ptr(st), st.numel(),
                                                   ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
        want_seq, want_sc = seq.cpu().numpy()[:, :int(lens.max())], sc.cpu().numpy()
        for opts in ({}, dict(so.NEUTRAL)):
            got_seq, got_sc = dev.generate(enc, mask, K, N, greedy, 1.0, **opts)
            assert np.array_equal(got_seq, want_seq) and np.array_equal(bits(got_sc), bits(want_sc))
    # stepwise on crafted logits: the two families side by side, every step
    V, K, Bc, Nc = 257, 3, 3, 12
    rng = np.random.default_rng(9)
    plain = DeviceSearchOpts(dev, Bc, K, V, Nc, BOS, EOS, PAD, plain=True)
    neutral = DeviceSearchOpts(dev, Bc, K, V, Nc, BOS, EOS, PAD, opts={})
    assert plain.state.numel() == neutral.state.numel()
    for step in range(Nc):
        x = random_logits(rng, Bc * K, V, step, 1.5 + 0.25 * step)
        plain.step(x, step), neutral.step(x, step)
        assert np.array_equal(plain.tokens, neutral.tokens) and np.array_equal(plain.src_rows, neutral.src_rows)
        assert np.array_equal(bits(plain.run_score), bits(neutral.run_score)) and np.array_equal(bits(plain.fin_score), bits(neutral.fin_score))
        assert plain.goes_on == neutral.goes_on
    for x, y in zip(plain.finish(), neutral.finish()):
        assert np.array_equal(x.view(np.int32), y.view(np.int32))


@pytest.fixture(scope="module")
def tiny_dev(gpu_device):
    cfg = AVSR_TINY.with_(max_target_positions=128)                    # room for bos + 64 steps
    return AVHubertForConditionalGeneration(cfg, synthetic_state_dict_avsr(cfg, 0), device=str(gpu_device)).dev


@pytest.mark.parametrize("V,K", [(4, 1), (4, 3), (4, 8), (61, 3), (257, 8), (1000, 1), (1000, 8), (2050, 3), (5000, 8)])
def test_crafted_logits_through_the_stepwise_opts_abi(tiny_dev, V, K):
    """random logits with exact ties and every option set of the CPU test; V = 4 runs out of finite candidates; K Vp = 8 x 5000 bytes
    of marks do not fit the LDS share and live in the search state"""
    B, N = 3, 64
    for i, opts in enumerate(RANDOM_OPTS):
        opts = dict(opts)
        if opts.get("num_return_sequences", 1) > K:
            opts["num_return_sequences"] = K
        for greedy in (False, True):
            lp, o = split(opts, greedy)
            k = 1 if greedy else K
            rng = np.random.default_rng([V, K, i, int(greedy)])
            ds = DeviceSearchOpts(tiny_dev, B, k, V, N, BOS, EOS, PAD, greedy, lp, opts=o)
            ck = so.OptsChecker(B, k, V, N, BOS, EOS, PAD, greedy, lp, **o)
            for step in range(N):
                x = random_logits(rng, B * k, V, step, eos_bias=-1.0 if V > 4 else 0.5)
                ck.step(x, step)
                ds.step(x, step)
                same_state(ds, ck, f"V={V} K={K} opts={opts} greedy={greedy} step {step}")
                if not ck.goes_on:
                    break
            same_result(ds, ck, f"V={V} K={K} opts={opts} greedy={greedy}")


def test_long_run_256_tokens_with_options(gpu_device):
    cfg = AVSR_TINY.with_(max_target_positions=640)
    sd = synthetic_state_dict_avsr(cfg, 3)
    a, v, mask, _ = synthetic_clips(2, 21, seed=5, ragged=True)
    model = AVHubertForConditionalGeneration(cfg, sd, device=str(gpu_device), search="device")
    N = 256
    opts = dict(no_repeat_ngram_size=3, repetition_penalty=1.2, num_return_sequences=5)
    seq, lens, scores, steps = stepwise(model, a, v, mask, 5, N, False, opts)
    assert 1 <= steps <= N and int(lens.max()) <= 1 + N
    out = model.generate(input_values=a, pixel_values=v, padding_mask=mask, num_beams=5, max_new_tokens=N, return_dict_in_generate=True, **opts)
    assert out.sequences.shape[0] == 10 and np.array_equal(out.sequences.numpy(), seq[:, :int(lens.max())])
    assert np.array_equal(bits(out.sequences_scores.numpy()), bits(scores))
    # no trigram occurs twice in a returned row
    for row, n in zip(seq, lens):
        grams = [tuple(row[i:i + 3]) for i in range(int(n) - 2)]
        assert len(grams) == len(set(grams))
    gseq, glens, _, gsteps = stepwise(model, a, v, mask, 1, N, True, dict(no_repeat_ngram_size=2, repetition_penalty=1.3))
    assert gsteps == N or (gseq == cfg.eos_token_id).any()


def test_c_abi_refuses_bad_options(tiny_dev):
    lib, h, cfg = tiny_dev.ctx.lib, tiny_dev.ctx._h, AVSR_TINY
    st = torch.empty((1 << 20,), dtype=torch.uint8, device=tiny_dev.device)
    beam, greedy = capi.RsAvsrSearch(3, 4, 0, 2, 1, 0, 1.0), capi.RsAvsrSearch(1, 4, 0, 2, 1, 1, 1.0)
    bad = [(beam, (0.0, 0, 0, 0, 1)), (beam, (-1.5, 0, 0, 0, 1)), (beam, (float("nan"), 0, 0, 0, 1)), (beam, (1.0, -1, 0, 0, 1)), (beam, (1.0, 0, -1, 0, 1)),
           (beam, (1.0, 0, 0, 3, 1)), (beam, (1.0, 0, 0, -1, 1)), (beam, (1.0, 0, 0, 0, 0)), (beam, (1.0, 0, 0, 0, 4)), (greedy, (1.0, 0, 0, 0, 2))]
    for sp, fields in bad:
        o = capi.RsAvsrSearchOpts(*fields)
        with pytest.raises(capi.RsError, match="RS_EINVAL"):
            tiny_dev.ctx.check(lib.rs_avsr_search_begin_opts(h, ctypes.byref(sp), ctypes.byref(o), 2, cfg.vocab_size, capi._ptr(st), st.numel(), None))
        assert lib.rs_avsr_search_state_bytes_opts(h, 2, sp.beams, 5, cfg.vocab_size, ctypes.byref(o)) == 0 or sp.greedy
    ok = capi.RsAvsrSearchOpts(1.2, 3, 2, 1, 3)
    tiny_dev.ctx.check(lib.rs_avsr_search_begin_opts(h, ctypes.byref(beam), ctypes.byref(ok), 2, cfg.vocab_size, capi._ptr(st), st.numel(), None))
    with pytest.raises(capi.RsError, match="RS_EWORKSPACE"):
        tiny_dev.ctx.check(lib.rs_avsr_search_begin_opts(h, ctypes.byref(beam), ctypes.byref(ok), 2, cfg.vocab_size, capi._ptr(st), 64, None))
    model = AVHubertForConditionalGeneration(AVSR_TINY, synthetic_state_dict_avsr(AVSR_TINY, 0), device=str(tiny_dev.device), search="device")
    a, v, mask, _ = synthetic_clips(2, 12, seed=1, ragged=True)
    with pytest.raises(ValueError, match="num_return_sequences"):
        model.generate(input_values=a, pixel_values=v, padding_mask=mask, num_beams=3, max_new_tokens=4, num_return_sequences=4)
    with pytest.raises(ValueError, match="num_return_sequences"):
        model.generate(input_values=a, pixel_values=v, padding_mask=mask, num_beams=1, max_new_tokens=4, num_return_sequences=2)
    with pytest.raises(ValueError, match="strictly positive"):
        model.generate(input_values=a, pixel_values=v, padding_mask=mask, num_beams=3, max_new_tokens=4, repetition_penalty=0.0)
    out = model.generate(input_values=a, pixel_values=v, padding_mask=mask, num_beams=3, max_new_tokens=6, min_length=5, num_return_sequences=2)
    assert out.shape[0] == 4 and out.shape[1] >= 5
