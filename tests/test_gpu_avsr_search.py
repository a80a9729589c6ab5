"""-m gpu: generate()'s searches on the device (rs_avsr_search_* / rs_avsr_generate; csrc/k_avsr_search.hip).

  stepwise      rs_avsr_decoder_step + rs_avsr_search_step, each step's logits copied out and given to the CPU checker
                (tests/avsr_search_checker.c): tokens, src_rows, running and finished scores (raw bits) and the stop word identical at
                every step; final sequences, lengths and scores identical
  generate      rs_avsr_generate == the stepwise run, bit for bit
  reference     generate(search="device") on the reference's goldens (avsr_ref_tiny / base / eos): ids identical, scores 1e-3
  crafted       exact ties, rows of -1e9, V = 4, V not a multiple of 4, K = 1 and 8 through the stepwise ABI == the checker
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
from test_avsr_search_host import tie_logits, drive_ties, BOS, PAD, EOS

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
TOL_SCORE = 1e-3
BASE_EOS_ALPHA = 14.0          # AVSR_BASE's eos logit sits 10.7 .. 24 below the best one on the golden clips (tiny: 5.1 .. 18, alpha 5.5 / 6.5)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.int32)


class DeviceSearch:
    """the stepwise ABI with the checker's attribute names (tokens, src_rows, run_score, fin_score, goes_on)"""

    def __init__(self, dev, B, K, V, max_new_tokens, bos, eos, pad, greedy=False, length_penalty=1.0):
        self.dev, self.B, self.K, self.V, self.N = dev, B, K, V, max_new_tokens
        self.lib, self.h = dev.ctx.lib, dev.ctx._h
        self.sp = capi.RsAvsrSearch(K, max_new_tokens, bos, eos, pad, int(greedy), float(length_penalty))
        need = int(self.lib.rs_avsr_search_state_bytes(self.h, B, K, 1 + max_new_tokens))
        assert need > 0
        self.state = torch.empty((need,), dtype=torch.uint8, device=dev.device)
        self.stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        dev.ctx.check(self.lib.rs_avsr_search_begin(self.h, ctypes.byref(self.sp), B, V, capi._ptr(self.state), self.state.numel(), self.stream))
        self.peek(0)

    def rows(self):
        tok, src = ctypes.c_void_p(), ctypes.c_void_p()
        self.dev.ctx.check(self.lib.rs_avsr_search_rows(self.h, ctypes.byref(self.sp), self.B, capi._ptr(self.state), self.state.numel(),
                                                        ctypes.byref(tok), ctypes.byref(src)))
        return tok, src

    def launch(self, logits_dev, step):
        self.dev.ctx.check(self.lib.rs_avsr_search_step(self.h, capi._ptr(logits_dev), int(step), ctypes.byref(self.sp), self.B, self.V,
                                                        capi._ptr(self.state), self.state.numel(), self.stream))

    def peek(self, step):
        R = self.B * self.K
        self.tokens, self.src_rows = np.zeros((R,), np.int32), np.zeros((R,), np.int32)
        self.run_score, self.fin_score = np.zeros((self.B, self.K), np.float32), np.zeros((self.B, self.K), np.float32)
        go = ctypes.c_int32(-1)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)                  # noqa: E731
        self.dev.ctx.check(self.lib.rs_avsr_search_peek(self.h, ctypes.byref(self.sp), self.B, capi._ptr(self.state), self.state.numel(), int(step),
                                                        p(self.tokens), p(self.src_rows), p(self.run_score), p(self.fin_score), ctypes.byref(go), self.stream))
        self.goes_on = bool(go.value)
        return self.goes_on

    def step(self, logits, step):
        """host logits [rows][pad4(V)] -> device, one step, state read back"""
        lg = torch.from_numpy(np.ascontiguousarray(logits, dtype=np.float32)).to(self.dev.device)
        assert lg.shape == (self.B * self.K, sr.pad4(self.V))
        self.launch(lg, step)
        return self.peek(step + 1)

    def finish(self):
        seq = torch.empty((self.B, 1 + self.N), dtype=torch.int32, device=self.dev.device)
        lens = torch.empty((self.B,), dtype=torch.int32, device=self.dev.device)
        scores = torch.empty((self.B,), dtype=torch.float32, device=self.dev.device)
        self.dev.ctx.check(self.lib.rs_avsr_search_finish(self.h, ctypes.byref(self.sp), self.B, capi._ptr(self.state), self.state.numel(), capi._ptr(seq),
                                                          capi._ptr(lens), capi._ptr(scores), self.stream))
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


def stepwise(model, a, v, mask, K, N, greedy, extra_steps=1):
    """decoder step + device search step by step, the checker on each step's logits -> (sequences, lengths, scores, steps)"""
    dev, cfg = model.dev, model.config
    lib, h = dev.ctx.lib, dev.ctx._h
    enc = model.avhubert(input_values=a, pixel_values=v, padding_mask=mask).last_hidden_state
    B, T = enc.shape[:2]
    dec = dev.decoding(enc, mask, K, 1 + N)
    ds = DeviceSearch(dev, B, K, cfg.vocab_size, N, cfg.bos_token_id, cfg.eos_token_id, cfg.pad_token_id, greedy)
    ck = sr.Checker(B, K, cfg.vocab_size, N, cfg.bos_token_id, cfg.eos_token_id, cfg.pad_token_id, greedy)
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
    for step in range(steps, min(steps + extra_steps, N)):           # steps issued after the stop leave the result untouched
        ds.launch(dec.logits, step)
        ds.peek(step + 1)
        assert not ds.goes_on
    after = same_result(ds, ck, "finish after extra steps")
    assert all(np.array_equal(x, y) for x, y in zip(before, after))
    return before + (steps,)


def device_generate_raw(model, a, v, mask, K, N, greedy):
    enc = model.avhubert(input_values=a, pixel_values=v, padding_mask=mask).last_hidden_state
    return model.dev.generate(enc, mask, K, N, greedy)


def eos_case(alpha):
    r = sr.EOS_RECIPE
    a, v, mask, _ = synthetic_clips(r["clips"], r["frames"], seed=r["seed"], ragged=True, min_frames=r["min_frames"])
    return sr.eos_recipe(AVSR_TINY, alpha, r["weights_seed"]), a, v, mask


@pytest.mark.parametrize("alpha", sr.EOS_ALPHAS + (sr.EARLY_STOP_ALPHA,))
def test_stepwise_bit_exact_and_generate_equals_it_tiny_eos(gpu_device, alpha):
    cfg, r = AVSR_TINY, sr.EOS_RECIPE
    sd, a, v, mask = eos_case(alpha)
    model = AVHubertForConditionalGeneration(cfg, sd, device=str(gpu_device), search="device")
    K, N = r["num_beams"], r["max_new_tokens"]
    for greedy in (False, True):
        k = 1 if greedy else K
        seq, lens, scores, steps = stepwise(model, a, v, mask, k, N, greedy)
        assert (seq == cfg.eos_token_id).any()
        if alpha == sr.EOS_ALPHAS[1]:
            assert int(lens.max()) < 1 + N                            # every result ended by eos (the beam search itself runs to the limit)
        if alpha == sr.EARLY_STOP_ALPHA:
            assert 1 <= steps < N                                     # the search stopped long before the length limit
        got_seq, got_scores = device_generate_raw(model, a, v, mask, k, N, greedy)
        assert np.array_equal(got_seq, seq[:, :int(lens.max())]), ("rs_avsr_generate != stepwise", greedy)
        assert np.array_equal(bits(got_scores), bits(scores))
    # beam search with one beam is not greedy search (scores, finished slots): it runs too
    stepwise(model, a, v, mask, 1, N, greedy=False)


def test_stepwise_bit_exact_base_with_an_eos_bias(gpu_device):
    """AVSR_BASE (vocabulary 1000), beams 5, 16 clips x 100 frames, 80 rows: the skinny-GEMM side of the decoder"""
    cfg = AVSR_BASE
    sd = sr.eos_recipe(cfg, BASE_EOS_ALPHA, 0)
    a, v, mask, _ = synthetic_clips(16, 100, seed=4242, ragged=True, min_frames=33)
    model = AVHubertForConditionalGeneration(cfg, sd, device=str(gpu_device), search="device")
    N = 24
    seq, lens, scores, steps = stepwise(model, a, v, mask, 5, N, greedy=False)
    print("base eos bias", BASE_EOS_ALPHA, "lengths", lens.tolist(), "steps", steps)
    assert (lens < 1 + N).sum() >= 2 and len(set(lens.tolist())) >= 2, "some clips must end early, at different lengths"
    got_seq, got_scores = device_generate_raw(model, a, v, mask, 5, N, greedy=False)
    assert np.array_equal(got_seq, seq[:, :int(lens.max())]) and np.array_equal(bits(got_scores), bits(scores))
    gseq, glens, _, _ = stepwise(model, a, v, mask, 1, N, greedy=True)
    got_seq, _ = device_generate_raw(model, a, v, mask, 1, N, greedy=True)
    assert np.array_equal(got_seq, gseq[:, :int(glens.max())])


def golden_inputs(name):
    g = np.load(os.path.join(HERE, "golden", f"avsr_ref_{name}.npz"))
    cfg = {"tiny": AVSR_TINY, "base": AVSR_BASE}[name]
    B, T = int(g["clips"]), int(g["frames"])
    a, v, mask, _ = synthetic_clips(B, T, seed=int(g["input_seed"]), ragged=True, min_frames=max(8, T // 3))
    assert hashlib.sha256(a.tobytes() + v.tobytes() + mask.tobytes()).digest() == bytes(g["input_sha256"].tolist())
    return g, cfg, synthetic_state_dict_avsr(cfg, int(g["weight_seed"])), a, v, mask


@pytest.mark.parametrize("products", ["exact", "x3"])
@pytest.mark.parametrize("name", ["tiny", "base"])
def test_device_search_vs_the_reference_goldens(gpu_device, name, products):
    g, cfg, sd, a, v, mask = golden_inputs(name)
    model = AVHubertForConditionalGeneration(cfg, sd, device=str(gpu_device), products=products, search="device")
    assert model.search == "device"
    n_new, K, kb = int(g["new_tokens"]), int(g["beams"]), int(g["beam_clips"])
    greedy = model.generate(input_values=a, pixel_values=v, padding_mask=mask, num_beams=1, max_new_tokens=n_new)
    assert greedy.dtype == torch.int64 and greedy.device.type == "cpu"
    assert np.array_equal(greedy.numpy(), g["greedy"]), "greedy ids differ from the reference's generate()"
    out = model.generate(input_values=a[:kb], pixel_values=v[:kb], padding_mask=mask[:kb], num_beams=K, max_new_tokens=n_new, return_dict_in_generate=True)
    assert np.array_equal(out.sequences.numpy(), g["beam"]), "beam-search ids differ from the reference's generate()"
    err = float(np.abs(out.sequences_scores.numpy() - g["beam_scores"]).max())
    print(f"avsr {name} {products} device search: beam score error {err:.2e}")
    assert err <= TOL_SCORE


@pytest.mark.parametrize("products", ["exact", "x3"])
@pytest.mark.parametrize("alpha", sr.EOS_ALPHAS)
def test_device_search_vs_the_reference_eos_golden(gpu_device, alpha, products):
    g = np.load(os.path.join(HERE, "golden", "avsr_ref_eos.npz"))
    cfg, r, s = AVSR_TINY, sr.EOS_RECIPE, f"_a{int(round(alpha * 10))}"
    sd, a, v, mask = eos_case(alpha)
    assert hashlib.sha256(a.tobytes() + v.tobytes() + mask.tobytes()).digest() == bytes(g["input_sha256"].tolist())
    model = AVHubertForConditionalGeneration(cfg, sd, device=str(gpu_device), products=products, search="device")
    kw = dict(input_values=a, pixel_values=v, padding_mask=mask, max_new_tokens=r["max_new_tokens"])
    assert np.array_equal(model.generate(**kw, num_beams=1).numpy(), g["greedy" + s])
    out = model.generate(**kw, num_beams=r["num_beams"], return_dict_in_generate=True)
    assert np.array_equal(out.sequences.numpy(), g["beam" + s])
    assert float(np.abs(out.sequences_scores.numpy() - g["beam_scores" + s]).max()) <= TOL_SCORE
    # and the host path on the same weights: the half of it that no golden reached before
    host = AVHubertForConditionalGeneration(cfg, sd, device=str(gpu_device), products=products, search="host")
    assert np.array_equal(host.generate(**kw, num_beams=1).numpy(), g["greedy" + s])
    assert np.array_equal(host.generate(**kw, num_beams=r["num_beams"]).numpy(), g["beam" + s])


def test_device_search_equals_host_search_on_fresh_clips(gpu_device, monkeypatch):
    cfg = AVSR_TINY
    sd = synthetic_state_dict_avsr(cfg, 0)
    a, v, mask, _ = synthetic_clips(3, 19, seed=77, ragged=True)
    monkeypatch.setenv("REAZONSPEECH_AVSR_SEARCH", "device")
    dev = AVHubertForConditionalGeneration(cfg, sd, device=str(gpu_device))
    monkeypatch.delenv("REAZONSPEECH_AVSR_SEARCH")
    host = AVHubertForConditionalGeneration(cfg, sd, device=str(gpu_device))
    assert (dev.search, host.search) == ("device", "host")
    kw = dict(input_values=a, pixel_values=v, padding_mask=mask)
    for beams in (4, 1):
        got = dev.generate(**kw, num_beams=beams, max_new_tokens=9, return_dict_in_generate=True)
        want = host.generate(**kw, num_beams=beams, max_new_tokens=9, return_dict_in_generate=True)
        assert torch.equal(got.sequences, want.sequences), beams
        assert (got.sequences_scores is None) == (want.sequences_scores is None)
        if beams > 1:
            assert float((got.sequences_scores - want.sequences_scores).abs().max()) <= TOL_SCORE
    with pytest.raises(ValueError, match="limit of 8"):
        dev.generate(**kw, num_beams=9, max_new_tokens=4)
    # argument checks of the C ABI
    lib, h = dev.dev.ctx.lib, dev.dev.ctx._h
    st = torch.empty((1 << 20,), dtype=torch.uint8, device=dev.device)
    for sp, code in ((capi.RsAvsrSearch(9, 4, 0, 2, 1, 0, 1.0), "RS_EINVAL"), (capi.RsAvsrSearch(0, 4, 0, 2, 1, 0, 1.0), "RS_EINVAL"),
                     (capi.RsAvsrSearch(2, cfg.max_target_positions, 0, 2, 1, 0, 1.0), "RS_EINVAL"), (capi.RsAvsrSearch(2, 4, 0, 2, 1, 1, 1.0), "RS_EINVAL")):
        with pytest.raises(capi.RsError, match=code):
            dev.dev.ctx.check(lib.rs_avsr_search_begin(h, ctypes.byref(sp), 2, cfg.vocab_size, capi._ptr(st), st.numel(), None))
    with pytest.raises(capi.RsError, match="RS_EWORKSPACE"):
        dev.dev.ctx.check(lib.rs_avsr_search_begin(h, ctypes.byref(capi.RsAvsrSearch(2, 4, 0, 2, 1, 0, 1.0)), 2, cfg.vocab_size, capi._ptr(st), 64, None))
    assert lib.rs_avsr_search_state_bytes(h, 2, 9, 5) == 0 and lib.rs_avsr_generate_state_bytes(h, 2, 19, 0, 5) == 0


@pytest.fixture(scope="module")
def tiny_dev(gpu_device):
    return AVHubertForConditionalGeneration(AVSR_TINY, synthetic_state_dict_avsr(AVSR_TINY, 0), device=str(gpu_device)).dev


def test_crafted_ties_through_the_stepwise_abi(tiny_dev):
    ds, first, second = drive_ties(lambda: DeviceSearch(tiny_dev, 1, 2, 5, 6, BOS, EOS, PAD))
    ck, cfirst, csecond = drive_ties(lambda: sr.Checker(1, 2, 5, 6, BOS, EOS, PAD))
    for got, want in ((first, cfirst), (second, csecond)):
        assert got[0] == want[0] and got[1] == want[1] and np.array_equal(bits(got[2]), bits(want[2]))
    assert first[0] == [3, 4] and second[1] == [0, 1]
    same_state(ds, ck, "ties")
    seq, lens, scores = same_result(ds, ck, "ties")
    assert seq[0, :4].tolist() == [BOS, 3, 1, EOS] and lens.tolist() == [4]


@pytest.mark.parametrize("V,K", [(4, 1), (4, 8), (5, 8), (61, 5), (257, 3), (1000, 8), (1003, 1), (2050, 2)])
def test_crafted_logits_through_the_stepwise_abi(tiny_dev, V, K):
    """seeded logits with planted exact ties, a row of all -1e9, a raised eos; V = 4, V not a multiple of 4, V around the 256 lanes"""
    B, N = 3, 12
    rng = np.random.default_rng(1000 * V + K)
    ds = DeviceSearch(tiny_dev, B, K, V, N, BOS, EOS, PAD)
    ck = sr.Checker(B, K, V, N, BOS, EOS, PAD)
    gd = DeviceSearch(tiny_dev, B * K, 1, V, N, BOS, EOS, PAD, greedy=True)
    gc = sr.Checker(B * K, 1, V, N, BOS, EOS, PAD, greedy=True)
    finished = False
    for step in range(N):
        x = np.full((B * K, sr.pad4(V)), 7.0e8, np.float32)           # the padding columns hold a value that would win if it were read
        x[:, :V] = np.round(2.0 * rng.standard_normal((B * K, V)) * 4) / 4          # quarter steps: exact ties are common
        x[:, EOS] += 1.5 + 0.25 * step
        x[rng.integers(0, B * K), :V] = -1.0e9
        if step == 3:
            x[:, :V] = x[0, :V]                                       # every row the same: values tie across parents
        for s, c in ((ds, ck), (gd, gc)):
            c.step(x, step)
            s.step(x, step)
            same_state(s, c, f"V={V} K={K} step {step} greedy={c.greedy}")
        finished |= bool(ck.is_fin.any())
        if not ck.goes_on and not gc.goes_on:
            break
    same_result(ds, ck, "beam")
    same_result(gd, gc, "greedy")
    assert finished


def test_batch_invariance(gpu_device):
    """a clip decoded alone (5 rows) and inside a batch of 16 (80 rows): both on the few-rows side of the decoder's 128-row GEMM switch;
    the clip is the longest of its batch, so its encoder output has the same bits too (tests/test_gpu_avsr.py)"""
    cfg = AVSR_TINY
    model = AVHubertForConditionalGeneration(cfg, sr.eos_recipe(cfg, 5.5, 0), device=str(gpu_device), search="device")
    a, v, mask, lens = synthetic_clips(16, 24, seed=31, ragged=True, min_frames=8)
    b = int(np.argmax(lens))
    assert int(lens[b]) == a.shape[1]
    kw = dict(num_beams=5, max_new_tokens=24, return_dict_in_generate=True)
    full = model.generate(input_values=a, pixel_values=v, padding_mask=mask, **kw)
    alone = model.generate(input_values=a[b:b + 1], pixel_values=v[b:b + 1], padding_mask=mask[b:b + 1], **kw)
    n = alone.sequences.shape[1]
    assert np.array_equal(full.sequences[b, :n].numpy(), alone.sequences[0].numpy()) and (full.sequences[b, n:] == cfg.pad_token_id).all()
    assert np.array_equal(bits(full.sequences_scores[b:b + 1].numpy()), bits(alone.sequences_scores.numpy()))


def test_long_run_256_tokens(gpu_device):
    """README.rst's max_new_tokens=256 with beams 5: the device search against the stepwise checker over up to 256 steps"""
    cfg = AVSR_TINY.with_(max_target_positions=640)
    sd = synthetic_state_dict_avsr(cfg, 3)
    a, v, mask, _ = synthetic_clips(2, 21, seed=5, ragged=True)
    model = AVHubertForConditionalGeneration(cfg, sd, device=str(gpu_device), search="device")
    N = 256
    seq, lens, scores, steps = stepwise(model, a, v, mask, 5, N, greedy=False)
    assert 1 <= steps <= N and int(lens.max()) <= 1 + N
    got_seq, got_scores = device_generate_raw(model, a, v, mask, 5, N, greedy=False)
    assert np.array_equal(got_seq, seq[:, :int(lens.max())]) and np.array_equal(bits(got_scores), bits(scores))
    out = model.generate(input_values=a, pixel_values=v, padding_mask=mask, num_beams=5, max_new_tokens=N)
    assert out.shape[1] <= 1 + N and np.array_equal(out.numpy(), got_seq)
