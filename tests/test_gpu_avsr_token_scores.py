"""-m gpu: what generate()'s device search records per token (the _scored entry points and <.., true> kernels of
csrc/k_avsr_search.hip: transformers' `scores`, `beam_indices`, compute_transition_scores).

  crafted       random logits with ties and -inf candidates through the stepwise _scored ABI, V = 4 .. 5000, K = 1 .. 8, every option
                set: every decision identical to the _opts entry points and the checker at every step; token_scores, token_lse,
                beam_indices and the step_scores dump == tests/avsr_token_scores_checker.c, bit for bit
  neutral       _scored with a NULL dump == _opts in sequences, lengths and scores, bit for bit (stepwise and generate)
  reference     generate(search="device", return_dict_in_generate=True, output_scores=True) on tests/golden/avsr_ref_token_scores.npz:
                sequences and beam_indices identical, transition scores (both normalisations) and every scores row within 1e-3
  generate      rs_avsr_generate_scored == decoder step + _step_scored, step by step, == the checker on those logits
  invariance    a clip's recorded arrays do not depend on the other clips of the batch: the search over crafted logits, and the whole
                generate() for a clip alone against the same clip in a batch of six
"""
import ctypes

import numpy as np
import pytest
import torch

from reazonspeech_amd.runtime import capi
from reazonspeech_amd.runtime.config import TINY
from reazonspeech_amd.runtime.avsr_config import AVSR_TINY, AVSR_BASE
from reazonspeech_amd.runtime.avsr_synth import synthetic_clips
from reazonspeech_amd.runtime.avsr_weights import synthetic_state_dict_avsr
from reazonspeech_amd.avsr import AVHubertForConditionalGeneration

import avsr_search_ref as sr
import avsr_token_scores_ref as ts
from test_avsr_search_opts_host import RANDOM_OPTS, random_logits, BOS, PAD, EOS
from test_avsr_token_scores_host import compare_with_golden      # asserts TOL_SCORE = 1e-3, tests/test_gpu_avsr_search_opts.py's
from test_gpu_avsr_search_opts import DeviceSearchOpts, c_opts, bits, split, same_state, recipe_inputs, BASE_EOS_ALPHA

pytestmark = pytest.mark.gpu


class DeviceSearchScored(DeviceSearchOpts):
    """the stepwise _scored ABI with the checker's attribute names; dump: keep every step's processed rows (NaN where no step wrote)"""

    def __init__(self, dev, B, K, V, max_new_tokens, bos, eos, pad, greedy=False, length_penalty=1.0, opts=None, dump=True):
        self.dev, self.B, self.K, self.V, self.N, self.plain, self.greedy = dev, B, K, V, max_new_tokens, False, greedy
        self.lib, self.h = dev.ctx.lib, dev.ctx._h
        self.sp = capi.RsAvsrSearch(K, max_new_tokens, bos, eos, pad, int(greedy), float(length_penalty))
        self.so = c_opts(opts or {})
        self.n_ret = self.so.num_return_sequences
        self.o = ctypes.byref(self.so)
        need = int(self.lib.rs_avsr_search_state_bytes_scored(self.h, B, K, 1 + max_new_tokens, V, self.o))
        assert need > int(self.lib.rs_avsr_search_state_bytes_opts(self.h, B, K, 1 + max_new_tokens, V, self.o)) > 0
        self.state = torch.empty((need,), dtype=torch.uint8, device=dev.device)
        self.step_scores = torch.full((max_new_tokens, B * K, sr.pad4(V)), float("nan"), device=dev.device) if dump else None
        self.stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        dev.ctx.check(self.lib.rs_avsr_search_begin_scored(self.h, ctypes.byref(self.sp), self.o, B, V, capi._ptr(self.state), self.state.numel(), self.stream))
        self.peek(0)

    def launch(self, logits_dev, step):
        self.dev.ctx.check(self.lib.rs_avsr_search_step_scored(self.h, capi._ptr(logits_dev), int(step), ctypes.byref(self.sp), self.o, capi._ptr(self.step_scores),
                                                               self.B, self.V, capi._ptr(self.state), self.state.numel(), self.stream))

    def peek(self, step):
        R = self.B * self.K
        self.tokens, self.src_rows = np.zeros((R,), np.int32), np.zeros((R,), np.int32)
        self.run_score, self.fin_score = np.zeros((self.B, self.K), np.float32), np.zeros((self.B, self.K), np.float32)
        go = ctypes.c_int32(-1)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)                  # noqa: E731
        self.dev.ctx.check(self.lib.rs_avsr_search_peek_scored(self.h, ctypes.byref(self.sp), self.o, self.B, capi._ptr(self.state), self.state.numel(), int(step),
                                                               p(self.tokens), p(self.src_rows), p(self.run_score), p(self.fin_score), ctypes.byref(go), self.stream))
        self.goes_on = bool(go.value)
        return self.goes_on

    def finish(self):
        """-> (sequences, lengths, scores); .recorded = (token_scores, token_lse, beam_indices), .steps_run"""
        n, d = self.n_ret, self.dev.device
        seq = torch.empty((self.B * n, 1 + self.N), dtype=torch.int32, device=d)
        lens = torch.empty((self.B * n,), dtype=torch.int32, device=d)
        scores = torch.empty((self.B * n,), dtype=torch.float32, device=d)
        tsc = torch.full((self.B * n, self.N), float("nan"), device=d)
        tl = torch.full((self.B * n, self.N), float("nan"), device=d)
        bi = None if self.greedy else torch.full((self.B * n, self.N), -7, dtype=torch.int32, device=d)
        steps = torch.full((1,), -7, dtype=torch.int32, device=d)
        self.dev.ctx.check(self.lib.rs_avsr_search_finish_scored(self.h, ctypes.byref(self.sp), self.o, self.B, capi._ptr(self.state), self.state.numel(),
                                                                 capi._ptr(seq), capi._ptr(lens), capi._ptr(scores), capi._ptr(tsc), capi._ptr(tl), capi._ptr(bi),
                                                                 capi._ptr(steps), self.stream))
        self.recorded = (tsc.cpu().numpy(), tl.cpu().numpy(), np.full((self.B * n, self.N), -1, np.int32) if bi is None else bi.cpu().numpy())
        self.steps_run = int(steps.cpu()[0])
        return seq.cpu().numpy(), lens.cpu().numpy(), scores.cpu().numpy()


def same_recorded(ds, ck, what):
    """finish_scored == the checker: sequences, lengths, scores, the three recorded arrays and the dump, raw bits"""
    seq, lens, scores = ds.finish()
    want_seq, want_lens, want_scores = ck.result()
    assert np.array_equal(seq, want_seq) and np.array_equal(lens, want_lens) and np.array_equal(bits(scores), bits(want_scores)), (what, "result")
    assert ds.steps_run == ck.steps, (what, "steps run", ds.steps_run, ck.steps)
    for name, got, want in zip(("token_scores", "token_lse", "beam_indices"), ds.recorded, ck.recorded()):
        same = np.array_equal(bits(got), bits(want)) if got.dtype == np.float32 else np.array_equal(got, want)
        assert same, (what, name, got, want)
    live = np.arange(1, ds.N + 1)[None, :] < lens[:, None]
    assert (ds.recorded[0][~live] == 0).all() and (ds.recorded[1][~live] == 0).all() and (ds.recorded[2][~live] == -1).all(), (what, "past the end")
    if ds.step_scores is not None:
        got = ds.step_scores.cpu().numpy()
        assert np.array_equal(bits(got[:ck.steps]), bits(ck.step_scores[:ck.steps])), (what, "step_scores")
        assert np.isnan(got[ck.steps:]).all(), (what, "a step that did not run wrote its rows")
    return seq, lens, scores


@pytest.fixture(scope="module")
def tiny_dev(gpu_device):
    cfg = AVSR_TINY.with_(max_target_positions=128)
    return AVHubertForConditionalGeneration(cfg, synthetic_state_dict_avsr(cfg, 0), device=str(gpu_device)).dev


@pytest.mark.parametrize("V,K,B", [(4, 1, 2), (4, 3, 3), (4, 8, 2), (61, 3, 3), (61, 8, 2), (300, 1, 2), (300, 8, 3), (5000, 3, 2), (5000, 8, 3)])
def test_crafted_logits_recorded_bit_exact_and_no_decision_changes(tiny_dev, V, K, B):
    """300 > 256: several columns per thread in Z; K Vp = 8 x 5000 bytes of marks live in the search state, not in LDS; V = 4 runs out of
    finite candidates (-inf scores are recorded); quarter-step logits tie exactly"""
    N = 10
    for i, opts in enumerate([{}] + RANDOM_OPTS):
        opts = dict(opts)
        if opts.get("num_return_sequences", 1) > K:
            opts["num_return_sequences"] = K
        for greedy in (False, True):
            lp, o = split(opts, greedy)
            k = 1 if greedy else K
            rng = np.random.default_rng([V, K, i, int(greedy)])
            ids = (B, k, V, N, BOS, EOS, PAD, greedy, lp)
            what = f"V={V} K={K} opts={opts} greedy={greedy}"
            ds, plain = DeviceSearchScored(tiny_dev, *ids, opts=o), DeviceSearchOpts(tiny_dev, *ids, opts=o)
            ck = ts.ScoredChecker(*ids, dump=True, **o)
            for step in range(N):
                x = random_logits(rng, B * k, V, step, eos_bias=-1.0 if V > 4 else 0.5)
                ck.step(x, step), ds.step(x, step), plain.step(x, step)
                same_state(ds, ck, f"{what} step {step}")
                same_state(plain, ck, f"{what} step {step} (_opts)")
                if not ck.goes_on:
                    break
            got = same_recorded(ds, ck, what)
            for x, y in zip(got, plain.finish()):
                assert np.array_equal(x.view(np.int32), y.view(np.int32)), (what, "_scored result != _opts result")


def test_neutral_scored_with_null_dump_equals_opts(gpu_device):
    cfg, r = AVSR_TINY, sr.EOS_RECIPE
    a, v, mask = recipe_inputs()
    model = AVHubertForConditionalGeneration(cfg, sr.eos_recipe(cfg, 5.5, r["weights_seed"]), device=str(gpu_device), search="device")
    dev = model.dev
    enc = model.avhubert(input_values=a, pixel_values=v, padding_mask=mask).last_hidden_state.contiguous()
    N = r["max_new_tokens"]
    for greedy, K in ((False, r["num_beams"]), (True, 1)):
        want_seq, want_sc = dev.generate(enc, mask, K, N, greedy, 1.0)
        got_seq, got_sc, rec = dev.generate(enc, mask, K, N, greedy, 1.0, record=True)        # no dump: step_scores NULL
        assert rec["step_scores"] is None and np.array_equal(got_seq, want_seq) and np.array_equal(bits(got_sc), bits(want_sc))
    V, K, B, Nc = 257, 3, 3, 12
    rng = np.random.default_rng(9)
    plain = DeviceSearchOpts(dev, B, K, V, Nc, BOS, EOS, PAD, opts={})
    scored = DeviceSearchScored(dev, B, K, V, Nc, BOS, EOS, PAD, opts={}, dump=False)
    for step in range(Nc):
        x = random_logits(rng, B * K, V, step, 1.5 + 0.25 * step)
        plain.step(x, step), scored.step(x, step)
        assert np.array_equal(plain.tokens, scored.tokens) and np.array_equal(plain.src_rows, scored.src_rows)
        assert np.array_equal(bits(plain.run_score), bits(scored.run_score)) and np.array_equal(bits(plain.fin_score), bits(scored.fin_score))
        assert plain.goes_on == scored.goes_on
    for x, y in zip(plain.finish(), scored.finish()):
        assert np.array_equal(x.view(np.int32), y.view(np.int32))
    # rs_avsr_search_rows serves a recording state: its front has the plain layout
    tok, src = scored.rows()
    ptok, _ = plain.rows()
    assert tok.value - scored.state.data_ptr() == ptok.value - plain.state.data_ptr() and src.value > tok.value


@pytest.fixture(scope="module")
def recipe_model(gpu_device):
    g, a, v, mask = ts.golden()
    cfg, r = AVSR_TINY, sr.EOS_RECIPE
    model = AVHubertForConditionalGeneration(cfg, sr.eos_recipe(cfg, float(g["alpha"]), r["weights_seed"]), device=str(gpu_device), search="device")
    return model, g, a, v, mask


@pytest.mark.parametrize("name", list(ts.GOLDEN_CASES))
def test_generate_output_equals_the_reference_golden(recipe_model, name):
    model, g, a, v, mask = recipe_model
    r = sr.EOS_RECIPE
    search, opts = ts.GOLDEN_CASES[name]
    greedy = search == "greedy"
    K, B, n = 1 if greedy else r["num_beams"], a.shape[0], opts.get("num_return_sequences", 1)
    out = model.generate(input_values=a, pixel_values=v, padding_mask=mask, num_beams=K, max_new_tokens=r["max_new_tokens"], return_dict_in_generate=True,
                         output_scores=True, **opts)
    seq = out.sequences.numpy()
    W = seq.shape[1] - 1
    lens = 1 + (out.beam_indices.numpy() >= 0).sum(axis=1) if not greedy else np.array([1 + (W if EOS_AT(row) < 0 else EOS_AT(row)) for row in seq])
    assert out.token_scores.shape == (B * n, W) and out.token_logprobs.shape == (B * n, W) and out.confidence.shape == (B * n,)
    assert (out.beam_indices is None) == greedy and (greedy or out.beam_indices.dtype == torch.int64)
    assert isinstance(out.scores, tuple) and out.scores[0].shape == (B * K, model.config.vocab_size) and out.scores[0].dtype == torch.float32
    tsc, lp = out.token_scores.numpy(), out.token_logprobs.numpy()
    bi = np.full(tsc.shape, -1, np.int32) if greedy else out.beam_indices.numpy().astype(np.int32)
    compare_with_golden(g, name, seq.astype(np.int32), None if greedy else out.sequences_scores.numpy(), tsc, tsc - lp, bi, lens,
                        None if opts else np.stack([s.numpy() for s in out.scores]), greedy)
    # compute_transition_scores, transformers' signature, from the recorded arrays; the gather over the dump agrees with them bit for bit
    assert torch.equal(model.compute_transition_scores(out.sequences, out.scores, out.beam_indices, normalize_logits=False), out.token_scores)
    assert torch.equal(model.compute_transition_scores(out.sequences, out.scores, out.beam_indices, normalize_logits=True), out.token_logprobs)
    live = np.arange(1, W + 1)[None, :] < lens[:, None]
    rows = np.repeat(np.arange(B), W).reshape(B, W) if greedy else bi
    for r_, p in zip(*np.nonzero(live)):
        assert bits(out.scores[p][rows[r_, p], seq[r_, p + 1]].numpy()) == bits(tsc[r_, p]), (name, "scores[p][beam_indices][token] != token_scores", r_, p)
    g_ = live.sum(axis=1)
    assert np.allclose(out.confidence.numpy(), np.exp(np.where(live, lp, 0).astype(np.float64).sum(axis=1) / g_), rtol=1e-12)
    assert (out.confidence.numpy() > 0).all() and (out.confidence.numpy() <= 1.0 + 1e-6).all()
    # without output_scores the same arrays and no dump
    out2 = model.generate(input_values=a, pixel_values=v, padding_mask=mask, num_beams=K, max_new_tokens=r["max_new_tokens"], return_dict_in_generate=True, **opts)
    assert out2.scores is None and torch.equal(out2.token_scores, out.token_scores) and torch.equal(out2.sequences, out.sequences)


def EOS_AT(row):
    """index of the first eos after bos in a greedy row, -1 if none: the number of generated tokens, eos included"""
    hit = np.nonzero(row[1:] == AVSR_TINY.eos_token_id)[0]
    return int(hit[0]) + 1 if hit.size else -1


def stepwise_scored(model, a, v, mask, K, N, greedy, opts):
    """decoder step + _step_scored step by step, the checker on each step's logits -> (DeviceSearchScored finished, checker)"""
    dev, cfg = model.dev, model.config
    lib, h = dev.ctx.lib, dev.ctx._h
    enc = model.avhubert(input_values=a, pixel_values=v, padding_mask=mask).last_hidden_state
    B, T = enc.shape[:2]
    dec = dev.decoding(enc, mask, K, 1 + N)
    ids = (B, K, cfg.vocab_size, N, cfg.bos_token_id, cfg.eos_token_id, cfg.pad_token_id, greedy, 1.0)
    ds = DeviceSearchScored(dev, *ids, opts=opts)
    ck = ts.ScoredChecker(*ids, dump=True, **opts)
    tok, src = ds.rows()
    for step in range(N):
        dev.ctx.check(lib.rs_avsr_decoder_step(h, tok, None if greedy else src, step, capi._ptr(dec.mask), B, T, K, 1 + N, capi._ptr(dec.logits),
                                               capi._ptr(dec.state), dec.state.numel(), ds.stream))
        ds.launch(dec.logits, step)
        ck.step(dec.logits.cpu().numpy(), step)
        ds.peek(step + 1)
        same_state(ds, ck, f"step {step}")
        if not ck.goes_on:
            break
    return ds, ck, same_recorded(ds, ck, "finish"), enc


def same_as_generate(model, enc, mask, K, N, greedy, opts, ds, result):
    seq, lens, scores = result
    got_seq, got_scores, rec = model.dev.generate(enc, mask, K, N, greedy, 1.0, record=True, dump_scores=True, **opts)
    L = int(lens.max())
    assert np.array_equal(got_seq, seq[:, :L]) and np.array_equal(bits(got_scores), bits(scores)), "rs_avsr_generate_scored != stepwise"
    assert rec["steps"] == ds.steps_run and np.array_equal(rec["lengths"], lens)
    tsc, tl, bi = ds.recorded
    assert np.array_equal(bits(rec["token_scores"]), bits(tsc[:, :L - 1])) and np.array_equal(bits(rec["token_lse"]), bits(tl[:, :L - 1]))
    assert greedy or np.array_equal(rec["beam_indices"], bi[:, :L - 1])
    want = ds.step_scores.cpu().numpy()[:ds.steps_run, :, :model.config.vocab_size]
    assert np.array_equal(bits(rec["step_scores"]), bits(want)), "the dump of rs_avsr_generate_scored != the stepwise dump"


@pytest.mark.parametrize("search", ["beam", "greedy"])
def test_generate_scored_equals_the_stepwise_run(recipe_model, search):
    model, g, a, v, mask = recipe_model
    r = sr.EOS_RECIPE
    greedy = search == "greedy"
    opts = dict(repetition_penalty=1.2, no_repeat_ngram_size=2, min_new_tokens=6)
    if not greedy:
        opts.update(num_return_sequences=2, early_stopping=True)
    K, N = 1 if greedy else r["num_beams"], r["max_new_tokens"]
    ds, ck, result, enc = stepwise_scored(model, a, v, mask, K, N, greedy, opts)
    same_as_generate(model, enc, mask, K, N, greedy, opts, ds, result)


def test_base_geometry_equals_its_checker(gpu_device):
    """AVSR_BASE (161M, vocabulary 1000: four columns per thread in Z), 2 clips, 5 beams, 8 tokens"""
    cfg = AVSR_BASE
    model = AVHubertForConditionalGeneration(cfg, sr.eos_recipe(cfg, BASE_EOS_ALPHA, 0), device=str(gpu_device), search="device")
    a, v, mask, _ = synthetic_clips(2, 40, seed=4242, ragged=True, min_frames=20)
    opts = dict(repetition_penalty=1.2, no_repeat_ngram_size=2, num_return_sequences=3)
    ds, ck, result, enc = stepwise_scored(model, a, v, mask, 5, 8, False, opts)
    same_as_generate(model, enc, mask, 5, 8, False, opts, ds, result)


@pytest.mark.parametrize("greedy", [False, True])
def test_a_clips_recorded_arrays_do_not_depend_on_the_batch(tiny_dev, greedy):
    """crafted logits: clip 1 of a batch of three and the same clip alone record the same bits for the hypotheses they return"""
    V, K, N, B = 300, 1 if greedy else 3, 10, 3
    opts = dict(repetition_penalty=1.3, no_repeat_ngram_size=2)
    if not greedy:
        opts["num_return_sequences"] = 2
    rng = np.random.default_rng(77)
    xs = [random_logits(rng, B * K, V, step, eos_bias=2.0 + 0.5 * step) for step in range(N)]
    both, alone = DeviceSearchScored(tiny_dev, B, K, V, N, BOS, EOS, PAD, greedy, opts=opts), DeviceSearchScored(tiny_dev, 1, K, V, N, BOS, EOS, PAD, greedy, opts=opts)
    for step in range(N):
        both.step(xs[step], step)
        alone.step(xs[step][K:2 * K], step)                              # the crafted logits do not depend on the prefixes: clip 1's rows
    n = both.n_ret
    res_b, res_a = both.finish(), alone.finish()
    assert int(res_a[1].min()) >= 2, "the clip must have finished hypotheses for the comparison to say anything"
    for x, y in zip(res_b, res_a):
        assert np.array_equal(x[n:2 * n].view(np.int32), y.view(np.int32))
    for name, x, y in zip(("token_scores", "token_lse", "beam_indices"), both.recorded, alone.recorded):
        if name == "beam_indices":
            y = np.where(y >= 0, y + K, y)                               # flat rows: clip 1 starts at row K
        assert np.array_equal(x[n:2 * n].view(np.int32), y.view(np.int32)), name


@pytest.mark.parametrize("search", ["beam", "greedy"])
def test_generate_records_the_same_bits_for_a_clip_alone_and_in_the_batch(recipe_model, search):
    """the whole path (encoder, decoder, search) at the batch's frame count: clips 1 and 4 alone == their rows of the batch of six"""
    model, g, a, v, mask = recipe_model
    greedy = search == "greedy"
    K, n = (1, 1) if greedy else (sr.EOS_RECIPE["num_beams"], 2)
    opts = dict(repetition_penalty=1.2, no_repeat_ngram_size=2)
    if not greedy:
        opts["num_return_sequences"] = n
    kw = dict(num_beams=K, max_new_tokens=sr.EOS_RECIPE["max_new_tokens"], return_dict_in_generate=True, output_scores=True, **opts)
    full = model.generate(input_values=a, pixel_values=v, padding_mask=mask, **kw)
    for c in (1, 4):
        one = model.generate(input_values=a[c:c + 1], pixel_values=v[c:c + 1], padding_mask=mask[c:c + 1], **kw)
        L, rows = one.sequences.shape[1], slice(c * n, (c + 1) * n)
        assert torch.equal(full.sequences[rows, :L], one.sequences) and (full.sequences[rows, L:] == model.config.pad_token_id).all()
        for name in ("token_scores", "token_logprobs"):
            x, y = getattr(full, name)[rows].numpy(), getattr(one, name).numpy()
            assert np.array_equal(bits(x[:, :L - 1]), bits(y)) and (x[:, L - 1:] == 0).all(), (search, c, name)
        assert bits(full.confidence[rows].numpy().astype(np.float32)).tolist() == bits(one.confidence.numpy().astype(np.float32)).tolist()
        if not greedy:
            x, y = full.beam_indices[rows].numpy(), one.beam_indices.numpy()
            assert np.array_equal(np.where(x[:, :L - 1] >= 0, x[:, :L - 1] - c * K, -1), y) and (x[:, L - 1:] == -1).all(), (search, c, "beam_indices")
        for p_ in range(len(one.scores)):                                  # the clip's rows of every step's dump
            assert np.array_equal(bits(full.scores[p_][c * K:(c + 1) * K].numpy()), bits(one.scores[p_].numpy())), (search, c, "scores", p_)


def test_c_abi_refuses_bad_scored_calls(tiny_dev):
    lib, h, cfg, d = tiny_dev.ctx.lib, tiny_dev.ctx._h, AVSR_TINY, tiny_dev.device
    beam, greedy = capi.RsAvsrSearch(3, 4, 0, 2, 1, 0, 1.0), capi.RsAvsrSearch(1, 4, 0, 2, 1, 1, 1.0)
    o = capi.RsAvsrSearchOpts(1.2, 2, 0, 0, 2)
    B, V = 2, cfg.vocab_size
    need = int(lib.rs_avsr_search_state_bytes_scored(h, B, 3, 5, V, ctypes.byref(o)))
    assert need > int(lib.rs_avsr_search_state_bytes_opts(h, B, 3, 5, V, ctypes.byref(o))) > 0
    assert lib.rs_avsr_search_state_bytes_scored(h, 0, 3, 5, V, ctypes.byref(o)) == 0 and lib.rs_avsr_search_state_bytes_scored(h, B, 9, 5, V, ctypes.byref(o)) == 0
    assert lib.rs_avsr_generate_state_bytes_scored(h, B, 0, 3, 5, ctypes.byref(o)) == 0
    st = torch.empty((need,), dtype=torch.uint8, device=d)
    arg = (capi._ptr(st), st.numel())
    with pytest.raises(capi.RsError, match="RS_EWORKSPACE"):
        tiny_dev.ctx.check(lib.rs_avsr_search_begin_scored(h, ctypes.byref(beam), ctypes.byref(o), B, V, capi._ptr(st), need - 512, None))
    tiny_dev.ctx.check(lib.rs_avsr_search_begin_scored(h, ctypes.byref(beam), ctypes.byref(o), B, V, *arg, None))
    seq = torch.empty((B * 2, 5), dtype=torch.int32, device=d)
    lens = torch.empty((B * 2,), dtype=torch.int32, device=d)
    f = torch.empty((B * 2, 4), dtype=torch.float32, device=d)
    i = torch.empty((B * 2, 4), dtype=torch.int32, device=d)
    p = capi._ptr
    for outs in ((None, p(f), p(i)), (p(f), None, p(i)), (p(f), p(f), None)):
        with pytest.raises(capi.RsError, match="RS_EINVAL"):
            tiny_dev.ctx.check(lib.rs_avsr_search_finish_scored(h, ctypes.byref(beam), ctypes.byref(o), B, *arg, p(seq), p(lens), None, *outs, None, None))
    tiny_dev.ctx.check(lib.rs_avsr_search_finish_scored(h, ctypes.byref(beam), ctypes.byref(o), B, *arg, p(seq), p(lens), None, p(f), p(f), p(i), None, None))
    assert (i.cpu().numpy() == -1).all() and (f.cpu().numpy() == 0).all(), "before any step nothing is finished: 0 / 0 / -1"
    with pytest.raises(capi.RsError, match="RS_EINVAL"):
        tiny_dev.ctx.check(lib.rs_avsr_search_step_scored(h, None, 0, ctypes.byref(beam), ctypes.byref(o), None, B, V, *arg, None))
    # greedy: beam_indices may be NULL
    tiny_dev.ctx.check(lib.rs_avsr_search_begin_scored(h, ctypes.byref(greedy), None, B, V, *arg, None))
    tiny_dev.ctx.check(lib.rs_avsr_search_finish_scored(h, ctypes.byref(greedy), None, B, *arg, p(seq), p(lens), None, p(f), p(f), None, None, None))
    # a context of another family
    other = capi.Context(TINY, 0)
    assert other.lib.rs_avsr_search_state_bytes_scored(other._h, B, 3, 5, V, ctypes.byref(o)) == 0
    with pytest.raises(capi.RsError, match="RS_EINVAL"):
        other.check(other.lib.rs_avsr_search_begin_scored(other._h, ctypes.byref(beam), ctypes.byref(o), B, V, *arg, None))
    with pytest.raises(capi.RsError, match="RS_EINVAL"):
        other.check(other.lib.rs_avsr_generate_scored(other._h, p(f), p(f), B, 4, ctypes.byref(beam), ctypes.byref(o), None, p(seq), p(lens), None, p(f), p(f), p(i),
                                                      None, *arg, None))
