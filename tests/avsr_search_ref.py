"""Helpers of the avsr device-search tests (tests/test_avsr_search_host.py, tests/test_gpu_avsr_search.py).  TEST INFRASTRUCTURE.

  Checker        tests/avsr_search_checker.c through ctypes: one step of csrc/k_avsr_search.hip's greedy / beam search restated in the
                 device's float32 order over a logits array; the state lives in numpy arrays here and is driven step by step
  run_checker    the whole search over a logits callback (a model, or a recorded / random stream)
  eos_recipe     the synthetic weights of tests/golden/make_avsr_eos_golden.py: AVSR_TINY whose decoder is biased towards eos
"""
import ctypes

import numpy as np

import checker_lib

MAX_K = 8


def lib():
    L = checker_lib.load("avsr_search_checker.c", link_oracle=False)
    L.rs_avsr_checker_greedy_step.restype = ctypes.c_int
    L.rs_avsr_checker_beam_step.restype = ctypes.c_int
    return L


def _fp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def _ip(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))


def pad4(v):
    return (v + 3) // 4 * 4


class Checker:
    """the search state of B clips; step(logits float32 [B * K][>= V], step) advances it and returns whether the search goes on"""

    def __init__(self, B, K, V, max_new_tokens, bos, eos, pad, greedy=False, length_penalty=1.0):
        assert 1 <= K <= MAX_K and (not greedy or K == 1)
        self.B, self.K, self.V, self.max_len = B, K, V, 1 + max_new_tokens
        self.bos, self.eos, self.pad, self.greedy, self.length_penalty = bos, eos, pad, greedy, float(length_penalty)
        R = B * K
        self.run_seq = np.full((B, K, self.max_len), pad, np.int32)
        self.run_seq[:, :, 0] = bos
        self.fin_seq = self.run_seq.copy()
        self.run_score = np.zeros((B, K), np.float32)
        self.run_score[:, 1:] = -1.0e9
        self.fin_score = np.full((B, K), -1.0e9, np.float32)
        self.fin_len = np.full((B, K), 1 if greedy else 0, np.int32)
        self.is_fin = np.zeros((B, K), np.int32)
        self.can = np.ones((B,), np.int32)                   # beam: can_improve; greedy: unfinished
        self.tokens = np.full((R,), bos, np.int32)
        self.src_rows = np.arange(R, dtype=np.int32)
        self.top_lp = np.zeros((B, 2 * K), np.float32)
        self.top_idx = np.zeros((B, 2 * K), np.int32)
        self.goes_on = True
        self.steps = 0

    def step(self, logits, step):
        """a step after the stop changes nothing, like the device's"""
        if not self.goes_on:
            return False
        logits = np.ascontiguousarray(logits, dtype=np.float32)
        assert logits.ndim == 2 and logits.shape[0] == self.B * self.K and logits.shape[1] >= self.V
        Vp = logits.shape[1]
        L = lib()
        if self.greedy:
            left = L.rs_avsr_checker_greedy_step(_fp(logits), self.B, self.V, Vp, int(step), self.max_len, self.eos, self.pad, _ip(self.run_seq),
                                                 _ip(self.can), _ip(self.fin_len), _ip(self.tokens))
            self.goes_on = left > 0
        else:
            rc = L.rs_avsr_checker_beam_step(_fp(logits), self.B, self.K, self.V, Vp, int(step), self.max_len, self.eos,
                                             ctypes.c_float(self.length_penalty), _ip(self.run_seq), _fp(self.run_score), _ip(self.fin_seq),
                                             _fp(self.fin_score), _ip(self.fin_len), _ip(self.is_fin), _ip(self.can), _ip(self.tokens),
                                             _ip(self.src_rows), _fp(self.top_lp), _ip(self.top_idx))
            if rc < 0:
                raise RuntimeError(f"avsr search checker: bad argument ({rc})")
            self.goes_on = bool(rc)
        self.steps = step + 1
        return self.goes_on

    def result(self):
        """-> (sequences int32 [B][max_len], lengths int32 [B], scores float32 [B])"""
        if self.greedy:
            return self.run_seq[:, 0].copy(), self.fin_len[:, 0].copy(), np.zeros((self.B,), np.float32)
        return self.fin_seq[:, 0].copy(), self.fin_len[:, 0].copy(), self.fin_score[:, 0].copy()

    def trimmed(self):
        seq, lens, scores = self.result()
        return seq[:, :int(lens.max())].astype(np.int64), scores


def run_checker(logits_fn, B, K, V, max_new_tokens, bos, eos, pad, greedy=False, length_penalty=1.0, on_step=None):
    """logits_fn(checker, step) -> float32 [B * K][>= V], called with the state the device decoder would see (checker.run_seq /
    .tokens / .src_rows before the step); runs to the stop or max_new_tokens"""
    ck = Checker(B, K, V, max_new_tokens, bos, eos, pad, greedy, length_penalty)
    for step in range(max_new_tokens):
        go = ck.step(logits_fn(ck, step), step)
        if on_step is not None:
            on_step(ck, step)
        if not go:
            break
    return ck


def model_logits_fn(cfg, sd, enc, padding_mask, K):
    """logits of oracle.avsr.decode_logits for the prefixes the checker holds (the reference re-feeds the whole prefix)"""
    import torch
    from oracle import avsr as oa
    enc_k = enc.repeat_interleave(K, dim=0)
    mask_k = torch.as_tensor(np.asarray(padding_mask)).repeat_interleave(K, dim=0)

    def fn(ck, step):
        ids = torch.from_numpy(ck.run_seq[:, :, :step + 1].reshape(ck.B * ck.K, step + 1).astype(np.int64))
        with torch.no_grad():
            return oa.decode_logits(cfg, sd, enc_k, mask_k, ids)[:, -1].float().numpy()
    return fn


EOS_ALPHAS = (5.5, 6.5)
EARLY_STOP_ALPHA = 7.5           # no golden: every clip ends within ten tokens and the beam search stops long before the length limit
EOS_RECIPE = dict(clips=6, frames=24, seed=11, min_frames=8, num_beams=3, max_new_tokens=24, weights_seed=0)


def eos_recipe(cfg, alpha, weights_seed=0):
    """the weights of tests/golden/make_avsr_eos_golden.py: synthetic_state_dict_avsr(cfg, weights_seed) with
    decoder.layer_norm.bias += alpha * e / (e . e), e = lm_head.weight[eos_token_id]: every eos logit rises by alpha"""
    from reazonspeech_amd.runtime.avsr_weights import synthetic_state_dict_avsr
    assert not cfg.share_decoder_input_output_embed
    sd = synthetic_state_dict_avsr(cfg, weights_seed)
    e = sd["lm_head.weight"][cfg.eos_token_id].double()
    sd["decoder.layer_norm.bias"] = (sd["decoder.layer_norm.bias"].double() + alpha * e / (e @ e)).float()
    return sd
