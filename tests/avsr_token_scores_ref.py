"""Helpers of the avsr recorded-score tests (tests/test_avsr_token_scores_host.py, tests/test_gpu_avsr_token_scores.py).
TEST INFRASTRUCTURE.

  ScoredChecker  tests/avsr_token_scores_checker.c through ctypes: avsr_search_opts_ref.OptsChecker that also keeps what the
                 _scored entry points of csrc/k_avsr_search.hip record: per hypothesis row and generated position the processed score
                 of the chosen token, the log-sum-exp of its row and the row it was taken from; optionally every step's processed rows
  golden         tests/golden/avsr_ref_token_scores.npz (make_avsr_token_scores_golden.py) with the inputs it was made from
"""
import ctypes
import hashlib
import os

import numpy as np

import avsr_search_ref as sr
import avsr_search_opts_ref as so
import checker_lib

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN_CASES = {"beam": ("beam", {}), "greedy": ("greedy", {}), "combined": ("beam", so.CASES["combined"][2]), "nret3": ("beam", so.CASES["nret3"][2])}


def lib():
    L = checker_lib.load("avsr_token_scores_checker.c", link_oracle=False, includes=("avsr_search_opts_checker.c", "avsr_search_checker.c"))
    L.rs_avsr_checker_scored_greedy_step.restype = ctypes.c_int
    L.rs_avsr_checker_scored_beam_step.restype = ctypes.c_int
    return L


def golden():
    g = np.load(os.path.join(HERE, "golden", "avsr_ref_token_scores.npz"))
    r = sr.EOS_RECIPE
    from reazonspeech_amd.runtime.avsr_synth import synthetic_clips
    a, v, mask, _ = synthetic_clips(r["clips"], r["frames"], seed=r["seed"], ragged=True, min_frames=r["min_frames"])
    assert hashlib.sha256(a.tobytes() + v.tobytes() + mask.tobytes()).digest() == bytes(g["input_sha256"].tolist()), "inputs drifted from the golden's"
    assert int(g["beams"]) == r["num_beams"] and int(g["new_tokens"]) == r["max_new_tokens"] and int(g["clips"]) == r["clips"]
    return g, a, v, mask


class ScoredChecker(so.OptsChecker):
    """OptsChecker with the recording; dump=True keeps every step's processed rows in .step_scores [max_new_tokens][B * K][Vp]"""

    def __init__(self, *args, dump=False, **kw):
        super().__init__(*args, **kw)
        shape = (self.B, self.K, self.max_len)
        self.run_ts, self.run_tl, self.run_bi = np.zeros(shape, np.float32), np.zeros(shape, np.float32), np.full(shape, -1, np.int32)
        self.fin_ts, self.fin_tl, self.fin_bi = np.zeros(shape, np.float32), np.zeros(shape, np.float32), np.full(shape, -1, np.int32)
        self.dump, self.step_scores = dump, None

    def step(self, logits, step):
        if not self.goes_on:
            return False
        logits = np.ascontiguousarray(logits, dtype=np.float32)
        assert logits.ndim == 2 and logits.shape[0] == self.B * self.K and logits.shape[1] >= self.V
        Vp, L, f = logits.shape[1], lib(), ctypes.c_float
        d = None
        if self.dump:
            if self.step_scores is None:
                self.step_scores = np.full((self.max_len - 1, self.B * self.K, Vp), np.nan, np.float32)
            d = sr._fp(self.step_scores[step])
        if self.greedy:
            left = L.rs_avsr_checker_scored_greedy_step(sr._fp(logits), self.B, self.V, Vp, int(step), self.max_len, self.eos, self.pad, f(self.penalty),
                                                        self.ngram, self.min_new, sr._ip(self.run_seq), sr._ip(self.can), sr._ip(self.fin_len),
                                                        sr._ip(self.tokens), sr._fp(self.run_ts), sr._fp(self.run_tl), d)
            self.goes_on = left > 0
        else:
            rc = L.rs_avsr_checker_scored_beam_step(sr._fp(logits), self.B, self.K, self.V, Vp, int(step), self.max_len, self.eos, f(self.length_penalty),
                                                    f(self.penalty), self.ngram, self.min_new, self.es, sr._ip(self.run_seq), sr._fp(self.run_score),
                                                    sr._ip(self.fin_seq), sr._fp(self.fin_score), sr._ip(self.fin_len), sr._ip(self.is_fin), sr._ip(self.can),
                                                    sr._ip(self.tokens), sr._ip(self.src_rows), sr._fp(self.top_lp), sr._ip(self.top_idx),
                                                    sr._fp(self.run_ts), sr._fp(self.run_tl), sr._ip(self.run_bi), sr._fp(self.fin_ts), sr._fp(self.fin_tl),
                                                    sr._ip(self.fin_bi), d)
            if rc < 0:
                raise RuntimeError(f"avsr token scores checker: bad argument ({rc})")
            self.goes_on = bool(rc)
        self.steps = step + 1
        return self.goes_on

    def recorded(self):
        """what the finish kernel writes -> (token_scores f32, token_lse f32, beam_indices i32), each [B * n][max_new_tokens]: positions
        past a hypothesis' generated tokens hold 0 / 0 / -1; greedy: beam_indices all -1"""
        n = 1 if self.greedy else self.n_ret
        N = self.max_len - 1
        _, lens, _ = self.result()
        src = (self.run_ts, self.run_tl, self.run_bi) if self.greedy else (self.fin_ts, self.fin_tl, self.fin_bi)
        ts, tl, bi = (x[:, :n, 1:].reshape(self.B * n, N).copy() for x in src)
        live = (np.arange(1, N + 1)[None, :] < lens[:, None])
        ts[~live], tl[~live], bi[~live] = 0.0, 0.0, -1
        if self.greedy:
            bi[:] = -1
        return ts, tl, bi


def run_search(logits_fn, B, K, V, max_new_tokens, bos, eos, pad, greedy=False, length_penalty=1.0, dump=False, **opts):
    ck = ScoredChecker(B, K, V, max_new_tokens, bos, eos, pad, greedy, length_penalty, dump=dump, **opts)
    for step in range(max_new_tokens):
        if not ck.step(logits_fn(ck, step), step):
            break
    return ck


def fold_running(token_scores_row, g, start):
    """the running score as the search forms it: start, then one float32 addition of each token's score in step order"""
    acc = np.float32(start)
    for p in range(g):
        acc = np.float32(np.float32(token_scores_row[p]) + acc)
    return acc
