"""Helpers of the avsr device-search OPTION tests (tests/test_avsr_search_opts_host.py, tests/test_gpu_avsr_search_opts.py).
TEST INFRASTRUCTURE.

  OptsChecker    tests/avsr_search_opts_checker.c through ctypes: tests/avsr_search_ref.py's Checker with rs_avsr_search_opts
                 (repetition_penalty, no_repeat_ngram_size, min_new_tokens, early_stopping, num_return_sequences)
  TorchSearch    the same search restated over transformers' OWN RepetitionPenaltyLogitsProcessor, NoRepeatNGramLogitsProcessor and
                 MinNewTokensLengthLogitsProcessor (in _get_logits_processor's order) and _beam_search's lines in numpy float32, with
                 torch.topk replaced by a stable sort (value descending, then index ascending: the device's documented order)
  CASES          the option cases of tests/golden/make_avsr_search_opts_golden.py
"""
import ctypes

import numpy as np

import avsr_search_ref as sr
import checker_lib

NEG = np.float32(-1.0e9)

NEUTRAL = dict(repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0, early_stopping=False, num_return_sequences=1)

# name -> (alpha of eos_recipe, length_penalty, generate() options, searches the case is stored for); the values of alpha and
# length_penalty are explained in make_avsr_search_opts_golden.py
CASES = {
    "rep13": (5.5, 1.0, dict(repetition_penalty=1.3), ("beam", "greedy")),
    "ngram2": (5.5, 1.0, dict(no_repeat_ngram_size=2), ("beam", "greedy")),
    "ngram3": (5.5, 1.0, dict(no_repeat_ngram_size=3), ("beam", "greedy")),
    "min8": (6.5, 1.0, dict(min_new_tokens=8), ("beam", "greedy")),
    "es_true": (5.5, 1.0, dict(early_stopping=True), ("beam",)),
    "never": (6.5, 2.0, dict(early_stopping="never"), ("beam",)),
    "nret3": (5.5, 1.0, dict(num_return_sequences=3), ("beam",)),
    "combined": (5.5, 1.0, dict(repetition_penalty=1.2, no_repeat_ngram_size=2, min_new_tokens=6, num_return_sequences=2, early_stopping=True),
                 ("beam",)),
}


def es_code(early_stopping):
    """transformers' early_stopping (False / True / "never") -> rs_avsr_search_opts.early_stopping"""
    if early_stopping == "never":
        return 2
    if early_stopping is True or early_stopping is False:
        return int(early_stopping)
    raise ValueError(f"early_stopping must be False, True or 'never', got {early_stopping!r}")


def with_neutral(opts):
    unknown = set(opts) - set(NEUTRAL)
    assert not unknown, unknown
    return {**NEUTRAL, **opts}


def lib():
    L = checker_lib.load("avsr_search_opts_checker.c", link_oracle=False, includes=("avsr_search_checker.c",))
    L.rs_avsr_checker_opts_greedy_step.restype = ctypes.c_int
    L.rs_avsr_checker_opts_beam_step.restype = ctypes.c_int
    L.rs_avsr_checker_opts_logp.restype = None
    return L


class OptsChecker(sr.Checker):
    """sr.Checker with the options; .step as there, .result() / .trimmed() return num_return_sequences rows per clip"""

    def __init__(self, B, K, V, max_new_tokens, bos, eos, pad, greedy=False, length_penalty=1.0, **opts):
        super().__init__(B, K, V, max_new_tokens, bos, eos, pad, greedy, length_penalty)
        o = with_neutral(opts)
        self.penalty, self.ngram, self.min_new = float(o["repetition_penalty"]), int(o["no_repeat_ngram_size"]), int(o["min_new_tokens"])
        self.es, self.n_ret = es_code(o["early_stopping"]), int(o["num_return_sequences"])
        assert self.penalty > 0 and self.ngram >= 0 and self.min_new >= 0 and 1 <= self.n_ret <= K and (not greedy or self.n_ret == 1)

    def step(self, logits, step):
        if not self.goes_on:
            return False
        logits = np.ascontiguousarray(logits, dtype=np.float32)
        assert logits.ndim == 2 and logits.shape[0] == self.B * self.K and logits.shape[1] >= self.V
        Vp, L, f = logits.shape[1], lib(), ctypes.c_float
        if self.greedy:
            left = L.rs_avsr_checker_opts_greedy_step(sr._fp(logits), self.B, self.V, Vp, int(step), self.max_len, self.eos, self.pad, f(self.penalty),
                                                      self.ngram, self.min_new, sr._ip(self.run_seq), sr._ip(self.can), sr._ip(self.fin_len),
                                                      sr._ip(self.tokens))
            self.goes_on = left > 0
        else:
            rc = L.rs_avsr_checker_opts_beam_step(sr._fp(logits), self.B, self.K, self.V, Vp, int(step), self.max_len, self.eos, f(self.length_penalty),
                                                  f(self.penalty), self.ngram, self.min_new, self.es, sr._ip(self.run_seq), sr._fp(self.run_score),
                                                  sr._ip(self.fin_seq), sr._fp(self.fin_score), sr._ip(self.fin_len), sr._ip(self.is_fin), sr._ip(self.can),
                                                  sr._ip(self.tokens), sr._ip(self.src_rows), sr._fp(self.top_lp), sr._ip(self.top_idx))
            if rc < 0:
                raise RuntimeError(f"avsr search opts checker: bad argument ({rc})")
            self.goes_on = bool(rc)
        self.steps = step + 1
        return self.goes_on

    def result(self):
        """-> (sequences int32 [B * n][max_len], lengths int32 [B * n], scores float32 [B * n]), clip-major"""
        if self.greedy:
            return super().result()
        n = self.n_ret
        return (self.fin_seq[:, :n].reshape(self.B * n, self.max_len).copy(), self.fin_len[:, :n].reshape(-1).copy(),
                self.fin_score[:, :n].reshape(-1).copy())


class TorchSearch(OptsChecker):
    """the restatement over transformers' processor classes; same state and methods as OptsChecker"""

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        from transformers.generation.logits_process import (LogitsProcessorList, MinNewTokensLengthLogitsProcessor, NoRepeatNGramLogitsProcessor,
                                                            RepetitionPenaltyLogitsProcessor)
        self.procs = LogitsProcessorList()                    # GenerationMixin._get_logits_processor's order
        if self.penalty != 1.0:
            self.procs.append(RepetitionPenaltyLogitsProcessor(penalty=self.penalty))
        if self.ngram > 0:
            self.procs.append(NoRepeatNGramLogitsProcessor(self.ngram))
        if self.min_new > 0:
            self.procs.append(MinNewTokensLengthLogitsProcessor(1, self.min_new, self.eos))

    def _process(self, ids, scores):
        import torch
        with torch.no_grad():
            out = self.procs(torch.from_numpy(np.ascontiguousarray(ids, dtype=np.int64)), torch.from_numpy(np.ascontiguousarray(scores, dtype=np.float32)))
        return out.numpy().astype(np.float32)

    def step(self, logits, step):
        if not self.goes_on:
            return False
        x = np.ascontiguousarray(logits, dtype=np.float32)[:, :self.V]
        B, K, V, cur = self.B, self.K, self.V, step + 1
        f32 = np.float32
        if self.greedy:
            s = self._process(self.run_seq[:, 0, :cur], x)
            nxt = np.where(self.can != 0, np.argmax(s, axis=1), self.pad).astype(np.int32)       # argmax: the first of equal values
            self.run_seq[:, 0, cur] = nxt
            self.tokens[:] = nxt
            self.fin_len[self.can != 0, 0] = step + 2
            self.can[:] = (self.can != 0) & (nxt != self.eos)
            self.goes_on = bool(self.can.any())
            self.steps = cur
            return self.goes_on
        logp = np.empty((B * K, V), f32)
        for r in range(B * K):
            row = np.ascontiguousarray(x[r])
            lib().rs_avsr_checker_opts_logp(sr._fp(row), V, sr._fp(logp[r]))
        logp = self._process(self.run_seq.reshape(B * K, -1)[:, :cur], logp)
        flat = (logp.reshape(B, K, V) + self.run_score[:, :, None]).astype(f32).reshape(B, K * V)
        top_idx = np.argsort(-flat, axis=1, kind="stable")[:, :2 * K]
        top_lp = np.take_along_axis(flat, top_idx, axis=1)
        parent, token = top_idx // V, top_idx % V
        ends = (token == self.eos) | (cur + 1 >= self.max_len)
        lp_run = (top_lp + ends.astype(f32) * NEG).astype(f32)                                    # _get_running_beams_for_next_iteration
        keep = np.argsort(-lp_run, axis=1, kind="stable")[:, :K]
        den = f32(float(cur) ** self.length_penalty)
        den_heur = f32(float(self.max_len - 1) ** self.length_penalty) if self.es == 2 and self.length_penalty > 0 else den
        just = ends & (np.arange(2 * K) < K)[None, :]                                             # _update_finished_beams
        full = (self.is_fin != 0).all(axis=1, keepdims=True) & (self.es == 1)
        can = (self.can != 0)[:, None]
        f = (top_lp / den).astype(f32)
        f = (f + full.astype(f32) * NEG).astype(f32)
        f = (f + (~can).astype(f32) * NEG).astype(f32)
        f = (f + (~just).astype(f32) * NEG).astype(f32)
        merged = np.concatenate([self.fin_score, f], axis=1)
        best = np.argsort(-merged, axis=1, kind="stable")[:, :K]
        old_run, old_fin, old_len, old_isfin = self.run_seq.copy(), self.fin_seq.copy(), self.fin_len.copy(), self.is_fin.copy()
        for b in range(B):
            cand = old_run[b][parent[b]].copy()                                                    # [2K][max_len]
            cand[:, cur] = token[b]
            for j in range(K):
                w, c = int(best[b, j]), int(keep[b, j])
                self.fin_seq[b, j] = old_fin[b, w] if w < K else cand[w - K]
                self.fin_len[b, j] = old_len[b, w] if w < K else cur + 1
                self.is_fin[b, j] = old_isfin[b, w] if w < K else int(just[b, w - K])
                self.run_seq[b, j] = cand[c]
                self.tokens[b * K + j] = token[b, c]
                self.src_rows[b * K + j] = b * K + parent[b, c]
        self.fin_score = np.take_along_axis(merged, best, axis=1).astype(f32)
        self.run_score = np.take_along_axis(lp_run, keep, axis=1).astype(f32)
        self.top_lp, self.top_idx = top_lp, top_idx.astype(np.int32)
        # _check_early_stop_heuristic and _beam_search_has_unfinished_sequences
        best_running = (self.run_score[:, :1] / den_heur).astype(f32)
        worst = np.where(self.is_fin != 0, self.fin_score.min(axis=1, keepdims=True), NEG)
        self.can[:] = (self.can != 0) & (best_running > worst).any(axis=1)
        open_beam = not (bool((self.is_fin != 0).all()) and self.es == 1)
        self.goes_on = bool(self.can.any()) and open_beam and not bool(ends.all())
        self.steps = cur
        return self.goes_on


def run_search(cls, logits_fn, B, K, V, max_new_tokens, bos, eos, pad, greedy=False, length_penalty=1.0, on_step=None, **opts):
    """sr.run_checker for OptsChecker / TorchSearch"""
    ck = cls(B, K, V, max_new_tokens, bos, eos, pad, greedy, length_penalty, **opts)
    for step in range(max_new_tokens):
        go = ck.step(logits_fn(ck, step), step)
        if on_step is not None:
            on_step(ck, step)
        if not go:
            break
    return ck
