"""`AVHubertModel` / `AVHubertForConditionalGeneration` of `reazonspeech.avsr` (pkg/avsr/src/avhubert/modeling_avhubert.py:119-213,
:216-391) on one MI355X.  Same call forms as the reference's classes for inference:

    model = AVHubertForConditionalGeneration.from_pretrained(path)            # or (config, state_dict) directly
    out = model.generate(**inputs, num_beams=5, max_new_tokens=256)           # README.rst
    enc = model.avhubert(input_values=..., pixel_values=..., padding_mask=...).last_hidden_state

Everything between the input tensors and the logits runs in librs_asr.so (csrc/k_avsr.hip, float32 like the reference); the search
over the logits is host logic (generation.py) or, with search="device", runs on the device too (csrc/k_avsr_search.hip).
Training-time arguments (labels, dropout, layerdrop) have no counterpart."""
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from ..runtime.avsr_config import AvsrConfig, AVSR_BASE
from ..runtime.avsr_model import AvsrDevice, resolve_search
from . import generation

AVHubertConfig = AvsrConfig


@dataclass
class AVHubertOutput:
    """modeling_avhubert.py:33-37"""
    last_hidden_state: Optional[torch.Tensor] = None
    hidden_states: Optional[torch.Tensor] = None
    attentions: Optional[torch.Tensor] = None


@dataclass
class Seq2SeqLMOutput:
    logits: Optional[torch.Tensor] = None
    encoder_last_hidden_state: Optional[torch.Tensor] = None


@dataclass
class BeamOutput:
    """generate(return_dict_in_generate=True).  The fields after `sequences_scores` are filled by search="device" only, W = the
    sequences' width - 1 generated positions, rows clip-major like `sequences`:
    scores          transformers' tuple, one float32 [B * num_beams][vocab] per step the search ran: the processed scores of every
                    hypothesis row in the order the step read them (-inf where a processor banned a token); only with output_scores=True
    beam_indices    int64 [B * n][W]: the row of `scores[p]` the token at position p was taken from, -1 past the end; None for greedy
    token_scores    float32 [B * n][W]: scores[p][beam_indices[., p]][sequences[., p + 1]], 0 past the end (eos is the last token)
    token_logprobs  float32 [B * n][W]: token_scores minus the log-sum-exp of that row of scores[p] (normalize_logits=True)
    confidence      float64 [B * n]: exp(mean of the hypothesis' token_logprobs); nan for a slot that never finished"""
    sequences: torch.Tensor
    sequences_scores: Optional[torch.Tensor] = None
    scores: Optional[tuple] = None
    beam_indices: Optional[torch.Tensor] = None
    token_scores: Optional[torch.Tensor] = None
    token_logprobs: Optional[torch.Tensor] = None
    confidence: Optional[torch.Tensor] = None


class AVHubertModel:
    """the encoder (modeling_avhubert.py:119-213)"""

    def __init__(self, config: AvsrConfig, state_dict=None, device="cuda", _dev=None, products=None):
        self.config = config
        self.dev = _dev if _dev is not None else AvsrDevice(config, state_dict, device, products=products)
        self.device = self.dev.device

    def forward(self, input_values=None, pixel_values=None, padding_mask=None, **kwargs):
        if input_values is None and pixel_values is None:
            raise ValueError("Either `input_values` or `pixel_values` must be passed")            # modeling_avhubert.py:181
        # :172-177 a missing modality contributes zero FEATURES in its half of the fused vector (rs_avsr_encoder_forward takes NULL for it)
        B, T = (input_values if input_values is not None else pixel_values).shape[:2]
        if padding_mask is None:
            padding_mask = np.zeros((B, T), np.float32)
        return AVHubertOutput(last_hidden_state=self.dev.encode(input_values, pixel_values, padding_mask))

    __call__ = forward


class AVHubertForConditionalGeneration:
    def __init__(self, config: AvsrConfig, state_dict, device="cuda", products=None, search=None):
        """products: None ($REAZONSPEECH_AVSR_PRODUCTS, default "exact") | "exact" | "x3" — runtime/avsr_model.py set_products
        search: None ($REAZONSPEECH_AVSR_SEARCH, default "host") | "host" (generation.py over the device logits) | "device"
        (rs_avsr_generate: greedy and beam search with up to 8 beams decided on the device, csrc/k_avsr_search.hip)"""
        if config.vocab_size is None:
            raise ValueError("the configuration does not define `vocab_size`")                    # modeling_avhubert.py:232-238
        self.search = resolve_search(search)
        self.config = config
        self.dev = AvsrDevice(config, state_dict, device, products=products)
        self.device = self.dev.device
        self.avhubert = AVHubertModel(config, _dev=self.dev)

    @classmethod
    def from_pretrained(cls, path, device="cuda", products=None, search=None):
        """a directory with config.json + model.safetensors / pytorch_model.bin under the reference's parameter names"""
        from ..runtime.avsr_weights import read_avsr
        cfg, sd = read_avsr(path)
        return cls(cfg, sd, device=device, products=products, search=search)

    def get_encoder(self):
        return self.avhubert

    def eval(self):
        return self

    def forward(self, input_values=None, pixel_values=None, padding_mask=None, decoder_input_ids=None, **kwargs):
        """teacher-forced logits (modeling_avhubert.py:256-314): decoder_input_ids int [B][L] -> logits float32 [B][L][V]"""
        enc = self.avhubert(input_values=input_values, pixel_values=pixel_values, padding_mask=padding_mask).last_hidden_state
        ids = np.asarray(decoder_input_ids.cpu() if torch.is_tensor(decoder_input_ids) else decoder_input_ids)
        B, L = ids.shape
        mask = padding_mask if padding_mask is not None else np.zeros(enc.shape[:2], np.float32)
        dec = self.dev.decoding(enc, mask, 1, L)
        logits = torch.empty((B, L, self.config.vocab_size), dtype=torch.float32, device=self.device)
        for t in range(L):
            logits[:, t] = dec.step(ids[:, t], t)
        return Seq2SeqLMOutput(logits=logits, encoder_last_hidden_state=enc)

    __call__ = forward

    @staticmethod
    def _device_options(opts, num_beams):
        """generate()'s search options -> AvsrDevice.search_opts' keywords, refused with transformers' own error types
        (generation/utils.py _validate_generation_mode / configuration_utils.py validate, logits_process.py constructors)"""
        out = {}
        p = opts.get("repetition_penalty", 1.0)
        if not isinstance(p, (int, float)) or isinstance(p, bool) or not p > 0:
            raise ValueError(f"`penalty` has to be a strictly positive float, but is {p}")
        out["repetition_penalty"] = float(p)
        n = opts.get("no_repeat_ngram_size", 0)
        if not isinstance(n, int) or n < 0:
            raise ValueError(f"`ngram_size` has to be a strictly positive integer, but is {n}")
        out["no_repeat_ngram_size"] = n
        m, ml = opts.get("min_new_tokens", 0), opts.get("min_length", 0)
        for name, val in (("min_new_tokens", m), ("min_length", ml)):
            if not isinstance(val, int) or val < 0:
                raise ValueError(f"`{name}` has to be a positive integer, but is {val}")
        out["min_new_tokens"] = max(m, ml - 1)                               # min_length counts the bos token, like max_length
        es = opts.get("early_stopping", False)
        if not (isinstance(es, bool) or es == "never"):
            raise ValueError(f"`early_stopping` must be a boolean or 'never', but is {es}.")
        out["early_stopping"] = es if num_beams > 1 else False               # a beam-search switch: greedy search never reads it
        r = opts.get("num_return_sequences", 1)
        if not isinstance(r, int) or r < 1:
            raise ValueError(f"`num_return_sequences` has to be a positive integer, but is {r}")
        if num_beams <= 1 and r > 1:
            raise ValueError(f"Greedy methods without beam search do not support `num_return_sequences` different than 1 (got {r}).")
        if r > max(1, num_beams):
            raise ValueError(f"`num_return_sequences` ({r}) has to be smaller or equal to `num_beams` ({num_beams}).")
        out["num_return_sequences"] = r
        return out

    def generate(self, input_values=None, pixel_values=None, padding_mask=None, num_beams=1, max_new_tokens=20, do_sample=False,
                 length_penalty=1.0, return_dict_in_generate=False, **kwargs):
        """transformers' generate() for the two modes the reference's README uses: greedy (num_beams 1) and beam search.
        -> LongTensor [B][<= 1 + max_new_tokens] starting with bos (CPU), or BeamOutput with `sequences_scores`
        With search="device" also repetition_penalty, no_repeat_ngram_size, min_new_tokens / min_length, early_stopping (False, True,
        "never") and num_return_sequences = n <= num_beams (sequences [B * n][L] clip-major, sequences_scores [B * n]), with
        transformers' semantics; do_sample, bad_words_ids and logits_processor lists stay refused.
        With search="device", return_dict_in_generate=True also records, on the device, every token's score (BeamOutput: beam_indices,
        token_scores, token_logprobs, confidence; compute_transition_scores() is served from them), and output_scores=True adds the
        `scores` tuple.  One difference from transformers: past a greedy row's eos transformers gathers the pad token's logit of a
        row fed with pad; here those positions are 0.0.  Without return_dict_in_generate nothing is recorded; search="host" ignores
        output_scores as before."""
        if do_sample:
            raise NotImplementedError("sampling is not built (the reference's documented call is deterministic beam search)")
        # transformers' generate() takes dozens of options; the ones that change the search and are not restated here must not be
        # dropped silently
        if "max_length" in kwargs and kwargs["max_length"] is not None:
            max_new_tokens = int(kwargs.pop("max_length")) - 1              # the prompt is the one bos token
        neutral = {"use_cache": None, "output_scores": None, "early_stopping": False, "num_return_sequences": 1, "num_beam_groups": 1,
                   "repetition_penalty": 1.0, "no_repeat_ngram_size": 0, "temperature": 1.0, "top_k": None, "top_p": None,
                   "attention_mask": None, "max_length": None}
        # the options the device search has (csrc/k_avsr_search.hip, rs_avsr_search_opts); the host path refuses them as before
        device_opts = {"early_stopping", "num_return_sequences", "repetition_penalty", "no_repeat_ngram_size", "min_new_tokens", "min_length"}
        on_device = self.search == "device"
        opts = {}
        for k, v in kwargs.items():
            if on_device and k in device_opts:
                if v is not None:
                    opts[k] = v
                continue
            if k not in neutral:
                hint = ' (search="device" has it)' if k in device_opts else ""
                raise TypeError(f"generate(): option `{k}` is not built{hint} (greedy and beam search with num_beams, max_new_tokens / max_length, length_penalty are)")
            if neutral[k] is not None and v is not None and v != neutral[k]:
                hint = '; search="device" has it' if k in device_opts else ""
                raise NotImplementedError(f"generate(): `{k}={v!r}` changes the search and is not built (only {neutral[k]!r}{hint})")
        if on_device and num_beams > AvsrDevice.MAX_DEVICE_BEAMS:
            raise ValueError(f"search='device': num_beams={num_beams} exceeds the device search's limit of {AvsrDevice.MAX_DEVICE_BEAMS} "
                             "(build the model with search='host' for wider beams)")
        if on_device:
            opts = self._device_options(opts, int(num_beams))
        enc = self.avhubert(input_values=input_values, pixel_values=pixel_values, padding_mask=padding_mask).last_hidden_state
        mask = padding_mask if padding_mask is not None else np.zeros(enc.shape[:2], np.float32)
        if self.search == "device":
            greedy = num_beams <= 1
            K = 1 if greedy else int(num_beams)
            if return_dict_in_generate:
                seq, scores, rec = self.dev.generate(enc, mask, K, int(max_new_tokens), greedy, float(length_penalty), record=True,
                                                     dump_scores=bool(kwargs.get("output_scores")), **opts)
                return self._scored_output(seq, None if greedy else scores, rec)
            seq, scores = self.dev.generate(enc, mask, K, int(max_new_tokens), greedy, float(length_penalty), **opts)
            scores = None if greedy else scores
        elif num_beams <= 1:
            seq, scores = generation.greedy_search(self.dev, enc, mask, int(max_new_tokens)), None
        else:
            seq, scores = generation.beam_search(self.dev, enc, mask, int(num_beams), int(max_new_tokens), float(length_penalty))
        seq = torch.from_numpy(np.ascontiguousarray(seq))
        if return_dict_in_generate:
            return BeamOutput(seq, None if scores is None else torch.from_numpy(np.ascontiguousarray(scores)))
        return seq

    def _scored_output(self, seq, scores, rec):
        """the arrays rs_avsr_generate_scored recorded -> BeamOutput; kept for compute_transition_scores"""
        ts, lse = rec["token_scores"], rec["token_lse"]
        live = np.arange(1, ts.shape[1] + 1)[None, :] < rec["lengths"][:, None]
        lp = np.where(live, ts - np.where(live, lse, 0.0), 0.0).astype(np.float32)
        g = live.sum(axis=1)
        with np.errstate(invalid="ignore", divide="ignore"):
            conf = np.exp(lp.astype(np.float64).sum(axis=1) / g)
        t = lambda x: torch.from_numpy(np.ascontiguousarray(x))                                     # noqa: E731
        out = BeamOutput(t(seq), None if scores is None else t(scores),
                         scores=None if rec["step_scores"] is None else tuple(t(x) for x in rec["step_scores"]),
                         beam_indices=None if rec["beam_indices"] is None else t(rec["beam_indices"].astype(np.int64)),
                         token_scores=t(ts), token_logprobs=t(lp), confidence=t(conf))
        self._scored = out
        return out

    def compute_transition_scores(self, sequences, scores=None, beam_indices=None, normalize_logits=False):
        """transformers' GenerationMixin.compute_transition_scores for the sequences of the last generate(search="device",
        return_dict_in_generate=True): float32 [B * n][W], served from the arrays the device recorded (`scores` and `beam_indices`
        are accepted for the signature's sake and not read, so output_scores=True is not needed).  normalize_logits=True returns
        token_logprobs.  Positions past a hypothesis' end hold 0 (also for greedy search, where transformers gathers the pad token's
        logit)."""
        last = getattr(self, "_scored", None)
        if last is None:
            raise ValueError('compute_transition_scores: no recorded generate() (search="device", return_dict_in_generate=True) precedes this call')
        sequences = torch.as_tensor(sequences)
        if sequences.shape != last.sequences.shape or not torch.equal(sequences.cpu().to(last.sequences.dtype), last.sequences):
            raise ValueError("compute_transition_scores: `sequences` are not those of the last recorded generate()")
        return (last.token_logprobs if normalize_logits else last.token_scores).clone()


def synthetic_model(config: AvsrConfig = AVSR_BASE, seed: int = 0, device="cuda", products=None, search=None):
    """seeded synthetic weights under the reference's parameter names (benchmarks / tests: no checkpoint is reachable offline)"""
    from ..runtime.avsr_weights import synthetic_state_dict_avsr
    return AVHubertForConditionalGeneration(config, synthetic_state_dict_avsr(config, seed), device=device, products=products, search=search)
