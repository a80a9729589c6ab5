"""The model object `load_model()` returns: FastConformer-RNNT on one MI355X.

It owns (through torch) every device buffer — weights, activations, workspace — and drives the
three stage entry points of librs_asr.so on torch's current HIP stream.  It stands where NeMo's
`EncDecRNNTBPEModel` stands in the reference (pkg/nemo-asr/src/transcribe.py:26-28, :48-53)
and exposes the one attribute the reference's post-processing touches: `.tokenizer`
(pkg/nemo-asr/src/decode.py:41,47).
"""
import gc
import os
import queue
import threading
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import capi, fusion
from .config import ModelConfig
from .weights import prepare_weights, DEFAULT_POS_CAP


@dataclass
class DecodedBatch:
    """host-side result of one batch: token ids and emission frames per utterance (+ the log-probability of the
    hypothesis when it came from the beam search)"""
    ids: List[List[int]]
    frames: List[List[int]]
    enc_lens: List[int]
    scores: Optional[List[float]] = None
    degraded: Optional[List[bool]] = None     # per utterance: the requested search overflowed its bound and a weaker one was used (espnet `_search`)
    # n-best (`AsrModel.nbest` / `decode(nbest=)`): per utterance the ranked list [(ids, frames, score, norm_score)], entry 0 = the
    # hypothesis above; None when not asked for
    nbest: Optional[List[list]] = None
    token_logprobs: Optional[List[List[float]]] = None   # `AsrModel.token_scores`: log-probability of every id under the model's own distribution


@dataclass
class AlignedBatch:
    """host-side result of `AsrModel.align_waveforms`: per utterance the frame and the log-probability of every given label on the
    best alignment, log P(text | audio) summed over all alignments, the best alignment's own score, and whether the text has an
    alignment at all (an infeasible one: -inf scores, frames -1, NaN log-probabilities)"""
    frames: List[List[int]]
    token_logprobs: List[List[float]]
    log_likelihood: List[float]
    alignment_log_prob: List[float]
    enc_lens: List[int]
    feasible: List[bool]


@dataclass
class RescoredBatch(DecodedBatch):
    """`DecodedBatch` of a model with `rescore` on (`AsrModel.rescore`): `rescored[b][k]` belongs to `nbest[b][k]`, the search's own
    order — (log P(text | audio) over all alignments, the best alignment's score, the token log-probabilities under the model's
    own distribution or None with `token_scores` off).  Re-ranking is the packages' business: nothing here changes the search's order."""
    rescored: Optional[List[list]] = None


def alsd_label_budget(t_frames: int, max_target_len) -> int:
    """labels a hypothesis may emit beyond the frames (oracle/alsd.py: float = multiple of T', int = absolute)"""
    return int(max_target_len * t_frames) if isinstance(max_target_len, float) else int(max_target_len)


class _Buffers:
    """activation / workspace buffers for one (B, Lmax) geometry"""

    def __init__(self, model, B, l_max):
        cfg, dev, ctx = model.cfg, model.device, model.ctx
        self.B, self.l_max = B, l_max
        self.l_pad = l_max + model.pad_left + model.pad_right
        self.t_max = max(ctx.mel_frames(self.l_pad), 1)
        self.tp_max = max(ctx.enc_frames(self.t_max), 1)
        model.ensure_pos_cap(self.tp_max)
        self.u_max = cfg.label_cap(self.tp_max)
        i32, f32 = torch.int32, torch.float32
        self.audio = torch.zeros((B, l_max), dtype=f32, device=dev)
        self.lens = torch.zeros((B,), dtype=i32, device=dev)
        self.feats = torch.empty((B, self.t_max, cfg.n_mels), dtype=f32, device=dev)
        self.n_frames = torch.zeros((B,), dtype=i32, device=dev)
        self.joint_enc = torch.empty((B, self.tp_max, cfg.joint_hidden), dtype=f32, device=dev)
        self.enc_lens = torch.zeros((B,), dtype=i32, device=dev)
        self.ids = torch.zeros((B, self.u_max), dtype=i32, device=dev)
        self.frames = torch.zeros((B, self.u_max), dtype=i32, device=dev)
        self.n_ids = torch.zeros((B,), dtype=i32, device=dev)
        self.scores = torch.zeros((B,), dtype=f32, device=dev)
        self.pops = torch.zeros((B,), dtype=i32, device=dev)     # "beam": prediction-network evaluations per utterance
        # hotwords (modified beam search, ALSD): each utterance's graph in the batch's `hw_set` (-1 = none); `stage` /
        # `fill_host` set both, `hw_set` None = the batch has no graph and the plain search runs
        self.graph_of = torch.full((B,), -1, dtype=i32, device=dev)
        self.h_graph_of = torch.full((B,), -1, dtype=i32).pin_memory()
        self.hw_set = None
        self.lm = None                  # n-gram LM of the batch (ALSD, modified beam search): (_NgramSet, alpha) or None; `stage` / `fill_host` set it
        self.ws_alsd = None              # beam-search scratch (grows with beam and alignment length): on first use
        self.score_bufs = None           # token scores (`AsrModel.score`): (workspace, logp, top1), on first use
        self.nbest_bufs = None           # n-best lists (`AsrModel.decode`): ids, frames, n_ids, scores, norm_scores, n_hyps, on first use
        self.want_nbest = 0              # entries asked for per utterance (`stage` / `fill_host` set it; 0 = the one hypothesis)
        self.nbest_n = 0                 # entries the last `decode` wrote per utterance (0 = it ran without lists)
        self.h_nbest = None              # the lists on the host (a pipeline worker copied them back)
        self.rescore_bufs = None         # n-best rescoring (`AsrModel.rescore_step`): workspace and per-entry outputs, on first use
        self.rescored_n = 0              # entries per utterance the last `rescore_step` scored (0 = it did not run)
        self.h_rescore = None            # its outputs on the host (a pipeline worker copied them back)
        self.ws = torch.empty((ctx.workspace_bytes(B, self.l_pad),), dtype=torch.uint8, device=dev)
        # the decoder of batch i overlaps the encoder of batch i+1 in the pipelined path: own scratch
        self.ws_dec = torch.empty((ctx.workspace_bytes(B, 16),), dtype=torch.uint8, device=dev)
        # pinned staging for the host boundary (inputs, and the hypotheses on the way back)
        self.h_audio = torch.zeros((B, l_max), dtype=f32).pin_memory()
        self.h_lens = torch.zeros((B,), dtype=i32).pin_memory()
        self.h_out = None
        self.step = -1                   # index of the pipeline step this buffer set currently carries (run_pipelined)
        self._model = model

    def narrow(self, l_max):
        """The same memory with the geometry of a batch whose longest utterance has `l_max` samples: tight padding for a
        group of short utterances without another allocation (the kernels take extents and strides as arguments and mask
        by per-utterance length, so results do not depend on the padded extent)."""
        l_max = (max(int(l_max), 1) + 63) // 64 * 64
        if l_max >= self.l_max:
            return self
        return _BufView(self, l_max)


class _BufView:
    """a `_Buffers` re-viewed for a smaller padded extent (see `_Buffers.narrow`); shares every allocation"""

    def __init__(self, base, l_max):
        model = base._model
        cfg, ctx = model.cfg, model.ctx
        self.base, self.B, self.l_max = base, base.B, l_max
        self.l_pad = l_max + model.pad_left + model.pad_right
        self.t_max = max(ctx.mel_frames(self.l_pad), 1)
        self.tp_max = max(ctx.enc_frames(self.t_max), 1)
        self.u_max = cfg.label_cap(self.tp_max)
        B = self.B

        def cut(t, *shape):
            n = 1
            for d in shape:
                n *= d
            return t.view(-1)[:n].view(*shape)

        # device and pinned staging re-viewed as contiguous [B][l_max] (the kernels take the row pitch as an argument):
        # the H2D copy of a narrowed batch is then ONE contiguous asynchronous copy — a column slice of the full-pitch
        # matrices made torch stage 164 MB through a pageable temporary, synchronously (profiles/r03x_host_timeline_ragged.txt)
        self.audio, self.lens = cut(base.audio, B, l_max), base.lens
        self.feats = cut(base.feats, B, self.t_max, cfg.n_mels)
        self.n_frames = base.n_frames
        self.joint_enc = cut(base.joint_enc, B, self.tp_max, cfg.joint_hidden)
        self.enc_lens = base.enc_lens
        self.ids = cut(base.ids, B, self.u_max)
        self.frames = cut(base.frames, B, self.u_max)
        self.n_ids, self.scores, self.pops = base.n_ids, base.scores, base.pops
        self.graph_of, self.h_graph_of, self.hw_set = base.graph_of, base.h_graph_of, None
        self.lm = None
        self.ws, self.ws_dec = base.ws, base.ws_dec
        self.h_audio, self.h_lens = cut(base.h_audio, B, l_max), base.h_lens
        self.h_out = None
        self.want_nbest, self.nbest_n, self.h_nbest = 0, 0, None
        self.rescored_n, self.h_rescore = 0, None
        self.step = -1

    def narrow(self, l_max):
        return self.base.narrow(l_max)

    @property
    def nbest_bufs(self):
        return self.base.nbest_bufs

    @nbest_bufs.setter
    def nbest_bufs(self, v):
        self.base.nbest_bufs = v

    @property
    def rescore_bufs(self):
        return self.base.rescore_bufs

    @rescore_bufs.setter
    def rescore_bufs(self, v):
        self.base.rescore_bufs = v

    @property
    def score_bufs(self):
        return self.base.score_bufs

    @score_bufs.setter
    def score_bufs(self, v):
        self.base.score_bufs = v

    @property
    def ws_alsd(self):
        return self.base.ws_alsd

    @ws_alsd.setter
    def ws_alsd(self, v):
        self.base.ws_alsd = v


class _HotwordSet:
    """the context graphs of a call on the device: one concatenated table (runtime/k2_hotwords.py: concat), checked by
    rs_hotwords_check before the upload"""

    def __init__(self, graphs, device):
        from . import k2_hotwords
        table = k2_hotwords.concat(graphs)
        capi.hotwords_check(table)                        # raises RsError(RS_EINVAL): nothing is uploaded or launched with a bad table
        self.n_graphs = len(graphs)
        self.dev = {k: torch.from_numpy(table[k]).to(device) for k in capi.HOTWORD_ARRAYS}
        self.struct = capi.RsHotwords(*[self.dev[k].data_ptr() if self.dev[k].numel() else None for k in capi.HOTWORD_ARRAYS],
                                      len(table["fail"]), len(table["child_tok"]), len(graphs), int(table["max_level"]))


class _NgramSet:
    """an n-gram LM on the device (runtime/ngram_lm.py: NgramLm), checked by rs_ngram_check before the upload"""

    def __init__(self, lm, device):
        capi.ngram_check(lm.arrays, lm.start, lm.order, lm.unk_logp)      # raises RsError(RS_EINVAL): nothing is uploaded with a bad table
        self.key = lm.key
        self.dev = {k: torch.from_numpy(lm.arrays[k]).to(device) for k in capi.NGRAM_ARRAYS}
        self.struct = capi.RsNgram(*[self.dev[k].data_ptr() if self.dev[k].numel() else None for k in capi.NGRAM_ARRAYS],
                                   lm.n_nodes, lm.n_children, lm.n_logits, lm.order, lm.start, float(lm.unk_logp))


class AsrModel:
    HOTWORD_SETS = 8        # graph sets kept on the device (least recently used dropped)

    def __init__(self, cfg: ModelConfig, state_dict, tokenizer, device="cuda", pos_cap: int = DEFAULT_POS_CAP,
                 pad_seconds: float = 0.5, precision: str = "bf16", pad_samples=None, qweights=None, resample: str = "host", token_scores: bool = False,
                 nbest: int = 0, rescore=None):
        """rescore: None (default), "likelihood" or "norm_likelihood": every n-best list is scored by full likelihood on the device
        right after the search (`rescore_step`: rs_rnnt_align_rows on the lists, one lattice per utterance with shared prefixes
        computed once) and the result is a `RescoredBatch`.  The two values differ in the key the packages re-rank by; the runtime
        keeps the search's order.  Needs a beam search and nbest >= 2 (ValueError otherwise, before anything is loaded).  May be
        changed later.
        nbest: 0 (default) = every search returns its one hypothesis; N >= 1 = the search also returns its N best hypotheses per
        utterance, ranked on the device (`DecodedBatch.nbest`; include/rs_asr.h rs_rnnt_mbs_nbest / rs_rnnt_beam_nbest state the
        ranking, rs_rnnt_alsd_nbest too).  Built for every beam search; N above the beam, or N > 1 with a
        greedy search, raises ValueError (`nbest_plan`).  May be changed later.
        token_scores: every decode is followed by `score` (rs_rnnt_token_scores, csrc/k_rnnt_scores.hip) on the same stream and
        `DecodedBatch.token_logprobs` is filled; off (default): nothing runs and nothing is allocated.  May be changed later.
        resample: where the packages' `norm_audio` work (resample to 16 kHz, average the channels) is done for input at another
        rate or with several channels: "host" (default) = scipy / soxr per utterance as before, "device" = `resample_batch`.
        precision: "bf16" = the throughput mode (bf16 GEMM operands, float32 accumulation and residual stream);
        "fp32" = the parity mode: float32 weights, activations and arithmetic end to end, what the reference computes
        (pkg/nemo-asr/src/transcribe.py:26-28, :48-53) — about 20x slower, 2.4 GB more weights."""
        cfg.validate()
        from .resample import check_mode
        self.resample = check_mode(resample)
        self.token_scores = bool(token_scores)
        self.cfg = cfg
        self.nbest = self.nbest_plan(nbest)     # (an impossible count is refused before anything is loaded)
        self.rescore = None
        self.rescore = self.rescore_plan(rescore)
        self._resample_tables = {}      # rate -> the plan's table on the device
        if precision not in ("bf16", "fp32", "fp32x3", "int8"):
            raise ValueError(f"precision must be 'bf16', 'fp32', 'fp32x3' or 'int8', not {precision!r}")
        # "int8" (the Zipformer family): onnxruntime's int8 graph restated — the float32 mode with every quantized Linear of
        # `qweights` ({icefall name: (Wq int8, sw, zw)}) as a dynamically quantized MatMul on the int8 matrix cores (csrc/k_int8.hip)
        self.i8 = precision == "int8"
        if self.i8 and (getattr(cfg, "family", "") != "k2" or not qweights):
            raise ValueError("precision 'int8' needs a Zipformer (k2) configuration and its quantized weights (qweights)")
        precision = "fp32" if self.i8 else precision
        # "fp32x3": the float32 mode (float32 weights, activations, accumulation, IEEE exp / divide) with every float32 PRODUCT of its
        # GEMMs formed from three bf16 matrix-core terms (csrc/k_f32.hip X3: hi / lo split, 16 mantissa bits per operand) — 2x the
        # float32 mode's speed; not an IEEE chain, but held to the same 256-row goldens (ids identical on every row of all three)
        self.x3 = precision == "fp32x3"
        precision = "fp32" if self.x3 else precision
        self.precision = precision
        if not torch.cuda.is_available():
            raise RuntimeError("reazonspeech_amd needs a ROCm GPU (MI355X / gfx950): torch.cuda.is_available() is "
                               "False and there is no CPU fallback for this path")
        self.cfg = cfg
        self.tokenizer = tokenizer
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"device {device!r}: only ROCm ('cuda[:N]') devices are supported")
        index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self.device = torch.device("cuda", index)
        self.pad_left = self.pad_right = int(pad_seconds * cfg.sample_rate)   # audio.py:80-82 via decode.py:4
        if pad_samples is not None:          # asymmetric padding in samples (espnet: PADDING = (16000, 8000), transcribe.py:10,69)
            self.pad_left, self.pad_right = int(pad_samples[0]), int(pad_samples[1])
        self._bufs = {}
        self._hw_sets = {}              # (graph keys) -> _HotwordSet
        self.hotwords = None            # the model's own HotwordGraph (nemo: load_model(hotwords=...)); None = no hotwords
        self.hotwords_score = 1.5
        self.ngram_lm = None            # the model's NgramLm (nemo, k2: load_model(ngram_lm_model=...)); None = no LM fusion
        self.ngram_lm_alpha = 0.0       # its weight in the search (ALSD, modified beam search); both may be set later
        self._lm_sets = {}              # NgramLm.key -> _NgramSet
        self._dec_lanes = []            # [(context, stream)] of the decode lanes beyond what was needed so far
        self._streams = None
        self._streams_prio = None
        self.pos_cap = 0
        with torch.cuda.device(self.device):
            self.ctx = capi.Context(cfg, index)
            if getattr(cfg, "family", "") == "k2":
                from .k2_weights import prepare_weights_k2
                self._k2_sd = state_dict          # the position tables are re-projected when a longer utterance arrives
                self._k2_q = qweights if self.i8 else None
                self._upload_k2(prepare_weights_k2(cfg, state_dict, pos_cap, f32=precision == "fp32", i8=self._k2_q))
                self.pos_cap = pos_cap
            elif cfg.espnet:
                from .weights_espnet import prepare_weights_espnet
                self._upload(prepare_weights_espnet(cfg, state_dict, pos_cap, f32=precision == "fp32"))
            else:
                self._upload(prepare_weights(cfg, state_dict, pos_cap, f32=precision == "fp32"))
            if precision == "fp32":
                self.ctx.set_option("precision_f32", 1)
                self.ctx.set_option("gemm_f32_x3", 1 if self.x3 else 0)
            if self.i8:
                self.ctx.set_option("precision_i8", 1)

    # ------------------------------------------------------------------------------------------
    def _upload(self, tensors):
        dev = {}
        for name, t in tensors.items():
            dev[name] = t.to(self.device, non_blocking=False).contiguous()
            self.ctx.set_tensor(name, dev[name])
        self._pos_w = [dev[f"L{i}.att.pos.w"] for i in range(self.cfg.n_layers)]
        self._set_pos_tables(dev["pos.table"], dev.get("pos.table.f32"))

    def _upload_k2(self, tensors):
        for name, t in tensors.items():
            dev = t.to(self.device, non_blocking=False).contiguous()
            for c in self._contexts():
                c.set_tensor(name, dev)
        for c in self._contexts():
            c.finalize()
            if self.precision == "fp32":
                c.set_option("precision_f32", 1)
                c.set_option("gemm_f32_x3", 1 if self.x3 else 0)
            if getattr(self, "i8", False):
                c.set_option("precision_i8", 1)

    def _contexts(self):
        return [self.ctx] + [c for c, _ in self._dec_lanes]

    def _set_pos_tables(self, table, table_f32=None):
        """register the relative-position table (bf16 [2*cap-1][d]) and the derived per-layer tensors: the table
        projected by every layer's linear_pos, computed once with the library's own GEMM (same kernel and row
        arithmetic as the per-call projection it replaces, so results are bit-identical) — 24 x [2*cap-1][d] bf16
        = 100 MB at cap 1024"""
        projs = []
        for i in range(self.cfg.n_layers):
            proj = torch.empty_like(table)
            self.ctx.gemm(table, self._pos_w[i], proj, flags=0)
            projs.append(proj)
        torch.cuda.synchronize(self.device)
        for c in self._contexts():
            c.set_tensor("pos.table", table)
            if table_f32 is not None:            # float32 parity mode: its layers project the rows they need per call
                c.set_tensor("pos.table.f32", table_f32)
            for i, proj in enumerate(projs):
                c.set_tensor(f"L{i}.att.pos_proj", proj)
            c.finalize()
            if self.precision == "fp32":         # (rs_finalize ran again: the option survives, set it anyway for new contexts)
                c.set_option("precision_f32", 1)
                c.set_option("gemm_f32_x3", 1 if self.x3 else 0)
        self.pos_cap = (table.shape[0] + 1) // 2

    def ensure_pos_cap(self, tp: int):
        """Long-form audio: the reference hands a whole file to the model as ONE utterance
        (pkg/nemo-asr/src/transcribe.py:44-53), so T' is unbounded.  The resident position tables cover T' up to
        `pos_cap`; a longer utterance grows them (next power of two) instead of failing."""
        if getattr(self.cfg, "family", "") == "k2":
            # the 50 Hz stack of a Zipformer has twice the output frames (+ 1): its position tables must cover that
            need = 2 * int(tp) + 2
            if need <= self.pos_cap:
                return
            from .k2_weights import prepare_weights_k2
            cap = 1 << (need - 1).bit_length()
            torch.cuda.synchronize(self.device)
            with torch.cuda.device(self.device):
                tensors = prepare_weights_k2(self.cfg, self._k2_sd, cap, i8=self._k2_q)
                self._upload_k2({k: v for k, v in tensors.items() if k.endswith("attw.pos_proj") or k == "pos.enc"})
            self.pos_cap = cap
            return
        if tp <= self.pos_cap:
            return
        from .weights import rel_pos_table
        cap = 1 << (int(tp) - 1).bit_length()
        torch.cuda.synchronize(self.device)          # nothing may still read the tables being replaced
        with torch.cuda.device(self.device):
            host = torch.from_numpy(rel_pos_table(self.cfg, cap))
            table = host.to(torch.bfloat16).to(self.device).contiguous()
            self._set_pos_tables(table, host.to(self.device).contiguous() if self.precision == "fp32" else None)

    BUCKET = 16000      # cached buffer sets are sized in whole seconds of audio

    def _decode_policy(self, ctx, B, pipelined, lanes=1):
        """Pick the decode kernel family for a call (all are bit-identical; tests/test_gpu_fullsize.py).  Measured on
        MI355X (profiles/r02o_pipeline_decode_variants_ab.txt, r02q_small_batch_decode_ab.txt, r02zz_decode_family_ab.txt):
          * ONE decode stream next to the encoder is on the critical path: what a step costs there is the number of
            launches and of workgroups that must find free CUs, not the length of each kernel on an idle chip: at
            B = 256 the wide-tile kernels with the exact joint (5 launches, 40-workgroup LSTM) give 65.5 ms per step,
            screened / narrow 66.5-68.5;
          * TWO decode lanes have an encoder period of slack each: then the family with the least exact-f32 work wins,
            because its CU time is what the GEMMs lose (screened joint + narrow tiles 59.0 ms, wide / exact 60.0);
          * small batches are decode-bound: narrow tiles + exact joint win (B = 32: 19.6 ms vs 25.8 wide, 22.6 screened);
          * big batches on an otherwise idle chip (sequential schedule): screened joint + narrow tiles (79.9 vs 84.7 ms).
        $RS_DECODE_SCREEN / $RS_DECODE_NARROW override (A/B runs)."""
        if "RS_DECODE_SCREEN" in os.environ or "RS_DECODE_NARROW" in os.environ:
            return
        if self is not None and self.cfg.decoding == "alsd" and B * self.cfg.beam_size >= 256:
            # ALSD runs the LSTM over the hundreds of hypothesis rows that took a label (about half of B x beam per alignment
            # step): that is throughput work, and the wide tiles re-read the weights a quarter as often as the narrow ones —
            # 133 vs 160 ms per step at B = 256, beam 4 (profiles/r05f_alsd_narrow_ab.txt); results are bit-identical
            ctx.set_option("decode_narrow", 0)
            ctx.set_option("decode_screen", 0)
            return
        if self is not None and self.cfg.decoding == "beam":          # (the screened joint serves the greedy searches only)
            ctx.set_option("decode_screen", 0)
            ctx.set_option("decode_narrow", 0 if (pipelined and lanes == 1 and B >= 128) else 1)
            return
        big = B >= 128
        critical = pipelined and lanes == 1
        ctx.set_option("decode_narrow", 0 if (critical and big) else 1)
        ctx.set_option("decode_screen", 1 if (big and not critical) else 0)

    def buffers(self, B, l_max) -> _Buffers:
        """a cached buffer set for B utterances of up to l_max samples.  Lengths are bucketed to whole seconds and a
        larger cached set of the same B is reused: the kernels mask by per-utterance length, so the result does not
        depend on the padded extent (tests: batch invariance), and consecutive transcribe() calls on clips of
        different lengths stop re-allocating pinned staging + workspace every time."""
        l_max = (max(int(l_max), 1) + self.BUCKET - 1) // self.BUCKET * self.BUCKET
        # any cached set that is long enough will do: `stage` narrows it to the batch at hand (`_Buffers.narrow`), so a
        # longer set costs nothing per call and a folder of files of mixed lengths settles on ONE set instead of cycling
        # through the four cached geometries (per-call latency by length: profiles/r03x_varied_lengths_latency_reuse.txt —
        # it follows frames + emitted tokens, e.g. 7.8 ms for 2.2 s, 10 ms for 5 s, 29 ms for 29 s of noise)
        fits = [k for k in self._bufs if k[0] == B and l_max <= k[1]]
        if fits:
            key = min(fits, key=lambda k: k[1])
            self._bufs[key] = self._bufs.pop(key)          # most recently used last
            return self._bufs[key]
        key = (B, l_max)
        if len(self._bufs) >= 4:           # keep HBM bounded: drop the least recently used geometry
            self._bufs.pop(next(iter(self._bufs)))
        with torch.cuda.device(self.device):
            self._bufs[key] = _Buffers(self, B, l_max)
        return self._bufs[key]

    @property
    def n_params(self):
        return self.cfg.n_params()

    # ------------------------------------------------------------------------------------------
    def run_device(self, buf: _Buffers, want_enc: Optional[torch.Tensor] = None):
        """front-end -> encoder -> greedy decode on data already in `buf.audio`/`buf.lens` (HBM).
        Outputs land in buf.ids / buf.frames / buf.n_ids.  rs_rnnt_greedy synchronises the stream."""
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream().cuda_stream
            self._decode_policy(self.ctx, buf.B, pipelined=False)
            self.ctx.frontend(buf.audio, buf.lens, self.pad_left, self.pad_right, buf.t_max, buf.feats,
                              buf.n_frames, buf.ws, stream)
            self.ctx.encoder(buf.feats, buf.n_frames, buf.B, buf.t_max, want_enc, buf.joint_enc, buf.enc_lens,
                             buf.ws, stream)
            self.decode(self.ctx, buf, buf.ws, stream)
            self.score(self.ctx, buf, stream)
            self.rescore_step(self.ctx, buf, stream)

    SCORE_CHUNK_ROWS = 4096     # (b, u) rows whose logits `score` asks room for at once (60 MB at V + 1 = 3001); fewer rows, more chunks, same bits

    def score(self, ctx, buf, stream, decoding=None):
        """with `token_scores` on: log-probability of every id the search just wrote, under the model's own distribution, into
        the buffer set's `score_bufs` (own workspace, allocated on first use like `ws_alsd`; `collect` reads it).  `decoding`: the
        search that ran when it was overridden for the call.  Synchronises the stream."""
        if not self.token_scores:
            return
        cfg = self.cfg
        B, u_cap = buf.B, buf.ids.shape[1]
        rows = min(self.SCORE_CHUNK_ROWS, B * u_cap)
        hidden = getattr(cfg, "decoder_dim", None) or cfg.pred_hidden          # (the Zipformer family's decoder rows are per chunk too)
        per_row = 4 * (2 * cfg.joint_hidden + (cfg.n_logits + 63) // 64 * 64 + 2 * hidden + 8)
        need = ctx.token_scores_workspace_bytes(B, u_cap) + (rows + 31) // 32 * 32 * per_row
        sb = buf.score_bufs
        if sb is None or sb[0].numel() < need or sb[1].numel() < B * u_cap:
            dev = self.device
            sb = (torch.empty((need,), dtype=torch.uint8, device=dev), torch.empty((B * u_cap,), dtype=torch.float32, device=dev),
                  torch.empty((B * u_cap,), dtype=torch.int32, device=dev))
            buf.score_bufs = sb
        logp, top1 = sb[1][:B * u_cap].view(B, u_cap), sb[2][:B * u_cap].view(B, u_cap)
        ctx.rnnt_token_scores(buf.joint_enc, buf.enc_lens, B, buf.tp_max, buf.ids, buf.frames, buf.n_ids, logp, top1, sb[0], stream,
                              frames_are_steps=(decoding or cfg.decoding) == "alsd")

    RESCORE_KEYS = ("likelihood", "norm_likelihood")

    def rescore_plan(self, rescore=None, nbest=None, decoding=None):
        """`rescore`: None = the model's own (`self.rescore`) -> None (off) or the key; ValueError with the reason for a value that is
        no key, a greedy search, or fewer than two entries per list (`nbest`: as `nbest_plan` takes it)."""
        r = getattr(self, "rescore", None) if rescore is None else rescore
        if r is None or r is False:
            return None
        if r not in self.RESCORE_KEYS:
            raise ValueError(f"rescore must be None, 'likelihood' or 'norm_likelihood', not {r!r}")
        if self.nbest_plan(nbest, decoding) < 2:
            raise ValueError(f"rescore={r!r} re-ranks an n-best list: it needs a beam search and nbest >= 2")
        return r

    def rescore_step(self, ctx, buf, stream, decoding=None, single=False):
        """with `rescore` on, after `decode` and `score` on the same stream: log P(text | audio) and the best alignment of EVERY
        entry of the n-best lists the search just left in `nbest_bufs`, viewed as [B x n][u_cap] text rows with row b n + k scored
        against utterance b (k < n_hyps[b], else skipped) while joint_enc is still resident — one rs_rnnt_align_rows call, the
        entries of a list sharing the lattice cells of their common prefixes (a batch whose rows x tp_max x (u_cap + 1) is beyond
        one call's bound takes several calls over runs of utterances, on the same joint_enc; ValueError only when the lists of ONE
        utterance are beyond it, or the label capacity is above `capi.ALIGN_U_CAP_MAX`).  With `token_scores` on, rs_rnnt_token_scores_rows
        on the same rows too.  Outputs stay in the buffer set's `rescore_bufs` (allocated on first use); `collect` reads them.
        `single`: a decode that ran WITHOUT lists (the espnet greedy fall-back) is scored as lists of one: buf.ids / n_ids, row b
        against utterance b.  Synchronises the stream."""
        buf.rescored_n = 0
        n = getattr(buf, "nbest_n", 0)
        if not self.rescore or not (n or single):
            return
        cfg = self.cfg
        if n:
            nb = buf.nbest_bufs
        else:
            n = 1
            nb = dict(ids=buf.ids[:, None], frames=buf.frames[:, None], n_ids=buf.n_ids[:buf.B, None],
                      n_hyps=torch.ones((buf.B,), dtype=torch.int32, device=self.device))
        B, u_cap = buf.B, nb["ids"].shape[2]
        R = B * n
        per = min(self.ALIGN_MAX_CELLS // (n * buf.tp_max * (u_cap + 1)), B)       # utterances whose lists one call takes
        if u_cap > capi.ALIGN_U_CAP_MAX or per < 1:
            raise ValueError(f"rescore: the {n} hypotheses of one utterance x {buf.tp_max} frames x {u_cap} labels are more than one call "
                             f"scores (at most {capi.ALIGN_U_CAP_MAX} labels and {self.ALIGN_MAX_CELLS} lattice cells: window the audio)")
        Rc = per * n
        decoding = decoding or cfg.decoding
        one = bool(cfg.max_symbols == 1 and decoding == "modified_beam_search")     # the topology the search moved in
        hidden = getattr(cfg, "decoder_dim", None) or cfg.pred_hidden
        per_row = 4 * (2 * cfg.joint_hidden + (cfg.n_logits + 63) // 64 * 64 + 2 * hidden + 16)
        chunk = (min(self.ALIGN_CHUNK_ROWS, Rc * buf.tp_max * (u_cap + 1)) + 31) // 32 * 32
        need = ctx.align_rows_workspace_bytes(B, Rc, buf.tp_max, u_cap) + chunk * per_row
        if self.token_scores:
            rows = (min(self.SCORE_CHUNK_ROWS, R * u_cap) + 31) // 32 * 32
            need = max(need, ctx.token_scores_rows_workspace_bytes(B, R, u_cap) + rows * per_row)
        rb = buf.rescore_bufs
        if rb is None or rb["ws"].numel() < need or tuple(rb["frames"].shape) != (R, u_cap):
            dev, i32, f32 = self.device, torch.int32, torch.float32
            rb = dict(ws=torch.empty((need,), dtype=torch.uint8, device=dev), row_utt=torch.empty((R,), dtype=i32, device=dev),
                      loglik=torch.empty((R,), dtype=f32, device=dev), best=torch.empty((R,), dtype=f32, device=dev),
                      frames=torch.empty((R, u_cap), dtype=i32, device=dev), logp=torch.empty((R, u_cap), dtype=f32, device=dev),
                      token_logp=torch.empty((R, u_cap), dtype=f32, device=dev))
            buf.rescore_bufs = rb
        with torch.cuda.stream(torch.cuda.ExternalStream(stream, device=self.device)):
            k = torch.arange(n, dtype=torch.int32, device=self.device)[None, :]
            b = torch.arange(B, dtype=torch.int32, device=self.device)[:, None]
            rb["row_utt"].copy_(torch.where(k < nb["n_hyps"][:B, None], b, -1).reshape(R))
        ids, n_ids = nb["ids"].reshape(R, u_cap), nb["n_ids"].reshape(R)
        done = [0, 0]
        for r0 in range(0, R, Rc):                           # (row_utt keeps naming the utterances of the whole batch)
            r1 = min(r0 + Rc, R)
            st = ctx.rnnt_align_rows(buf.joint_enc, buf.enc_lens, B, buf.tp_max, rb["row_utt"][r0:r1], ids[r0:r1], n_ids[r0:r1],
                                     rb["loglik"][r0:r1], rb["best"][r0:r1], rb["frames"][r0:r1], rb["logp"][r0:r1], rb["ws"], stream,
                                     one_per_frame=one)
            done = [done[0] + st[0], done[1] + st[1]]
        rb["stats"] = (done[0], done[1])
        if self.token_scores:
            ctx.rnnt_token_scores_rows(buf.joint_enc, buf.enc_lens, B, buf.tp_max, rb["row_utt"], ids, nb["frames"].reshape(R, u_cap), n_ids,
                                       rb["token_logp"], None, rb["ws"], stream, frames_are_steps=decoding == "alsd")
        buf.rescored_n = n

    RESCORE_HOST = ("loglik", "best", "token_logp")

    def rescored_lists(self, rs, nb, B, n):
        """host copies of `rescore_bufs` and `nbest_bufs` -> per utterance [(log_likelihood, alignment_log_prob, token_logprobs or
        None)], entry k for entry k of the list"""
        out = []
        for b in range(B):
            rows = []
            for k in range(int(nb["n_hyps"][b])):
                r, m = b * n + k, int(nb["n_ids"][b, k])
                rows.append((float(rs["loglik"][r]), float(rs["best"][r]), rs["token_logp"][r, :m].tolist() if self.token_scores else None))
            out.append(rows)
        return out

    def score_view(self, buf):
        """the [B][u_cap] log-probabilities `score` left for this batch (None with `token_scores` off)"""
        if not self.token_scores or buf.score_bufs is None:
            return None
        B, u_cap = buf.B, buf.ids.shape[1]
        return buf.score_bufs[1][:B * u_cap].view(B, u_cap)

    def _search_ws(self, buf, n):
        """the buffer set's workspace of the beam searches, grown to `n` bytes"""
        if buf.ws_alsd is None or buf.ws_alsd.numel() < n:       # (a narrowed view may have sized it for a shorter batch)
            buf.ws_alsd = torch.empty((n,), dtype=torch.uint8, device=self.device)
        return buf.ws_alsd

    def nbest_plan(self, nbest=None, decoding=None):
        """`nbest`: None = the model's own (`self.nbest`), or the entries per utterance for this call -> the count the search is run
        with, 0 = the one hypothesis as ever.  ValueError with the reason for a count the model's search cannot give."""
        n = getattr(self, "nbest", 0) if nbest is None else nbest
        if n is None or (isinstance(n, int) and not isinstance(n, bool) and n == 0):
            return 0
        if not (isinstance(n, int) and not isinstance(n, bool) and 1 <= n <= 8):
            raise ValueError(f"nbest must be an integer in 1..8, not {n!r}")
        decoding = decoding or self.cfg.decoding
        if decoding not in ("alsd", "beam", "modified_beam_search"):
            if n > 1:
                raise ValueError(f"nbest={n} needs a beam search: the greedy search ({decoding!r}) keeps one hypothesis")
            return 0
        if n > self.cfg.beam_size:
            raise ValueError(f"nbest={n} is above the beam ({self.cfg.beam_size}): the search keeps no more hypotheses than that")
        return n

    def _nbest_bufs(self, buf, n):
        """the buffer set's n-best outputs for `n` entries per utterance at the batch's label capacity, allocated on first use"""
        B, u_cap = buf.B, buf.ids.shape[1]
        nb = buf.nbest_bufs
        if nb is None or tuple(nb["ids"].shape) != (B, n, u_cap):
            dev, i32, f32 = self.device, torch.int32, torch.float32
            nb = dict(ids=torch.zeros((B, n, u_cap), dtype=i32, device=dev), frames=torch.zeros((B, n, u_cap), dtype=i32, device=dev),
                      n_ids=torch.zeros((B, n), dtype=i32, device=dev), scores=torch.zeros((B, n), dtype=f32, device=dev),
                      norm_scores=torch.zeros((B, n), dtype=f32, device=dev), n_hyps=torch.zeros((B,), dtype=i32, device=dev))
            buf.nbest_bufs = nb
        return nb

    def _nbest_head(self, buf, nb, stream):
        """entry 0 of every list into buf.ids / frames / n_ids / scores, on `stream`: the search's one result, where `score`,
        `collect` and the pipeline's copies read it"""
        with torch.cuda.stream(torch.cuda.ExternalStream(stream, device=self.device)):
            buf.ids.copy_(nb["ids"][:, 0]); buf.frames.copy_(nb["frames"][:, 0])
            buf.n_ids.copy_(nb["n_ids"][:, 0]); buf.scores.copy_(nb["scores"][:, 0])

    def decode(self, ctx, buf: _Buffers, ws, stream, max_pops=None, decoding=None, nbest=None):
        """stage 3 on `stream`: the checkpoint's decoding strategy (cfg.decoding).  Greedy fills buf.ids / buf.frames
        (emission frames); ALSD fills buf.ids / buf.frames (alignment steps i = frame + labels before) / buf.scores; the
        modified beam search of the Zipformer family fills buf.ids / buf.frames (frames) / buf.scores.  All synchronise the stream.
        `nbest`: entries per utterance of the ranked list the search also leaves in the buffer set's `nbest_bufs` (`collect` reads
        them into `DecodedBatch.nbest`); None = what the batch was staged with (`buf.want_nbest`), 0 = none.  Entry 0 is copied into
        buf.ids / frames / n_ids / scores, so everything after the search reads what it reads without lists."""
        cfg = self.cfg
        n_best = self.nbest_plan(nbest, decoding) if nbest is not None else getattr(buf, "want_nbest", 0)
        buf.nbest_n = 0
        if max_pops is not None or decoding is not None:     # per-call overrides (the caller's retry policy): never written into self.cfg
            cfg = cfg.with_(**({"beam_max_pops": int(max_pops)} if max_pops is not None else {}), **({"decoding": decoding} if decoding is not None else {}))
        hw = getattr(buf, "hw_set", None)                  # the batch has at least one graph; graph_of goes with a hotword set only
        hot = dict(hotwords=hw.struct, graph_of=buf.graph_of) if hw is not None else {}
        lm = getattr(buf, "lm", None)                      # with an n-gram LM and / or graphs in the batch: the LM / HW forms of the search
        fused = dict(lm=lm[0].struct, lm_alpha=lm[1]) if lm is not None else {}
        if cfg.decoding == "beam" and n_best:             # ... with upstream's sort_nbest(kept_hyps)[:nbest] (rs_rnnt_beam_nbest: the same kernels)
            nb = self._nbest_bufs(buf, n_best)
            sws = self._search_ws(buf, ctx.beam_workspace_bytes(buf.B, cfg.beam_size, buf.tp_max, cfg.beam_max_pops, hotwords=hw is not None,
                                                                lm=lm is not None, nbest=n_best))
            ctx.rnnt_beam_nbest(buf.joint_enc, buf.enc_lens, buf.B, buf.tp_max, cfg.beam_size, cfg.beam_score_norm, cfg.beam_max_pops, n_best,
                                nb["ids"], nb["n_ids"], nb["scores"], nb["norm_scores"], nb["n_hyps"], buf.pops, sws, stream, frames=nb["frames"],
                                **hot, **fused)
            self._nbest_head(buf, nb, stream)
            buf.nbest_n = n_best
        elif cfg.decoding == "beam":
            sws = self._search_ws(buf, ctx.beam_workspace_bytes(buf.B, cfg.beam_size, buf.tp_max, cfg.beam_max_pops, hotwords=hw is not None,
                                                                lm=lm is not None))
            ctx.rnnt_beam(buf.joint_enc, buf.enc_lens, buf.B, buf.tp_max, cfg.beam_size, cfg.beam_score_norm, cfg.beam_max_pops,
                          buf.ids, buf.n_ids, buf.scores, buf.pops, sws, stream, frames=buf.frames, **hot, **fused)
        elif cfg.decoding == "modified_beam_search" and n_best:      # ... with its ranked list (rs_rnnt_mbs_nbest: the same kernels)
            nb = self._nbest_bufs(buf, n_best)
            sws = self._search_ws(buf, ctx.mbs_nbest_workspace_bytes(buf.B, cfg.beam_size, buf.tp_max, buf.ids.shape[1], n_best))
            ctx.rnnt_mbs_nbest(buf.joint_enc, buf.enc_lens, buf.B, buf.tp_max, cfg.beam_size, cfg.blank_penalty, cfg.mbs_length_norm, n_best,
                               nb["ids"], nb["frames"], nb["n_ids"], nb["scores"], nb["norm_scores"], nb["n_hyps"], sws, stream, **hot, **fused)
            self._nbest_head(buf, nb, stream)
            buf.nbest_n = n_best
        elif cfg.decoding == "modified_beam_search":      # Zipformer family: sherpa-onnx's second method (csrc/k_rnnt_mbs.hip)
            sws = self._search_ws(buf, ctx.mbs_workspace_bytes(buf.B, cfg.beam_size, buf.tp_max, buf.ids.shape[1], hotwords=hw is not None,
                                                               lm=lm is not None))
            ctx.rnnt_mbs(buf.joint_enc, buf.enc_lens, buf.B, buf.tp_max, cfg.beam_size, cfg.blank_penalty, cfg.mbs_length_norm,
                         buf.ids, buf.frames, buf.n_ids, buf.scores, sws, stream, **hot, **fused)
        elif cfg.decoding == "alsd" and n_best:           # ... with the ranked list of finished hypotheses (rs_rnnt_alsd_nbest: the same kernels)
            nb = self._nbest_bufs(buf, n_best)
            sws = self._search_ws(buf, ctx.alsd_nbest_workspace_bytes(buf.B, cfg.beam_size, buf.tp_max, cfg.alsd_max_target_len, n_best))
            ctx.rnnt_alsd_nbest(buf.joint_enc, buf.enc_lens, buf.B, buf.tp_max, cfg.beam_size, cfg.alsd_max_target_len, cfg.beam_score_norm,
                                False, n_best, nb["ids"], nb["frames"], nb["n_ids"], nb["scores"], nb["norm_scores"], nb["n_hyps"], sws, stream,
                                **hot, **fused)
            self._nbest_head(buf, nb, stream)
            buf.nbest_n = n_best
        elif cfg.decoding == "alsd":
            sws = self._search_ws(buf, ctx.alsd_workspace_bytes(buf.B, cfg.beam_size, buf.tp_max, cfg.alsd_max_target_len,
                                                                hotwords=hw is not None, lm=lm is not None))
            ctx.rnnt_alsd(buf.joint_enc, buf.enc_lens, buf.B, buf.tp_max, cfg.beam_size, cfg.alsd_max_target_len, cfg.beam_score_norm,
                          False, buf.ids, buf.frames, buf.n_ids, buf.scores, sws, stream, **hot, **fused)
        else:
            ctx.rnnt_greedy(buf.joint_enc, buf.enc_lens, buf.B, buf.tp_max, buf.u_max, buf.ids, buf.frames, buf.n_ids,
                            ws, stream)

    # ------------------------------------------------------------------------------------------
    def run_encoder(self, buf: _Buffers, stream, ctx=None):
        """front-end + encoder of one batch on `stream` (asynchronous)"""
        ctx = ctx or self.ctx
        ctx.frontend(buf.audio, buf.lens, self.pad_left, self.pad_right, buf.t_max, buf.feats, buf.n_frames,
                     buf.ws, stream)
        ctx.encoder(buf.feats, buf.n_frames, buf.B, buf.t_max, None, buf.joint_enc, buf.enc_lens, buf.ws, stream)

    def run_pipelined(self, bufs: Sequence[_Buffers], steps: int, after_decode=None, from_host: bool = False,
                      dec_streams: int = 1, before_encoder=None, fill=None, enc_streams: Optional[int] = None):
        """Process `steps` batches as a pipeline with up to len(bufs) batches in flight: the throughput-bound front-end +
        encoder of batch i+1 (i+2) runs on one HIP stream while the latency-bound decode of batch i (and i+1) — a
        dependency chain of small launches that leaves most CUs idle — runs on one (two) more streams, each driven by a
        worker thread (ctypes releases the GIL; the decode entry points synchronise only their own stream).  Every batch
        is fully decoded when this returns.

        bufs            resident buffer sets; step i uses bufs[i % len(bufs)] (or what `fill` returned for it) and waits
                        for that set's previous decode.  n decode lanes (`dec_streams`; batch i goes to lane i mod n)
                        need at least n + 1 sets.
        after_decode    `after_decode(buf)` on the decode worker right after batch `buf.step` is decoded (and, with
                        `from_host`, its hypotheses are in `buf.h_out` on the host).  Hooks run in batch order whichever
                        lane finishes first (a hook may issue a collective: every rank has to issue them in the same
                        order, from one thread at a time).
        from_host       every batch is first copied from its pinned host buffer (H2D on the encoder stream) and its
                        hypotheses are copied back after decode: the host-to-host boundary of SURVEY.md §8(d).
        fill            `fill(i, buf) -> buf or a narrowed view of it`: a stager thread calls it for step i as soon as the
                        buffer set's previous use is over, to put batch i into the pinned staging buffers (implies
                        `from_host`) while the GPU works on the batches before it; the encoder of step i waits for it.
        before_encoder  `before_encoder(i)` on the caller's thread right before batch i's encoder is enqueued.
        enc_streams     encoder lanes: consecutive batches' front-end + encoder alternate between that many HIP streams (each
                        batch has its own workspace in its buffer set); needs dec_streams + enc_streams buffer sets.  None:
                        `encoder_lanes()` = ONE lane ($RS_ENC_STREAMS overrides) — two lanes were measured slower at B = 256
                        (profiles/r04f_ab_RS_ENC_STREAMS.txt) AND at B = 32 / 64 / 128, whose launches leave a third to half of
                        the CUs idle (profiles/r06_11_small_batch_enc_lanes_ab.txt).
                        (Also measured and dropped in round 6: the LAST batch's greedy decode split by rows over the decode
                        lanes to shorten the drain — 55.15 vs 55.45 ms per step over 20 steps, no gain.)"""
        nb = len(bufs)
        if enc_streams is None:
            enc_streams = self.encoder_lanes(bufs[0].B, nb, dec_streams)
        assert enc_streams >= 1 and (enc_streams == 1 or nb >= dec_streams + enc_streams), "n encoder lanes + m decode lanes need n + m buffer sets"
        assert nb >= 2 or steps <= 1, "the pipeline needs two buffer sets"
        assert dec_streams >= 1 and (dec_streams == 1 or nb >= dec_streams + 1), "n decode streams need n + 1 buffer sets"
        from_host = from_host or fill is not None
        with torch.cuda.device(self.device):
            # the decode chain of ONE stream is latency-critical (its workgroups should take the first free slots: high
            # priority); with several decode lanes each has whole extra encoder periods of slack and normal priority
            # leaves the GEMM rounds alone (profiles/r02w_bench_ab.txt)
            dec_prio = int(os.environ.get("RS_DECODE_PRIORITY", "0" if dec_streams >= 2 else "-1"))
            if self._streams is None or self._streams_prio != dec_prio:
                enc = self._streams[0] if self._streams is not None else torch.cuda.Stream(device=self.device)
                self._streams = (enc,)
                self._streams_prio = dec_prio
                self._dec_lanes = [(c, None) for c, _ in self._dec_lanes]       # keep the contexts, remake the streams
            while len(self._streams) < enc_streams:
                self._streams = self._streams + (torch.cuda.Stream(device=self.device),)
            enc_lanes = self._streams[:enc_streams]
            dec_cus = int(os.environ.get("RS_DECODE_CUS", "0"))
            while len(self._dec_lanes) < dec_streams:
                self._dec_lanes.append((self.ctx.clone(), None))
            dec_lanes = []
            for k in range(dec_streams):
                ctx_d, st = self._dec_lanes[k]
                if st is None:
                    if dec_cus > 0:
                        # decode confined to a slice of the chip (A/B knob): raw HIP stream with a CU mask
                        raw = capi.create_stream(self.device.index, dec_cus, self.ctx.n_cus(), dec_prio)
                        st = torch.cuda.ExternalStream(raw, device=self.device)
                    else:
                        st = torch.cuda.Stream(device=self.device, priority=dec_prio)
                    self._dec_lanes[k] = (ctx_d, st)
                self._decode_policy(ctx_d, bufs[0].B, pipelined=True, lanes=dec_streams)
                dec_lanes.append((ctx_d, st))
            for es in enc_lanes:
                es.wait_stream(torch.cuda.current_stream())
            queues = [queue.Queue() for _ in dec_lanes]
            done = [threading.Event() for _ in range(steps)]
            hooked = [threading.Event() for _ in range(steps)]
            staged = [threading.Event() for _ in range(steps)]
            views = [None] * steps
            errors = []
            stop = threading.Event()

            def worker(lane):
                ctx_d, stream = dec_lanes[lane]
                jobs = queues[lane]
                with torch.cuda.device(self.device):
                    while True:
                        item = jobs.get()
                        if item is None:
                            return
                        i, buf, ev = item
                        try:
                            stream.wait_event(ev)
                            # decode scratch lives past the encoder's scratch in buf.ws_dec
                            self.decode(ctx_d, buf, buf.ws_dec, stream.cuda_stream)
                            self.score(ctx_d, buf, stream.cuda_stream)
                            self.rescore_step(ctx_d, buf, stream.cuda_stream)
                            if from_host:
                                with torch.cuda.stream(stream):
                                    buf.h_out = (buf.n_ids.cpu(), buf.ids.cpu(), buf.frames.cpu(), buf.enc_lens.cpu(),
                                                 buf.scores.cpu() if self.cfg.has_scores else None)
                                    if self.token_scores:
                                        buf.h_out = buf.h_out + (self.score_view(buf).cpu(),)
                                    buf.h_nbest = {k: t.cpu() for k, t in buf.nbest_bufs.items()} if buf.nbest_n else None
                                    buf.h_rescore = {k: buf.rescore_bufs[k].cpu() for k in self.RESCORE_HOST} if buf.rescored_n else None
                            if after_decode is not None:
                                if i > 0:
                                    hooked[i - 1].wait()
                                after_decode(buf)
                        except Exception as e:          # surfaced on the caller's thread below
                            errors.append(e)
                        finally:
                            hooked[i].set()
                            done[i].set()

            def stager():
                # host side of the pipeline: batch i goes into its pinned staging buffers as soon as the buffer set is
                # free again (its previous batch decoded, hence its H2D long finished)
                for i in range(steps):
                    try:
                        while i >= nb and not done[i - nb].wait(0.05):
                            if stop.is_set():
                                return
                        if errors or stop.is_set():
                            return
                        views[i] = fill(i, bufs[i % nb])
                    except Exception as e:
                        errors.append(e)
                    finally:
                        staged[i].set()

            threads = [threading.Thread(target=worker, args=(k,), daemon=True) for k in range(len(dec_lanes))]
            if fill is not None:
                threads.append(threading.Thread(target=stager, daemon=True))
            for th in threads:
                th.start()
            # whatever happens while batches are being enqueued (an RsError from the encoder, an allocation failure, an exception
            # of the caller's before_encoder hook), the workers and the stager are always released and joined before it propagates
            try:
                for i in range(steps):
                    if fill is not None:
                        staged[i].wait()
                        if errors:
                            break
                        buf = views[i]
                    else:
                        buf = bufs[i % nb]
                        if i >= nb:
                            done[i - nb].wait()           # this buffer set's previous decode must be finished
                    buf.step = i
                    if before_encoder is not None:
                        before_encoder(i)
                    enc_stream = enc_lanes[i % len(enc_lanes)]
                    if from_host:
                        with torch.cuda.stream(enc_stream):          # only the columns this batch's geometry reads
                            w = buf.l_max
                            buf.audio[:, :w].copy_(buf.h_audio[:, :w], non_blocking=True)
                            buf.lens.copy_(buf.h_lens, non_blocking=True)
                            if getattr(buf, "hw_set", None) is not None:
                                buf.graph_of.copy_(buf.h_graph_of, non_blocking=True)
                    self.run_encoder(buf, enc_stream.cuda_stream)
                    ev = torch.cuda.Event()
                    ev.record(enc_stream)
                    queues[i % len(queues)].put((i, buf, ev))          # batch i goes to decode lane i mod lanes
            finally:
                stop.set()              # releases the stager
                for q in queues:
                    q.put(None)
                for th in threads:
                    th.join()
            for es in enc_lanes:
                torch.cuda.current_stream().wait_stream(es)
            for _, ds in dec_lanes:
                torch.cuda.current_stream().wait_stream(ds)
            if errors:
                raise errors[0]

    def encoder_lanes(self, B: int, n_sets: int, dec_streams: int) -> int:
        """encoder lanes `run_pipelined` uses for batches of B utterances when the caller does not say ($RS_ENC_STREAMS overrides)"""
        e = os.environ.get("RS_ENC_STREAMS")
        want = int(e) if e else 1
        return max(1, min(want, n_sets - dec_streams))

    def new_buffers(self, B, l_max) -> _Buffers:
        """an un-cached buffer set (the pipelined path keeps two batches in flight)"""
        with torch.cuda.device(self.device):
            return _Buffers(self, B, (max(int(l_max), 1) + 63) // 64 * 64)

    # ---- hotwords (Zipformer family: modified beam search; NeMo family: ALSD) ---------------------------------------------------
    def hotword_set(self, graphs):
        """the device table of a tuple of distinct HotwordGraph: built, checked (rs_hotwords_check) and uploaded once, then
        found again by content"""
        key = tuple(g.key for g in graphs)
        hs = self._hw_sets.pop(key, None)
        if hs is None:
            if len(self._hw_sets) >= self.HOTWORD_SETS:
                self._hw_sets.pop(next(iter(self._hw_sets)))
            with torch.cuda.device(self.device):
                hs = _HotwordSet(graphs, self.device)
        self._hw_sets[key] = hs                           # most recently used last
        return hs

    # ---- n-gram LM (ALSD, modified beam search) -----------------------------------------------------------------------------------------
    def ngram_set(self, lm):
        """the device table of an NgramLm: checked (rs_ngram_check) and uploaded once, then found again by content"""
        ns = self._lm_sets.pop(lm.key, None)
        if ns is None:
            if len(self._lm_sets) >= 2:
                self._lm_sets.pop(next(iter(self._lm_sets)))
            with torch.cuda.device(self.device):
                ns = _NgramSet(lm, self.device)
        self._lm_sets[lm.key] = ns
        return ns

    def lm_plan(self, ngram_lm=None):
        """`ngram_lm`: None = the model's own (`self.ngram_lm`, `self.ngram_lm_alpha`), or (NgramLm or None, alpha) for this call
        -> (device table, alpha), or None when the call runs without an LM (no model, or alpha 0)"""
        lm, alpha = (self.ngram_lm, self.ngram_lm_alpha) if ngram_lm is None else ngram_lm
        if lm is None or not alpha:
            return None
        if not (np.isfinite(alpha) and alpha > 0):
            raise ValueError(f"ngram_lm_alpha must be a finite number >= 0, not {alpha!r}")
        if self.cfg.decoding not in fusion.FUSED:          # (the packages refuse their greedy searches first, in their own words)
            raise ValueError(fusion.rule_of(self.cfg).plan_lm_refusal.format(repr(self.cfg.decoding)))
        return self.ngram_set(lm), float(alpha)

    def graph_plan(self, hotwords, n):
        """`hotwords`: None, or one HotwordGraph / None per utterance -> (device set, [graph index per utterance, -1 = none]) or None"""
        if hotwords is None:
            return None
        if len(hotwords) != n:
            raise ValueError(f"hotwords: {len(hotwords)} entries for {n} utterances")
        if all(g is None for g in hotwords):
            return None
        if self.cfg.decoding not in fusion.FUSED:          # greedy has no hypotheses to bias
            raise ValueError(fusion.rule_of(self.cfg).plan_hotwords_refusal.format(repr(self.cfg.decoding)))
        distinct, index = [], {}
        for g in hotwords:
            if g is not None and g.key not in index:
                index[g.key] = len(distinct)
                distinct.append(g)
        return self.hotword_set(tuple(distinct)), [index[g.key] if g is not None else -1 for g in hotwords]

    @staticmethod
    def _set_graphs(buf, plan, members=None):
        """the batch's graph indices into the pinned staging of `buf`; -> whether the batch has a graph (else the plain search runs)"""
        buf.hw_set = None
        if plan is None:
            return False
        hw, graph_of = plan
        rows = graph_of if members is None else [graph_of[i] for i in members]
        if all(g < 0 for g in rows):
            return False
        h = buf.h_graph_of.numpy()
        h[:] = -1
        h[:len(rows)] = rows
        buf.hw_set = hw
        return True

    def fill_host(self, waveforms: Sequence[np.ndarray], buf, hotwords=None, members=None, lm=None, nbest=0):
        """copy host waveforms (16 kHz mono float32, un-padded) into the buffer set's pinned staging buffers; the tail of
        every row is zeroed (the kernels mask by length, this only keeps the padding deterministic).  Returns the view of
        `buf` narrowed to this batch's longest utterance."""
        assert len(waveforms) <= buf.B
        longest = max((len(w) for w in waveforms), default=0)
        view = buf.narrow(longest)
        assert view.l_max >= longest
        # one native call for the whole batch (it runs without the interpreter lock: a per-utterance numpy copy would
        # queue behind whatever Python thread holds it — the ids -> text post-processing of an earlier batch)
        capi.host_stage_rows(view.h_audio, view.l_max, waveforms, buf.h_lens)
        # `hotwords`: the call's `graph_plan`, `members`: this batch's positions in it (the H2D copy is run_pipelined's)
        self._set_graphs(view, hotwords, members)
        view.lm = lm                             # the call's `lm_plan`
        view.want_nbest = nbest                  # the call's `nbest_plan`
        return view

    def stage(self, waveforms: Sequence[np.ndarray], l_max: Optional[int] = None, buf: Optional[_Buffers] = None, hotwords=None,
              ngram_lm=None, nbest=None) -> _Buffers:
        """copy host waveforms (16 kHz mono float32, un-padded) into a pinned buffer and on to HBM; `hotwords`: the call's
        `graph_plan` (every utterance of it is in this batch), None = no hotwords; `ngram_lm`: as `lm_plan` takes it (None = the
        model's own LM, if it has one); `nbest`: as `nbest_plan` takes it (None = the model's own count)"""
        B = len(waveforms)
        longest = max((len(w) for w in waveforms), default=0)
        l_max = max(int(l_max or 0), longest, 1)
        l_max = (l_max + 63) // 64 * 64          # rows stay 256-B aligned
        if buf is None:
            buf = self.buffers(B, l_max)
        assert buf.B == B and buf.l_max >= longest
        buf = buf.narrow(l_max)                  # the set itself when it has exactly this extent, else a tight view of it
        ha = buf.h_audio.numpy()
        hl = buf.h_lens.numpy()
        for b, w in enumerate(waveforms):
            n = len(w)
            ha[b, :n] = np.asarray(w, dtype=np.float32)
            ha[b, n:] = 0.0
            hl[b] = n
        with torch.cuda.device(self.device):
            buf.audio.copy_(buf.h_audio, non_blocking=True)
            buf.lens.copy_(buf.h_lens, non_blocking=True)
            if self._set_graphs(buf, hotwords):
                buf.graph_of.copy_(buf.h_graph_of, non_blocking=True)
            buf.lm = self.lm_plan(ngram_lm)
            buf.want_nbest = self.nbest_plan(nbest)
        return buf

    RESAMPLE_CHUNK = 1 << 28        # float32 samples (1 GiB) one rs_resample launch takes in, and at most writes

    def resample_batch(self, waveforms, rates) -> List[np.ndarray]:
        """`norm_audio` for a list on the device: waveforms[i] ([L] or [channels, L], any float type) at rates[i] Hz -> float32
        16 kHz mono arrays, in the caller's order.  The list is grouped by (rate, channel count); each group is uploaded and
        resampled by rs_resample (csrc/k_resample.hip) in chunks of at most RESAMPLE_CHUNK raw samples, and the rows are copied
        back into host arrays (the callers — staging, espnet's window planning, k2's padding — consume host arrays).  The filter
        is runtime/resample.py: plan(rate), also when soxr is installed.  16 kHz mono input passes through (as float32); a rate
        whose filter the kernel does not take (more than 2^24 taps, or a window that does not fit its LDS) goes through the host
        path with a warning.  A row's result does not depend on what else is in the list."""
        from . import resample as rs
        assert len(waveforms) == len(rates)
        out = [None] * len(waveforms)
        groups = {}
        for i, (w, r) in enumerate(zip(waveforms, rates)):
            w = np.asarray(w)
            if w.ndim not in (1, 2):
                raise ValueError(f"waveform {i}: expected [L] or [channels, L], got shape {w.shape}")
            if int(r) == rs.SAMPLERATE and (w.ndim == 1 or w.shape[0] == 1):
                out[i] = np.ascontiguousarray(w.reshape(-1), dtype=np.float32)
                continue
            groups.setdefault((int(r), 1 if w.ndim == 1 else w.shape[0]), []).append(i)
        for (rate, channels), members in groups.items():
            try:
                pl = rs.plan(rate)
                rs.check_window(pl)
            except ValueError as e:             # only these two: any other refusal by rs_resample is a bug and raises
                for i in members:
                    out[i] = rs.host_fallback(waveforms[i], rate, str(e))
                continue
            lo = 0
            while lo < len(members):            # a chunk: raw samples and padded output both within RESAMPLE_CHUNK (one row always fits)
                hi, raw, longest = lo, 0, 0
                while hi < len(members):
                    n = np.asarray(waveforms[members[hi]]).shape[-1]
                    if hi > lo and (raw + n * channels > self.RESAMPLE_CHUNK or (hi - lo + 1) * rs.n_out(max(longest, n), pl.up, pl.down) > self.RESAMPLE_CHUNK):
                        break
                    raw, longest, hi = raw + n * channels, max(longest, n), hi + 1
                chunk = members[lo:hi]
                rows = self._resample_chunk([waveforms[i] for i in chunk], rate, channels, pl)
                for i, row in zip(chunk, rows):
                    out[i] = row
                lo = hi
        return out

    def _resample_chunk(self, waves, rate, channels, pl):
        """one rs_resample launch: rows of one (rate, channels) -> [float32 array]"""
        from . import resample as rs
        host, offs, lens = rs.pack_rows(waves, channels)
        n_outs = [rs.n_out(n, pl.up, pl.down) for n in lens]
        pitch = max((max(n_outs) + 63) // 64 * 64, 64)
        B = len(waves)
        with torch.cuda.device(self.device):
            x = torch.from_numpy(host).to(self.device)
            row_off = torch.tensor(offs, dtype=torch.int64).to(self.device)
            row_len = torch.tensor(lens, dtype=torch.int32).to(self.device)
            out = torch.empty((B, pitch), dtype=torch.float32, device=self.device)
            out_lens = torch.empty((B,), dtype=torch.int32, device=self.device)
            self.ctx.resample(x, row_off, row_len, B, channels, self.resample_table(rate, pl), pl.up, pl.down, pl.numtaps, out, 0,
                              out_lens, torch.cuda.current_stream().cuda_stream)
            h_out, h_lens = out.cpu(), out_lens.cpu().tolist()
        assert h_lens == n_outs, (h_lens, n_outs)
        return [h_out[b, :n].numpy().copy() for b, n in enumerate(n_outs)]

    def resample_table(self, rate, pl):
        """the plan's phase-major table on the device, uploaded once per rate"""
        table = self._resample_tables.get(rate)
        if table is None:
            table = self._resample_tables[rate] = torch.from_numpy(pl.table.copy()).to(self.device)
        return table

    def collect(self, buf, host=None, decoding=None) -> DecodedBatch:
        """hypotheses of a decoded batch as host lists; `host` = the (n_ids, ids, frames, enc_lens, scores) tensors a
        pipeline worker already copied back (buf.h_out), otherwise they are fetched here; `decoding`: the search that
        produced them when it was overridden for the call (see `decode`)"""
        decoding = decoding or self.cfg.decoding
        from_worker = host is not None
        if host is None:
            host = (buf.n_ids.cpu(), buf.ids.cpu(), buf.frames.cpu(), buf.enc_lens.cpu(),
                    buf.scores.cpu() if decoding in ("alsd", "beam", "modified_beam_search") else None)
            lp = self.score_view(buf)
            if lp is not None:
                host = host + (lp.cpu(),)
        n, ids, frames, el = (t.numpy() for t in host[:4])
        if decoding == "alsd":      # alignment step i = frame + labels emitted before
            frames = frames - np.arange(frames.shape[1], dtype=frames.dtype)[None, :]
            scores = host[4].numpy().tolist()
        elif decoding in ("beam", "modified_beam_search"):    # frames = the frame each label was appended at ([UPSTREAM] NeMo Hypothesis.timestep)
            scores = host[4].numpy().tolist()
        else:
            scores = None
        res = DecodedBatch([ids[b, :n[b]].tolist() for b in range(buf.B)],
                           [frames[b, :n[b]].tolist() for b in range(buf.B)], el.tolist(), scores)
        if len(host) > 5:
            lp = host[5].numpy()
            res.token_logprobs = [lp[b, :n[b]].tolist() for b in range(buf.B)]
        if getattr(buf, "nbest_n", 0):
            nb = buf.h_nbest if from_worker and buf.h_nbest is not None else {k: t.cpu() for k, t in buf.nbest_bufs.items()}
            nb = {k: t.numpy() for k, t in nb.items()}
            res.nbest = self.nbest_lists(nb, buf.B, decoding)
            if getattr(buf, "rescored_n", 0):               # (the lists of `nbest_bufs` were scored: `rescore_step`)
                rs = buf.h_rescore if from_worker and buf.h_rescore is not None else {k: buf.rescore_bufs[k].cpu() for k in self.RESCORE_HOST}
                res = RescoredBatch(**{f: getattr(res, f) for f in res.__dataclass_fields__},
                                    rescored=self.rescored_lists({k: t.numpy() for k, t in rs.items()}, nb, buf.B, buf.rescored_n))
        elif getattr(buf, "rescored_n", 0):                 # a decode without lists, scored as lists of one
            rs = {k: buf.rescore_bufs[k].cpu().numpy() for k in self.RESCORE_HOST}
            one = dict(n_hyps=np.ones((buf.B,), np.int32), n_ids=n[:buf.B, None])
            res = RescoredBatch(**{f: getattr(res, f) for f in res.__dataclass_fields__}, rescored=self.rescored_lists(rs, one, buf.B, 1))
        return res

    @staticmethod
    def nbest_lists(nb, B, decoding):
        """the host copies of a buffer set's n-best outputs -> per utterance [(ids, frames, score, norm_score)], best first"""
        out = []
        for b in range(B):
            rows = []
            for r in range(int(nb["n_hyps"][b])):
                m = int(nb["n_ids"][b, r])
                fr = nb["frames"][b, r, :m]
                if decoding == "alsd":           # alignment step i = frame + labels emitted before
                    fr = fr - np.arange(m, dtype=fr.dtype)
                rows.append((nb["ids"][b, r, :m].tolist(), fr.tolist(), float(nb["scores"][b, r]), float(nb["norm_scores"][b, r])))
            out.append(rows)
        return out

    ALIGN_MAX_CELLS = 0x3fffffff      # B x tp_max x (u_cap + 1) one rs_rnnt_align call takes (include/rs_asr.h); a larger batch is halved
    ALIGN_CHUNK_ROWS = 16384    # lattice rows whose logits `align_waveforms` asks room for at once; fewer rows, more chunks, same bits

    def align_waveforms(self, waveforms: Sequence[np.ndarray], label_rows: Sequence[Sequence[int]], max_batch: int = 256,
                        one_per_frame: Optional[bool] = None) -> AlignedBatch:
        """host float32 waveforms and the token ids of their known texts -> the forced alignment and the likelihood of every text
        (rs_rnnt_align, csrc/k_rnnt_align.hip): front-end and encoder as `transcribe_waveforms` runs them, then the transducer
        lattice of (audio, text) instead of a search.  `one_per_frame`: a label also advances the frame; None = the topology the
        model's own searches move in (`cfg.max_symbols == 1`: the Zipformer family).  Up to `max_batch` utterances run as one
        batch, sorted by length (a batch whose lattice is beyond one call's bound is halved); a row's bits do not depend on its
        batch.  Results come back in the caller's order."""
        n = len(waveforms)
        if len(label_rows) != n:
            raise ValueError(f"align_waveforms: {n} waveforms but {len(label_rows)} texts")
        one = bool(self.cfg.max_symbols == 1 if one_per_frame is None else one_per_frame)
        labels = [[int(i) for i in row] for row in label_rows]
        longest = max((len(r) for r in labels), default=0)
        if longest > capi.ALIGN_U_CAP_MAX:
            raise ValueError(f"align_waveforms: a text of {longest} tokens; at most {capi.ALIGN_U_CAP_MAX} are supported (window the audio)")
        out = AlignedBatch([None] * n, [None] * n, [None] * n, [None] * n, [None] * n, [None] * n)
        waveforms = [np.asarray(w, dtype=np.float32) for w in waveforms]
        order = sorted(range(n), key=lambda i: (len(waveforms[i]), i))
        cfg = self.cfg
        hidden = getattr(cfg, "decoder_dim", None) or cfg.pred_hidden
        per_row = 4 * (2 * cfg.joint_hidden + (cfg.n_logits + 63) // 64 * 64 + 2 * hidden + 16)
        groups = [order[g0:g0 + max_batch] for g0 in range(0, n, max_batch)]
        while groups:
            group = groups.pop(0)
            B = len(group)
            buf = self.stage([waveforms[i] for i in group])
            u_cap = max(max(len(labels[i]) for i in group), 1)
            if B * buf.tp_max * (u_cap + 1) > self.ALIGN_MAX_CELLS:          # the lattice of the batch is beyond the entry's bound
                if B == 1:
                    raise ValueError(f"align_waveforms: {buf.tp_max} frames x {u_cap} tokens is more than one call aligns (window the audio)")
                groups[:0] = [group[:B // 2], group[B // 2:]]
                continue
            ids = np.zeros((B, u_cap), np.int32)
            for k, i in enumerate(group):
                ids[k, :len(labels[i])] = labels[i]
            n_ids = np.asarray([len(labels[i]) for i in group], np.int32)
            with torch.cuda.device(self.device):
                dev = self.device
                stream = torch.cuda.current_stream().cuda_stream
                self.run_encoder(buf, stream)
                ids_d, n_d = torch.from_numpy(ids).to(dev), torch.from_numpy(n_ids).to(dev)
                loglik, best = torch.empty((B,), device=dev), torch.empty((B,), device=dev)
                frames = torch.full((B, u_cap), -1, dtype=torch.int32, device=dev)
                logp = torch.full((B, u_cap), float("nan"), device=dev)
                rows = min(self.ALIGN_CHUNK_ROWS, B * buf.tp_max * (u_cap + 1))
                ws = torch.empty((self.ctx.align_workspace_bytes(B, buf.tp_max, u_cap) + (rows + 31) // 32 * 32 * per_row,),
                                 dtype=torch.uint8, device=dev)
                self.ctx.rnnt_align(buf.joint_enc, buf.enc_lens, B, buf.tp_max, ids_d, n_d, loglik, best, frames, logp, ws, stream,
                                    one_per_frame=one)
                loglik, best, frames, logp, el = (t.cpu().numpy() for t in (loglik, best, frames, logp, buf.enc_lens))
            for k, i in enumerate(group):
                m = int(n_ids[k])
                out.frames[i], out.token_logprobs[i] = frames[k, :m].tolist(), logp[k, :m].tolist()
                out.log_likelihood[i], out.alignment_log_prob[i] = float(loglik[k]), float(best[k])
                out.enc_lens[i], out.feasible[i] = int(el[k]), bool(np.isfinite(loglik[k]))
        return out

    def align_candidates(self, waveforms: Sequence[np.ndarray], candidate_rows: Sequence[Sequence[Sequence[int]]], max_batch: int = 256,
                         one_per_frame: Optional[bool] = None, share: bool = True):
        """several candidate texts per utterance, scored on one lattice per batch (rs_rnnt_align_rows, csrc/k_rnnt_align.hip):
        `candidate_rows[i]` is a list of token-id lists for utterance i.  Front-end and encoder run ONCE per utterance; the texts
        of an utterance share the lattice cells of their common label prefixes (`share=False`: RS_ALIGN_NO_SHARING, the same bits).
        Every number equals, bit for bit, what `align_waveforms` gives for that (audio, text) pair.  Batches as `align_waveforms`
        makes them (a batch whose R x tp_max x (u_cap + 1) is beyond one call's bound is halved by utterance); an utterance with
        more than `capi.ALIGN_ROWS_PER_UTT_MAX` candidates takes one call per that many, on the same encoder output.
        -> ([AlignedBatch per utterance, its lists running over the utterance's candidates], (lattice rows computed, lattice rows
        there are without sharing))"""
        n = len(waveforms)
        if len(candidate_rows) != n:
            raise ValueError(f"align_candidates: {n} waveforms but {len(candidate_rows)} candidate lists")
        one = bool(self.cfg.max_symbols == 1 if one_per_frame is None else one_per_frame)
        cands = [[[int(i) for i in row] for row in rows] for rows in candidate_rows]
        longest = max((len(r) for rows in cands for r in rows), default=0)
        if longest > capi.ALIGN_U_CAP_MAX:
            raise ValueError(f"align_candidates: a text of {longest} tokens; at most {capi.ALIGN_U_CAP_MAX} are supported (window the audio)")
        out = [AlignedBatch(*[[None] * len(rows) for _ in range(6)]) for rows in cands]
        stats = [0, 0]
        waveforms = [np.asarray(w, dtype=np.float32) for w in waveforms]
        order = sorted(range(n), key=lambda i: (len(waveforms[i]), i))
        cfg = self.cfg
        hidden = getattr(cfg, "decoder_dim", None) or cfg.pred_hidden
        per_row = 4 * (2 * cfg.joint_hidden + (cfg.n_logits + 63) // 64 * 64 + 2 * hidden + 16)
        cap = capi.ALIGN_ROWS_PER_UTT_MAX
        groups = [order[g0:g0 + max_batch] for g0 in range(0, n, max_batch)]
        while groups:
            group = groups.pop(0)
            B = len(group)
            # the calls of this batch: (position in the batch, utterance, candidate), utterance by utterance, at most `cap` of each
            passes = max((-(-len(cands[i]) // cap) for i in group), default=0)
            calls = [[(k, i, j) for k, i in enumerate(group) for j in range(p * cap, min((p + 1) * cap, len(cands[i])))] for p in range(passes)]
            if not calls:
                continue
            buf = self.stage([waveforms[i] for i in group])
            u_cap = max(max((len(r) for i in group for r in cands[i]), default=0), 1)
            if max(len(c) for c in calls) * buf.tp_max * (u_cap + 1) > self.ALIGN_MAX_CELLS:
                if B == 1:
                    raise ValueError(f"align_candidates: {buf.tp_max} frames x {u_cap} tokens x {len(calls[0])} texts is more than one call "
                                     f"aligns (window the audio, or pass fewer texts)")
                groups[:0] = [group[:B // 2], group[B // 2:]]
                continue
            with torch.cuda.device(self.device):
                dev = self.device
                stream = torch.cuda.current_stream().cuda_stream
                self.run_encoder(buf, stream)
                el = buf.enc_lens.cpu().numpy()
                for rows in calls:
                    R = len(rows)
                    ids = np.zeros((R, u_cap), np.int32)
                    for r, (k, i, j) in enumerate(rows):
                        ids[r, :len(cands[i][j])] = cands[i][j]
                    n_ids = np.asarray([len(cands[i][j]) for _, i, j in rows], np.int32)
                    row_utt = np.asarray([k for k, _, _ in rows], np.int32)
                    ids_d, n_d, utt_d = (torch.from_numpy(a).to(dev) for a in (ids, n_ids, row_utt))
                    loglik, best = torch.empty((R,), device=dev), torch.empty((R,), device=dev)
                    frames = torch.full((R, u_cap), -1, dtype=torch.int32, device=dev)
                    logp = torch.full((R, u_cap), float("nan"), device=dev)
                    chunk = min(self.ALIGN_CHUNK_ROWS, R * buf.tp_max * (u_cap + 1))
                    ws = torch.empty((self.ctx.align_rows_workspace_bytes(B, R, buf.tp_max, u_cap) + (chunk + 31) // 32 * 32 * per_row,),
                                     dtype=torch.uint8, device=dev)
                    done = self.ctx.rnnt_align_rows(buf.joint_enc, buf.enc_lens, B, buf.tp_max, utt_d, ids_d, n_d, loglik, best, frames, logp,
                                                    ws, stream, one_per_frame=one, share=share)
                    stats[0] += done[0]
                    stats[1] += done[1]
                    loglik, best, frames, logp = (t.cpu().numpy() for t in (loglik, best, frames, logp))
                    for r, (k, i, j) in enumerate(rows):
                        m, o = int(n_ids[r]), out[i]
                        o.frames[j], o.token_logprobs[j] = frames[r, :m].tolist(), logp[r, :m].tolist()
                        o.log_likelihood[j], o.alignment_log_prob[j] = float(loglik[r]), float(best[r])
                        o.enc_lens[j], o.feasible[j] = int(el[k]), bool(np.isfinite(loglik[r]))
        return out, (stats[0], stats[1])

    def transcribe_waveforms_sharded(self, waveforms: Sequence[np.ndarray], max_batch: int = 256, hotwords=None, ngram_lm=None) -> DecodedBatch:
        """SPMD form of `transcribe_waveforms` for one process per GPU (`torch.distributed` initialised, RCCL):
        every rank passes the same list, decodes its length-balanced shard on its own GPU and receives all
        hypotheses (ids, frames, encoder lengths and — beam search — scores) in the caller's order after the path's one
        collective (runtime/dist.py: sharded_decode).  With a single process it is `transcribe_waveforms`.  `hotwords` (one
        HotwordGraph or None per utterance) follows each utterance to the rank that decodes it."""
        from . import dist as rdist
        if self.token_scores:
            raise ValueError("token_scores is on: transcribe_waveforms_sharded does not gather token log-probabilities; "
                             "use transcribe_waveforms on each rank, or turn token_scores off")
        if self.rescore:
            raise ValueError("rescore is on: transcribe_waveforms_sharded does not gather rescored n-best lists; use "
                             "transcribe_waveforms on each rank, or set rescore to None")
        if self.nbest:
            raise ValueError("nbest is on: transcribe_waveforms_sharded does not gather n-best lists; use transcribe_waveforms on each "
                             "rank, or set nbest to 0")

        def run_local(indices, batch):
            # `batch`: the chunk size of the dealing plan (ragged input is dealt as length-sorted chunks, balanced over the
            # ranks: runtime/dist.py shard_balanced) — this rank's batches are exactly its chunks
            res = self.transcribe_waveforms([waveforms[i] for i in indices], max_batch=min(max_batch, batch),
                                            hotwords=None if hotwords is None else [hotwords[i] for i in indices], ngram_lm=ngram_lm)
            return res.ids, res.frames, res.enc_lens, res.scores

        ids, frames, enc_lens, scores = rdist.sharded_decode([len(w) for w in waveforms], run_local, max_batch=max_batch)
        return DecodedBatch(ids, frames, enc_lens, scores if self.cfg.has_scores else None)

    LONGEST_FIRST = True    # batch order of a long list (A/B hook of scripts/ragged_order_ab.py)
    POOL_SETS = 4       # resident batches of the host-to-host pipeline (encoder(i+2) || decode(i+1), decode(i) + one being staged)

    def _pool(self, B, l_max, n_sets):
        """buffer sets of the host-to-host pipeline, kept across calls (pinned staging is expensive to allocate);
        bucketed to whole seconds like `buffers`, one geometry at a time"""
        l_max = (max(int(l_max), 1) + self.BUCKET - 1) // self.BUCKET * self.BUCKET
        key = getattr(self, "_pool_key", None)
        if key is None or key[0] != B or not (l_max <= key[1] <= 2 * l_max) or len(self._pool_sets) < n_sets:
            self._pool_sets = []              # drop the old geometry before allocating the new one
            self._pool_key = (B, l_max)
            with torch.cuda.device(self.device):
                self._pool_sets = [_Buffers(self, B, l_max) for _ in range(n_sets)]
        return self._pool_sets[:n_sets]

    def transcribe_waveforms(self, waveforms: Sequence[np.ndarray], max_batch: int = 256, on_batch=None, hotwords=None, ngram_lm=None,
                             nbest=None) -> DecodedBatch:
        """host float32 waveforms -> token ids / frames (the batched boundary).

        `on_batch(indices, decoded)`: called once per batch, in batch order, as soon as that batch's hypotheses are on
        the host (`indices` = positions in `waveforms`, `decoded` = their DecodedBatch) — on a decode worker thread
        while the GPU is already busy with the following batches, so host post-processing (ids -> text) overlaps.

        Up to `max_batch` utterances run as one batch.  Longer lists are sorted by length, cut into batches of
        `max_batch` (each padded only to ITS longest utterance) and pushed through the persistent pipeline of
        `run_pipelined` — four resident batches, two decode lanes, a stager thread that fills the pinned buffers of
        batch i+2 / i+3 while the GPU works on the batches before them, H2D on the encoder stream, hypotheses copied back
        by the decode workers: no drain between batches.  Results come back in the caller's order.

        `hotwords` (modified beam search or ALSD): None, or one HotwordGraph (runtime/k2_hotwords.py) or None per
        utterance.  The distinct graphs of the call become one device table (`hotword_set`) and every utterance's graph index
        travels with it through sorting and grouping; a batch without any graph runs the plain search.

        `ngram_lm` (ALSD, modified beam search): None = the model's own n-gram LM and weight (`self.ngram_lm`, `self.ngram_lm_alpha`), or
        (NgramLm or None, alpha) for this call; alpha 0 or no model = the search without an LM (`lm_plan`).

        `nbest`: None = the model's own count (`self.nbest`), or the entries per utterance for this call (0 = none): the result's
        `nbest` then holds every utterance's ranked list (`nbest_plan`: ValueError for a count the search cannot give)."""
        n = len(waveforms)
        n_best = self.nbest_plan(nbest)
        rescoring = self.rescore_plan(None, n_best) is not None      # (ValueError for a call whose lists are shorter than two)
        if n == 0:
            return RescoredBatch([], [], [], nbest=[], rescored=[]) if rescoring else DecodedBatch([], [], [], nbest=[] if n_best else None)
        waveforms = [np.asarray(w, dtype=np.float32) for w in waveforms]
        plan = self.graph_plan(hotwords, n)
        lm = self.lm_plan(ngram_lm)
        if n <= max_batch:
            buf = self.stage(waveforms, hotwords=plan, ngram_lm=ngram_lm, nbest=n_best)
            self.run_device(buf)
            res = self.collect(buf)
            if on_batch is not None:
                on_batch(list(range(n)), res)
            return res
        order = sorted(range(n), key=lambda i: (len(waveforms[i]), i))
        ids, frames, enc_lens, scores = [None] * n, [None] * n, [None] * n, [None] * n
        logprobs = [None] * n if self.token_scores else None
        lists = [None] * n if n_best else None
        rescored = [None] * n if rescoring else None
        groups = [order[i:i + max_batch] for i in range(0, n, max_batch)]
        # longest batch first: what is left after the last encoder is one decode, and the shortest batch's is the shortest
        # (a ragged list's drain shrinks from the longest batch's decode to the shortest's)
        if self.LONGEST_FIRST:
            groups.reverse()
        l_max = max(len(w) for w in waveforms)
        n_sets = min(self.POOL_SETS, len(groups))
        pool = self._pool(max_batch, l_max, n_sets)

        def fill(i, buf):
            return self.fill_host([waveforms[k] for k in groups[i]], buf, hotwords=plan, members=groups[i], lm=lm, nbest=n_best)

        # `on_batch` runs on its own thread, in batch order: a decode lane that ran the caller's post-processing itself
        # would start its next batch that much later (ids -> text is ~25 ms of Python per 256 utterances)
        post_q = queue.Queue() if on_batch is not None else None
        post_err = []

        def post_worker():
            while True:
                item = post_q.get()
                if item is None:
                    return
                try:
                    if not post_err:
                        on_batch(*item)
                except Exception as e:          # surfaced on the caller's thread below
                    post_err.append(e)

        def harvest(buf):
            res = self.collect(buf, host=buf.h_out)
            group = groups[buf.step]
            for k, i in enumerate(group):
                ids[i], frames[i], enc_lens[i] = res.ids[k], res.frames[k], res.enc_lens[k]
                scores[i] = res.scores[k] if res.scores is not None else None
                if logprobs is not None:
                    logprobs[i] = res.token_logprobs[k]
                if lists is not None:
                    lists[i] = res.nbest[k]
                if rescored is not None:
                    rescored[i] = res.rescored[k]
            if post_q is not None:
                m = len(group)
                extra = dict(rescored=res.rescored[:m]) if rescored is not None else {}
                post_q.put((group, (RescoredBatch if extra else DecodedBatch)(
                    res.ids[:m], res.frames[:m], res.enc_lens[:m], res.scores[:m] if res.scores is not None else None,
                    token_logprobs=res.token_logprobs[:m] if logprobs is not None else None,
                    nbest=res.nbest[:m] if lists is not None else None, **extra)))

        post = None
        if post_q is not None:
            post = threading.Thread(target=post_worker, daemon=True)
            post.start()
        # The post-processing thread allocates ~10^5 small objects per batch; a generation-2 collection triggered in the
        # middle of the pipeline holds the interpreter lock for 50-60 ms (profiles/r03n_host_timeline.txt) and every
        # decode lane behind it: the cyclic collector is paused for the duration of the call (nothing here makes cycles).
        # (process-global, so only for the duration of the call, and only the automatic trigger: gc.collect() still works for
        # a host application's other threads; `pause_gc=False` on the model opts out)
        gc_was_on = gc.isenabled() and getattr(self, "pause_gc", True)
        if gc_was_on:
            gc.disable()
        try:
            self.run_pipelined(pool, len(groups), after_decode=harvest, fill=fill, dec_streams=2 if n_sets >= 3 else 1)
        finally:
            if post is not None:
                post_q.put(None)
                post.join()
            if gc_was_on:
                gc.enable()
        if post_err:
            raise post_err[0]
        if rescored is not None:
            return RescoredBatch(ids, frames, enc_lens, scores if self.cfg.has_scores else None, token_logprobs=logprobs, nbest=lists,
                                 rescored=rescored)
        return DecodedBatch(ids, frames, enc_lens, scores if self.cfg.has_scores else None, token_logprobs=logprobs, nbest=lists)
