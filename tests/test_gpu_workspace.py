"""-m gpu: every workspace query covers what its entry point uses.

Each case allocates the queried size plus a 4096-byte tail filled with 0xA5, hands the entry point EXACTLY the queried size, runs it
once and checks that the call returned RS_OK (the wrappers raise otherwise) and that the tail is untouched.  The query and the carve
are one layout function run twice (csrc/rs_arena.h), so this holds by construction; the test is what keeps it so.

  encoder + greedy     nemo (TINY), espnet (ESPNET_TINY), k2 (ZIPFORMER_TINY), each in bf16 and float32, through rs_workspace_bytes;
                       3 utterances of 0.5 - 1.5 s, one of them too short for the subsampling (a zero-length row)
  searches             ALSD beam 4, ESPnet beam 3, modified beam search K = 4, on the projection the encoder case produced
  rs_ctc_align         three ground truths, one empty
  avsr                 encoder, decoder state (begin + one step), rs_avsr_generate_opts with 2 beams and 8 new tokens; 2 clips of 8 frames.
                       The search state's optional pieces: go2 is taken with early_stopping=True, the marks where an options kernel runs
                       (no_repeat_ngram_size here) AND beams x vocabulary exceeds the 32768-byte LDS share.  AVSR_TINY's 61 tokens keep the
                       marks in LDS, so the cases are: no options; the n-gram ban (neither piece); + early_stopping (go2); a 16500-token
                       vocabulary with the ban (marks) and with both options (go2 and marks).  Each case first checks, against the plain
                       query, that exactly the pieces it names were taken.  One stepwise case (V = 5000, K = 8, both pieces) has the
                       marks as the last bytes before the guarded tail.

At these sizes the espnet subsampling always takes the batch as one chunk (a chunk smaller than B needs 2 GiB of conv0 output or
65535 frames in a pass); the chunked layout is held by the monotonicity tests of tests/test_gpu_espnet_longform.py."""
import ctypes

import numpy as np
import pytest
import torch

from reazonspeech_amd.avsr import AVHubertForConditionalGeneration
from reazonspeech_amd.espnet.asr import ctc_segmentation as cs
from reazonspeech_amd.espnet.asr.model import EspnetModel, synthetic_token_list
from reazonspeech_amd.k2.asr.model import K2Model, synthetic_tokens
from reazonspeech_amd.runtime import capi
from reazonspeech_amd.runtime.avsr_config import AVSR_TINY
from reazonspeech_amd.runtime.avsr_synth import synthetic_clips
from reazonspeech_amd.runtime.avsr_weights import synthetic_state_dict_avsr
from reazonspeech_amd.runtime.config import ESPNET_TINY, TINY
from reazonspeech_amd.runtime.k2_config import ZIPFORMER_TINY
from reazonspeech_amd.runtime.k2_weights import synthetic_state_dict_k2
from reazonspeech_amd.runtime.model import AsrModel
from reazonspeech_amd.runtime.synth import synthetic_batch
from reazonspeech_amd.runtime.tokenizer import SyntheticTokenizer
from reazonspeech_amd.runtime.weights import synthetic_state_dict
from reazonspeech_amd.runtime.weights_espnet import synthetic_state_dict_espnet

pytestmark = pytest.mark.gpu
TAIL = 4096
WIDE_VOCAB = 16500


def align256(n):
    return (n + 255) // 256 * 256


class Guarded:
    """`need` bytes of workspace followed by a tail of 0xA5; `.ws` is the view of exactly `need` bytes"""

    def __init__(self, need, device="cuda:0"):
        assert need > 0
        self.full = torch.empty((need + TAIL,), dtype=torch.uint8, device=device)
        self.full[need:] = 0xA5
        self.ws = self.full[:need]

    def intact(self):
        torch.cuda.synchronize()
        return bool((self.full[-TAIL:] == 0xA5).all())


def am_of(family, precision):
    if family == "nemo":
        return AsrModel(TINY, synthetic_state_dict(TINY, 0), SyntheticTokenizer(TINY.vocab_size), device="cuda:0", pad_seconds=0.0, precision=precision)
    if family == "espnet":
        return EspnetModel(ESPNET_TINY, synthetic_state_dict_espnet(ESPNET_TINY, 11, blank_bias=12.0, dec_gain=8.0), synthetic_token_list(ESPNET_TINY.vocab_size, 11), device="cuda:0",
                           precision=precision).am
    return K2Model(ZIPFORMER_TINY, synthetic_state_dict_k2(ZIPFORMER_TINY, 3), synthetic_tokens(ZIPFORMER_TINY.vocab_size, 3), device="cuda:0",
                   precision=precision).am


def waves():
    audio, _ = synthetic_batch(3, 1.5, seed=9)
    return [audio[0, :24000], audio[1, :40], audio[2, :8000]]            # 1.5 s, too short for any family's subsampling, 0.5 s


def encode_and_decode(am):
    """front-end, encoder and greedy decode in a workspace of exactly rs_workspace_bytes -> (buffers, guard)"""
    buf = am.stage(waves(), buf=am.new_buffers(3, 24000))
    guard = Guarded(am.ctx.workspace_bytes(buf.B, buf.l_pad))
    buf.ws = guard.ws
    am.run_device(buf)
    return buf, guard


@pytest.fixture(scope="module")
def encoded(gpu_device):
    """family -> (model, buffers after the bf16 run): the projections the search cases decode"""
    return {}


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
@pytest.mark.parametrize("family", ["nemo", "espnet", "k2"])
def test_encoder_and_greedy(gpu_device, encoded, family, precision):
    am = am_of(family, precision)
    buf, guard = encode_and_decode(am)
    assert guard.intact()
    lens = buf.enc_lens.cpu().tolist()
    assert lens[1] == 0 and min(lens[0], lens[2]) > 0, lens
    assert int(buf.n_ids.cpu()[1]) == 0
    if precision == "bf16":
        encoded[family] = (am, buf)


def projection(encoded, family):
    if family not in encoded:
        am = am_of(family, "bf16")
        encoded[family] = (am, encode_and_decode(am)[0])
    return encoded[family]


def outputs(buf, cap):
    dev = buf.joint_enc.device
    ids = torch.zeros((buf.B, cap), dtype=torch.int32, device=dev)
    return ids, torch.zeros_like(ids), torch.zeros((buf.B,), dtype=torch.int32, device=dev), torch.zeros((buf.B,), dtype=torch.float32, device=dev)


def test_alsd(gpu_device, encoded):
    am, buf = projection(encoded, "nemo")
    ids, steps, n_ids, scores = outputs(buf, 2 * buf.tp_max)
    guard = Guarded(am.ctx.alsd_workspace_bytes(buf.B, 4, buf.tp_max, 1.0))
    am.ctx.rnnt_alsd(buf.joint_enc, buf.enc_lens, buf.B, buf.tp_max, 4, 1.0, True, False, ids, steps, n_ids, scores, guard.ws,
                     torch.cuda.current_stream().cuda_stream)
    assert guard.intact()


def test_espnet_beam(gpu_device, encoded):
    am, buf = projection(encoded, "espnet")
    ids, frames, n_ids, scores = outputs(buf, 2 * buf.tp_max + 16)
    pops = torch.zeros_like(n_ids)
    guard = Guarded(am.ctx.beam_workspace_bytes(buf.B, 3, buf.tp_max, 0))
    am.ctx.rnnt_beam(buf.joint_enc, buf.enc_lens, buf.B, buf.tp_max, 3, True, 0, ids, n_ids, scores, pops, guard.ws,
                     torch.cuda.current_stream().cuda_stream, frames=frames)
    assert guard.intact()


def test_modified_beam_search(gpu_device, encoded):
    am, buf = projection(encoded, "k2")
    ids, frames, n_ids, scores = outputs(buf, buf.ids.shape[1])
    guard = Guarded(am.ctx.mbs_workspace_bytes(buf.B, 4, buf.tp_max, ids.shape[1]))
    am.ctx.rnnt_mbs(buf.joint_enc, buf.enc_lens, buf.B, buf.tp_max, 4, 0.0, True, ids, frames, n_ids, scores, guard.ws,
                    torch.cuda.current_stream().cuda_stream)
    assert guard.intact()


def test_ctc_align(gpu_device, encoded):
    am, _ = projection(encoded, "espnet")
    chars = ["<blank>", "a", "b", "ab", "c", "abc"]
    gt, gt_lens, _ = cs.pack_ground_truth(cs.CtcSegmentationParameters(char_list=chars), ["abcab", "", "cabbac"])
    B, tp_max, V = 3, 23, len(chars)
    rng = np.random.default_rng(5)
    z = rng.standard_normal((B * tp_max, V)).astype(np.float32)
    probs = torch.from_numpy(np.exp(z) / np.exp(z).sum(axis=1, keepdims=True)).float().cuda()
    enc_lens = torch.tensor([20, 4, 23], dtype=torch.int32, device="cuda")
    frames = torch.zeros((B, gt.shape[1]), dtype=torch.int32, device="cuda")
    status = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    guard = Guarded(am.ctx.ctc_align_workspace_bytes(B, tp_max, gt.shape[1], gt.shape[2]))
    am.ctx.ctc_align(probs, enc_lens, B, tp_max, torch.from_numpy(gt).cuda(), torch.from_numpy(gt_lens).cuda(), 0, frames, status, guard.ws,
                     torch.cuda.current_stream().cuda_stream)
    assert guard.intact()
    assert status.cpu().tolist() == [0, 0, 0]


def avsr_of(cfg, device):
    model = AVHubertForConditionalGeneration(cfg, synthetic_state_dict_avsr(cfg, 0), device=str(device), search="device")
    a, v, mask, _ = synthetic_clips(2, 8, seed=3)
    return model.dev, a, v, mask


@pytest.fixture(scope="module")
def avsr(gpu_device):
    return avsr_of(AVSR_TINY, gpu_device)


@pytest.fixture(scope="module")
def avsr_wide(gpu_device):
    """a vocabulary at which the marks of a clip's 2 rows (2 x 16500 bytes) exceed the 32768-byte LDS share and live in the state"""
    return avsr_of(AVSR_TINY.with_(vocab_size=WIDE_VOCAB), gpu_device)


def avsr_encode(avsr):
    dev, a, v, mask = avsr
    guard = Guarded(int(dev.ctx.lib.rs_avsr_workspace_bytes(dev.ctx._h, 2, 8)))
    dev._ws = guard.ws                     # `encode` keeps a workspace that is large enough and passes its size
    enc = dev.encode(a, v, mask)
    assert dev._ws.data_ptr() == guard.ws.data_ptr() and dev._ws.numel() == guard.ws.numel()
    return enc, guard


def test_avsr_encoder(avsr):
    enc, guard = avsr_encode(avsr)
    assert guard.intact()
    assert enc.shape[:2] == (2, 8) and bool(torch.isfinite(enc).all())


def test_avsr_decoder_state(avsr):
    dev, _, _, mask = avsr
    enc, _ = avsr_encode(avsr)
    beams, max_len = 2, 9
    guard = Guarded(int(dev.ctx.lib.rs_avsr_decoder_state_bytes(dev.ctx._h, 2, 8, beams, max_len)))
    dev._state = guard.ws
    dec = dev.decoding(enc, mask, beams, max_len)
    assert dec.state.data_ptr() == guard.ws.data_ptr() and dec.state.numel() == guard.ws.numel()
    logits = dec.step(np.full((2 * beams,), dev.cfg.bos_token_id), 0)
    assert guard.intact()
    assert bool(torch.isfinite(logits).all())


def search_state_bytes(dev, B, beams, max_len, vocab, **opts):
    so = dev.search_opts(**opts)
    return int(dev.ctx.lib.rs_avsr_search_state_bytes_opts(dev.ctx._h, B, beams, max_len, vocab, ctypes.byref(so)))


# (model, options) -> the optional pieces the search state holds: go2 with early_stopping=True, marks where an options kernel runs and
# beams x vocabulary padded to 4 exceeds 32768 bytes
GENERATE_CASES = [("avsr", {}, set()),
                  ("avsr", {"no_repeat_ngram_size": 2}, set()),                    # an options kernel, its marks in LDS
                  ("avsr", {"no_repeat_ngram_size": 2, "early_stopping": True}, {"go2"}),
                  ("avsr_wide", {"no_repeat_ngram_size": 2}, {"marks"}),
                  ("avsr_wide", {"no_repeat_ngram_size": 2, "early_stopping": True}, {"go2", "marks"})]


@pytest.mark.parametrize("which,opts,pieces", GENERATE_CASES, ids=["plain", "ngram", "ngram+es", "wide-ngram", "wide-ngram+es"])
def test_avsr_generate(request, which, opts, pieces):
    model = request.getfixturevalue(which)
    dev, _, _, mask = model
    enc, _ = avsr_encode(model)
    beams, new_tokens = 2, 8
    # the pieces this case claims are the ones the layout takes: each adds its 256-aligned extent to the plain search state
    V = dev.cfg.vocab_size
    plain = search_state_bytes(dev, 2, beams, 1 + new_tokens, V)
    extra = (align256(4 * (1 + new_tokens + 1)) if "go2" in pieces else 0) + (align256(2 * beams * ((V + 3) // 4 * 4)) if "marks" in pieces else 0)
    assert search_state_bytes(dev, 2, beams, 1 + new_tokens, V, **opts) == plain + extra
    so = dev.search_opts(**opts)
    guard = Guarded(int(dev.ctx.lib.rs_avsr_generate_state_bytes_opts(dev.ctx._h, 2, 8, beams, 1 + new_tokens, ctypes.byref(so))))
    dev._gen_state = guard.ws
    seq, scores = dev.generate(enc, mask, beams, new_tokens, False, **opts)
    assert dev._gen_state.data_ptr() == guard.ws.data_ptr() and dev._gen_state.numel() == guard.ws.numel()
    assert guard.intact()
    assert seq.shape[0] == 2 and np.all(np.isfinite(scores))


def test_avsr_search_state_with_both_optional_pieces(avsr):
    """the stepwise ABI at V = 5000, K = 8 with early_stopping=True and an n-gram ban: go2 and the marks (8 x 5000 bytes, above the LDS
    share) are the LAST pieces of the state, so the guarded tail sits right behind what the step kernel marks"""
    dev = avsr[0]
    lib, h = dev.ctx.lib, dev.ctx._h
    B, K, V, N = 2, 8, 5000, 8
    opts = {"no_repeat_ngram_size": 2, "early_stopping": True}
    need = search_state_bytes(dev, B, K, 1 + N, V, **opts)
    assert need == search_state_bytes(dev, B, K, 1 + N, V) + align256(4 * (1 + N + 1)) + align256(B * K * V)
    guard = Guarded(need)
    sp, so = dev.search_params(K, N, False), dev.search_opts(**opts)
    st = (capi._ptr(guard.ws), guard.ws.numel(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    dev.ctx.check(lib.rs_avsr_search_begin_opts(h, ctypes.byref(sp), ctypes.byref(so), B, V, *st))
    logits = torch.from_numpy(np.random.default_rng(8).standard_normal((B * K, V)).astype(np.float32)).to(dev.device)
    for step in range(3):
        dev.ctx.check(lib.rs_avsr_search_step_opts(h, capi._ptr(logits), step, ctypes.byref(sp), ctypes.byref(so), B, V, *st))
    seq = torch.empty((B, 1 + N), dtype=torch.int32, device=dev.device)
    lens = torch.empty((B,), dtype=torch.int32, device=dev.device)
    scores = torch.empty((B,), dtype=torch.float32, device=dev.device)
    dev.ctx.check(lib.rs_avsr_search_finish_opts(h, ctypes.byref(sp), ctypes.byref(so), B, st[0], st[1], capi._ptr(seq), capi._ptr(lens), capi._ptr(scores), st[2]))
    assert guard.intact()
    assert bool(torch.isfinite(scores).all())
