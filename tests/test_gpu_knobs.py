"""-m gpu: the A/B switches of reazonspeech_amd/csrc/rs_knobs.h on the loaded library (rs_debug_set_knob / rs_debug_get_knob through
tests/knobs.py), and two forms that only a switch reaches, on the tiny ESPnet model of tests/test_gpu_espnet.py:

  RS_SUB_IM2COL   the gathered patch matrix of Conv2dSubsampling: a larger workspace, the same bits, and a launch with a workspace
                  sized for the other form is refused with RS_EWORKSPACE before anything is enqueued
  RS_ATTN64       the head_dim-64 attention geometries "0", "4,4" (default) and "2,2": the same bits
"""
import ctypes

import pytest
import torch

from knobs import get_knob, knob, set_knob
from reazonspeech_amd.runtime import capi
from reazonspeech_amd.runtime.config import ESPNET_TINY
from reazonspeech_amd.runtime.synth import synthetic_batch
from reazonspeech_amd.runtime.weights_espnet import synthetic_state_dict_espnet
from reazonspeech_amd.espnet.asr.model import EspnetModel, synthetic_token_list

pytestmark = pytest.mark.gpu
RS_EINVAL, RS_EWORKSPACE = -1, -3


@pytest.fixture(scope="module")
def am(gpu_device):
    sd = synthetic_state_dict_espnet(ESPNET_TINY, 3)
    return EspnetModel(ESPNET_TINY, sd, synthetic_token_list(ESPNET_TINY.vocab_size, 3), device="cuda:0").am


def staged(am, seconds, seed):
    """utterances of the given lengths (the first is the longest) in a buffer set of their own"""
    audio, _ = synthetic_batch(len(seconds), seconds[0], seed=seed)
    waves = [audio[b, :int(s * 16000)] for b, s in enumerate(seconds)]
    return am.stage(waves, buf=am.new_buffers(len(waves), len(waves[0])))


def forward(am, buf, ws):
    """front-end, encoder and greedy search in the caller's workspace -> (joint projection, ids)"""
    buf.joint_enc.zero_()
    with torch.cuda.device(am.device):
        stream = torch.cuda.current_stream().cuda_stream
        am.ctx.frontend(buf.audio, buf.lens, am.pad_left, am.pad_right, buf.t_max, buf.feats, buf.n_frames, ws, stream)
        am.ctx.encoder(buf.feats, buf.n_frames, buf.B, buf.t_max, None, buf.joint_enc, buf.enc_lens, ws, stream)
        am.decode(am.ctx, buf, ws, stream)
        torch.cuda.synchronize()
    return buf.joint_enc.clone(), am.collect(buf).ids


def workspace(am, buf):
    return torch.empty((am.ctx.workspace_bytes(buf.B, buf.l_pad),), dtype=torch.uint8, device=am.device)


def test_round_trip_on_the_loaded_library(am):
    lib = am.ctx.lib
    assert get_knob(lib, "RS_BEAM_SPEC") == 3 and get_knob(lib, "RS_ATTN64_NW") == 4
    with knob(lib, "RS_BEAM_SPEC", 5):
        assert get_knob(lib, "RS_BEAM_SPEC") == 5
        with pytest.raises(ZeroDivisionError):
            with knob(lib, "RS_ATTN64_NW", 2):
                assert get_knob(lib, "RS_ATTN64_NW") == 2
                1 / 0
        assert get_knob(lib, "RS_ATTN64_NW") == 4                 # the helper's finally put the previous value back
    assert get_knob(lib, "RS_BEAM_SPEC") == 3
    value = ctypes.c_int(77)
    assert lib.rs_debug_set_knob(b"NO_SUCH_SWITCH", 1) == RS_EINVAL
    assert lib.rs_debug_get_knob(b"NO_SUCH_SWITCH", ctypes.byref(value)) == RS_EINVAL and value.value == 77
    with pytest.raises(KeyError):
        set_knob(lib, "NO_SUCH_SWITCH", 1)
    # the older per-switch exports write the same rows
    lib.rs_debug_set_gemm_pairs.argtypes = [ctypes.c_int]
    lib.rs_debug_set_gemm_pairs.restype = None
    with knob(lib, "RS_GEMM_PAIRS", get_knob(lib, "RS_GEMM_PAIRS")):
        lib.rs_debug_set_gemm_pairs(1)
        assert get_knob(lib, "RS_GEMM_PAIRS") == 1
    assert get_knob(lib, "RS_GEMM_PAIRS") == 2


def test_sub_im2col_sizes_the_workspace_and_keeps_the_bits(am):
    lib = am.ctx.lib
    buf = staged(am, (10.0, 6.1, 1.3), seed=31)
    ws0 = workspace(am, buf)
    in_place = forward(am, buf, ws0)
    assert sum(len(x) for x in in_place[1]) > 0
    with knob(lib, "RS_SUB_IM2COL", 1):
        ws1 = workspace(am, buf)
        assert ws1.numel() > ws0.numel()
        gathered = forward(am, buf, ws1)
        # the size check precedes every launch: a workspace sized for the other form is refused, nothing is enqueued
        with pytest.raises(capi.RsError) as e:
            with torch.cuda.device(am.device):
                am.ctx.encoder(buf.feats, buf.n_frames, buf.B, buf.t_max, None, buf.joint_enc, buf.enc_lens, ws0,
                               torch.cuda.current_stream().cuda_stream)
        assert e.value.code == RS_EWORKSPACE
    assert torch.equal(gathered[0], in_place[0]) and gathered[1] == in_place[1]
    assert workspace(am, buf).numel() == ws0.numel()


def test_attn64_geometries_are_bit_identical(am):
    lib = am.ctx.lib
    buf = staged(am, (10.0, 1.3), seed=32)
    assert buf.tp_max > 6 * 32                                     # more than one key chunk in every geometry (at most 6 blocks of 32 keys)
    ws = workspace(am, buf)
    want = forward(am, buf, ws)                                    # the default: 4 key blocks per chunk, 4 waves
    assert sum(len(x) for x in want[1]) > 0
    for kbc, nw in ((0, 4), (4, 4), (2, 2)):
        with knob(lib, "RS_ATTN64", kbc), knob(lib, "RS_ATTN64_NW", nw):
            got = forward(am, buf, ws)
        assert torch.equal(got[0], want[0]) and got[1] == want[1], (kbc, nw)
