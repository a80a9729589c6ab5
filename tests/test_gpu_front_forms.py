"""-m gpu: the second forms of the three kernels in front of the first encoder layer against their first forms, bit for bit.

csrc/k_frontend.hip   logmel_kernel<true>   (filterbank and span in LDS, window in registers)   against  RS_LOGMEL_OLD
csrc/k_subsample.hip  sub_conv0_dw1_run_kernel (a workgroup per run of SUB_RUN = 12 output rows, the bottom conv0 row carried
                      in registers into the next row)                                              against  RS_SUB_CONV0_OLD
                      sub_dw_run_kernel     (a workgroup per run of DW_RUN = 6 output rows, every input row read once)
                                                                                                   against  RS_SUB_DW_OLD

Every second form keeps its per-element arithmetic and only changes which thread computes what and where the operands wait, so
`equal bits` is the whole statement; tests/test_gpu_frontend_edges.py and tests/test_gpu_subsample_edges.py hold the default forms
to the float64 references.  Here are the seams of the new geometries.

log-mel, per kind: one ragged batch through rs_frontend_logmel under both forms; audio tails hold NaN, outputs are NaN-filled with
sentinels behind them.  Equal bits of the features, of the workspace (the raw log-mel: rows past n_frames stay unwritten NaN under
both forms) and of n_frames.  Lengths: the ones of test_gpu_frontend_edges.py plus the frame counts around a workgroup's 16 frames
(4 per wave, transformed in pairs): 15 16 17 31 33, 3 and 5 (a half-filled pair), one frame, no frame.  Once more with t_max = 17
(below the 31- and 33-frame rows, and a pair cut in half by t_max), once more with pad_left = pad_right = 8000.

subsampling: one-layer TINY encoders with sub_channels 64 and 256, in both precisions, read through the `sub_out` tap.  The default
(both second forms) against each switch alone.  t_max 37 41 46 50 99 (none a multiple of 4) give T2 = 10 11 12 13 25 = SUB_RUN - 2,
- 1, + 0, + 1 and 2 SUB_RUN + 1 output rows of conv0 + dw1, and T3 = 5 6 6 7 13 = DW_RUN - 1, + 0, + 1 and 2 DW_RUN + 1 of the
depthwise stage.  Rows of every batch: the full length, lengths with L2 (and L3) strictly inside a run, L1 odd and L1 even (the
a_ok edge at the bottom conv0 row), and a zero-length row.  Every row also equals the same utterance alone (t_max = n_frames).
"""
import functools

import numpy as np
import pytest
import torch

from knobs import get_knob, knob
from reazonspeech_amd.runtime.config import ESPNET_TINY, TINY
from reazonspeech_amd.runtime.k2_config import ZIPFORMER_TINY
from reazonspeech_amd.runtime.k2_weights import synthetic_state_dict_k2
from reazonspeech_amd.runtime.model import AsrModel
from reazonspeech_amd.runtime.weights import synthetic_state_dict
from reazonspeech_amd.runtime.weights_espnet import synthetic_state_dict_espnet
from test_gpu_frontend_edges import ESPNET, ESPNET_CLAMPED, KALDI, NEMO, FRAMES
from test_gpu_subsample_edges import run

pytestmark = pytest.mark.gpu
SENTINEL = 64
N_MELS = 80
SUB_RUN, DW_RUN = 12, 6              # csrc/k_subsample.hip
FRAMES_PER_WORKGROUP = 16            # csrc/k_frontend.hip: WAVES * FRAMES_PER_WAVE

SEAM_FRAMES = (15, 16, 17, 31, 33, 3, 5, 1, 0)
# samples that give SEAM_FRAMES frames: n = L // 160 | 1 + L // 128 (never 0: the last entry is one frame again) | (L + 80) // 160
SEAMS = {0: tuple(160 * n + 7 for n in SEAM_FRAMES),
         1: tuple(128 * (n - 1) + 5 for n in SEAM_FRAMES[:-1]) + (0,),
         2: tuple(160 * n - 80 + 3 for n in SEAM_FRAMES[:-1]) + (40,)}
LENGTHS = {0: NEMO + SEAMS[0], 1: ESPNET + ESPNET_CLAMPED + SEAMS[1], 2: KALDI + SEAMS[2]}


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def noise(n, seed):
    return (0.1 * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


def logmel(model, rows, pad, t_max):
    """one rs_frontend_logmel call -> bits of (features [B][t_max][n_mels], workspace, n_frames); sentinels checked here"""
    dev, B = model.device, len(rows)
    width = (max(max(len(r) for r in rows), 1) + 63) // 64 * 64
    host = np.full((B, width), np.nan, np.float32)
    for b, r in enumerate(rows):
        host[b, :len(r)] = r
    n = B * t_max * N_MELS
    with torch.cuda.device(dev):
        audio = torch.from_numpy(host).to(dev)
        lens = torch.tensor([len(r) for r in rows], dtype=torch.int32, device=dev)
        feats = torch.full((n + SENTINEL,), float("nan"), dtype=torch.float32, device=dev)
        ws = torch.full((n + SENTINEL,), float("nan"), dtype=torch.float32, device=dev)
        n_frames = torch.full((B + SENTINEL,), -7, dtype=torch.int32, device=dev)
        model.ctx.frontend(audio, lens, pad, pad, t_max, feats[:n], n_frames[:B], ws[:n], torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    assert torch.isnan(feats[n:]).all() and torch.isnan(ws[n:]).all(), "written behind the features or the workspace"
    assert (n_frames[B:] == -7).all(), "written behind n_frames"
    return feats[:n].view(torch.int32).cpu(), ws[:n].view(torch.int32).cpu(), n_frames[:B].cpu()


FAMILIES = {0: (TINY, synthetic_state_dict), 1: (ESPNET_TINY, synthetic_state_dict_espnet), 2: (ZIPFORMER_TINY, synthetic_state_dict_k2)}


@pytest.fixture(scope="module", params=[0, 1, 2], ids=["nemo", "espnet", "kaldi"])
def front(request, gpu_device):
    kind = request.param
    cfg, make = FAMILIES[kind]
    model = AsrModel(cfg, make(cfg, 3), None, device="cuda:0", pad_seconds=0.0)
    rows = [noise(L, 500 * kind + i) for i, L in enumerate(LENGTHS[kind])]
    return kind, model, rows


@pytest.mark.parametrize("variant", ["ragged", "t_max_17", "pad_8000"])
def test_logmel_forms_agree_bit_for_bit(front, variant):
    kind, model, rows = front
    lib = model.ctx.lib
    pad = 8000 if variant == "pad_8000" else 0
    counts = [FRAMES[kind](len(r) + 2 * pad) for r in rows]
    t_max = 17 if variant == "t_max_17" else max(counts)
    if variant == "ragged":
        assert {0, 1, 3, 5, 15, 16, 17, 31, 33} - ({0} if kind == 1 else set()) <= set(counts)
        assert FRAMES_PER_WORKGROUP - 1 in counts and 2 * FRAMES_PER_WORKGROUP + 1 in counts
    if variant == "t_max_17":
        assert max(counts) > t_max
    assert get_knob(lib, "RS_LOGMEL_OLD") == 0
    new = logmel(model, rows, pad, t_max)
    with knob(lib, "RS_LOGMEL_OLD", 1):
        old = logmel(model, rows, pad, t_max)
    assert new[2].tolist() == old[2].tolist() == counts
    feats_new, feats_old = new[0].view(len(rows), t_max, N_MELS), old[0].view(len(rows), t_max, N_MELS)
    differ = [len(rows[b]) for b in range(len(rows)) if not torch.equal(feats_new[b], feats_old[b])]
    assert not differ, f"features differ between the forms for the rows of {differ} samples"
    assert torch.equal(new[1], old[1]), "the raw log-mel in the workspace differs between the forms"
    assert torch.isfinite(new[0].view(torch.float32)).all()


# ---- subsampling ----------------------------------------------------------------------------------------------------------------
SUB_CONFIGS = {"c64": TINY.with_(n_layers=1), "c256": TINY.with_(n_layers=1, sub_channels=256)}
SUB_CASES = [(name, mode) for name in SUB_CONFIGS for mode in ("bf16", "fp32")]
# t_max -> n_frames of the batch's rows
SUB_BATCHES = {37: (37, 35, 6, 0),
               41: (41, 38, 9, 0),
               46: (46, 45, 21, 0),
               50: (50, 47, 26, 0),
               99: (99, 97, 53, 51, 7, 0)}


def conv_len(n):
    return (n - 1) // 2 + 1 if n > 0 else 0


def test_the_batches_cover_the_seams():
    t2 = sorted(conv_len(conv_len(t)) for t in SUB_BATCHES)
    assert t2 == [SUB_RUN - 2, SUB_RUN - 1, SUB_RUN, SUB_RUN + 1, 2 * SUB_RUN + 1]
    assert {conv_len(x) for x in t2} == {DW_RUN - 1, DW_RUN, DW_RUN + 1, 2 * DW_RUN + 1}
    assert all(t % 4 for t in SUB_BATCHES)
    lens = [(conv_len(n), conv_len(conv_len(n)), conv_len(conv_len(conv_len(n)))) for n in SUB_BATCHES[99]]
    assert any(l1 % 2 for l1, _, _ in lens) and any(l1 and not l1 % 2 for l1, _, _ in lens)
    assert any(0 < l2 % SUB_RUN and l2 < 2 * SUB_RUN for _, l2, _ in lens)          # L2 strictly inside a run, rows below it masked
    assert any(0 < l3 % DW_RUN and l3 < 2 * DW_RUN for _, _, l3 in lens)
    assert all(0 in rows for rows in SUB_BATCHES.values())


@functools.lru_cache(maxsize=None)
def sub_inputs(t_max):
    n_frames = SUB_BATCHES[t_max]
    feats = np.random.default_rng(100 + t_max).standard_normal((len(n_frames), t_max, N_MELS)).astype(np.float32)
    for b, n in enumerate(n_frames):
        feats[b, n:] = 0.0
    return feats, n_frames


@pytest.fixture(scope="module", params=SUB_CASES, ids=[f"{n}-{m}" for n, m in SUB_CASES])
def sub_model(request, gpu_device):
    name, mode = request.param
    cfg = SUB_CONFIGS[name]
    return AsrModel(cfg, synthetic_state_dict(cfg, 3), None, device="cuda:0", pad_seconds=0.0, precision=mode)


@pytest.mark.parametrize("t_max", sorted(SUB_BATCHES))
def test_subsampling_forms_agree_bit_for_bit_and_with_the_row_alone(sub_model, t_max):
    model, lib = sub_model, sub_model.ctx.lib
    cfg = model.cfg
    feats, n_frames = sub_inputs(t_max)
    assert get_knob(lib, "RS_SUB_CONV0_OLD") == 0 and get_knob(lib, "RS_SUB_DW_OLD") == 0
    new, lens = run(model, feats, n_frames, t_max)
    assert lens == [cfg.enc_frames(n) for n in n_frames]
    for switch in ("RS_SUB_CONV0_OLD", "RS_SUB_DW_OLD"):
        with knob(lib, switch, 1):
            old, lens_old = run(model, feats, n_frames, t_max)
        assert lens_old == lens
        differ = [n_frames[b] for b in range(len(n_frames)) if not np.array_equal(bits(new[b]), bits(old[b]))]
        assert not differ, f"{switch}: sub_out differs between the forms for the rows of {differ} frames"
    for b, n in enumerate(n_frames):
        if lens[b] < 1:
            continue
        alone, lens_alone = run(model, feats[b:b + 1, :n], [n], n)
        assert lens_alone == [lens[b]]
        assert np.array_equal(bits(new[b, :lens[b]]), bits(alone[0])), f"the row of {n} frames alone differs from the row in the batch"
