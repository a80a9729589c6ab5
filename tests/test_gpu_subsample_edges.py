"""-m gpu: the two subsamplings (csrc/k_subsample.hip: enc_lens_kernel, sub_conv0_dw1_kernel<>, sub_dw_kernel, sub_dw_f32_kernel;
csrc/k_espnet.hip: sub2d_conv0_kernel<>, im2col3x3s2_kernel; the GEMMs between them) at their length edges, read through the
`sub_out` tap of rs_encoder_set_taps.

Synthetic features (standard_normal, zeroed past each row's n_frames as the front-end leaves them) go straight into
rs_encoder_forward of one-layer encoders:
    nemo_c64    TINY                        dw_striding x8, C = 64: sub_dw_kernel's fpb = 256 / (C / 8) = 32 output bins per workgroup
    nemo_c256   TINY, sub_channels = 256    the shipped model's geometry: fpb = 8, two workgroups per row of Fout = 10 bins, the second
                                            one half empty (the `fo >= Fout` early-out)
    espnet      ESPNET_TINY                 Conv2dSubsampling x4, C = 256
each in the throughput mode and with precision="fp32".  One batch per configuration, t_max = 65:
    NeMo   n_frames 0 1 2 3 4 5 7 8 9 15 16 17 31 33 64 65      lengths (n - 1) // 2 + 1 three times
    ESPnet n_frames 0 1 2 3 6 7 8 9 10 11 14 15 31 33 64 65     lengths (n - 3) // 2 + 1 twice, no output row below 7 frames

Asserted
  lengths          enc_lens == the oracle's; one more launch with n_frames = 0 .. 200 == rs_enc_frames == ModelConfig.enc_frames
  batch invariance every row's valid sub_out rows are bit-identical to the same utterance alone with t_max = n_frames — the sharp
                   check on the `tm >= t_max` row clamp and zeroed taps of sub_conv0_dw1, on the row masks after every stage and on
                   rows[] of sub2d_conv0; both modes
  values, fp32     per utterance, against the float64 oracle (oracle.*.subsampling on .double() inputs, recipe "fp32"):
                       max |device - ref64| <= max(FACTOR * max |oracle32 - ref64|, 4 * 2^-23 * max |ref64|)
                   FACTOR = 8, the project's factor for two float32 evaluations of one formula that differ in summation order only
                   (tests/test_gpu_avsr_features.py); here the exact-f32 MFMA chain against torch's
  values, bf16     per utterance, against the oracle's "bf16" recipe: max and mean of |device - oracle_bf16| are at most the same
                   statistic of |oracle_bf16 - oracle_fp32|.  A device that follows the recipe differs from it only where another
                   summation order flips a bf16 rounding; the recipe differs from float32 at EVERY rounding point; so the recipe's
                   own gap — a reference-only quantity — is the yardstick, with factor 1
  last row         the same statements for the LAST valid output row of every utterance on its own: where a wrong mask lands
  finite           the whole tap, rows of zero-length utterances included; a sentinel behind it is untouched

Measured on an MI355X, worst over the utterances of a batch (whole utterance | last row):
    fp32, device error / oracle32 error         nemo_c64 2.53 | 3.97    nemo_c256 3.31 | 4.36    espnet 6.85 | 6.02
    bf16, max  |device - recipe| / recipe gap   nemo_c64 0.22 | 0.25    nemo_c256 0.08 | 0.12    espnet 0.07 | 0.003
    bf16, mean |device - recipe| / recipe gap   nemo_c64 0.09 | 0.23    nemo_c256 0.05 | 0.14    espnet 0.009 | 0.003
(espnet fp32: the dense 3 x 3 conv is a K = 9 * 256 = 2304 product, the longest sum of the three configurations; absolute errors
are 3e-5 .. 8e-5 on values up to 44.)
"""
import functools

import numpy as np
import pytest
import torch

from oracle import espnet as oe, model as om
from reazonspeech_amd.runtime.config import ESPNET_TINY, TINY
from reazonspeech_amd.runtime.model import AsrModel
from reazonspeech_amd.runtime.weights import synthetic_state_dict
from reazonspeech_amd.runtime.weights_espnet import synthetic_state_dict_espnet

pytestmark = pytest.mark.gpu
FACTOR = 8.0
FLOOR = 4 * 2.0 ** -23
SENTINEL = 64
T_MAX = 65
WEIGHT_SEED = 3
NEMO_FRAMES = (0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 33, 64, 65)
ESPNET_FRAMES = (0, 1, 2, 3, 6, 7, 8, 9, 10, 11, 14, 15, 31, 33, 64, 65)
CONFIGS = {"nemo_c64": TINY.with_(n_layers=1), "nemo_c256": TINY.with_(n_layers=1, sub_channels=256),
           "espnet": ESPNET_TINY.with_(n_layers=1)}
CASES = [(name, mode) for name in CONFIGS for mode in ("bf16", "fp32")]


@functools.lru_cache(maxsize=None)
def state_dict(name):
    cfg = CONFIGS[name]
    return synthetic_state_dict_espnet(cfg, WEIGHT_SEED) if cfg.espnet else synthetic_state_dict(cfg, WEIGHT_SEED)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """-> (features float32 [B][T_MAX][n_mels] zeroed past each row's n_frames, n_frames tuple)"""
    cfg = CONFIGS[name]
    n_frames = ESPNET_FRAMES if cfg.espnet else NEMO_FRAMES
    feats = np.random.default_rng(11).standard_normal((len(n_frames), T_MAX, cfg.n_mels)).astype(np.float32)
    for b, n in enumerate(n_frames):
        feats[b, n:] = 0.0
    return feats, n_frames


@functools.lru_cache(maxsize=None)
def references(name):
    """the oracle's subsampling of the batch, once per configuration -> dict(ref64, fp32, bf16: float64 [B][T'][d]; lens)"""
    cfg, sd = CONFIGS[name], state_dict(name)
    feats, n_frames = inputs(name)
    sub = oe.subsampling if cfg.espnet else om.subsampling
    f, n = torch.from_numpy(feats), torch.tensor(n_frames)
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    with torch.no_grad():
        ref64, lens = sub(cfg, sd64, f.double(), n, "fp32")
        fp32, _ = sub(cfg, sd, f, n, "fp32")
        bf16, _ = sub(cfg, sd, f, n, "bf16")
    assert ref64.dtype == torch.float64 and fp32.dtype == bf16.dtype == torch.float32
    return {"ref64": ref64.numpy(), "fp32": fp32.double().numpy(), "bf16": bf16.double().numpy(), "lens": lens.tolist()}


def run(model, feats, n_frames, t_max):
    """rs_encoder_forward on host features [B][t_max][n_mels] -> (sub_out float32 [B][T'][d], enc_lens list)"""
    cfg, dev, ctx = model.cfg, model.device, model.ctx
    B = len(n_frames)
    tp = cfg.enc_frames(t_max)
    assert tp >= 1 and feats.shape == (B, t_max, cfg.n_mels)
    samples = (t_max - 1) * cfg.hop_length if cfg.espnet else t_max * cfg.hop_length
    assert ctx.mel_frames(samples) == t_max
    n = B * tp * cfg.d_model
    with torch.cuda.device(dev):
        d_feats = torch.from_numpy(np.ascontiguousarray(feats)).to(dev)
        d_n = torch.tensor(n_frames, dtype=torch.int32, device=dev)
        ws = torch.empty((ctx.workspace_bytes(B, samples),), dtype=torch.uint8, device=dev)
        joint = torch.empty((B, tp, cfg.joint_hidden), dtype=torch.float32, device=dev)
        enc_lens = torch.full((B,), -7, dtype=torch.int32, device=dev)
        tap = torch.full((n + SENTINEL,), float("nan"), dtype=torch.float32, device=dev)
        ctx.set_taps(sub_out=tap)
        try:
            ctx.encoder(d_feats, d_n, B, t_max, None, joint, enc_lens, ws, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
        finally:
            ctx.set_taps()
    got = tap.cpu().numpy()
    assert np.isnan(got[n:]).all(), "written behind the sub_out tap"
    assert np.isfinite(got[:n]).all(), "the sub_out tap holds a value that is not finite"
    return got[:n].reshape(B, tp, cfg.d_model), enc_lens.cpu().tolist()


class Case:
    def __init__(self, name, mode):
        self.name, self.mode, self.cfg = name, mode, CONFIGS[name]
        self.model = AsrModel(self.cfg, state_dict(name), None, device="cuda:0", pad_seconds=0.0, precision=mode)
        self.feats, self.n_frames = inputs(name)
        self.batch, self.enc_lens = run(self.model, self.feats, self.n_frames, T_MAX)
        self.alone = {}          # row -> sub_out [T'][d] of the utterance alone with t_max = n_frames (rows with an output row only)
        for b, n in enumerate(self.n_frames):
            if self.cfg.enc_frames(n) >= 1:
                out, lens = run(self.model, self.feats[b:b + 1, :n], [n], n)
                assert lens == [self.cfg.enc_frames(n)]
                self.alone[b] = out[0]


@pytest.fixture(scope="module", params=CASES, ids=[f"{n}-{m}" for n, m in CASES])
def case(request, gpu_device):
    return Case(*request.param)


def test_enc_lens_equal_the_oracles(case):
    assert case.enc_lens == references(case.name)["lens"] == [case.cfg.enc_frames(n) for n in case.n_frames]


def test_enc_lens_for_every_frame_count_up_to_200(case):
    cfg = case.cfg
    counts = list(range(201))
    feats = np.zeros((len(counts), 200, cfg.n_mels), np.float32)
    _, lens = run(case.model, feats, counts, 200)
    assert lens == [case.model.ctx.enc_frames(n) for n in counts] == [cfg.enc_frames(n) for n in counts]
    rule = (lambda n: (n - 3) // 2 + 1 if n >= 3 else 0) if cfg.espnet else (lambda n: (n - 1) // 2 + 1 if n > 0 else 0)
    stages = 2 if cfg.espnet else 3
    assert lens == [functools.reduce(lambda n, _: rule(n), range(stages), n) for n in counts]


def test_a_row_in_the_batch_equals_the_row_alone_bit_for_bit(case):
    bad = []
    assert sorted(case.alone) == [b for b, n in enumerate(case.enc_lens) if n >= 1]
    for b, alone in case.alone.items():
        n = case.enc_lens[b]
        assert alone.shape[0] == n
        got = case.batch[b, :n]
        if not np.array_equal(got.view(np.int32), alone.view(np.int32)):
            rows = np.nonzero((got.view(np.int32) != alone.view(np.int32)).any(axis=1))[0].tolist()
            bad.append((case.n_frames[b], "output rows that differ", rows, float(np.abs(got - alone).max())))
    assert not bad, bad


def statistics(case):
    """per utterance with an output row: (n_frames, whole-utterance and last-row (device error, yardstick) pairs)"""
    ref = references(case.name)
    for b, n in enumerate(case.enc_lens):
        if n < 1:
            continue
        dev = case.batch[b, :n].astype(np.float64)
        for part, rows in (("all", slice(0, n)), ("last", slice(n - 1, n))):
            yield case.n_frames[b], part, dev[rows], ref["ref64"][b, rows], ref["fp32"][b, rows], ref["bf16"][b, rows]


def test_values_within_the_yardstick(case):
    bad, worst = [], {}
    for n_frames, part, dev, ref64, fp32, bf16 in statistics(case):
        if case.mode == "fp32":
            err, yard, floor = np.abs(dev - ref64).max(), np.abs(fp32 - ref64).max(), FLOOR * np.abs(ref64).max()
            ratio = err / yard
            print(f"{case.name} fp32 n_frames={n_frames} {part}: device - ref64 {err:.3e}  oracle32 - ref64 {yard:.3e}  ratio {ratio:.2f}  floor {floor:.3e}")
            worst[part] = max(worst.get(part, 0.0), ratio)
            if not err <= max(FACTOR * yard, floor):
                bad.append((n_frames, part, err, yard, floor))
        else:
            e, y = np.abs(dev - bf16), np.abs(bf16 - fp32)
            print(f"{case.name} bf16 n_frames={n_frames} {part}: device - oracle_bf16 max {e.max():.3e} mean {e.mean():.3e}  "
                  f"oracle_bf16 - oracle_fp32 max {y.max():.3e} mean {y.mean():.3e}  fractions {e.max() / y.max():.3f} {e.mean() / y.mean():.3f}")
            worst[part + " max"] = max(worst.get(part + " max", 0.0), e.max() / y.max())
            worst[part + " mean"] = max(worst.get(part + " mean", 0.0), e.mean() / y.mean())
            if not (e.max() <= y.max() and e.mean() <= y.mean()):
                bad.append((n_frames, part, e.max(), y.max(), e.mean(), y.mean()))
    print(f"{case.name} {case.mode}: worst {({k: round(float(v), 3) for k, v in worst.items()})}")
    assert not bad, bad
