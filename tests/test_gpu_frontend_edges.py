"""-m gpu: rs_frontend_logmel (csrc/k_frontend.hip: logmel_kernel kinds 0 / 1 / 2, feat_normalize_kernel, feat_mvn_kernel) called at
the ABI on the utterance lengths where its per-utterance logic changes, against the float64 references of tests/frontend_ref.py.

One ragged batch per kind (one launch), every row once more alone in a buffer of its own frame count.  Audio is
0.1 * standard_normal with a fixed seed; the unused tail of every audio row holds NaN, the outputs are NaN-filled and have
sentinels behind them (features, workspace, n_frames), checked after every launch.

Lengths in samples
  kind 0 (NeMo, n = L // 160)       0 1 159 160 161 319 320 400 | 2559 2560 2561 2719 2720 (15 | 16 | 17 frames: 16 per workgroup, 4 per
                                    wave, transformed in pairs) | 5119 5120 5280 (31 | 32 | 33) | 8160 (51: the normaliser's row groups,
                                    RG = 1000 / 20 = 50, take a second pass) | 33600 (210) | 480000 (3000: float32 statistics of a long sum)
  kind 0, pad_left = pad_right = 8000   0 1 159 160 161 2560 2561: bit-identical to the rows padded on the host and run with pad 0
  kind 1 (ESPnet, n = 1 + L // 128) compared: 257 258 383 384 511 512 1919 1920 1921 2047 2048 4095 4096 26000
                                    not compared: 1 2 128 255 256 — torch refuses to reflect-pad 256 samples onto these, so the
                                    reference has no answer; what the device computes there is THE KERNEL'S OWN RULE (reflect once about
                                    each end, then clamp to sample 0).  Asserted for them: frame count, finite values, zeros past the valid
                                    frames, the same bits alone and in the batch.
  kind 2 (kaldi, n = (L + 80) // 160)   1 79 (no frame) 80 81 100 200 239 240 241 399 400 401 2479 2480 2481 2639 2640 5200 26000.
                                    The kernel reflects an index at most 8 times.  A frame starts at most 120 samples before the signal
                                    and ends at most 160 (n - 1) + 279 - (L - 1) <= 200 samples past it (160 n <= L + 80); one reflection
                                    turns "d outside one edge" into "d - L outside the other", so ceil(200 / L) reflections suffice: 3 at
                                    L = 80, the shortest signal with a frame, and fewer above — within the 8
                                    (tests/test_frontend_ref_host.py counts them with the reference's loop-to-convergence).

Per row: n_frames equals the formula; frames past it are exactly 0; the row alone equals the row in the batch bit for bit; kind 0
with exactly one frame is all zeros (feat_normalize_kernel's documented deviation: the reference's unbiased variance is 0 / 0 = NaN);
every other compared row satisfies
    max |device - ref64| <= max(FACTOR * max |oracle32 - ref64|, 4 * 2^-23 * max |ref64|)
where oracle32 is the project's float32 oracle on that row alone.  FACTOR = 8 is the one tests/test_gpu_avsr_features.py states
for the same 8 x 8 x 8 transform (k_fft512.h) against pocketfft's summation order and logf against libm's log; the second term
keeps a row whose oracle happens to be exact (the all-zero rows: log(guard)) at four float32 roundings of the largest value.
One all-zero row per kind: kinds 1 and 2 are held to the same bound (every value is log(guard), normalised for kind 1); for kind 0
only finite values are asserted — every frame is log(2^-24), the deviations from the mean are rounding noise and the reference
divides them by std + 1e-5 = 1e-5, so its own answer is noise times 1e5.
kind 0 once more with t_max = 20 under a 33-frame row: sentinels, zeros and finite values only — nothing is written past t_max.

Measured on an MI355X, max over the compared rows of max |device - ref64| / max |oracle32 - ref64|:
    kind 0  1.31      kind 1  3.23 (errors of 3e-7 .. 1.4e-6 on values of 3: one or two float32 roundings of the log)      kind 2  1.56
"""
import numpy as np
import pytest
import torch

import frontend_ref as fr
from oracle import espnet as oe, model as om, zipformer as oz
from reazonspeech_amd.runtime.config import ESPNET_TINY, TINY
from reazonspeech_amd.runtime.k2_config import ZIPFORMER_TINY
from reazonspeech_amd.runtime.k2_weights import synthetic_state_dict_k2
from reazonspeech_amd.runtime.model import AsrModel
from reazonspeech_amd.runtime.weights import synthetic_state_dict
from reazonspeech_amd.runtime.weights_espnet import synthetic_state_dict_espnet

pytestmark = pytest.mark.gpu
FACTOR = 8.0
FLOOR = 4 * 2.0 ** -23
SENTINEL = 64
N_MELS = 80

NEMO = (0, 1, 159, 160, 161, 319, 320, 400, 2559, 2560, 2561, 2719, 2720, 5119, 5120, 5280, 8160, 33600, 480000)
NEMO_PAD = (0, 1, 159, 160, 161, 2560, 2561)
ESPNET = (257, 258, 383, 384, 511, 512, 1919, 1920, 1921, 2047, 2048, 4095, 4096, 26000)
ESPNET_CLAMPED = (1, 2, 128, 255, 256)
KALDI = (1, 79, 80, 81, 100, 200, 239, 240, 241, 399, 400, 401, 2479, 2480, 2481, 2639, 2640, 5200, 26000)
ZERO_ROW = {0: 2560, 1: 1920, 2: 2480}          # samples of the all-zero row of each kind
FRAMES = {0: fr.nemo_frames, 1: fr.espnet_frames, 2: fr.kaldi_frames}


def noise(n, seed):
    return (0.1 * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


def launch(model, rows, pad=0, t_max=None):
    """one rs_frontend_logmel call -> (features float32 [B][t_max][n_mels], n_frames list); the sentinels are checked here"""
    kind = {"nemo": 0, "espnet": 1, "k2": 2}[getattr(model.cfg, "family", "nemo")]
    dev = model.device
    B = len(rows)
    if t_max is None:
        t_max = max(max(FRAMES[kind](len(r) + 2 * pad) for r in rows), 1)
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
    got, got_ws, got_n = feats.cpu().numpy(), ws.cpu().numpy(), n_frames.cpu().numpy()
    assert np.isnan(got[n:]).all(), "written behind the feature buffer"
    assert np.isnan(got_ws[n:]).all(), "written behind the workspace"
    assert (got_n[B:] == -7).all(), "written behind n_frames"
    assert np.isfinite(got[:n]).all(), "a feature inside [B][t_max][n_mels] was left unwritten or is not finite"
    return got[:n].reshape(B, t_max, N_MELS), got_n[:B].tolist()


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


class Kind:
    """a model of one family, its batch run once and every row run alone once"""

    def __init__(self, kind, model, sd, lengths):
        self.kind, self.model, self.sd, self.cfg = kind, model, sd, model.cfg
        self.lengths = list(lengths)
        self.rows = [noise(L, 1000 * kind + i) for i, L in enumerate(self.lengths)] + [np.zeros(ZERO_ROW[kind], np.float32)]
        self.batch, self.n_frames = launch(model, self.rows)
        self.alone = [launch(model, [r]) for r in self.rows]

    def ref64(self, x):
        if self.kind == 0:
            return fr.nemo_logmel(self.cfg, self.sd, x)
        if self.kind == 1:
            return fr.espnet_logmel(self.cfg, self.sd, x)
        return fr.kaldi_fbank(self.cfg, x)

    def oracle32(self, x):
        t = torch.from_numpy(x)
        if self.kind == 0:
            return om.frontend(self.cfg, self.sd, t[None], torch.tensor([len(x)]))[0][0].double().numpy()
        if self.kind == 1:
            return oe.frontend(self.cfg, self.sd, t[None], torch.tensor([len(x)]))[0][0].double().numpy()
        return oz.fbank(self.cfg, t).double().numpy()

    def check_exact(self):
        """frame counts, zeros past them, batch == alone"""
        bad = []
        for b, x in enumerate(self.rows):
            n = FRAMES[self.kind](len(x))
            (alone, n_alone) = self.alone[b]
            if self.n_frames[b] != n or n_alone != [n]:
                bad.append((len(x), "n_frames", self.n_frames[b], n_alone, n))
            if self.batch[b, n:].any() or alone[0, n:].any():
                bad.append((len(x), "frames past n_frames are not zero"))
            if not np.array_equal(bits(self.batch[b, :n]), bits(alone[0, :n])):
                bad.append((len(x), "the row alone differs from the row in the batch", float(np.abs(self.batch[b, :n] - alone[0, :n]).max())))
        assert not bad, bad

    def check_bound(self, rows):
        """rows: indices into self.rows -> worst device / yardstick ratio"""
        bad, worst = [], 0.0
        for b in rows:
            x = self.rows[b]
            ref = self.ref64(x)
            n = ref.shape[0]
            err = np.abs(self.batch[b, :n].astype(np.float64) - ref).max()
            yard = np.abs(self.oracle32(x)[:n] - ref).max()
            floor = FLOOR * np.abs(ref).max()
            ratio = err / yard if yard > 0 else 0.0
            print(f"kind {self.kind} L={len(x)} n={n}: device - ref64 {err:.3e}  oracle32 - ref64 {yard:.3e}  ratio {ratio:.2f}  floor {floor:.3e}"
                  f"{'  (all-zero row)' if not x.any() else ''}")
            worst = max(worst, ratio)
            if not err <= max(FACTOR * yard, floor):
                bad.append((len(x), err, yard, floor))
        print(f"kind {self.kind}: worst ratio {worst:.2f}")
        assert not bad, bad


@pytest.fixture(scope="module")
def nemo(gpu_device):
    sd = synthetic_state_dict(TINY, 3)
    return Kind(0, AsrModel(TINY, sd, None, device="cuda:0", pad_seconds=0.0), sd, NEMO)


@pytest.fixture(scope="module")
def espnet(gpu_device):
    sd = synthetic_state_dict_espnet(ESPNET_TINY, 3)
    return Kind(1, AsrModel(ESPNET_TINY, sd, None, device="cuda:0", pad_seconds=0.0), sd, ESPNET + ESPNET_CLAMPED)


@pytest.fixture(scope="module")
def kaldi(gpu_device):
    sd = synthetic_state_dict_k2(ZIPFORMER_TINY, 3)
    return Kind(2, AsrModel(ZIPFORMER_TINY, sd, None, device="cuda:0", pad_seconds=0.0), sd, KALDI)


# ---- kind 0 ---------------------------------------------------------------------------------------------------------------------
def test_nemo_frame_counts_zeros_and_batch_bits(nemo):
    nemo.check_exact()


def test_nemo_one_frame_is_all_zeros(nemo):
    for b, L in enumerate(nemo.lengths):
        if L // 160 == 1:
            assert not nemo.batch[b].any() and not nemo.alone[b][0].any(), L


def test_nemo_within_the_float32_yardstick(nemo):
    nemo.check_bound([b for b, L in enumerate(nemo.lengths) if L // 160 >= 2])


def test_nemo_all_zero_row_is_finite(nemo):
    """every frame is log(2^-24): the reference divides rounding noise by std + eps = 1e-5, so only finite values are asserted
    (`launch` asserts them for the whole buffer; here the row is shown to be what it is)"""
    b = len(nemo.lengths)
    assert nemo.n_frames[b] == ZERO_ROW[0] // 160 and np.isfinite(nemo.batch[b]).all()


def test_nemo_folded_padding_equals_padding_on_the_host(nemo):
    rows = [noise(L, 2000 + i) for i, L in enumerate(NEMO_PAD)]
    folded, n_folded = launch(nemo.model, rows, pad=8000)
    padded, n_padded = launch(nemo.model, [np.pad(r, 8000) for r in rows])
    assert n_folded == n_padded == [(L + 16000) // 160 for L in NEMO_PAD]
    assert folded.shape == padded.shape
    for b, L in enumerate(NEMO_PAD):
        assert np.array_equal(bits(folded[b]), bits(padded[b])), L


def test_nemo_nothing_is_written_past_t_max(nemo):
    """t_max = 20 under rows of 33, 16, 17, 1 and 0 frames: the sentinels behind the features and the workspace, finite values (all
    asserted in `launch`) and zeros past min(n, t_max)"""
    lengths = (5280, 2560, 2720, 161, 0)
    got, _ = launch(nemo.model, [noise(L, 3000 + i) for i, L in enumerate(lengths)], t_max=20)
    for b, L in enumerate(lengths):
        assert not got[b, min(L // 160, 20):].any(), L


# ---- kind 1 ---------------------------------------------------------------------------------------------------------------------
def test_espnet_frame_counts_zeros_and_batch_bits(espnet):
    espnet.check_exact()


def test_espnet_within_the_float32_yardstick(espnet):
    espnet.check_bound([b for b, L in enumerate(espnet.lengths) if L > 256] + [len(espnet.lengths)])


# ---- kind 2 ---------------------------------------------------------------------------------------------------------------------
def test_kaldi_frame_counts_zeros_and_batch_bits(kaldi):
    kaldi.check_exact()
    assert kaldi.n_frames[:2] == [0, 0]


def test_kaldi_within_the_float32_yardstick(kaldi):
    kaldi.check_bound([b for b, L in enumerate(kaldi.lengths) if L >= 80] + [len(kaldi.lengths)])
