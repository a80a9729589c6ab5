"""-m gpu: `AVHubertFeatureExtractor(features="device")` — rs_avsr_logfbank / rs_avsr_pixels (csrc/k_avsr_features.hip) against the
host extractor of reazonspeech_amd/avsr/feature_extraction.py.

  video    `pixel_values` equal to the host path's, element for element (np.array_equal): frame sizes with even, odd and
           half-to-even crop margins, more / fewer / as many video frames as audio rows, clips with one modality, ragged batches
           (padding frames hold lut[0]), BGR input, max_sample_size, frame sizes mixed in one batch
  audio    exact: all-zero audio, a batch against its clips alone, NaN-filled output buffers with sentinels behind them
           bounded: noise clips at the lengths where the frame count, the pairing of frames and the stacking change, against the
           host path (logfbank in float64).  The yardstick is the same algorithm evaluated on the CPU in float32 (`cpu32` below:
           float32 pre-emphasis, scipy's single-precision rfft, float32 filter product, log and LayerNorm):
               max |device - host64| <= 8 * max |cpu32 - host64|      per case
           — 8 for the different summation order of the 8 x 8 x 8 transform against pocketfft's and logf against libm's log.
  package  generate() on the device-made tensors == generate() on the same tensors copied to the host as numpy (plumbing, exact)
"""
import numpy as np
import pytest
import scipy.fft
import torch

from reazonspeech_amd.avsr import AVHubertFeatureExtractor, AVHubertProcessor, synthetic_model
from reazonspeech_amd.runtime import avsr_features as af
from reazonspeech_amd.runtime.avsr_config import AVSR_TINY

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [(88, 88), (96, 96), (89, 91), (100, 120)]
BOUNDED_LENGTHS = [1, 400, 401, 560, 561, 400 + 160 * 3, 400 + 160 * 4, 4321]
FACTOR = 8.0


def noise(n, seed):
    return (0.1 * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


def samples_for_rows(rows):
    """samples that stack to exactly `rows` rows (4 * rows frames)"""
    return 400 + 160 * (4 * rows - 1)


def crops(n, H, W, seed, channels=1):
    shape = (n, H, W) if channels == 1 else (n, H, W, 3)
    return np.random.default_rng(seed).integers(0, 256, size=shape, dtype=np.uint8)


def both(raw_audio, raw_video, **kw):
    """-> (host dict of numpy arrays, device dict copied to the host)"""
    host = AVHubertFeatureExtractor(features="host", **kw)(raw_audio=raw_audio, raw_video=raw_video)
    dev = AVHubertFeatureExtractor(features="device", device=DEV, **kw)(raw_audio=raw_audio, raw_video=raw_video)
    for k in ("input_values", "pixel_values", "padding_mask"):
        assert torch.is_tensor(dev[k]) and dev[k].is_cuda and dev[k].dtype == torch.float32, k
        assert tuple(dev[k].shape) == host[k].shape and host[k].dtype == np.float32, (k, tuple(dev[k].shape), host[k].shape)
    return host, {k: v.cpu().numpy() for k, v in dev.items()}


def cpu32(audio, stack=4, normalize=True):
    """`input_values` of one clip by the host path's algorithm with every step in float32"""
    s = np.asarray(audio, np.float32)
    s = np.append(s[0], s[1:] - np.float32(0.97) * s[:-1]).astype(np.float32)
    n = len(s)
    frames = 1 if n <= 400 else 1 + int(np.ceil((n - 400) / 160))
    padded = np.concatenate([s, np.zeros(((frames - 1) * 160 + 400 - n,), np.float32)])
    idx = np.arange(400)[None, :] + (np.arange(frames) * 160)[:, None]
    spec = scipy.fft.rfft(padded[idx], 512)
    assert spec.dtype == np.complex64
    pspec = np.square(np.abs(spec)) / np.float32(512)
    feat = pspec @ af.mel_matrix().astype(np.float32).T
    assert feat.dtype == np.float32
    fb = np.log(np.where(feat == 0, np.float32(np.finfo(float).eps), feat))
    if len(fb) % stack:
        fb = np.concatenate([fb, np.zeros((stack - len(fb) % stack, 26), np.float32)])
    iv = fb.reshape(-1, stack * 26)
    if normalize:
        mu = iv.mean(-1, keepdims=True)
        iv = (iv - mu) / np.sqrt(((iv - mu) ** 2).mean(-1, keepdims=True) + np.float32(1e-5))
    assert iv.dtype == np.float32
    return iv


# ---- video, exact ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", SIZES)
def test_pixels_equal_the_host_paths(H, W):
    """one batch per frame size: as many, more and fewer video frames than audio rows, ragged audio lengths"""
    rows = [6, 5, 3]
    audio = [noise(samples_for_rows(r), 10 + r) for r in rows]
    video = [crops(n_v, H, W, 20 + n_v) for n_v in (6, 9, 2)]
    host, dev = both(audio, video)
    assert dev["pixel_values"].shape == (3, 6, 1, 88, 88)
    assert np.array_equal(dev["pixel_values"], host["pixel_values"])
    assert np.array_equal(dev["padding_mask"], host["padding_mask"])
    lut = af.pixel_lut(0.421, 0.165)
    assert np.all(dev["pixel_values"][1, 5:] == lut[0]) and np.all(dev["pixel_values"][2, 3:] == lut[0])      # padding frames


def test_pixels_single_modality_clips_in_one_batch():
    audio = [noise(samples_for_rows(5), 1), None, noise(samples_for_rows(4), 2)]
    video = [crops(7, 88, 88, 3), crops(6, 88, 88, 4), None]
    host, dev = both(audio, video)
    assert dev["pixel_values"].shape == (3, 6, 1, 88, 88)
    assert np.array_equal(dev["pixel_values"], host["pixel_values"])
    assert np.array_equal(dev["padding_mask"], host["padding_mask"])
    assert not dev["input_values"][1].any() and np.array_equal(dev["input_values"][1], host["input_values"][1])   # no audio: zero rows
    assert np.all(dev["pixel_values"][2] == af.pixel_lut(0.421, 0.165)[0])                                          # no video: grey level 0
    # and a batch without any video, a single clip given without a list
    host, dev = both(noise(2000, 5), None)
    assert np.array_equal(dev["pixel_values"], host["pixel_values"])


@pytest.mark.parametrize("H,W", [(90, 94), (88, 88), (97, 101)])
def test_pixels_bgr_input(H, W):
    """(90, 94): top 1, left 3 — nine bytes into a 32-bit word"""
    audio = [noise(samples_for_rows(4), 7), noise(samples_for_rows(3), 8)]
    video = [crops(5, H, W, 9, channels=3), crops(3, H, W, 10, channels=3)]
    host, dev = both(audio, video)
    assert np.array_equal(dev["pixel_values"], host["pixel_values"])


def test_pixels_bgr_extremes():
    """the fixed-point grey of saturated colours: (255, 255, 255) -> 255 exactly"""
    v = np.zeros((4, 88, 88, 3), np.uint8)
    v[0], v[1, ..., 0], v[2, ..., 1], v[3, ..., 2] = 255, 255, 255, 255
    host, dev = both(None, v)
    assert np.array_equal(dev["pixel_values"], host["pixel_values"])


def test_max_sample_size_smaller_than_t():
    audio = [noise(samples_for_rows(7), 11), noise(samples_for_rows(4), 12)]
    video = [crops(7, 96, 96, 13), crops(5, 96, 96, 14)]
    host, dev = both(audio, video, max_sample_size=5)
    assert dev["pixel_values"].shape == (2, 5, 1, 88, 88) and dev["input_values"].shape == (2, 5, 104)
    assert dev["padding_mask"].shape == (2, 7)                                    # the mask keeps length T
    assert np.array_equal(dev["pixel_values"], host["pixel_values"])
    assert np.array_equal(dev["padding_mask"], host["padding_mask"])


def test_frame_sizes_mixed_in_one_batch():
    """two launches write one `pixel_values`; the host path cannot stack such a batch, so every clip is compared alone"""
    audio = [noise(samples_for_rows(4), 15), noise(samples_for_rows(4), 16), noise(samples_for_rows(2), 17)]
    video = [crops(4, 96, 96, 18), crops(6, 89, 91, 19, channels=3), None]
    dev = AVHubertFeatureExtractor(features="device", device=DEV)(raw_audio=audio, raw_video=video)
    host = AVHubertFeatureExtractor()
    for b in range(3):
        want = host(raw_audio=audio[b], raw_video=video[b])["pixel_values"][0]
        got = dev["pixel_values"][b].cpu().numpy()
        assert np.array_equal(got[:len(want)], want)
        assert np.all(got[len(want):] == af.pixel_lut(0.421, 0.165)[0])


def test_float_frames_fall_back_to_the_host_path_with_one_warning():
    audio = [noise(samples_for_rows(3), 21), noise(samples_for_rows(2), 22)]
    video = [crops(3, 88, 88, 23).astype(np.float32) / 255.0, crops(2, 88, 88, 24)]
    with pytest.warns(RuntimeWarning, match="on the host") as rec:
        dev = AVHubertFeatureExtractor(features="device", device=DEV)(raw_audio=audio, raw_video=video)
    assert len([w for w in rec if issubclass(w.category, RuntimeWarning)]) == 1
    want = AVHubertFeatureExtractor()(raw_audio=audio, raw_video=video)
    for k in want:
        assert dev[k].is_cuda and np.array_equal(dev[k].cpu().numpy(), want[k])


def test_crop_size_no_multiple_of_four_falls_back_to_the_host_path():
    audio, video = noise(samples_for_rows(3), 25), crops(3, 96, 96, 26)
    want = AVHubertFeatureExtractor(image_crop_size=86)(raw_audio=audio, raw_video=video)
    with pytest.warns(RuntimeWarning, match="on the host"):
        dev = AVHubertFeatureExtractor(features="device", device=DEV, image_crop_size=86)(raw_audio=audio, raw_video=video)
    for k in want:
        assert dev[k].is_cuda and np.array_equal(dev[k].cpu().numpy(), want[k])


# ---- audio, exact ---------------------------------------------------------------------------------------------------------------
def test_all_zero_audio():
    """5 frames: stacked row 0 is 104 times log(eps) and normalises to exact zeros; row 1 is one frame of log(eps) and 78 zeros.
    Tolerance of the partial row: the mean and the variance are float32 sums of F = 104 terms, each within F * 2^-24 relative to
    the largest term (Higham, Accuracy and Stability, §4.2), in two implementations: 4 * F * 2^-24 * max |row|."""
    n = 400 + 160 * 4
    host, dev = both(np.zeros(n, np.float32), crops(2, 88, 88, 31))
    iv = dev["input_values"][0]
    assert iv.shape == (2, 104)
    assert np.all(iv[0] == 0.0)
    tol = 4 * 104 * 2.0 ** -24 * np.abs(host["input_values"][0, 1]).max()
    print(f"all-zero audio, partial row: max |device - host| {np.abs(iv[1] - host['input_values'][0, 1]).max():.3e} (allowed {tol:.3e})")
    assert np.abs(iv[1] - host["input_values"][0, 1]).max() <= tol
    assert np.all(iv[1, 26:] == iv[1, 26]) and np.all(iv[1, :26] == iv[1, 0])


def test_rows_of_a_batch_are_the_clips_alone_bit_for_bit():
    lens = [4321, 400 + 160 * 4, 16000, 1]
    audio = [noise(n, 40 + i) for i, n in enumerate(lens)]
    video = [crops(3, 88, 88, 50 + i) for i in range(4)]
    fe = AVHubertFeatureExtractor(features="device", device=DEV)
    together = fe(raw_audio=audio, raw_video=video)["input_values"].cpu().numpy()
    assert together.shape == (4, 25, 104)
    for b in range(4):
        alone = fe(raw_audio=audio[b], raw_video=video[b])["input_values"].cpu().numpy()[0]
        assert np.array_equal(together[b, :len(alone)].view(np.int32), alone.view(np.int32)), b
        assert not together[b, len(alone):].any()


def test_outputs_stay_inside_their_buffers():
    """NaN-filled outputs with 64 sentinel floats behind them: every element is written with a finite value, no sentinel is"""
    dev = torch.device(DEV)
    idx = torch.device(DEV).index
    stream = torch.cuda.current_stream(dev).cuda_stream
    tw, fb_idx, fb_w = af.device_tables(dev)
    lens = [4321, 400 + 160 * 4, -1, 401]
    clips = [noise(n, 60 + i) for i, n in enumerate(lens) if n > 0]
    B, T, F = 4, 8, 104                                                  # T = 8 > the longest clip's 7 rows
    audio = torch.from_numpy(np.concatenate(clips)).to(dev)
    off, pos = [], 0
    for n in lens:
        off.append(pos)
        pos += max(n, 0)
    out = torch.full((B * T * F + 64,), float("nan"), device=dev)
    af.logfbank(idx, audio, torch.tensor(off, dtype=torch.int64, device=dev), torch.tensor(lens, dtype=torch.int32, device=dev), B, T, 4, True,
                tw, fb_idx, fb_w, out, stream)
    got = out.cpu().numpy()
    assert np.isfinite(got[:B * T * F]).all() and np.isnan(got[B * T * F:]).all()
    assert not got[:B * T * F].reshape(B, T, F)[2].any()                 # the clip without audio
    crop, H, W = 88, 89, 91
    frames = torch.from_numpy(crops(5, H, W, 70).reshape(-1)).to(dev)
    fidx = torch.tensor([[0, 1, 2, 3, 4, -1, -1, -1], [4, 4, 4, -1, -1, -1, -1, -1], [-1] * 8, [9, 0, 0, 0, 0, 0, 0, 0]], dtype=torch.int32, device=dev)
    lut = torch.from_numpy(af.pixel_lut(0.421, 0.165)).to(dev)
    n = B * T * crop * crop
    pout = torch.full((n + 64,), float("nan"), device=dev)
    top, left = af.crop_window(H, W, crop)
    af.pixels(idx, frames, 5, H, W, 1, fidx, 8, B, T, crop, top, left, lut, pout, stream)
    got = pout.cpu().numpy()
    assert np.isfinite(got[:n]).all() and np.isnan(got[n:]).all()
    assert np.all(got[:n].reshape(B, T, -1)[3, 0] == af.pixel_lut(0.421, 0.165)[0])     # an index past the last frame reads as grey level 0


# ---- audio, bounded -------------------------------------------------------------------------------------------------------------
def bounded_case(n, normalize=True):
    """-> (max, rms of device - host64, max, rms of cpu32 - host64)"""
    x = noise(n, 1000 + n)
    host, dev = both(x, None, normalize=normalize)
    h64, d = host["input_values"][0].astype(np.float64), dev["input_values"][0].astype(np.float64)
    c = cpu32(x, normalize=normalize).astype(np.float64)
    assert d.shape == h64.shape == c.shape
    ed, ec = d - h64, c - h64
    return np.abs(ed).max(), np.sqrt(np.mean(ed ** 2)), np.abs(ec).max(), np.sqrt(np.mean(ec ** 2))


@pytest.mark.parametrize("n", BOUNDED_LENGTHS)
def test_logfbank_within_the_float32_yardstick(n):
    dmax, drms, cmax, crms = bounded_case(n)
    print(f"n={n}: device - host64 max {dmax:.3e} rms {drms:.3e};  cpu32 - host64 max {cmax:.3e} rms {crms:.3e};  ratio {dmax / cmax if cmax else float('inf'):.2f}")
    assert dmax <= FACTOR * cmax


def test_logfbank_without_layernorm_within_the_float32_yardstick():
    dmax, drms, cmax, crms = bounded_case(4321, normalize=False)
    print(f"n=4321, normalize=False: device - host64 max {dmax:.3e} rms {drms:.3e};  cpu32 - host64 max {cmax:.3e} rms {crms:.3e}")
    assert dmax <= FACTOR * cmax


# ---- through the package ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def package_inputs():
    rows = [21, 13, 8]
    audio = [noise(samples_for_rows(r) - 37 * i, 80 + i) for i, r in enumerate(rows)]
    video = [crops(n_v, 96, 96, 90 + i) for i, n_v in enumerate((20, 13, 9))]
    proc = AVHubertProcessor(AVHubertFeatureExtractor(features="device", device=DEV))
    dev = proc(raw_audio=audio, raw_video=video)
    host = AVHubertProcessor(AVHubertFeatureExtractor())(raw_audio=audio, raw_video=video)
    return dev, host


def test_extractor_outputs_have_the_host_paths_shapes(package_inputs):
    dev, host = package_inputs
    assert set(dev) == set(host) == {"input_values", "pixel_values", "padding_mask"}
    for k in host:
        assert tuple(dev[k].shape) == host[k].shape and dev[k].dtype == torch.float32 and host[k].dtype == np.float32 and dev[k].is_cuda
    assert dev["input_values"].shape == (3, 21, 104) and dev["pixel_values"].shape == (3, 21, 1, 88, 88)


@pytest.mark.parametrize("search", ["host", "device"])
def test_generate_takes_the_device_tensors(package_inputs, search):
    dev, _ = package_inputs
    model = synthetic_model(AVSR_TINY, seed=3, device=DEV, search=search)
    as_numpy = {k: v.cpu().numpy() for k, v in dev.items()}
    for beams in (1, 5):
        got = model.generate(**dev, num_beams=beams, max_new_tokens=12, return_dict_in_generate=True)
        want = model.generate(**as_numpy, num_beams=beams, max_new_tokens=12, return_dict_in_generate=True)
        assert torch.equal(got.sequences, want.sequences), (search, beams)
        if beams > 1:
            assert torch.equal(got.sequences_scores, want.sequences_scores), (search, beams)
    enc_d = model.avhubert(**dev).last_hidden_state
    enc_h = model.avhubert(**as_numpy).last_hidden_state
    assert torch.equal(enc_d, enc_h)
