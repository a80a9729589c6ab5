"""Host half of `features="device"` (reazonspeech_amd/runtime/avsr_features.py) that needs no GPU: the option and its environment
default, the pieces factored out of feature_extraction.py (mel matrix, alignment expression, crop window) against inlined copies of
what the host path did before, the grey-level table against `_transform`, `plan()` against the host path, and the exported symbols."""
import ctypes
import os

import numpy as np
import pytest

from reazonspeech_amd.avsr import AVHubertFeatureExtractor, AVHubertProcessor
from reazonspeech_amd.avsr import feature_extraction as fx
from reazonspeech_amd.runtime import avsr_features as af

ALIGN_CASES = [(12, 12), (13, 12), (5, 12), (30, 7)]         # (n_v, Ta)
SIZES = [(88, 88), (96, 96), (89, 91), (100, 120)]            # (H, W)


def logfbank_as_it_was(signal, samplerate=16000, winlen=0.025, winstep=0.01, nfilt=26, nfft=512, preemph=0.97):
    """`feature_extraction.logfbank` before the mel matrix was factored out, copied whole"""
    def hz2mel(hz):
        return 2595.0 * np.log10(1.0 + hz / 700.0)

    def mel2hz(mel):
        return 700.0 * (10.0 ** (mel / 2595.0) - 1.0)

    signal = np.asarray(signal, dtype=np.float64)
    signal = np.append(signal[0], signal[1:] - preemph * signal[:-1])
    flen, fstep = int(round(winlen * samplerate)), int(round(winstep * samplerate))
    n = len(signal)
    frames = 1 if n <= flen else 1 + int(np.ceil((n - flen) / fstep))
    padded = np.concatenate([signal, np.zeros(((frames - 1) * fstep + flen - n,))])
    idx = np.arange(flen)[None, :] + (np.arange(frames) * fstep)[:, None]
    pspec = np.square(np.abs(np.fft.rfft(padded[idx], nfft))) / nfft
    melpoints = np.linspace(hz2mel(0.0), hz2mel(samplerate / 2.0), nfilt + 2)
    bins = np.floor((nfft + 1) * mel2hz(melpoints) / samplerate)
    fb = np.zeros((nfilt, nfft // 2 + 1))
    for j in range(nfilt):
        for i in range(int(bins[j]), int(bins[j + 1])):
            fb[j, i] = (i - bins[j]) / (bins[j + 1] - bins[j])
        for i in range(int(bins[j + 1]), int(bins[j + 2])):
            fb[j, i] = (bins[j + 2] - i) / (bins[j + 2] - bins[j + 1])
    feat = pspec @ fb.T
    return np.log(np.where(feat == 0, np.finfo(float).eps, feat))


def test_features_option_and_environment_default(monkeypatch, tmp_path):
    monkeypatch.delenv("REAZONSPEECH_AVSR_FEATURES", raising=False)
    assert AVHubertFeatureExtractor().features == "host"
    assert AVHubertFeatureExtractor(features="device").features == "device"
    assert AVHubertFeatureExtractor(features="device", device="cuda:0").device == "cuda:0"
    monkeypatch.setenv("REAZONSPEECH_AVSR_FEATURES", "device")
    assert AVHubertFeatureExtractor().features == "device"
    assert AVHubertFeatureExtractor(features="host").features == "host"          # the argument wins
    monkeypatch.setenv("REAZONSPEECH_AVSR_FEATURES", "")
    assert AVHubertFeatureExtractor().features == "host"                          # an empty variable is an unset one
    monkeypatch.setenv("REAZONSPEECH_AVSR_FEATURES", "gpu")
    with pytest.raises(ValueError):
        AVHubertFeatureExtractor()
    monkeypatch.delenv("REAZONSPEECH_AVSR_FEATURES")
    with pytest.raises(ValueError):
        AVHubertFeatureExtractor(features="cuda")
    fe = AVHubertFeatureExtractor()
    fe.features = "nowhere"                                                        # changed later: checked when it is used
    with pytest.raises(ValueError):
        fe(raw_audio=np.zeros(800, np.float32), raw_video=np.zeros((2, 88, 88), np.uint8))
    fe.features = "host"
    assert isinstance(fe(raw_audio=np.zeros(800, np.float32), raw_video=np.zeros((2, 88, 88), np.uint8))["input_values"], np.ndarray)
    (tmp_path / "preprocessor_config.json").write_text('{"stack_order_audio": 4, "image_crop_size": 88}', encoding="utf-8")
    assert AVHubertFeatureExtractor.from_pretrained(str(tmp_path), features="device").features == "device"
    assert AVHubertFeatureExtractor.from_pretrained(str(tmp_path)).features == "host"


def test_processor_passes_features_through(monkeypatch, tmp_path):
    from test_avsr_host import make_processor_dir
    monkeypatch.delenv("REAZONSPEECH_AVSR_FEATURES", raising=False)
    make_processor_dir(str(tmp_path))
    assert AVHubertProcessor.from_pretrained(str(tmp_path), features="device").feature_extractor.features == "device"
    assert AVHubertProcessor.from_pretrained(str(tmp_path)).feature_extractor.features == "host"


def test_device_path_refuses_files_and_mouth_extraction_like_the_host_path():
    """raised before any device work: needs no GPU"""
    fe = AVHubertFeatureExtractor(features="device")
    with pytest.raises(RuntimeError, match="librosa"):
        fe(raw_audio="clip.wav", raw_video=np.zeros((2, 88, 88), np.uint8))
    with pytest.raises(RuntimeError, match="mediapipe"):
        fe(raw_audio=np.zeros(800, np.float32), raw_video="clip.mp4")
    with pytest.raises(RuntimeError, match="mediapipe"):
        fe(raw_audio=np.zeros(800, np.float32), raw_video=np.zeros((2, 88, 88), np.uint8), extract_mouth=True)


def test_factored_mel_matrix_leaves_logfbank_unchanged():
    x = (0.1 * np.random.default_rng(11).standard_normal(4321)).astype(np.float32)
    got, want = fx.logfbank(x), logfbank_as_it_was(x)
    assert got.dtype == np.float64 and got.shape == want.shape == (26, 26)
    assert np.array_equal(got, want)
    assert af.mel_matrix().shape == (26, 257)


def test_mel_table_is_the_mel_matrix_banded():
    tw, idx, w = af.mel_table()
    fb = af.mel_matrix()
    dense = np.zeros_like(fb)
    for m in range(26):
        k0, cnt = idx[m]
        assert 0 <= k0 and k0 + cnt <= 257 and 0 < cnt <= af.FB_MAXW
        dense[m, k0:k0 + cnt] = w[m, :cnt]
        assert not w[m, cnt:].any()
    assert np.array_equal(dense, fb.astype(np.float32))
    j = np.arange(256)
    assert np.allclose(tw[:, 0] + 1j * tw[:, 1], np.exp(-2j * np.pi * j / 512), atol=1e-7)


def test_lut_is_transform_of_every_grey_level():
    for mean, std, crop in [(fx.IMAGE_MEAN, fx.IMAGE_STD, 88), (0.5, 0.25, 4), (0.0, 1.0, 88)]:
        fe = AVHubertFeatureExtractor(image_mean=mean, image_std=std, image_crop_size=crop)
        frames = np.broadcast_to(np.arange(256, dtype=np.uint8)[:, None, None, None], (256, 1, crop, crop))
        want = fe._transform(frames).astype(np.float32)
        lut = af.pixel_lut(mean, std)
        assert lut.dtype == np.float32 and lut.shape == (256,)
        assert np.array_equal(lut.view(np.int32), want[:, 0, 0, 0].view(np.int32))
        assert np.array_equal(np.broadcast_to(lut[:, None, None, None], want.shape), want)


def audio_of_rows(rows, rng):
    """a clip that stacks to exactly `rows` rows: 4 * rows frames"""
    return (0.1 * rng.standard_normal(400 + 160 * (4 * rows - 1))).astype(np.float32)


@pytest.mark.parametrize("n_v,Ta", ALIGN_CASES)
@pytest.mark.parametrize("H,W", SIZES)
def test_plan_frame_idx_and_crop_window_are_the_host_paths(n_v, Ta, H, W):
    """every source frame is one grey level and every row / column of the frame is marked, so the host path's `pixel_values` name
    the frame it gathered and the window it cut"""
    rng = np.random.default_rng(n_v * 1000 + Ta)
    fe = AVHubertFeatureExtractor()
    audio = audio_of_rows(Ta, rng)
    video = np.zeros((n_v, H, W), np.uint8)
    video += (np.arange(n_v, dtype=np.uint8) * 3)[:, None, None]
    host = fe(raw_audio=audio, raw_video=video)
    assert host["pixel_values"].shape == (1, Ta, 1, 88, 88)
    p = af.plan(fe, [audio], [video])
    assert (p.B, p.T, p.T_out, len(p.groups)) == (1, Ta, Ta, 1)
    g = p.groups[0]
    assert (g.H, g.W, g.channels, g.n_frames) == (H, W, 1, n_v)
    assert g.frame_idx.dtype == np.int32 and g.frame_idx.shape == (1, Ta)
    # the frame: which grey level the host path shows at each row
    lut = af.pixel_lut(fe.image_mean, fe.image_std)
    assert np.array_equal(lut[video[g.frame_idx[0], 0, 0]], host["pixel_values"][0, :, 0, 0, 0])
    # the window: a frame whose pixels name their own row and column
    marks = np.zeros((1, H, W), np.uint8)
    marks[0] = (np.arange(H)[:, None] * 7 + np.arange(W)[None, :]) % 251
    want = fe._transform(marks[:, None])[0, 0]
    assert np.array_equal(lut[marks[0, g.top:g.top + 88, g.left:g.left + 88]], want.astype(np.float32))
    assert (g.top, g.left) == (int(round((H - 88) / 2.0)), int(round((W - 88) / 2.0)))
    assert np.array_equal(p.padding_mask, host["padding_mask"])


def test_plan_batches_pads_and_groups():
    rng = np.random.default_rng(5)
    fe = AVHubertFeatureExtractor(max_sample_size=6)
    a0, a2 = audio_of_rows(8, rng), audio_of_rows(3, rng)
    v0, v1 = np.zeros((7, 96, 96), np.uint8), np.zeros((5, 90, 100, 3), np.uint8)
    p = af.plan(fe, [a0, None, a2], [v0, v1, None])
    assert (p.B, p.T, p.T_out) == (3, 8, 6)
    assert p.row_len.tolist() == [len(a0), -1, len(a2)] and p.row_off.tolist() == [0, len(a0), len(a0)]
    assert p.padding_mask.shape == (3, 8)                               # the mask keeps length T, like the host path
    assert p.padding_mask.tolist() == [[0] * 8, [0] * 5 + [1] * 3, [0] * 3 + [1] * 5]
    g0, g1 = p.groups
    assert (g0.H, g0.W, g0.channels, g0.n_frames) == (96, 96, 1, 7) and (g1.H, g1.W, g1.channels, g1.n_frames) == (90, 100, 3, 5)
    assert g0.frame_idx[0].tolist() == af.align_index(8, 7)[:6].tolist()
    assert g0.frame_idx[1].tolist() == [-2] * 6 and g0.frame_idx[2].tolist() == [-1] * 6      # the clip without video is written once
    assert g1.frame_idx[1].tolist() == [0, 1, 2, 3, 4, -1]
    assert g1.frame_idx[0].tolist() == [-2] * 6 and g1.frame_idx[2].tolist() == [-2] * 6
    with pytest.raises(ValueError):
        af.plan(AVHubertFeatureExtractor(stack_order_audio=9), [a0], [v0])
    with pytest.raises(ValueError):
        af.plan(AVHubertFeatureExtractor(sr=8000), [a0], [v0])
    with pytest.raises(ValueError):
        af.plan(AVHubertFeatureExtractor(image_crop_size=86), [a0], [v0])


def test_library_exports_the_feature_entry_points():
    from reazonspeech_amd.runtime import capi
    lib = ctypes.CDLL(capi._LIB_PATH)
    for name in ("rs_avsr_logfbank", "rs_avsr_pixels"):
        assert name in capi.EXPORTS and hasattr(lib, name)
    # refused before anything is enqueued (and before the device is touched): needs no GPU
    lib.rs_avsr_logfbank.argtypes = [ctypes.c_int] + [ctypes.c_void_p] * 3 + [ctypes.c_int] * 4 + [ctypes.c_void_p] * 5
    lib.rs_avsr_pixels.argtypes = ([ctypes.c_int, ctypes.c_void_p, ctypes.c_int64] + [ctypes.c_int] * 3 + [ctypes.c_void_p] + [ctypes.c_int] * 6
                                   + [ctypes.c_void_p] * 3)
    buf = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(buf) + 15) & ~15
    logf = lambda B=1, T=4, stack=4, ptr=p: lib.rs_avsr_logfbank(0, ptr, p, p, B, T, stack, 1, p, p, p, p, None)
    assert logf(B=-1) == logf(T=0) == logf(stack=0) == logf(stack=9) == logf(ptr=None) == capi.RS_EINVAL
    assert logf(B=0) == capi.RS_OK
    pix = lambda B=1, T=4, H=96, W=96, ch=1, pitch=4, crop=88, top=4, left=4, ptr=p: lib.rs_avsr_pixels(
        0, ptr, 2, H, W, ch, p, pitch, B, T, crop, top, left, p, p, None)
    for bad in (dict(B=-1), dict(T=0), dict(ch=2), dict(ch=4), dict(pitch=3), dict(top=9), dict(left=9), dict(top=-1), dict(left=-1),
                dict(H=80), dict(W=87), dict(crop=86), dict(crop=0), dict(ptr=None), dict(ptr=p + 1)):
        assert pix(**bad) == capi.RS_EINVAL, bad
    assert pix(B=0) == capi.RS_OK
