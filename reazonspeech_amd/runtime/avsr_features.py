"""The device path of `AVHubertFeatureExtractor` (`features="device"`; rs_avsr_logfbank / rs_avsr_pixels, csrc/k_avsr_features.hip).

`reazonspeech_amd/avsr/feature_extraction.py` makes the encoder's inputs in numpy, one clip at a time: logfbank in float64, the
4-frame stacker and a LayerNorm for the audio; a nearest-frame gather, a centre crop, / 255 and a normalisation into float32 for
the video.  With `features="device"` the raw input goes up instead — one flat float32 buffer of samples and one flat uint8 buffer
of mouth crops per (H, W, channels) group, through pinned memory — and two kernels make the same three tensors on the device.
This module is the host half: what both paths share (the mel matrix, the alignment expression, the crop window), `plan()` (every
table and index the kernels are handed), the ctypes calls and `extract_batch()`.

Pinned to THIS repository's host path, which stays as it is: `pixel_values` is the host path's to the last bit (the grey-level
table is evaluated with its numpy float32 operations), `input_values` is the same algorithm in float32 where the host path runs
logfbank in float64 (tests/test_gpu_avsr_features.py bounds the difference by the float32 evaluation on the CPU).  ADVICE.md
finding 4: the reference's python_speech_features applies the pre-emphasis in float32 and the host path in float64; the device
path does not take a side of its own — its yardstick is the host path."""
import collections
import functools
import os
import warnings

import numpy as np

FEATURE_MODES = ("host", "device")
NFILT, NFFT, WINLEN, WINSTEP, SAMPLERATE = 26, 512, 400, 160, 16000
FB_MAXW = 48                    # columns of the banded filter table (include/rs_asr.h: RS_AVSR_FBANK_MAXW); the widest filter has 47 taps
MAX_STACK = 8

FeaturePlan = collections.namedtuple(
    "FeaturePlan", "B T T_out stack normalize crop audio row_off row_len groups padding_mask lut")
VideoGroup = collections.namedtuple("VideoGroup", "H W channels top left frames n_frames frame_idx")


def resolve_features(features):
    """features: None ($REAZONSPEECH_AVSR_FEATURES, default "host") | "host" | "device" — where AVHubertFeatureExtractor computes"""
    features = features or os.environ.get("REAZONSPEECH_AVSR_FEATURES") or "host"          # an empty variable is an unset one
    if features not in FEATURE_MODES:
        raise ValueError(f"features={features!r}: one of {FEATURE_MODES}")
    return features


# ---- what the host path and the device path both call ----------------------------------------------------------------------------
def _hz2mel(hz):
    return 2595.0 * np.log10(1.0 + hz / 700.0)


def _mel2hz(mel):
    return 700.0 * (10.0 ** (mel / 2595.0) - 1.0)


def mel_matrix(samplerate=SAMPLERATE, nfilt=NFILT, nfft=NFFT):
    """[UPSTREAM] python_speech_features.get_filterbanks: `nfilt` triangular filters spaced on the 2595 log10(1 + f / 700) mel scale
    between 0 and sr / 2 with FFT-bin edges floor((nfft + 1) f / sr) -> float64 [nfilt][nfft / 2 + 1]"""
    melpoints = np.linspace(_hz2mel(0.0), _hz2mel(samplerate / 2.0), nfilt + 2)
    bins = np.floor((nfft + 1) * _mel2hz(melpoints) / samplerate)
    fb = np.zeros((nfilt, nfft // 2 + 1))
    for j in range(nfilt):
        for i in range(int(bins[j]), int(bins[j + 1])):
            fb[j, i] = (i - bins[j]) / (bins[j + 1] - bins[j])
        for i in range(int(bins[j + 1]), int(bins[j + 2])):
            fb[j, i] = (bins[j + 2] - i) / (bins[j + 2] - bins[j + 1])
    return fb


def align_index(n_audio, n_video):
    """feature_extraction_avhubert.py:139-158: the video frame shown at each of `n_audio` stacked audio rows, nearest-frame, in the
    reference's float32 arithmetic -> int64 [n_audio]"""
    n_audio, n_video = int(n_audio), int(n_video)
    return np.minimum(np.floor(np.arange(n_audio, dtype=np.float32) * n_video / n_audio), n_video - 1).astype(np.int64)


def crop_window(h, w, crop):
    """CenterCrop's (top, left): Python's round, so an odd margin rounds half to even"""
    return int(round((h - crop) / 2.0)), int(round((w - crop) / 2.0))


def n_frames(n, winlen=WINLEN, winstep=WINSTEP):
    """frames logfbank makes of `n` samples"""
    return 1 if n <= winlen else 1 + -(-(n - winlen) // winstep)


# ---- tables ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def mel_table():
    """-> (twiddle f32[256][2] = (cos, -sin)(2 pi j / 512), fb_idx i32[26][2] = (first bin, taps), fb_w f32[26][FB_MAXW]): the mel
    matrix banded — every filter is one run of non-zero taps — and the transform's twiddles, as rs_avsr_logfbank reads them"""
    fb = mel_matrix()
    idx = np.zeros((NFILT, 2), np.int32)
    w = np.zeros((NFILT, FB_MAXW), np.float32)
    for m in range(NFILT):
        nz = np.flatnonzero(fb[m])
        k0, cnt = (int(nz[0]), int(nz[-1] - nz[0] + 1)) if len(nz) else (0, 0)
        assert cnt <= FB_MAXW
        idx[m] = k0, cnt
        w[m, :cnt] = fb[m, k0:k0 + cnt]
    ang = 2.0 * np.pi * np.arange(NFFT // 2) / NFFT
    tw = np.stack([np.cos(ang), -np.sin(ang)], axis=1).astype(np.float32)
    for t in (tw, idx, w):
        t.setflags(write=False)
    return tw, idx, w


def pixel_lut(image_mean, image_std):
    """lut[u] = what `_transform` makes of the uint8 grey level u, with its numpy float32 operations -> float32 [256]"""
    x = np.arange(256, dtype=np.uint8).astype(np.float32)
    x = x / 255.0
    return ((x - image_mean) / image_std).astype(np.float32)


# ---- plan -----------------------------------------------------------------------------------------------------------------------
def is_device_video(v):
    """uint8 frames [T][H][W] or [T][H][W][3]: what rs_avsr_pixels reads (anything else is not divided by 255 by the reference,
    or is no array of frames at all: the host path decides)"""
    return isinstance(v, np.ndarray) and v.dtype == np.uint8 and v.ndim in (3, 4) and (v.ndim == 3 or v.shape[3] == 3)


def plan(fe, raw_audio, raw_video):
    """Everything the two launches are handed, for lists of decoded clips (`None` = the modality is missing):
      audio [sum n] float32 + row_off / row_len (-1: no audio);  T = the longest clip in stacked rows, T_out = min(T, max_sample_size);
      per (H, W, channels) group: the crop window, its clips' uint8 frames (a list, concatenated by the caller into the pinned
      buffer), and frame_idx int32 [B][T_out] into them (-1 padding / no video, -2 a clip of another group);
      padding_mask float32 [B][T] (it keeps length T under max_sample_size, like the host path); lut float32 [256]."""
    stack, crop = int(fe.stack_order_audio), int(fe.image_crop_size)
    if not 1 <= stack <= MAX_STACK:
        raise ValueError(f"features='device': stack_order_audio={stack} outside 1..{MAX_STACK}")
    if crop < 4 or crop % 4:
        raise ValueError(f"features='device': image_crop_size={crop} is no positive multiple of 4 (the model takes multiples of 8)")
    if int(fe.sr) != SAMPLERATE:
        raise ValueError(f"features='device': the kernel is built for sr={SAMPLERATE} (25 ms / 10 ms = {WINLEN} / {WINSTEP} samples), got sr={fe.sr}")
    B = len(raw_audio)
    assert len(raw_video) == B
    audio, rows, row_len = [], [], []
    for a, v in zip(raw_audio, raw_video):
        assert a is not None or v is not None
        if a is None:
            row_len.append(-1)
            rows.append(len(v))
            continue
        a = np.ascontiguousarray(a, dtype=np.float32)
        if a.ndim != 1 or len(a) < 1:
            raise ValueError(f"raw_audio must be a non-empty 1-D array of samples, got shape {a.shape}")
        audio.append(a)
        row_len.append(len(a))
        rows.append(-(-n_frames(len(a)) // stack))
    T = max(rows)
    T_out = min(T, int(fe.max_sample_size)) if fe.max_sample_size else T
    row_off = np.zeros((B,), np.int64)
    pos = 0
    for b in range(B):
        row_off[b] = pos
        pos += max(row_len[b], 0)
    keys = {}
    for b, v in enumerate(raw_video):
        if v is not None:
            keys.setdefault((v.shape[1], v.shape[2], 3 if v.ndim == 4 else 1), []).append(b)
    if not keys:                                                        # no clip has video: one launch that writes lut[0] everywhere
        keys[(crop, crop, 1)] = []
    groups = []
    for gi, ((H, W, ch), members) in enumerate(keys.items()):
        if crop > H or crop > W:
            raise ValueError(f"image_crop_size={crop} does not fit the {H} x {W} frames")
        top, left = crop_window(H, W, crop)
        idx = np.full((B, T_out), -2, np.int32)
        if gi == 0:
            idx[[b for b in range(B) if raw_video[b] is None]] = -1
        base, frames = 0, []
        for b in members:
            n_v, n_a = len(raw_video[b]), rows[b]
            if n_v < 1:
                raise ValueError("raw_video must hold at least one frame")
            src = align_index(n_a, n_v) if n_a != n_v else np.arange(n_a, dtype=np.int64)
            row = np.full((T,), -1, np.int64)
            row[:n_a] = src + base
            idx[b] = row[:T_out]
            frames.append(raw_video[b])
            base += n_v
        groups.append(VideoGroup(H, W, ch, top, left, frames, base, idx))
    mask = np.zeros((B, T), np.float32)
    for b in range(B):
        mask[b, rows[b]:] = 1.0
    return FeaturePlan(B, T, T_out, stack, bool(fe.normalize), crop, audio, row_off, np.asarray(row_len, np.int32), groups, mask,
                       pixel_lut(fe.image_mean, fe.image_std))


# ---- the calls ------------------------------------------------------------------------------------------------------------------
def _check(rc, what, detail):
    from . import capi
    if rc != capi.RS_OK:
        raise capi.RsError(rc, f"{what}: {detail}")


def logfbank(device_index, audio, row_off, row_len, B, T, stack, normalize, twiddle, fb_idx, fb_w, out, stream):
    """rs_avsr_logfbank (include/rs_asr.h) on torch tensors of one device: -> out f32 [B][T][26 * stack], asynchronous on `stream`"""
    from . import capi
    from ctypes import c_void_p
    rc = capi.load().rs_avsr_logfbank(int(device_index), capi._ptr(audio), capi._ptr(row_off), capi._ptr(row_len), int(B), int(T), int(stack),
                                      int(bool(normalize)), capi._ptr(twiddle), capi._ptr(fb_idx), capi._ptr(fb_w), capi._ptr(out), c_void_p(stream))
    _check(rc, "rs_avsr_logfbank", f"B={B} T={T} stack={stack}")


def pixels(device_index, frames, n_frames, H, W, channels, frame_idx, idx_pitch, B, T, crop, top, left, lut, out, stream):
    """rs_avsr_pixels (include/rs_asr.h): -> out f32 [B][T][crop][crop], asynchronous on `stream`"""
    from . import capi
    from ctypes import c_void_p
    rc = capi.load().rs_avsr_pixels(int(device_index), capi._ptr(frames), int(n_frames), int(H), int(W), int(channels), capi._ptr(frame_idx),
                                    int(idx_pitch), int(B), int(T), int(crop), int(top), int(left), capi._ptr(lut), capi._ptr(out), c_void_p(stream))
    _check(rc, "rs_avsr_pixels", f"B={B} T={T} frames {n_frames} x {H} x {W} x {channels}, crop {crop} at ({top}, {left}), pitch {idx_pitch}")


_tables = {}


def device_tables(device):
    """the mel table on `device` (made once per device)"""
    import torch
    key = str(device)
    if key not in _tables:
        _tables[key] = tuple(torch.from_numpy(np.array(t)).to(device) for t in mel_table())
    return _tables[key]


def _pinned(torch, arrays, dtype, np_dtype):
    """1-D arrays back to back in one pinned buffer (at least four elements, so that a batch without any still has an address)"""
    n = sum(a.size for a in arrays)
    buf = torch.empty((max(n, 4),), dtype=dtype, pin_memory=True)
    host = buf.numpy()
    pos = 0
    for a in arrays:
        host[pos:pos + a.size] = np.asarray(a, dtype=np_dtype).reshape(-1)
        pos += a.size
    if pos < host.size:
        host[pos:] = 0
    return buf


def extract_batch(fe, raw_audio, raw_video, device="cuda"):
    """`AVHubertFeatureExtractor.__call__` for lists of decoded clips on the device -> {"input_values" f32 [B][T'][26 * stack],
    "pixel_values" f32 [B][T'][1][crop][crop], "padding_mask" f32 [B][T]} as torch tensors on `device`, T' = min(T, max_sample_size).
    A batch with video frames that are not uint8, or a crop size that is no multiple of 4, goes through the host path as a whole
    (one warning) and is uploaded."""
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("features='device' needs a ROCm GPU (MI355X / gfx950): torch.cuda.is_available() is False")
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"device {device!r}: only ROCm ('cuda[:N]') devices are supported")
    index = device.index if device.index is not None else torch.cuda.current_device()
    device = torch.device("cuda", index)
    raw_video = [None if v is None else np.asarray(v) for v in raw_video]
    why = None
    if any(v is not None and not is_device_video(v) for v in raw_video):
        why = "the batch holds video frames that are not uint8 [T][H][W] / [T][H][W][3] (the reference does not scale them by 1 / 255)"
    elif int(fe.image_crop_size) < 4 or int(fe.image_crop_size) % 4:
        why = f"image_crop_size={fe.image_crop_size} is no multiple of 4 (rs_avsr_pixels stores four pixels of a row at once)"
    if why:
        warnings.warn(f"features='device': {why}; the whole batch is extracted on the host", RuntimeWarning, stacklevel=3)
        host = fe._extract_host(raw_audio, raw_video, False)
        return {k: torch.from_numpy(np.ascontiguousarray(v)).to(device) for k, v in host.items()}
    p = plan(fe, raw_audio, raw_video)
    F = NFILT * p.stack
    with torch.cuda.device(device):
        stream = torch.cuda.current_stream().cuda_stream
        tw, fb_idx, fb_w = device_tables(device)
        audio = _pinned(torch, p.audio, torch.float32, np.float32).to(device, non_blocking=True)
        meta = np.concatenate([p.row_len.reshape(-1)] + [g.frame_idx.reshape(-1) for g in p.groups]).astype(np.int32)
        meta = _pinned(torch, [meta], torch.int32, np.int32).to(device, non_blocking=True)
        row_off = _pinned(torch, [p.row_off], torch.int64, np.int64).to(device, non_blocking=True)
        small = _pinned(torch, [p.lut, p.padding_mask], torch.float32, np.float32).to(device, non_blocking=True)
        lut, mask = small[:256], small[256:256 + p.B * p.T].view(p.B, p.T)
        iv = torch.empty((p.B, p.T_out, F), dtype=torch.float32, device=device)
        pv = torch.empty((p.B, p.T_out, 1, p.crop, p.crop), dtype=torch.float32, device=device)
        logfbank(index, audio, row_off, meta[:p.B], p.B, p.T_out, p.stack, p.normalize, tw, fb_idx, fb_w, iv, stream)
        at = p.B
        for g in p.groups:
            frames = _pinned(torch, g.frames, torch.uint8, np.uint8).to(device, non_blocking=True)
            idx = meta[at:at + p.B * p.T_out]
            at += p.B * p.T_out
            pixels(index, frames, g.n_frames, g.H, g.W, g.channels, idx, p.T_out, p.B, p.T_out, p.crop, g.top, g.left, lut, pv, stream)
    return {"input_values": iv, "pixel_values": pv, "padding_mask": mask}
