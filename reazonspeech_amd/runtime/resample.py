"""Filter plans of the device resampler (`load_model(resample="device")`, `AsrModel.resample_batch`, rs_resample).

`norm_audio` (nemo/asr/audio.py) resamples every channel to 16 kHz, then averages the channels — on the host, one utterance at
a time.  `resample="device"` does that work in one HIP kernel per (rate, channel count) group (csrc/k_resample.hip).  This
module is its host half: the polyphase layout of the filter, the closed form of the output in float64 that the tests and
scripts/resample_ab.py compare the kernel with, and the helper through which the three packages normalise their input.

The filter is ALWAYS `audio._hq_filter(up, down)`, the Kaiser-windowed sinc the host path uses when soxr is not installed.  When
soxr IS importable the host path calls soxr instead (it then is the reference's `librosa.resample`), while the device path still
uses this filter: the two options then differ inside soxr's transition band and at the 24-bit level elsewhere (the measured
difference of the two filters: the docstring of nemo/asr/audio.py) instead of at float32 rounding.

Output, exactly (`scipy.signal.resample_poly(x, up, down, window=h)[:n_out]`, checked to zero difference in float64):
    n_out = ceil(L * up / down)                                    (integer arithmetic)
    y[n]  = sum over 0 <= m < L of x[m] * up * h[half + n * down - m * up]        for tap indices inside [0, numtaps)
"""
import collections
import functools
import warnings
from fractions import Fraction

import numpy as np

SAMPLERATE = 16000
RESAMPLE_MODES = ("host", "device")
MAX_TAPS = 1 << 24              # a rate whose filter is longer is resampled on the host (with a warning)
KERNEL_WINDOW = 16384           # float32 samples of LDS one workgroup of rs_resample has for a window (csrc/k_resample.hip: RSMP_LDS_FLOATS)

ResamplePlan = collections.namedtuple("ResamplePlan", "up down numtaps half table")


def check_mode(resample):
    """ValueError for anything but "host" / "device" (needs no GPU: `load_model` calls this before any device work)"""
    if resample not in RESAMPLE_MODES:
        raise ValueError(f"resample must be one of {RESAMPLE_MODES}, got {resample!r}")
    return resample


def ratio(orig_sr, target_sr=SAMPLERATE):
    """(up, down) = the reduced target / orig"""
    r = Fraction(int(target_sr), int(orig_sr))
    return r.numerator, r.denominator


def taps_per_phase(numtaps, up):
    """columns of the phase-major table: ceil(numtaps / up) rounded up to a multiple of 4 (the kernel loads four taps at once)"""
    return (-(-numtaps // up) + 3) // 4 * 4


def n_out(length, up, down):
    """librosa's output length ceil(L * up / down), in integers"""
    return -(-int(length) * int(up) // int(down))


def estimate_taps(up, down):
    """numtaps of `_hq_filter(up, down)` without designing it"""
    from scipy.signal import kaiserord
    from ..nemo.asr.audio import SOXR_HQ_PASSBAND, SOXR_HQ_REJECTION_DB
    nyq = 0.5 / max(up, down)
    return kaiserord(SOXR_HQ_REJECTION_DB, (1.0 - SOXR_HQ_PASSBAND) * nyq / 0.5)[0] | 1


@functools.lru_cache(maxsize=16)
def plan(orig_sr, target_sr=SAMPLERATE):
    """-> ResamplePlan(up, down, numtaps, half, table) of a rate, cached.  up / down = Fraction(target, orig); h =
    `audio._hq_filter(up, down)` (numtaps odd); half = (numtaps - 1) // 2; table = float32(up * h) phase-major:
    table[p][j] = float32(up * h[p + j * up]), shape [up][taps_per_phase(numtaps, up)], zero beyond numtaps.
    Equal rates give the identity plan (1, 1, 1, 0, [[1, 0, 0, 0]]): the kernel then only averages the channels.
    ValueError when the filter would have more than MAX_TAPS taps."""
    up, down = ratio(orig_sr, target_sr)
    if up == down == 1:
        h = np.ones(1)
    else:
        if estimate_taps(up, down) > MAX_TAPS:
            raise ValueError(f"{orig_sr} Hz -> {target_sr} Hz: the filter of the ratio {up}/{down} has more than 2^24 taps")
        from ..nemo.asr.audio import _hq_filter
        h = _hq_filter(up, down)
    numtaps = len(h)
    assert numtaps % 2 == 1
    cols = taps_per_phase(numtaps, up)
    flat = np.zeros(up * cols, np.float32)
    flat[:numtaps] = (up * h).astype(np.float32)
    table = np.ascontiguousarray(flat.reshape(cols, up).T)               # [p][j] = flat[p + j * up]
    table.setflags(write=False)
    return ResamplePlan(up, down, numtaps, (numtaps - 1) // 2, table)


def check_window(pl):
    """ValueError when the samples the 256 outputs of one workgroup reach over (csrc/k_resample.hip: Wi) do not fit KERNEL_WINDOW:
    `resample_batch` then takes the host path instead of launching (rs_resample itself refuses such a plan with RS_EINVAL)"""
    window = 255 * pl.down // pl.up + 2 + pl.table.shape[1]
    if window > KERNEL_WINDOW:
        raise ValueError(f"the ratio {pl.up}/{pl.down} with {pl.numtaps} taps needs a window of {window} samples per workgroup, "
                         f"more than the {KERNEL_WINDOW} the kernel holds")


def pack_rows(waves, channels):
    """rows of one channel count -> (their [channels][L] float32 planes back to back, the rows' offsets, their lengths): rs_resample's
    x, row_off, row_len on the host"""
    lens = [np.asarray(w).shape[-1] for w in waves]
    host = np.empty((max(sum(lens) * channels, 1),), np.float32)
    offs, pos = [], 0
    for w, n in zip(waves, lens):
        offs.append(pos)
        host[pos:pos + n * channels] = np.asarray(w).reshape(-1)
        pos += n * channels
    return host, offs, lens


def reference(x, orig_sr, indices=None, target_sr=SAMPLERATE):
    """The closed form above in float64, with the float32 taps of `plan(orig_sr).table`, for the output indices `indices` (default:
    all n_out of them).  x: [L] or [channels, L]; the channels are averaged (each filtered, then the mean).
    -> (y, mag): y[k] = the output at indices[k]; mag[k] = sum over channels and taps of |tap * sample| / channels, the magnitude
    the rounding-error bound of a float32 evaluation scales with."""
    pl = plan(int(orig_sr), int(target_sr))
    x = np.asarray(x, dtype=np.float64)
    x = x[None, :] if x.ndim == 1 else x
    C, L = x.shape
    total = n_out(L, pl.up, pl.down)
    idx = np.arange(total, dtype=np.int64) if indices is None else np.asarray(indices, dtype=np.int64)
    assert idx.size == 0 or (idx.min() >= 0 and idx.max() < total)
    c = pl.half + idx * pl.down
    p, q = c % pl.up, c // pl.up
    taps = pl.table.astype(np.float64)
    y, mag = np.zeros(len(idx)), np.zeros(len(idx))
    for j in range(pl.table.shape[1]):                                   # tap index p + j * up <-> sample q - j
        m = q - j
        ok = (m >= 0) & (m < L)
        if not ok.any():
            continue
        t = np.where(ok, taps[p, j], 0.0)
        xs = x[:, np.clip(m, 0, max(L - 1, 0))] if L else np.zeros((C, len(idx)))
        y += (t * xs).sum(axis=0) / C
        mag += np.abs(t * xs).sum(axis=0) / C
    return y, mag


def error_bound(y, mag, orig_sr, channels, target_sr=SAMPLERATE):
    """|computed - y| allowed for a float32 evaluation in ANY summation order (Higham, Accuracy and Stability, §3.1 / §4.2: one
    rounding per product and per addition, n_terms = channels * ceil(numtaps / up) terms, two more for the mean) plus the
    rounding of the result: (n_terms + 2) * 2^-24 * mag + 2^-24 * |y|"""
    pl = plan(int(orig_sr), int(target_sr))
    n_terms = channels * -(-pl.numtaps // pl.up)
    return (n_terms + 2) * 2.0 ** -24 * np.asarray(mag) + 2.0 ** -24 * np.abs(y)


def norm_batch(model, audios, norm_audio):
    """What every `norm_audio` call site of the three packages goes through: -> [float32 16 kHz mono waveform] for a list of
    AudioData.  `model.resample == "device"`: ONE `model.resample_batch` call for the whole list; otherwise `norm_audio` (the
    package's own) per item, as before."""
    if getattr(model, "resample", "host") == "device":
        return model.resample_batch([a.waveform for a in audios], [a.samplerate for a in audios])
    return [norm_audio(a).waveform for a in audios]


def host_fallback(waveform, rate, why):
    """one utterance through the host path, said out loud"""
    from ..nemo.asr.audio import norm_audio, AudioData
    warnings.warn(f"resample='device': {why}; this utterance is resampled on the host", RuntimeWarning, stacklevel=3)
    return np.ascontiguousarray(norm_audio(AudioData(np.asarray(waveform), int(rate))).waveform, dtype=np.float32)
