"""float64 restatements of the three log-mel front-ends of csrc/k_frontend.hip (`kind` 0, 1, 2), one utterance per call, plain numpy,
written from the formulas the float32 oracles cite (oracle/model.py frontend, oracle/espnet.py frontend, oracle/zipformer.py fbank)
and calling none of them.  tests/test_frontend_ref_host.py pins them to those oracles and to the committed HF golden;
tests/test_gpu_frontend_edges.py compares the device with them.

The tables (window, mel banks, MVN statistics) and the scalar constants (pre-emphasis, log guard, eps) are the float32 values the
device uploads or takes as kernel arguments, promoted to float64: what is measured against these references is arithmetic, not the
rounding of a table.  (kind 2 takes the oracle's own window and banks, which tests/test_k2_host.py holds to the uploaded ones at
float32 resolution.)
"""
import numpy as np

N_FFT = 512


def _f32(v) -> float:
    """a configuration scalar as the float32 the kernel receives, in float64"""
    return float(np.float32(v))


def _t64(t) -> np.ndarray:
    return np.asarray(t.detach().cpu().numpy() if hasattr(t, "detach") else t, dtype=np.float32).astype(np.float64)


# ---- frame counts --------------------------------------------------------------------------------------------------------------
def nemo_frames(L: int, hop: int = 160) -> int:
    """[UPSTREAM] FilterbankFeatures.get_seq_len, center=True: floor((L + 2 (n_fft / 2) - n_fft) / hop) = floor(L / hop)"""
    return L // hop


def espnet_frames(L: int, hop: int = 128) -> int:
    """[UPSTREAM] espnet2 Stft with center=True keeps every frame of torch.stft: 1 + floor(L / hop)"""
    return 1 + L // hop


def kaldi_frames(L: int, shift: int = 160) -> int:
    """[UPSTREAM] kaldi NumFrames, snip_edges = false: floor((L + shift / 2) / shift)"""
    return (L + shift // 2) // shift


# ---- kind 0: NeMo AudioToMelSpectrogramPreprocessor -----------------------------------------------------------------------------
def nemo_logmel(cfg, sd, x, pad_left: int = 0, pad_right: int = 0) -> np.ndarray:
    """x [L] -> normalised log-mel float64 [floor(Lp / hop)][n_mels], Lp = pad_left + L + pad_right.

    pad_audio (zeros on both sides) -> pre-emphasis y[0] = x[0], y[i] = x[i] - c x[i - 1] -> zero centre padding of n_fft / 2 ->
    frames of n_fft samples every hop, Hann(win_length) centred in the n_fft frame -> |rfft|^2 -> fb @ power -> log(x + 2^-24)
    -> per feature: mean and UNBIASED std over the frames, (x - mean) / (std + eps).  One frame: 0 / 0 = NaN, as upstream."""
    x = np.concatenate([np.zeros(pad_left), np.asarray(x, np.float64), np.zeros(pad_right)])
    L = len(x)
    n = nemo_frames(L, cfg.hop_length)
    if n == 0:
        return np.zeros((0, cfg.n_mels))
    y = x.copy()
    y[1:] = x[1:] - _f32(cfg.preemph) * x[:-1]
    padded = np.concatenate([np.zeros(N_FFT // 2), y, np.zeros(N_FFT // 2)])
    window = np.zeros(N_FFT)
    off = (N_FFT - cfg.win_length) // 2
    window[off:off + cfg.win_length] = _t64(sd["preprocessor.featurizer.window"])
    idx = (np.arange(n) * cfg.hop_length)[:, None] + np.arange(N_FFT)[None, :]
    spec = np.fft.rfft(padded[idx] * window, axis=1)
    power = spec.real ** 2 + spec.imag ** 2
    fb = _t64(sd["preprocessor.featurizer.fb"]).reshape(cfg.n_mels, -1)
    logmel = np.log(power @ fb.T + _f32(cfg.log_guard))
    mean = logmel.mean(axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        std = np.sqrt(((logmel - mean) ** 2).sum(axis=0) / (n - 1))
        return (logmel - mean) / (std + _f32(cfg.norm_eps))


# ---- kind 1: ESPnet DefaultFrontend + GlobalMVN ----------------------------------------------------------------------------------
def espnet_logmel(cfg, sd, x) -> np.ndarray:
    """x [L], L > n_fft / 2 -> float64 [1 + L // hop][n_mels].

    reflect padding of n_fft / 2 (x[-k] = x[k], x[L - 1 + k] = x[L - 1 - k]; undefined for L <= n_fft / 2, as in torch) -> frames of
    n_fft every hop, PERIODIC Hann(n_fft) -> |rfft|^2 -> power @ melmat -> log(max(x, 1e-10)) -> (x - mean) / std (GlobalMVN)."""
    from reazonspeech_amd.runtime.weights_espnet import hann_periodic
    x = np.asarray(x, np.float64)
    L = len(x)
    if L <= N_FFT // 2:
        raise ValueError(f"reflect padding of {N_FFT // 2} samples is undefined for {L} samples")
    n = espnet_frames(L, cfg.hop_length)
    padded = np.pad(x, N_FFT // 2, mode="reflect")
    idx = (np.arange(n) * cfg.hop_length)[:, None] + np.arange(N_FFT)[None, :]
    spec = np.fft.rfft(padded[idx] * hann_periodic(cfg.win_length).astype(np.float64), axis=1)
    power = spec.real ** 2 + spec.imag ** 2
    logmel = np.log(np.maximum(power @ _t64(sd["frontend.logmel.melmat"]), _f32(cfg.log_guard)))
    std = np.maximum(_t64(sd["normalize.std"]), _f32(cfg.norm_eps))
    return (logmel - _t64(sd["normalize.mean"])) / std


# ---- kind 2: kaldi-native-fbank as sherpa-onnx configures it ---------------------------------------------------------------------
def kaldi_reflect(idx: np.ndarray, L: int):
    """[UPSTREAM] kaldi ExtractWindow, snip_edges = false: an index outside [0, L) is reflected about the edge WITHOUT repeating the
    edge sample (-1 -> 0, L -> L - 1), again and again until it is inside.  -> (indices, bounces the worst index needed)"""
    idx = np.array(idx, dtype=np.int64)
    bounces = 0
    while True:
        low, high = idx < 0, idx >= L
        if not (low | high).any():
            return idx, bounces
        idx = np.where(low, -idx - 1, np.where(high, 2 * L - 1 - idx, idx))
        bounces += 1


def kaldi_fbank(cfg, x) -> np.ndarray:
    """x [L] -> log-mel energies float64 [(L + 80) // 160][n_mels].

    frame f covers [shift f + shift / 2 - N / 2, .. + N) = [160 f - 120, 160 f + 280), outside indices reflected (kaldi_reflect);
    per frame: subtract the mean, y[i] = x[i] - c x[i - 1] with y[0] = x[0] - c x[0], Povey window, zero-pad to 512, |rfft|^2,
    mel banks, log(max(x, FLT_EPSILON)).  Window and banks: the oracle's own float32 tables, promoted."""
    from oracle import zipformer as oz
    x = np.asarray(x, np.float64)
    L = len(x)
    N, S = cfg.frame_length, cfg.frame_shift
    n = kaldi_frames(L, S)
    if n == 0:
        return np.zeros((0, cfg.n_mels))
    window = oz.povey_window(N).astype(np.float32).astype(np.float64)
    banks = oz.kaldi_mel_banks(cfg).astype(np.float32).astype(np.float64)
    idx = (np.arange(n) * S + S // 2 - N // 2)[:, None] + np.arange(N)[None, :]
    idx, _ = kaldi_reflect(idx, L)
    fr = x[idx]
    fr = fr - fr.mean(axis=1, keepdims=True)
    prev = np.concatenate([fr[:, :1], fr[:, :-1]], axis=1)
    fr = (fr - _f32(cfg.preemph) * prev) * window
    spec = np.fft.rfft(np.pad(fr, ((0, 0), (0, cfg.n_fft - N))), axis=1)
    power = spec.real ** 2 + spec.imag ** 2
    return np.log(np.maximum(power @ banks.T, float(np.finfo(np.float32).eps)))


def kaldi_bounces(L: int, N: int = 400, S: int = 160) -> int:
    """reflections the worst sample index of an L-sample utterance needs (0 when it has no frame)"""
    n = kaldi_frames(L, S)
    if n == 0:
        return 0
    idx = (np.arange(n) * S + S // 2 - N // 2)[:, None] + np.arange(N)[None, :]
    return kaldi_reflect(idx, L)[1]
