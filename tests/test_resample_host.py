"""CPU: the host half of `resample="device"` (reazonspeech_amd/runtime/resample.py) — the polyphase plan of the host path's filter,
the float64 closed form the GPU tests compare the kernel with (against scipy's resample_poly), the output length, the option's
argument check in the three `load_model`s and the C ABI's new entry point."""
import ctypes
import re

import numpy as np
import pytest
from scipy.signal import resample_poly

from reazonspeech_amd import build as rs_build
from reazonspeech_amd.nemo.asr.audio import _hq_filter
from reazonspeech_amd.runtime import capi, resample as rs

RATES = (48000, 44100, 22050, 11025, 8000)
RATIOS = {48000: (1, 3), 44100: (160, 441), 32000: (1, 2), 22050: (320, 441), 11025: (640, 441), 8000: (2, 1)}


@pytest.mark.parametrize("rate", RATES)
def test_plan_is_the_host_filter_phase_major(rate):
    pl = rs.plan(rate)
    up, down = RATIOS[rate]
    h = _hq_filter(up, down)
    assert (pl.up, pl.down, pl.numtaps, pl.half) == (up, down, len(h), (len(h) - 1) // 2) and len(h) % 2 == 1
    cols = -(-len(h) // up)
    assert pl.table.dtype == np.float32 and pl.table.shape == (up, (cols + 3) // 4 * 4)
    want = (up * h).astype(np.float32)
    for p in range(0, up, max(1, up // 7)):                        # a phase's row = every up-th tap from p on, then zeros
        row = want[p::up]
        assert np.array_equal(pl.table[p, :len(row)], row) and not pl.table[p, len(row):].any()
    assert np.array_equal(pl.table.T.reshape(-1)[:len(h)], want) and not pl.table.T.reshape(-1)[len(h):].any()
    assert rs.plan(rate) is pl                                     # cached per rate


def test_identity_plan_and_oversized_filters():
    pl = rs.plan(16000)
    assert (pl.up, pl.down, pl.numtaps, pl.half) == (1, 1, 1, 0) and pl.table.tolist() == [[1.0, 0.0, 0.0, 0.0]]
    assert rs.estimate_taps(160, 441) == rs.plan(44100).numtaps
    with pytest.raises(ValueError, match="2\\^24 taps"):
        rs.plan(16000 * 6007 + 1)                                  # coprime with 16000: a filter of tens of millions of taps


def scipy_form(x, rate):
    """resample_poly with the plan's float32 taps (what `reference` sums), cut to librosa's length, channels averaged"""
    pl = rs.plan(rate)
    h32 = pl.table.T.reshape(-1)[:pl.numtaps].astype(np.float64) / pl.up        # resample_poly multiplies the window by up
    y = resample_poly(np.asarray(x, np.float64), pl.up, pl.down, axis=-1, window=h32)[..., :rs.n_out(np.shape(x)[-1], pl.up, pl.down)]
    return y.mean(axis=0) if y.ndim > 1 else y


@pytest.mark.parametrize("rate,shape", [(48000, (4001,)), (44100, (3000,)), (22050, (2000,)), (11025, (1500,)), (8000, (900,)),
                                        (44100, (573,)), (44100, (2, 2500)), (48000, (2, 1234))])
def test_reference_equals_resample_poly(rate, shape):
    """Two stated deviations from `resample_poly(..., window=h)` with the float64 `h`: scipy is given the float32-rounded taps of
    `plan().table`, because `reference` is defined on those (they are what the kernel multiplies with); and the 1e-12 is relative to
    max|want|, not per element (an output near a zero crossing has no relative accuracy in either evaluation).  What that leaves open
    is closed elsewhere: test_plan_* pins table == float32(up * h), and test_the_float32_taps_are_the_host_paths_filter bounds the
    distance to the float64 taps' result per output."""
    x =0.1 * np.random.default_rng(rate + shape[-1]).standard_normal(shape)
    y, mag = rs.reference(x, rate)
    want = scipy_form(x, rate)
    assert y.shape == want.shape == (rs.n_out(shape[-1], *RATIOS[rate]),)
    assert np.abs(y - want).max() <= 1e-12 * np.abs(want).max()
    assert (mag >= np.abs(y) * (1 - 1e-12)).all()                  # sum of |terms| bounds |sum|
    pick = np.array([0, len(y) // 3, len(y) - 1])
    ys, ms = rs.reference(x, rate, pick)                           # chosen indices give the same numbers
    assert np.array_equal(ys, y[pick]) and np.array_equal(ms, mag[pick])


def test_the_float32_taps_are_the_host_paths_filter():
    """the host path filters with the float64 taps: the device path's float32 table moves a result by float32 rounding only"""
    x = 0.1 * np.random.default_rng(3).standard_normal(4000)
    pl = rs.plan(44100)
    host = resample_poly(x, pl.up, pl.down, window=_hq_filter(pl.up, pl.down))[:rs.n_out(4000, pl.up, pl.down)]
    y, mag = rs.reference(x, 44100)
    assert (np.abs(y - host) <= 2.0 ** -24 * mag).all()


@pytest.mark.parametrize("rate", RATES + (32000,))
def test_output_length(rate):
    up, down = RATIOS[rate]
    for L in sorted({1, 2, max(down - 1, 1), down, down + 1}):
        want = int(np.ceil(L * 16000 / rate))
        assert rs.n_out(L, up, down) == want
        assert len(rs.reference(np.ones(L), rate)[0]) == want
    assert rs.n_out(0, up, down) == 0 and rs.n_out(2 ** 31 - 1, up, down) == -(-(2 ** 31 - 1) * up // down)


def test_load_model_rejects_an_unknown_option_before_any_device_work():
    from reazonspeech_amd.nemo.asr import load_model as nemo_load
    from reazonspeech_amd.espnet.asr import load_model as espnet_load
    from reazonspeech_amd.k2.asr import load_model as k2_load
    from reazonspeech_amd.runtime.config import TINY
    for load, kw in ((nemo_load, dict(config=TINY)), (espnet_load, dict(synthetic=True)), (k2_load, dict(synthetic=True))):
        with pytest.raises(ValueError, match="resample must be one of"):
            load(resample="bogus", **kw)
    assert rs.check_mode("host") == "host" and rs.check_mode("device") == "device"


def test_norm_batch_keeps_the_host_path_for_a_model_without_the_option():
    from reazonspeech_amd.nemo.asr.audio import norm_audio, AudioData

    class Plain:
        pass

    a = AudioData(0.1 * np.random.default_rng(5).standard_normal((2, 800)), 8000)
    got = rs.norm_batch(Plain(), [a], norm_audio)
    assert len(got) == 1 and np.array_equal(got[0], norm_audio(a).waveform)

    class Device:
        resample = "device"

        def resample_batch(self, waveforms, rates):
            self.seen = (waveforms, rates)
            return ["rows"]

    m = Device()
    assert rs.norm_batch(m, [a], norm_audio) == ["rows"] and m.seen[1] == [8000] and m.seen[0][0] is a.waveform


def test_the_library_exports_rs_resample():
    assert "rs_resample" in capi.EXPORTS
    lib = ctypes.CDLL(rs_build.build())
    assert hasattr(lib, "rs_resample")
    header = open(rs_build.os.path.join(rs_build.os.path.dirname(rs_build.HERE), "include", "rs_asr.h")).read()
    assert re.search(r"\bint\s+rs_resample\s*\(\s*rs_ctx\s*\*\s*ctx\s*,\s*const\s+float\s*\*\s*x\s*,\s*const\s+int64_t\s*\*\s*row_off\s*,", header)
    assert "#define RS_ABI_VERSION 7" in header
    lib.rs_resample.argtypes = capi.load().rs_resample.argtypes
    assert lib.rs_resample(None, None, None, None, 1, 1, None, 1, 3, 565, None, 64, 0, None, None) == capi.RS_EINVAL    # no context: refused
