"""-m gpu: `resample="device"` — rs_resample (csrc/k_resample.hip) against the float64 closed form of runtime/resample.py, and the
option through the three packages.

What is exact: an input that is 1.0 at isolated samples gives every output at most one non-zero term, so the output must BE the
float32 table entry (0.5 x it with a silent second channel) and 0 elsewhere — this pins every tap index and every phase; rows of a
batch are bit-identical to the same rows alone; a model with the option returns what a default model returns for the rows
`resample_batch` produced.  What is bounded: random signals, per output, by
    |got - y| <= (n_terms + 2) 2^-24 sum|t_k x_k| + 2^-24 |y|,     n_terms = channels * ceil(numtaps / up)
(resample.error_bound: Higham's bound for a float32 sum of products in any order, one rounding per product and per addition, two
more operations for the mean of the channels, and the rounding of the result) — a worst-case bound from the number format, not a
measurement.  The rms error of every random case is printed."""
import importlib

import numpy as np
import pytest
import torch

from reazonspeech_amd.runtime import resample as rs
from reazonspeech_amd.runtime.config import TINY, ESPNET_TINY
from reazonspeech_amd.runtime.k2_config import ZIPFORMER_TINY

pytestmark = pytest.mark.gpu
K2_PAD = 14400                                   # k2's 0.9 s of padding in samples


@pytest.fixture(scope="module")
def am(gpu_device):
    from reazonspeech_amd.nemo.asr import load_model
    return load_model(device="cuda:0", config=TINY, resample="device")


def noise(shape, seed):
    return (0.1 * np.random.default_rng(seed).standard_normal(shape)).astype(np.float32)


def check_bound(got, x, rate, indices=None):
    """every output within the derived bound of the closed form; -> rms error"""
    y, mag = rs.reference(x, rate, indices)
    got = np.asarray(got, np.float64) if indices is None else np.asarray(got, np.float64)[indices]
    assert got.shape == y.shape
    err = np.abs(got - y)
    bound = rs.error_bound(y, mag, rate, 1 if np.ndim(x) == 1 else np.shape(x)[0])
    worst = int(np.argmax(err - bound)) if len(err) else 0
    assert (err <= bound).all(), f"{rate} Hz: output {worst}: |err| {err[worst]:.3e} > bound {bound[worst]:.3e}"
    return float(np.sqrt(np.mean(err ** 2))) if len(err) else 0.0


def launch(am, waves, rate, out_offset=0, slack=0):
    """rs_resample on caller-made buffers -> (out [B][pitch], out_lens, the floats behind the last row), all on the host.  The
    output buffer starts as NaN and carries 64 sentinel floats behind it."""
    pl = rs.plan(rate)
    waves = [np.asarray(w, np.float32) for w in waves]
    channels = 1 if waves[0].ndim == 1 else waves[0].shape[0]
    lens = [w.shape[-1] for w in waves]
    offs = np.concatenate([[0], np.cumsum([n * channels for n in lens])[:-1]]).astype(np.int64)
    flat = np.concatenate([w.reshape(-1) for w in waves] + [np.zeros(1, np.float32)])
    pitch = out_offset + max(rs.n_out(n, pl.up, pl.down) for n in lens) + slack
    B, dev = len(waves), am.device
    store = torch.full((B * pitch + 64,), float("nan"), dtype=torch.float32, device=dev)
    store[B * pitch:] = 7.0
    out = store[:B * pitch].view(B, pitch)
    out_lens = torch.full((B,), -1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        am.ctx.resample(torch.from_numpy(flat).to(dev), torch.from_numpy(offs).to(dev), torch.tensor(lens, dtype=torch.int32, device=dev), B,
                        channels, torch.from_numpy(pl.table.copy()).to(dev), pl.up, pl.down, pl.numtaps, out, out_offset, out_lens,
                        torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    return out.cpu().numpy(), out_lens.cpu().numpy(), store[B * pitch:].cpu().numpy()


# ---- impulse trains: exact -------------------------------------------------------------------------------------------------------

def impulse_case(rate, count):
    """1.0 at m_i = i * s + i, i = 1 .. count, with s a multiple of `down` wider than the filter: m_i mod down takes `count`
    residues, no output sees two impulses and every tap of every impulse lands inside the row
    -> (x, the exact expected output, its non-zero terms)"""
    pl = rs.plan(rate)
    span = -(-pl.numtaps // pl.up)                                   # input samples one output reaches over
    s = pl.down * (span // pl.down + 1)
    assert s > span and s % pl.down == 0
    m = np.arange(1, count + 1, dtype=np.int64) * (s + 1)
    assert len(set((m % pl.down).tolist())) == min(count, pl.down)
    x = np.zeros(int(m[-1]) + s, np.float32)
    x[m] = 1.0
    flat = pl.table.T.reshape(-1)                                    # float32(up * h)[k], zero beyond numtaps
    want = np.zeros(rs.n_out(len(x), pl.up, pl.down), np.float32)
    hits = 0
    for mi in m:                                                     # tap k = half + n * down - m * up inside [0, numtaps)
        n_lo = -(-(int(mi) * pl.up - pl.half) // pl.down)
        n_hi = (int(mi) * pl.up - pl.half + pl.numtaps - 1) // pl.down
        assert 0 <= n_lo and n_hi < len(want)
        n = np.arange(n_lo, n_hi + 1)
        assert not want[n].any()
        want[n] = flat[pl.half + n * pl.down - mi * pl.up]
        hits += len(n)
    return x, want, hits


@pytest.mark.parametrize("rate,count", [(44100, 441), (48000, 3), (8000, 2)])
def test_impulse_trains_give_the_table_bit_for_bit(am, rate, count):
    x, want, hits = impulse_case(rate, count)
    pl = rs.plan(rate)
    if rate == 44100:
        assert hits == pl.numtaps                                    # 441 residues x every phase: each tap of the filter exactly once
        assert np.array_equal(np.sort(want[want != 0]), np.sort(pl.table[pl.table != 0]))
    mono, stereo = am.resample_batch([x, np.stack([x, np.zeros_like(x)])], [rate, rate])
    assert mono.dtype == np.float32 and mono.shape == want.shape
    assert np.array_equal(mono, want)
    assert np.array_equal(stereo, np.float32(0.5) * want)


# ---- random signals: the derived bound -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("channels", [1, 2, 3])
@pytest.mark.parametrize("rate", [48000, 44100, 32000, 22050, 11025, 8000])
def test_random_signals_within_the_bound(am, rate, channels):
    L = rate // 2 + 37
    x = noise((channels, L) if channels > 1 else (L,), rate + channels)
    got = am.resample_batch([x], [rate])[0]
    assert got.dtype == np.float32 and got.shape == (rs.n_out(L, *rs.ratio(rate)),)
    rms = check_bound(got, x, rate)
    print(f"resample {rate} Hz x{channels}: rms error {rms:.3e} (signal rms {np.sqrt(np.mean(got.astype(np.float64) ** 2)):.3e})")


def test_sixteen_khz_passes_through_or_is_only_averaged(am):
    mono, stereo = noise(1000, 1), noise((3, 777), 2)
    got = am.resample_batch([mono, stereo, mono.astype(np.float64)[None, :]], [16000, 16000, 16000])
    assert np.array_equal(got[0], mono) and np.array_equal(got[2], mono)
    assert got[1].shape == (777,)
    check_bound(got[1], stereo, 16000)
    want = (stereo[0] + stereo[1] + stereo[2]) / np.float32(3)       # the kernel's order: sum in channel order, one division
    assert np.array_equal(got[1], want)


# ---- edges -----------------------------------------------------------------------------------------------------------------------------

def test_short_rows(am):
    waves = [noise(L, 10 + L) for L in (0, 1, 7, 573)]
    got = am.resample_batch(waves + [noise(2, 5)], [44100] * 4 + [8000])
    assert [len(g) for g in got] == [0, 1, 3, 208, 4]
    for g, w in zip(got[:4], waves):
        check_bound(g, w, 44100)
    check_bound(got[4], noise(2, 5), 8000)


@pytest.mark.parametrize("rate", [44100, 48000, 8000])
def test_both_ends_of_a_one_second_row(am, rate):
    x = noise(rate, 77)
    got = am.resample_batch([x], [rate])[0]
    assert len(got) == 16000
    edge = np.concatenate([np.arange(600), np.arange(16000 - 600, 16000)])
    check_bound(got, x, rate, edge)


def test_output_layout_offset_pitch_lengths_and_sentinel(am):
    waves = [noise(4410, 1), noise(0, 2), noise(44100 // 3, 3), noise(1, 4)]
    n_outs = [1600, 0, 5334, 1]
    out, lens, tail = launch(am, waves, 44100, out_offset=K2_PAD, slack=777)
    assert lens.tolist() == n_outs and out.shape == (4, K2_PAD + 5334 + 777)
    assert (tail == 7.0).all()                                       # nothing behind the last row's pitch was touched
    for b, (w, n) in enumerate(zip(waves, n_outs)):
        assert not out[b, :K2_PAD].any() and not out[b, K2_PAD + n:].any() and not np.isnan(out[b]).any()
        check_bound(out[b, K2_PAD:K2_PAD + n], w, 44100)
    plain, lens0, tail0 = launch(am, waves, 44100)                   # the same rows without an offset: the same bits
    assert lens0.tolist() == n_outs and (tail0 == 7.0).all()
    for b, n in enumerate(n_outs):
        assert np.array_equal(plain[b, :n], out[b, K2_PAD:K2_PAD + n]) and not plain[b, n:].any()
    short, lens1, tail1 = launch(am, waves[:1], 44100, slack=-600)   # a pitch shorter than the row: the row is cut, nothing spills
    assert lens1.tolist() == [1600] and (tail1 == 7.0).all() and np.array_equal(short[0], plain[0, :1000])


def test_bad_arguments_are_refused_before_anything_is_enqueued(am):
    from reazonspeech_amd.runtime import capi
    dev = am.device
    x, off, ln = torch.zeros(8, device=dev), torch.zeros(1, dtype=torch.int64, device=dev), torch.ones(1, dtype=torch.int32, device=dev)
    table, out, ol = torch.zeros(4, device=dev), torch.zeros((1, 8), device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    for kw in (dict(up=0), dict(down=0), dict(numtaps=2), dict(channels=0), dict(out_offset=9), dict(down=70000, numtaps=1)):
        a = dict(up=1, down=1, numtaps=1, channels=1, out_offset=0)
        a.update(kw)
        with pytest.raises(capi.RsError) as e:
            am.ctx.resample(x, off, ln, 1, a["channels"], table, a["up"], a["down"], a["numtaps"], out, a["out_offset"], ol, 0)
        assert e.value.code == capi.RS_EINVAL, kw


def test_a_rate_the_kernel_does_not_take_goes_through_the_host_with_a_warning(am):
    from reazonspeech_amd.nemo.asr.audio import norm_audio, AudioData
    x = noise(30000, 8)
    with pytest.warns(RuntimeWarning, match="resampled on the host"):
        got = am.resample_batch([x], [1600000])                      # 1/100: a window of more than 16384 samples per workgroup
    assert np.array_equal(got[0], np.asarray(norm_audio(AudioData(x, 1600000)).waveform, np.float32))


# ---- 64-bit indices ----------------------------------------------------------------------------------------------------------------

def test_a_row_whose_sample_products_pass_two_to_the_31(am):
    L = 13_700_000                                                   # n * down reaches 2.19e9 at the end of the row
    x = noise(L, 31)
    got = am.resample_batch([x], [44100])[0]
    assert len(got) == 4_970_522
    assert (len(got) - 1) * 441 > 2 ** 31
    pick = np.concatenate([np.random.default_rng(9).integers(0, len(got), 4096), np.arange(len(got) - 4096, len(got))])
    check_bound(got, x, 44100, pick)


# ---- batch invariance --------------------------------------------------------------------------------------------------------------

def test_rows_do_not_depend_on_their_batch(am):
    spec = [(48000, 1, 30011), (44100, 1, 9000), (44100, 1, 44100), (48000, 2, 5000), (8000, 1, 701), (44100, 1, 3), (22050, 3, 12345)]
    waves = [noise((c, n) if c > 1 else (n,), 100 + i) for i, (_, c, n) in enumerate(spec)]
    rates = [r for r, _, _ in spec]
    together = am.resample_batch(waves, rates)
    for i, (w, r) in enumerate(zip(waves, rates)):
        alone = am.resample_batch([w], [r])[0]
        assert np.array_equal(alone, together[i]), spec[i]
    am.RESAMPLE_CHUNK, keep = 40000, am.RESAMPLE_CHUNK               # the same list cut into several launches
    try:
        chunked = am.resample_batch(waves, rates)
    finally:
        am.RESAMPLE_CHUNK = keep
    assert all(np.array_equal(a, b) for a, b in zip(chunked, together))


# ---- end to end: the option through the three packages -------------------------------------------------------------------------------

def inputs(seconds=2.5):
    return [(noise((2, int(48000 * seconds)), 41), 48000), (noise(int(44100 * seconds) + 11, 42), 44100)]


def check_package(pkg, interface, device_model, default_model, fields):
    """`transcribe_batch` and `transcribe` of `pkg`: the model with the option on the raw input == a default model on the rows
    `resample_batch` produced, field for field"""
    raw = inputs()
    rows = device_model.resample_batch([w for w, _ in raw], [r for _, r in raw])
    assert all(r.dtype == np.float32 and r.ndim == 1 for r in rows)
    given = [interface.AudioData(w, r) for w, r in raw]
    ready = [interface.AudioData(r, 16000) for r in rows]
    cfg = interface.TranscribeConfig(verbose=False)
    got, want = pkg.transcribe_batch(device_model, given, cfg), pkg.transcribe_batch(default_model, ready, cfg)
    for a, r, g, w in zip(given, ready, got, want):
        one, one_want = pkg.transcribe(device_model, a, cfg), pkg.transcribe(default_model, r, cfg)
        for f in fields:
            assert getattr(g, f) == getattr(w, f), f
            assert getattr(one, f) == getattr(one_want, f) == getattr(w, f), f
    return got


def test_nemo_end_to_end(am):
    from reazonspeech_amd.nemo.asr import load_model, interface
    pkg = importlib.import_module("reazonspeech_amd.nemo.asr.transcribe")
    default = load_model(device="cuda:0", config=TINY)
    assert (am.resample, default.resample) == ("device", "host")
    check_package(pkg, interface, am, default, ("text", "subwords", "segments"))


def test_espnet_end_to_end(gpu_device):
    from reazonspeech_amd.espnet.asr import interface
    from reazonspeech_amd.espnet.asr.model import EspnetModel, synthetic_token_list
    from reazonspeech_amd.runtime.weights_espnet import synthetic_state_dict_espnet
    pkg = importlib.import_module("reazonspeech_amd.espnet.asr.transcribe")
    # '<unk>' and ',' replaced by two more kanji: a recognised text holding either has more characters than the aligner gives
    # timings for, and the segment loop then raises IndexError (in the reference too) — random weights can emit them
    spare = iter(chr(0x4E00 + 8192 + k) for k in range(2))
    tokens = [next(spare) if t in ("<unk>", ",") else t for t in synthetic_token_list(ESPNET_TINY.vocab_size, 3)]
    sd = synthetic_state_dict_espnet(ESPNET_TINY, 3)
    dev, default = (EspnetModel(ESPNET_TINY, sd, tokens, device="cuda:0", resample=r) for r in ("device", "host"))
    assert (dev.resample, default.resample) == ("device", "host")
    check_package(pkg, interface, dev, default, ("text", "segments"))


def test_k2_end_to_end(gpu_device):
    from reazonspeech_amd.k2.asr import load_model, interface
    pkg = importlib.import_module("reazonspeech_amd.k2.asr.transcribe")
    dev, default = (load_model(device="cuda:0", config=ZIPFORMER_TINY, seed=3, resample=r) for r in ("device", "host"))
    assert (dev.resample, default.resample) == ("device", "host")
    check_package(pkg, interface, dev, default, ("text", "subwords"))


def test_the_fake_models_see_the_device_rows(am):
    """the stand-ins of tests/espnet_fake.py and tests/k2_fake.py derive text and times from the samples they are handed: with the
    option they must be handed the rows of `resample_batch` — the same float32 samples — through `transcribe`"""
    import espnet_fake
    import k2_fake
    from reazonspeech_amd.espnet.asr import interface as ei
    from reazonspeech_amd.k2.asr import interface as ki
    etr = importlib.import_module("reazonspeech_amd.espnet.asr.transcribe")
    ktr = importlib.import_module("reazonspeech_amd.k2.asr.transcribe")

    def with_option(model):
        model.resample, model.resample_batch = "device", am.resample_batch
        return model

    for w, r in inputs(seconds=1.5):
        row = am.resample_batch([w], [r])[0]
        got = etr.transcribe(with_option(espnet_fake.FakeEspnetModel()), ei.AudioData(w, r), ei.TranscribeConfig(verbose=False))
        want = etr.transcribe(espnet_fake.FakeEspnetModel(), ei.AudioData(row, 16000), ei.TranscribeConfig(verbose=False))
        assert got == want and got.text
        fake, plain = with_option(k2_fake.FakeRecognizer()), k2_fake.FakeRecognizer()
        got = ktr.transcribe(fake, ki.AudioData(w, r))
        want = ktr.transcribe(plain, ki.AudioData(row, 16000))
        assert got == want and got.subwords and fake.seen == plain.seen == [(16000, len(row) + 2 * K2_PAD, 0.0)]
