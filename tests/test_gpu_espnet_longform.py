"""-m gpu: the cut points of long recordings on the device (rs_ctc_find_blank, csrc/k_ctc_blank.hip), `find_blank_batch`, and
recordings of any length through `transcribe_batch` with `segmentation="device"`.

Nothing here has a tolerance.  The kernel must return the reference's own cuts on the 120 blank columns of
tests/golden/reference_espnet.json and this package's host `find_blank` on columns built around the 64-frame step of the kernel;
`find_blank_batch` must return `find_blank` window for window; and `transcribe_batch` under "device" must return what
`transcribe` under "host" returns for every recording, field for field."""
import importlib
import json
import os

import numpy as np
import pytest
import torch

import espnet_fake as fk

from reazonspeech_amd.runtime import capi
from reazonspeech_amd.runtime.config import ESPNET_TINY
from reazonspeech_amd.runtime.synth import synthetic_batch
from reazonspeech_amd.runtime.weights_espnet import synthetic_state_dict_espnet
from reazonspeech_amd.espnet.asr.model import EspnetModel, synthetic_token_list
from reazonspeech_amd.espnet.asr import ctc as ectc, interface

etr = importlib.import_module("reazonspeech_amd.espnet.asr.transcribe")
pytestmark = pytest.mark.gpu

GOLD = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_espnet.json")))
STEP = 64                                      # frames a wavefront takes per step (csrc/k_ctc_blank.hip: BLANK_WAVE)
QUIET = interface.TranscribeConfig(verbose=False)


def make_model(beam_size=1):
    sd = synthetic_state_dict_espnet(ESPNET_TINY, 3)
    return EspnetModel(ESPNET_TINY, sd, synthetic_token_list(ESPNET_TINY.vocab_size, 3), device="cuda:0", beam_size=beam_size)


@pytest.fixture(scope="module")
def tiny(gpu_device):
    return make_model()


@pytest.fixture(scope="module")
def ctx(tiny):
    return tiny.am.ctx                         # the blank finder reads no weights: any context with a CTC head serves


def device_cuts(ctx, cases, threshold, tp_max=None, enc_lens=None):
    """cases: [(n_samples, float32 column)] -> int32 [B][2] of ONE launch.  Row b of the buffer holds its column and NaN in every
    cell past it (a NaN that was read as a frame would change the runs), and `cuts` is prefilled with -7."""
    B = len(cases)
    tp_max = tp_max or max(len(col) for _, col in cases) + 3
    host = np.full((B, tp_max), np.nan, np.float32)
    for b, (_, col) in enumerate(cases):
        host[b, :len(col)] = col
    blank = torch.from_numpy(host.reshape(-1)).cuda()
    lens = torch.tensor([len(col) for _, col in cases] if enc_lens is None else enc_lens, dtype=torch.int32, device="cuda")
    ns = torch.tensor([n for n, _ in cases], dtype=torch.int32, device="cuda")
    cuts = torch.full((B, 2), -7, dtype=torch.int32, device="cuda")
    ctx.ctc_find_blank(blank, lens, ns, B, tp_max, threshold, cuts, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return cuts.cpu().numpy()


def host_cut(n, col, threshold):
    """this package's host `find_blank` on a given column; only the LENGTH of the samples is read, so none are allocated"""
    return list(ectc.find_blank(fk.ColumnModel(col), np.broadcast_to(np.float32(0), (n,)), threshold))


def test_kernel_equals_the_reference_goldens(ctx):
    pats = fk.blank_patterns()
    assert len(pats) == len(GOLD["find_blank"]) == 120
    assert min(len(col) for _, col in pats) == 1 and max(len(col) for _, col in pats) == 89 > STEP      # rows on both sides of a step
    assert sum(want[0] < n for (n, _), want in zip(pats, GOLD["find_blank"])) == 81                     # real cuts, not the (n, n) fallback
    got = device_cuts(ctx, pats, 0.98, tp_max=92)
    for b, ((n, col), want) in enumerate(zip(pats, GOLD["find_blank"])):
        assert got[b].tolist() == want, (b, n, len(col), col.tolist())


def column(T, runs, low=0.5, high=0.99):
    col = np.full(T, low, np.float32)
    for first, after in runs:
        col[first:after] = high
    return col


def step_cases():
    """(label, n_samples, column) around the kernel's 64-frame step"""
    rng = np.random.default_rng(17)
    out = []
    for T in (1, 2, 63, 64, 65, 127, 128, 129, 640):
        for k in range(3):                                   # random runs, short ones and ones longer than a step
            col = np.full(T, 0.5, np.float32)
            t = int(rng.integers(0, 4)) if k else 1
            while t < T:
                run = int(rng.integers(1, 100 if k == 2 else 12))
                col[t:t + run] = 0.99 if rng.random() < 0.6 else 0.7      # 0.7: silent at the second threshold only
                t += run + int(rng.integers(1, 9))
            if T > 2 and k == 1:
                col[-1] = 0.5                                # the last run is closed by the last frame
            out.append((f"T={T}/{k}", 320000, col))
    for edge in (63, 64, 128):
        out.append((f"begins at {edge}", 320000, column(200, [(edge, edge + 9), (10, 14)])))
        out.append((f"ends at {edge}", 320000, column(200, [(edge - 11, edge), (150, 156)])))
        out.append((f"one frame at {edge}", 320000, column(200, [(edge, edge + 1)])))
    out.append(("spans three steps", 320000, column(300, [(40, 200), (210, 230)])))
    out.append(("spans three whole steps", 320000, column(321, [(64, 256)])))
    out.append(("equal lengths", 1000, column(99, [(10, 20), (50, 60), (70, 75)])))
    out.append(("equal lengths across a step", 4000, column(199, [(60, 70), (120, 130)])))
    out.append(("all silent", 320000, column(130, [(0, 130)])))
    out.append(("all speech", 320000, column(130, [])))
    out.append(("open at the end", 320000, column(100, [(10, 15), (80, 100)])))
    out.append(("open at the end of a whole step", 320000, column(128, [(10, 15), (100, 128)])))
    out.append(("starts at frame 0", 320000, column(100, [(0, 30), (50, 55)])))
    out.append(("starts at frame 0, longer than a step", 320000, column(150, [(0, 70), (90, 95)])))
    for T in (70, 640):
        for n in (1, 7, T, 320000, 2 ** 31 - 1):
            out.append((f"n={n}", n, column(T, [(3, 9), (20, 66), (68, 69)])))
    edge = np.float32(0.98)
    below, above = np.nextafter(edge, np.float32(0)), np.nextafter(edge, np.float32(1))
    col = np.full(40, 0.5, np.float32)
    col[5:12], col[15:25], col[28:38] = edge, above, below
    out.append(("float32(0.98) and its neighbours", 320000, col))
    out.append(("no frames", 12345, np.zeros(0, np.float32)))
    return out


def test_kernel_equals_the_host_find_blank_around_the_step(ctx):
    cases = step_cases()
    assert not np.float32(0.98) > 0.98                       # numpy compares a float32 with a Python float in float32: 0.98f is NOT silent
    pairs = [(n, col) for _, n, col in cases]
    for threshold in (0.98, 0.5):
        got = device_cuts(ctx, pairs, threshold)
        real = 0
        for b, (label, n, col) in enumerate(cases):
            want = host_cut(n, col, threshold)
            real += want[0] < n
            assert got[b].tolist() == want, (threshold, label, n, len(col))
        assert real >= len(cases) // 2                       # most cases have a real cut: the comparison is not one of fallbacks
    by = {label: (n, col) for label, n, col in cases}
    assert host_cut(*by["equal lengths"], 0.98) == [100, 200]                             # the first of two stretches of 100 samples
    n, col = by["float32(0.98) and its neighbours"]
    assert host_cut(n, col, 0.98) == [int(15 / 41 * n), int(25 / 41 * n)]                 # only the frames ABOVE float32(0.98)
    assert host_cut(*by["open at the end"], 0.98) == [int(10 / 101 * 320000), int(15 / 101 * 320000)]
    assert host_cut(*by["starts at frame 0"], 0.98) == [int(50 / 101 * 320000), int(55 / 101 * 320000)]
    assert host_cut(*by["no frames"], 0.98) == [12345, 12345]


def test_rows_with_lengths_outside_the_buffer_are_marked_and_not_read(ctx):
    col = column(20, [(4, 9)])
    cases = [(32000, col)] * 4
    got = device_cuts(ctx, cases, 0.98, tp_max=23, enc_lens=[20, 24, -1, 23])
    want = host_cut(32000, col, 0.98)
    assert got[0].tolist() == want and want[0] < 32000
    assert got[1].tolist() == [-1, -1] and got[2].tolist() == [-1, -1]
    # enc_lens == tp_max is inside: the three NaN cells are frames now, and NaN > threshold is False like on the host
    assert got[3].tolist() == host_cut(32000, np.concatenate([col, np.full(3, np.nan, np.float32)]), 0.98)


def test_invalid_arguments_are_refused_before_anything_runs(ctx):
    B, tp_max = 2, 8
    blank = torch.full((B * tp_max,), 0.99, device="cuda")
    lens = torch.full((B,), 8, dtype=torch.int32, device="cuda")
    ns = torch.full((B,), 4000, dtype=torch.int32, device="cuda")
    cuts = torch.full((B, 2), -7, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    for args in ((blank, lens, ns, 0, tp_max, 0.98, cuts), (blank, lens, ns, -1, tp_max, 0.98, cuts), (blank, lens, ns, B, 0, 0.98, cuts),
                 (None, lens, ns, B, tp_max, 0.98, cuts), (blank, None, ns, B, tp_max, 0.98, cuts), (blank, lens, None, B, tp_max, 0.98, cuts),
                 (blank, lens, ns, B, tp_max, 0.98, None)):
        with pytest.raises(capi.RsError) as e:
            ctx.ctc_find_blank(*args, stream)
        assert e.value.code == capi.RS_EINVAL
    torch.cuda.synchronize()
    assert torch.all(cuts == -7)
    ctx.ctc_find_blank(blank, lens, ns, B, tp_max, 0.98, cuts, stream)                    # and the good call runs
    torch.cuda.synchronize()
    assert cuts.cpu().tolist() == [[4000, 4000]] * 2         # all silent: the only run is open at the end


def test_workspace_of_a_longer_geometry_covers_every_shorter_one(ctx):
    """a pool of pieces runs as a narrowed view of a buffer set that was sized for whole seconds (`AsrModel.buffers`): the
    workspace asked for the longer extent must cover every shorter one, also where the subsampling works in chunks of
    utterances (here: 96 windows of about 20 s, more than one chunk) and the chunk size steps with the length"""
    sizes = [ctx.workspace_bytes(96, n) for n in range(300000, 352001, 128)]
    assert all(a <= b for a, b in zip(sizes, sizes[1:])), [(300000 + 128 * k, a, b) for k, (a, b) in enumerate(zip(sizes, sizes[1:])) if a > b][:4]
    assert sizes[0] < sizes[-1]


def test_workspace_of_a_longer_geometry_covers_every_shorter_one_in_float32(gpu_device):
    """the same for a context with the float32 weights registered (`precision="fp32"`): its query is the larger of the bf16
    and the float32 layouts, the float32 one dominates, and both reserve the subsampling chunk by the same rule"""
    sd = synthetic_state_dict_espnet(ESPNET_TINY, 3)
    ctx = EspnetModel(ESPNET_TINY, sd, synthetic_token_list(ESPNET_TINY.vocab_size, 3), device="cuda:0", precision="fp32").am.ctx
    sizes = [ctx.workspace_bytes(96, n) for n in range(300000, 352001, 128)]
    assert all(a <= b for a, b in zip(sizes, sizes[1:])), [(300000 + 128 * k, a, b) for k, (a, b) in enumerate(zip(sizes, sizes[1:])) if a > b][:4]
    assert sizes[0] < sizes[-1]


# ---- find_blank_batch against find_blank under "host" ----------------------------------------------------------------

def test_find_blank_batch_equals_find_blank(tiny):
    audio, _ = synthetic_batch(5, 9.0, seed=21)
    windows = [audio[b, :n] for b, n in enumerate((144000, 61234, 100001, 8000, 123457))]
    tiny.segmentation = "host"
    col = tiny.ctc_posteriors(windows[0])[:, tiny.asr_model.blank_id]
    # untrained weights need not reach 0.98: also take a threshold from the model, the highest quantile of the first window's
    # blank column at which the HOST finds a real cut
    quantile = next((q for q in (0.9, 0.8, 0.7, 0.6, 0.5, 0.4, 0.3, 0.2, 0.1)
                     if ectc.find_blank(tiny, windows[0], float(np.quantile(col, q))).start < len(windows[0])), None)
    assert quantile is not None, "no threshold gives the first window a real cut"
    for threshold in (0.98, float(np.quantile(col, quantile))):
        want = [ectc.find_blank(tiny, w, threshold) for w in windows]
        if threshold != 0.98:
            assert want[0].start < len(windows[0])
        got = tiny.find_blank_batch(windows, threshold)
        assert got == want and all(isinstance(g, ectc.Blank) for g in got), threshold
        assert tiny.find_blank_batch(windows, threshold, max_batch=2) == want, threshold
    assert tiny.find_blank_batch([]) == []


# ---- end to end: transcribe_batch under "device" against transcribe under "host" --------------------------------------

SECONDS = (47.0, 23.0, 5.0, 0.5, 61.0)


def recordings():
    return [interface.AudioData(synthetic_batch(1, s, seed=300 + k)[0][0], 16000) for k, s in enumerate(SECONDS)]


def check_long_recordings(model, audios):
    model.segmentation = "host"
    host = [etr.transcribe(model, a, QUIET) for a in audios]
    passes = []
    inner = model._blank_pass

    def counted(buf, col, stream):
        passes.append(buf.B)
        return inner(buf, col, stream)

    model._blank_pass = counted
    model.segmentation = "device"
    try:
        dev = etr.transcribe_batch(model, audios)
    finally:
        model.segmentation = "host"
        del model._blank_pass
    assert len(dev) == len(host) == len(audios)
    for k, (d, h) in enumerate(zip(dev, host)):
        assert d.text == h.text, k
        assert [(s.start_seconds, s.end_seconds, s.text) for s in d.segments] == [(s.start_seconds, s.end_seconds, s.text) for s in h.segments], k
    assert dev == host
    return host, passes


def test_long_recordings_through_transcribe_batch_equal_transcribe(tiny):
    audios = recordings()
    host, passes = check_long_recordings(tiny, audios)
    window = etr.WINDOW_SECONDS * 16000
    plan = etr.plan_windows([len(a.waveform) for a in audios], window,
                            lambda reqs: [ectc.find_blank(tiny, audios[i].waveform[o:o + n]) for i, o, n in reqs])
    n_pieces = sum(len(p) for p in plan)
    assert [len(p) for p in plan][2:4] == [1, 1] and n_pieces >= 3 + 2 + 1 + 1 + 4
    assert sum(len(r.segments) for r in host) > n_pieces     # alignments, not one whole-piece segment per fallback
    # one blank pass per ROUND of the lockstep plan (the windows of the 47 s, 23 s and 61 s recordings side by side), not per window
    rounds = max(len(p) for p in plan) - 1
    assert len(passes) == rounds and sum(passes) == sum(len(p) - 1 for p in plan) and passes[0] == 3


def test_long_recordings_with_the_beam_search(gpu_device):
    """these untrained weights overflow the search's bound in most windows (14 of the 16 pieces when this was written), and
    `transcribe` then decodes such a window — and only it — greedily.  The pool must do the same: without
    `isolate_overflow` the whole chunk would turn greedy and the windows that the beam search does finish would differ."""
    model = make_model(beam_size=3)
    assert model.am.cfg.decoding == "beam"
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)      # an untrained joint may overflow a window: both paths then decode IT greedily
        check_long_recordings(model, recordings())
