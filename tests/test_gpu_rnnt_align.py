"""-m gpu: transducer forced alignment and transcript likelihood on the device (rs_rnnt_align, csrc/k_rnnt_align.hip) against the C
checker (tests/rnnt_align_checker.c: the entry restated serially on the oracle library in the device's float32 order): loglik, best
and logp BITS, frames, and the slots the call must leave alone, given the device's own joint-encoder projection.

  the scene, per family and topology   the 7 ragged utterances of tests/test_gpu_token_scores.py with the device's greedy ids as
                                the texts; lengths are then cut so that the batch holds: a zero-frame row with an empty text, a
                                row with frames and an empty text, U = 1, the richest row whole (U = u_cap); standard topology: a
                                row with T = 1 and U >= 2 (every label on one frame), a Viterbi path with two labels on one frame,
                                a Viterbi path that differs from the greedy frames; one label per frame: a row with U = T and a
                                row with U = T + 1 (infeasible: -inf, -1, NaN, its neighbours unaffected); where the greedy
                                search put several labels on a frame (nemo) the texts are prefixes of its ids
  random transcripts            no blank, no <unk>; random projections: U + 1 > 256 at T = 8 (more cells than threads), T > 256 at
                                U = 3, and the real output widths (nemo 3001 / 640 / two LSTM layers, k2 10 720 / 512, the espnet
                                120M decoder 2600 / 512 / 640)
  chunking, batch invariance    the minimum workspace (32 lattice rows per chunk; a boundary splits a frame's cells) == a generous
                                one; an utterance alone == inside the ragged batch
  cross-check                   rs_rnnt_token_scores on the returned (ids, frames) gives logp bit for bit
  errors                        before any launch; a bad id, the blank in a text, a count above u_cap: NaN / -1 in that row,
                                RS_EINVAL after the sync, the other rows keep their bits
  the public surface            per family: align_text on transcribe's own text, align_text_batch, 9 utterances at max_batch = 4,
                                transcribe unchanged before and after
"""
import math

import numpy as np
import pytest
import torch

import rnnt_align_ref as A
import token_scores_ref as R
from reazonspeech_amd.runtime import capi
from reazonspeech_amd.runtime.avsr_config import AVSR_TINY
from reazonspeech_amd.runtime.config import ESPNET_TINY, TINY, WIDE2
from reazonspeech_amd.runtime.k2_config import ZIPFORMER_TINY
from test_gpu_token_scores import build, dev_i32, device_scores, public, scene as greedy_scene

pytestmark = pytest.mark.gpu
FAMILIES = ("nemo", "espnet", "k2")
CASES = [(f, one) for f in FAMILIES for one in (False, True)]
RECHOOSE = "re-choose the inputs (seed / lengths) of this fixture: the batch must hold "
GENEROUS = 64 << 20


def device_align(am, f, lens, ids, n, one, workspace="generous", want_code=None):
    """rs_rnnt_align -> dict(loglik, best [B]; frames, logp [B][u_cap]); slots the call must not touch hold -9 / 7.0"""
    B, Tp, _ = f.shape
    u_cap = ids.shape[1]
    dev = am.device
    loglik, best = torch.full((B,), 7.0, device=dev), torch.full((B,), 7.0, device=dev)
    frames = torch.full((B, u_cap), -9, dtype=torch.int32, device=dev)
    logp = torch.full((B, u_cap), 7.0, dtype=torch.float32, device=dev)
    least = am.ctx.align_workspace_bytes(B, Tp, u_cap)
    ws = torch.empty((least if workspace == "minimum" else least + GENEROUS,), dtype=torch.uint8, device=dev)
    args = (f, dev_i32(am, lens), B, Tp, dev_i32(am, ids), dev_i32(am, n), loglik, best, frames, logp, ws, torch.cuda.current_stream().cuda_stream)
    if want_code is None:
        am.ctx.rnnt_align(*args, one_per_frame=one)
    else:
        with pytest.raises(capi.RsError) as e:
            am.ctx.rnnt_align(*args, one_per_frame=one)
        assert e.value.code == want_code
    torch.cuda.synchronize()
    return dict(loglik=loglik.cpu().numpy(), best=best.cpu().numpy(), frames=frames.cpu().numpy(), logp=logp.cpu().numpy())


def same_bits(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def check(am, sd, f, lens, texts, one, workspace="generous", u_cap=None):
    """device == checker: bits of loglik / best / logp, frames, untouched slots -> (device results, ids, n)"""
    u_cap = u_cap or max(max(len(t) for t in texts), 1)
    ids, n = R.pack(texts, u_cap)
    got = device_align(am, f, lens, ids, n, one, workspace)
    want = A.align_checker(am.cfg, sd, f.cpu().numpy(), np.asarray(lens, np.int32), ids, n, one_per_frame=one)
    valid = np.arange(u_cap)[None, :] < n[:, None]
    assert (got["frames"][~valid] == -9).all() and (got["logp"][~valid] == 7.0).all(), "slots at u >= n_ids must be left untouched"
    for key in ("loglik", "best"):
        assert same_bits(got[key], want[key]), (key, got[key], want[key])
    assert (got["frames"][valid] == want["frames"][valid]).all(), (got["frames"], want["frames"])
    assert same_bits(got["logp"][valid], want["logp"][valid])
    return got, ids, n


def shape_scene(rows, lens, one):
    """the texts (the greedy ids) and the lengths of the alignment scene: lengths cut on rows with >= 2 labels, the richest row whole"""
    texts = [list(r[0]) for r in rows]
    lens = [int(t) for t in lens]
    count = [len(t) for t in texts]
    free = sorted((b for b in range(len(rows)) if count[b] >= 2), key=lambda b: (count[b], b))
    if free:
        free.pop()                                          # the richest row stays whole: U = u_cap
    if not one:
        if free:
            lens[free.pop(0)] = 1                           # every label on one frame
    else:                                                   # (an LSTM family's greedy search emits several labels on a frame: its
        if free:                                            #  texts are cut to prefixes that one label per frame can hold)
            b = free.pop(0)
            k = min(count[b], lens[b])
            texts[b], lens[b] = texts[b][:k], k             # U = T
        if free:
            b = free.pop(0)
            k = min(count[b], lens[b] + 1)
            texts[b], lens[b] = texts[b][:k], k - 1         # U = T + 1: no alignment
        for b in free:
            if count[b] > lens[b]:
                texts[b] = texts[b][:max(lens[b] // 2, 2)]
    return texts, lens


_scenes = {}


def scene(family, one):
    if (family, one) not in _scenes:
        am, sd, cfg, f, lens, rows = greedy_scene(family)
        texts, alens = shape_scene(rows, lens, one)
        got, ids, n = check(am, sd, f, alens, texts, one)
        print(f"{family} one_per_frame={one}: frames {lens} -> {alens}, labels {n.tolist()}, loglik {got['loglik'].tolist()}, "
              f"best {got['best'].tolist()}")
        _scenes[(family, one)] = (am, sd, cfg, f, alens, texts, rows, got, ids, n)
    return _scenes[(family, one)]


@pytest.mark.parametrize("family,one", CASES)
def test_scene_device_equals_checker(gpu_device, family, one):
    am, sd, cfg, f, lens, texts, rows, got, ids, n = scene(family, one)
    B = len(texts)
    T, U = lens, [len(t) for t in texts]
    fr = [got["frames"][b, :U[b]].tolist() for b in range(B)]
    z = [b for b in range(B) if T[b] == 0 and U[b] == 0]
    assert z, RECHOOSE + "a zero-frame row with an empty text"
    assert all(got["loglik"][b] == 0.0 and got["best"][b] == 0.0 for b in z)
    blanks = [b for b in range(B) if T[b] > 0 and U[b] == 0]
    assert blanks, RECHOOSE + "a row with frames and an empty text"
    assert all(np.isfinite(got["loglik"][b]) and got["loglik"][b] < 0 and got["loglik"][b].tobytes() == got["best"][b].tobytes() for b in blanks)
    assert any(u == 1 for u in U), RECHOOSE + "a row with one label"
    assert max(U) == ids.shape[1], "the richest row reaches u_cap"
    feasible = [b for b in range(B) if np.isfinite(got["loglik"][b])]
    for b in feasible:
        assert got["loglik"][b] >= got["best"][b] and all(0 <= t < T[b] for t in fr[b])
        assert all(y > x for x, y in zip(fr[b], fr[b][1:])) if one else all(y >= x for x, y in zip(fr[b], fr[b][1:]))
    if not one:
        assert len(feasible) == B
        assert any(T[b] == 1 and U[b] >= 2 and fr[b] == [0] * U[b] for b in range(B)), RECHOOSE + "a row with T = 1 and U >= 2"
        assert any(len(set(fr[b])) < len(fr[b]) for b in feasible), RECHOOSE + "a Viterbi path with two labels on one frame"
    else:
        assert any(U[b] == T[b] and U[b] >= 2 and fr[b] == list(range(T[b])) for b in feasible), RECHOOSE + "a row with U = T"
        none = [b for b in range(B) if U[b] == T[b] + 1 and U[b] >= 2]
        assert none, RECHOOSE + "a row with U = T + 1"
        for b in range(B):
            if U[b] > T[b]:
                assert got["loglik"][b] == -math.inf and got["best"][b] == -math.inf and fr[b] == [-1] * U[b]
                assert np.isnan(got["logp"][b, :U[b]]).all()
    whole = [b for b in feasible if U[b] >= 2 and T[b] == greedy_scene(family)[4][b]]           # rows whose length was not cut here
    differ = [b for b in whole if fr[b] != list(rows[b][1])[:U[b]]]
    print(f"{family} one_per_frame={one}: Viterbi frames differ from the greedy frames on rows {differ} of {whole}")
    if not one:                                              # (one label per frame: a peaked model's greedy path may be the best one)
        assert differ, RECHOOSE + "a Viterbi path that differs from the greedy frames"


def random_case(am, cfg, lens, counts, seed):
    J = cfg.joiner_dim if R.is_k2(cfg) else cfg.joint_hidden
    V = cfg.vocab_size if R.is_k2(cfg) else cfg.n_logits
    g = torch.Generator().manual_seed(seed)
    B, Tp = len(lens), max(max(lens), 1)
    f = (torch.randn((B, Tp, J), generator=g) * (0.8 + 0.4 * torch.rand((B, 1, 1), generator=g))).to(am.device).contiguous()
    banned = {cfg.blank_id, getattr(cfg, "unk_id", -1)}
    ok = torch.tensor([v for v in range(V) if v not in banned])
    texts = [ok[torch.randint(0, len(ok), (u,), generator=g)].tolist() for u in counts]
    return f, texts


@pytest.mark.parametrize("family,one,lens,counts", [
    ("nemo", False, [8, 5, 8], [300, 256, 2]),              # U + 1 > 256 at T = 8: more cells on a diagonal than threads
    ("espnet", False, [300, 257], [3, 1]),                  # T > 256 at U = 3
    ("k2", True, [300, 257, 2], [3, 0, 3]),                 # the same, one label per frame (the last row: no alignment)
    ("k2", True, [70, 64], [66, 64]),                       # one label per frame, diagonals across a 64-lane word of back-pointers
    ("k2", False, [8, 3], [259, 64]),
])
def test_random_transcripts_at_the_toy_widths(gpu_device, family, one, lens, counts):
    am, sd, cfg = greedy_scene(family)[:3]
    f, texts = random_case(am, cfg, lens, counts, 4)
    got, ids, n = check(am, sd, f, lens, texts, one)
    assert np.isfinite(got["loglik"][0])
    check(am, sd, f, lens, texts, one, workspace="minimum")


@pytest.mark.parametrize("shape", ["nemo-3001", "k2-10720", "espnet-120m-decoder"])
def test_real_output_widths(gpu_device, shape):
    if shape == "nemo-3001":
        am, sd, cfg, _ = build("nemo", WIDE2)
        assert (cfg.n_logits, cfg.joint_hidden, cfg.pred_layers) == (3001, 640, 2)
    elif shape == "k2-10720":
        am, sd, cfg, _ = build("k2", ZIPFORMER_TINY.with_(vocab_size=10720, decoder_dim=512, joiner_dim=512).validate())
    else:
        am, sd, cfg, _ = build("espnet", ESPNET_TINY.with_(vocab_size=2600, pred_hidden=512, joint_hidden=640).validate())
    one = R.is_k2(cfg)
    lens, counts = [6, 4, 0, 1], [3, 4, 0, 1]
    f, texts = random_case(am, cfg, lens, counts, 2)
    got, ids, n = check(am, sd, f, lens, texts, one)
    assert np.isfinite(got["loglik"][[0, 1, 3]]).all() and got["loglik"][2] == 0.0
    a = check(am, sd, f, lens, texts, one, workspace="minimum")[0]        # 46 lattice rows: two chunks
    assert all(same_bits(a[k], got[k]) for k in got)


@pytest.mark.parametrize("family,one", CASES)
def test_chunking_gives_the_same_bits(gpu_device, family, one):
    am, sd, cfg, f, lens, texts, rows, got, ids, n = scene(family, one)
    # the compacted lattice: utterance by utterance, by anti-diagonal; the minimum workspace cuts it every 32 rows
    base, split = 0, False
    for b, (T, t) in enumerate(zip(lens, texts)):
        U = len(t)
        if T == 0 or (one and U > T):
            continue
        order = sorted(((tt, u) for tt in range(T) for u in range(U + 1)), key=lambda c: (c[0] + c[1], c[1]))
        chunk = {c: (base + i) // 32 for i, c in enumerate(order)}
        split = split or any(chunk[(tt, 0)] != chunk[(tt, U)] for tt in range(T))
        base += len(order)
    assert base > 64, RECHOOSE + "more than two chunks of lattice rows"
    assert split, RECHOOSE + "a chunk boundary inside a frame's row of cells"
    J = cfg.joiner_dim if R.is_k2(cfg) else cfg.joint_hidden
    V = cfg.vocab_size if R.is_k2(cfg) else cfg.n_logits
    H = cfg.decoder_dim if R.is_k2(cfg) else cfg.pred_hidden
    assert GENEROUS > (base + 31) // 32 * 32 * 4 * (3 * J + (V + 63) // 64 * 64 + 2 * H + 64), "generous = one chunk"
    small = check(am, sd, f, lens, texts, one, workspace="minimum")[0]
    assert all(same_bits(small[k], got[k]) for k in got)


@pytest.mark.parametrize("family,one", CASES)
def test_alone_equals_inside_the_ragged_batch(gpu_device, family, one):
    am, sd, cfg, f, lens, texts, rows, got, ids, n = scene(family, one)
    rich = sorted((b for b in range(len(texts)) if np.isfinite(got["loglik"][b]) and lens[b] > 0), key=lambda b: -len(texts[b]))[:2]
    assert rich and texts[rich[0]]
    for b in rich:
        alone = check(am, sd, f[b:b + 1, :lens[b]].contiguous(), lens[b:b + 1], texts[b:b + 1], one)[0]
        k = len(texts[b])
        assert alone["loglik"].tobytes() == got["loglik"][b:b + 1].tobytes() and alone["best"].tobytes() == got["best"][b:b + 1].tobytes()
        assert alone["frames"][0, :k].tolist() == got["frames"][b, :k].tolist() and same_bits(alone["logp"][0, :k], got["logp"][b, :k])


@pytest.mark.parametrize("family,one", CASES)
def test_token_scores_on_the_alignment_give_logp(gpu_device, family, one):
    am, sd, cfg, f, lens, texts, rows, got, ids, n = scene(family, one)
    ok = np.isfinite(got["loglik"])
    n_ok = np.where(ok, n, 0).astype(np.int32)
    frames = np.where(got["frames"] < 0, 0, got["frames"]).astype(np.int32)
    lp, _ = device_scores(am, f, lens, ids, frames, n_ok)
    assert n_ok.sum() > 10
    for b in range(len(texts)):
        assert same_bits(lp[b, :n_ok[b]], got["logp"][b, :n_ok[b]]), (family, one, b)


def test_bad_entries_are_refused_without_touching_anything_else(gpu_device):
    am, sd, cfg, f, lens, texts, rows, good, ids, n = scene("nemo", False)
    rich = sorted(range(len(texts)), key=lambda b: -len(texts[b]))[:3]
    assert all(len(texts[b]) >= 2 for b in rich)
    bad_i, bad_n = ids.copy(), n.copy()
    bad_i[rich[0], 1] = cfg.n_logits                        # an id outside the vocabulary
    bad_i[rich[1], 0] = cfg.blank_id                        # the blank in a text
    bad_n[rich[2]] = ids.shape[1] + 1                       # a count above u_cap
    got = device_align(am, f, lens, bad_i, bad_n, False, want_code=capi.RS_EINVAL)
    want = A.align_checker(cfg, sd, f.cpu().numpy(), np.asarray(lens, np.int32), bad_i, bad_n, want_rc=-1)
    for b in rich:
        k = min(int(bad_n[b]), ids.shape[1])
        assert np.isnan(got["loglik"][b]) and np.isnan(got["best"][b])
        assert (got["frames"][b, :k] == -1).all() and np.isnan(got["logp"][b, :k]).all()
        assert (got["frames"][b, k:] == -9).all()
    for b in (b for b in range(len(texts)) if b not in rich):
        k = int(n[b])
        for key in ("loglik", "best"):
            assert got[key][b].tobytes() == good[key][b].tobytes() == want[key][b].tobytes()
        assert got["frames"][b, :k].tolist() == good["frames"][b, :k].tolist() and same_bits(got["logp"][b, :k], good["logp"][b, :k])
    neg = n.copy()
    neg[rich[0]] = -1                                       # a negative count
    device_align(am, f, lens, ids, neg, False, want_code=capi.RS_EINVAL)


def test_argument_errors_come_before_any_launch(gpu_device):
    am, sd, cfg, f, lens, texts, rows, good, ids, n = scene("nemo", False)
    B, Tp, _ = f.shape
    dev = am.device
    z = lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)       # noqa: E731
    ll, best, frames, logp = torch.full((B,), 7.0, device=dev), torch.full((B,), 7.0, device=dev), z(B, 8) - 9, torch.full((B, 8), 7.0, device=dev)
    least = am.ctx.align_workspace_bytes(B, Tp, 8)
    ws = torch.empty((least,), dtype=torch.uint8, device=dev)
    el = dev_i32(am, lens)
    args = lambda ctx, **kw: ctx.rnnt_align(f, el, B, Tp, z(B, 8), z(B), ll, best, frames, logp, ws, 0, **kw)   # noqa: E731
    with pytest.raises(capi.RsError, match="workspace") as e:
        args(am.ctx, ws_bytes=least - 1)
    assert e.value.code == capi.RS_EINVAL
    for other in (capi.Context(AVSR_TINY, 0), capi.Context(TINY, 0)):   # an AV-HuBERT context; a context that was never finalized
        with pytest.raises(RuntimeError):
            other.align_workspace_bytes(B, Tp, 8)
        with pytest.raises(capi.RsError) as e:
            args(other)
        assert e.value.code == capi.RS_EINVAL
        other.close()
    lib, h = am.ctx.lib, am.ctx._h
    p = lambda t: t.data_ptr()                                          # noqa: E731
    full = (p(f), p(el), B, Tp, p(z(B, 8)), p(z(B)), 8, 0, p(ll), p(best), p(frames), p(logp), p(ws), least, None)
    for at, value in ((2, -1), (3, -1), (6, -1), (7, 2), (6, capi.ALIGN_U_CAP_MAX + 1), (0, None), (8, None), (12, None)):
        bad = list(full)
        bad[at] = value
        assert lib.rs_rnnt_align(h, *bad) == capi.RS_EINVAL, (at, value)
    assert lib.rs_rnnt_align_workspace_bytes(h, B, Tp, capi.ALIGN_U_CAP_MAX + 1) == 0 and lib.rs_rnnt_align_workspace_bytes(h, 0, Tp, 8) == 0
    assert lib.rs_rnnt_align_workspace_bytes(h, 1, 4, capi.ALIGN_U_CAP_MAX) > 0
    torch.cuda.synchronize()
    assert (ll == 7.0).all() and (frames == -9).all() and (logp == 7.0).all()              # nothing was written
    args(am.ctx)                                            # every text empty: the all-blank paths
    torch.cuda.synchronize()
    assert (frames == -9).all() and (logp == 7.0).all() and same_bits(ll.cpu().numpy(), best.cpu().numpy())
    assert all((v == 0.0) if t == 0 else (v < 0) for v, t in zip(ll.cpu().tolist(), lens))


# ---- the public surface -------------------------------------------------------------------------------------------------------
def tokenise(family, model, text):
    mod = __import__(f"reazonspeech_amd.{family}.asr.align", fromlist=["x"])
    try:
        return mod.text_ids(model, text)
    except ValueError:
        return None


@pytest.mark.parametrize("family", FAMILIES)
def test_public_path(gpu_device, family):
    am, model, tr, iface, audios, waves = public(family)
    pkg = __import__(f"reazonspeech_amd.{family}.asr", fromlist=["x"])
    cfg = iface.TranscribeConfig(verbose=False)
    before = tr.transcribe_batch(model, audios, cfg)
    one_before = tr.transcribe(model, audios[1], cfg)
    ids = [list(r.token_ids) for r in before]               # (`public` loads the models with token_scores: the results carry ids)
    assert sum(len(x) for x in ids) > 5
    # the text of `transcribe` where the package's tokeniser reads the emitted ids back from it, the ids themselves elsewhere (a
    # piece that decodes to "" or a greedy re-segmentation makes a text read as other ids than the search emitted)
    texts = [r.text if tokenise(family, model, r.text) == i else i for r, i in zip(before, ids)]
    print(f"{family}: {sum(isinstance(t, str) for t in texts)} of {len(texts)} texts go through the tokeniser; labels {[len(i) for i in ids]}")
    if family != "nemo":
        assert any(isinstance(t, str) and t for t in texts), RECHOOSE + "a text the tokeniser reads back"
    batch = pkg.align_text_batch(model, audios, texts, cfg)
    seconds = [len(w) / 16000.0 for w in waves]
    for k, (r, i) in enumerate(zip(batch, ids)):
        assert isinstance(r, iface.AlignedTranscribeResult) and r.token_ids == i and r.text == before[k].text
        assert r.feasible and math.isfinite(r.log_likelihood) and r.log_likelihood >= r.alignment_log_prob
        assert r.norm_log_likelihood == r.log_likelihood / max(len(i), 1) and len(r.token_logprobs) == len(i)
        assert all(v <= 1e-6 for v in r.token_logprobs)
        # inside the audio the model was given, on the clock of `transcribe`: nemo pads 0.5 s on both sides inside the front-end and
        # takes the left one off its times, k2's times are on the audio with 0.9 s on both sides, espnet's are clamped to the window;
        # the last encoder frame may begin up to one stride before the end
        pad = {"nemo": 0.5 + 0.08, "k2": 2 * 0.9, "espnet": 0.0}[family]
        times = r.token_seconds if family == "espnet" else [s.seconds for s in r.subwords]
        assert all(0.0 <= t <= seconds[k] + pad for t in times) and all(y >= x for x, y in zip(times, times[1:]))
        if family != "nemo":
            assert len(times) == len(i)
    single = pkg.align_text(model, audios[1], texts[1], cfg)
    assert single == batch[1]
    # 9 utterances at max_batch = 4 == one batch
    run = am.align_waveforms if family == "nemo" else model.am.align_waveforms
    prep = {"nemo": lambda: [np.ascontiguousarray(w, np.float32) for w in waves],
            "k2": lambda: [a.waveform for a in tr._prepare_batch(model, audios)],
            "espnet": lambda: [np.pad(np.asarray(w, np.float32), tr.PADDING, mode="constant") for w in waves]}[family]()
    kw = {"one_per_frame": False} if family == "espnet" else {}
    whole, parts = run(prep, ids, **kw), run(prep, ids, max_batch=4, **kw)
    assert whole == parts and whole.log_likelihood == [r.log_likelihood for r in batch] and whole.frames == parts.frames
    owner = am if family == "nemo" else model.am               # a batch whose lattice is beyond one call's bound is halved: same results
    cells = max(owner.stage(prep).tp_max * (len(i) + 1) for i in ids)
    owner.ALIGN_MAX_CELLS = 3 * cells
    try:
        assert run(prep, ids, **kw) == whole
        owner.ALIGN_MAX_CELLS = cells // 2
        with pytest.raises(ValueError, match="window the audio"):
            run(prep, ids, **kw)
    finally:
        del owner.ALIGN_MAX_CELLS
    # an infeasible text does not raise
    if family == "k2":
        r = pkg.align_text(model, iface.AudioData(np.zeros(160, np.float32), 16000), [5] * 400, cfg)
        assert r.feasible is False and r.log_likelihood == -math.inf and r.alignment_log_prob == -math.inf and r.subwords == []
    # transcribe is what it was
    after = tr.transcribe_batch(model, audios, cfg)
    assert after == before and tr.transcribe(model, audios[1], cfg) == one_before
