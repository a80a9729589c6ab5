"""-m gpu: several texts per utterance on one lattice (rs_rnnt_align_rows, rs_rnnt_token_scores_rows; csrc/k_rnnt_align.hip,
csrc/k_rnnt_scores.hip).  Every comparison is exact equality of bits: row r of the rows entry against rs_rnnt_align /
rs_rnnt_token_scores on a batch of R utterances whose row r is a copy of utterance row_utt[r] (the guarantee of include/rs_asr.h),
against the C checker (tests/rnnt_align_checker.c) on the same replicated batch, and `stats` against the sharing rule restated in
tests/rnnt_align_rows_ref.py.

  the group scene, family x topology   utterances of 9, 5 and 2 frames (random projections).  Utterance 0: [a b c d], [a b x y],
                                [a b x z] (a chain through two donors), [a b c d] again, [a b] (a prefix), [f] (nothing shared);
                                utterance 1: the empty text alone; utterance 2: [a b c] first (infeasible with one label per frame:
                                never a donor), then [a b] and [a]; one -1 row inside utterance 0's group with sentinels in its slots
  chunking                      the minimum workspace (32 lattice rows per chunk: groups straddle chunks) == a generous one
  the sharing flag              RS_ALIGN_NO_SHARING == sharing, stats[0] == stats[1] under the flag
  identity                      row_utt = arange(B), one text each == rs_rnnt_align
  more cells than DP threads    U = 300 sharing 290 labels with its donor, T = 3 (standard) and T = 301 (one per frame)
  real output widths            3001 / 10 720 logits: one utterance, T = 4, three texts
  errors                        row_utt >= B, decreasing, 65 rows on one utterance: RS_EINVAL and nothing written; a bad id in a row
                                that would have been a donor: NaN / -1 there, the rows after it keep their bits; argument errors
                                before any launch
  rs_rnnt_token_scores_rows     == rs_rnnt_token_scores on replicated frames for greedy results and for ALSD's alignment steps;
                                skipped rows untouched
  the public surface            per family, a synthetic tiny model with its beam search, nbest = 3, rescore = "likelihood", token scores
                                on: every entry's log_likelihood / alignment_log_prob == align_text of (the same audio, the entry's
                                ids); the list in descending order, search_rank a permutation consistent with the search's own list,
                                ties in its order; entry 0 is the result; every entry carries token_logprobs and the search's own
                                best carries the ones it carries without rescoring; score_texts == align_text per text;
                                align_candidates with and without sharing; rescore off == a model that never had it
"""
import numpy as np
import pytest
import torch

import rnnt_align_ref as A
import rnnt_align_rows_ref as RR
import token_scores_ref as R
from reazonspeech_amd.runtime import capi
from reazonspeech_amd.runtime.avsr_config import AVSR_TINY
from reazonspeech_amd.runtime.config import ESPNET_TINY, TINY, WIDE2  # noqa: F401
from reazonspeech_amd.runtime.k2_config import ZIPFORMER_TINY
from test_gpu_rnnt_align import GENEROUS, device_align, random_case, same_bits
from test_gpu_token_scores import build, dev_i32, device_beam_rows, device_scores, public, scene as greedy_scene

pytestmark = pytest.mark.gpu
FAMILIES = ("nemo", "espnet", "k2")
CASES = [(f, one) for f in FAMILIES for one in (False, True)]
KEYS = ("loglik", "best", "frames", "logp")


def device_align_rows(am, f, lens, row_utt, ids, n, one, workspace="generous", share=True, want_code=None):
    """rs_rnnt_align_rows -> (dict(loglik, best [R]; frames, logp [R][u_cap]), stats); untouched slots hold 7.0 / -9"""
    B, Tp, _ = f.shape
    Rn, u_cap = ids.shape
    dev = am.device
    loglik, best = torch.full((Rn,), 7.0, device=dev), torch.full((Rn,), 7.0, device=dev)
    frames = torch.full((Rn, u_cap), -9, dtype=torch.int32, device=dev)
    logp = torch.full((Rn, u_cap), 7.0, dtype=torch.float32, device=dev)
    least = am.ctx.align_rows_workspace_bytes(B, Rn, Tp, u_cap)
    ws = torch.empty((least if workspace == "minimum" else least + GENEROUS,), dtype=torch.uint8, device=dev)
    args = (f, dev_i32(am, lens), B, Tp, dev_i32(am, row_utt), dev_i32(am, ids), dev_i32(am, n), loglik, best, frames, logp, ws,
            torch.cuda.current_stream().cuda_stream)
    stats = None
    if want_code is None:
        stats = am.ctx.rnnt_align_rows(*args, one_per_frame=one, share=share)
    else:
        with pytest.raises(capi.RsError) as e:
            am.ctx.rnnt_align_rows(*args, one_per_frame=one, share=share)
        assert e.value.code == want_code
    torch.cuda.synchronize()
    return dict(loglik=loglik.cpu().numpy(), best=best.cpu().numpy(), frames=frames.cpu().numpy(), logp=logp.cpu().numpy()), stats


def replicated(am, sd, f, lens, row_utt, ids, n, one, checker=True):
    """what the guarantee names: rs_rnnt_align (and the C checker) on the batch whose row r is a copy of utterance row_utt[r]"""
    fr, lr = RR.replicate(f, lens, row_utt)
    want = device_align(am, fr, lr, ids, n, one)
    if checker:
        c = A.align_checker(am.cfg, sd, fr.cpu().numpy(), np.asarray(lr, np.int32), ids, n, one_per_frame=one)
        valid = np.arange(ids.shape[1])[None, :] < n[:, None]
        assert same_bits(c["loglik"], want["loglik"]) and same_bits(c["best"], want["best"])
        assert (c["frames"][valid] == want["frames"][valid]).all() and same_bits(c["logp"][valid], want["logp"][valid])
    return want


def assert_rows(got, want, row_utt, n):
    """rows with an utterance: every slot as rs_rnnt_align leaves it (the untouched ones included); skipped rows: the sentinels"""
    for r, u in enumerate(row_utt):
        if u < 0:
            assert got["loglik"][r] == 7.0 and got["best"][r] == 7.0 and (got["frames"][r] == -9).all() and (got["logp"][r] == 7.0).all(), r
        else:
            for k in KEYS:
                assert same_bits(got[k][r], want[k][r]), (r, k, got[k][r], want[k][r])


def labels(cfg, count, seed=0):
    V = cfg.vocab_size if R.is_k2(cfg) else cfg.n_logits
    banned = {cfg.blank_id, getattr(cfg, "unk_id", -1)}
    ok = [v for v in range(V) if v not in banned]
    g = torch.Generator().manual_seed(seed)
    return [ok[i] for i in torch.randperm(len(ok), generator=g)[:count].tolist()], V


_groups = {}


def group_scene(family, one):
    """once per case: the scene, what the guarantee gives for it, and the device's result with sharing on a generous workspace"""
    if (family, one) not in _groups:
        am, sd, cfg = greedy_scene(family)[:3]
        lens = [9, 5, 2]
        f, _ = random_case(am, cfg, lens, [0, 0, 0], 6)
        (a, b, c, d, x, y, z, q), V = labels(cfg, 8)
        texts = [[a, b, c, d], [a, b, x, y], [a, b, x, z], [q, q], [a, b, c, d], [a, b], [q], [], [a, b, c], [a, b], [a]]
        row_utt = [0, 0, 0, -1, 0, 0, 0, 1, 2, 2, 2]
        ids, n = R.pack(texts, 5)                            # u_cap above the longest text: the pitch is not the length
        want = replicated(am, sd, f, lens, row_utt, ids, n, one)
        got, stats = device_align_rows(am, f, lens, row_utt, ids, n, one)
        plan = RR.plan(row_utt, lens, texts, V, cfg.blank_id, one, u_cap=5)
        print(f"{family} one_per_frame={one}: m {plan['m']}, donor {plan['donor']}, stats {stats}, loglik {got['loglik'].tolist()}")
        _groups[(family, one)] = (am, sd, cfg, f, lens, texts, row_utt, ids, n, want, got, stats, plan)
    return _groups[(family, one)]


@pytest.mark.parametrize("family,one", CASES)
def test_group_scene_equals_align_on_replicated_frames(gpu_device, family, one):
    am, sd, cfg, f, lens, texts, row_utt, ids, n, want, got, stats, plan = group_scene(family, one)
    assert plan["err"] == 0 and plan["m"][:7] == [0, 2, 3, 0, 4, 2, 0] and plan["donor"][:7] == [-1, 0, 1, -1, 0, 0, -1]
    assert (plan["m"][8:], plan["donor"][8:]) == (([0, 0, 1], [-1, -1, 9]) if one else ([0, 2, 1], [-1, 8, 8]))
    assert_rows(got, want, row_utt, n)
    assert stats == plan["stats"] and stats[0] < stats[1]
    assert np.isfinite(got["loglik"][[0, 1, 2, 4, 5, 6, 7, 9, 10]]).all() and got["loglik"][0].tobytes() == got["loglik"][4].tobytes()
    assert (got["loglik"][8] == -np.inf) == bool(one)


@pytest.mark.parametrize("family,one", CASES)
def test_chunking_gives_the_same_bits(gpu_device, family, one):
    am, sd, cfg, f, lens, texts, row_utt, ids, n, want, got, stats, plan = group_scene(family, one)
    start = np.cumsum([0] + plan["owned"])
    assert stats[0] > 64 and any(start[r] // 32 != (start[r + 1] - 1) // 32 for r in (1, 2, 4, 5)), "a group must straddle chunks"
    small, small_stats = device_align_rows(am, f, lens, row_utt, ids, n, one, workspace="minimum")
    assert small_stats == stats and all(same_bits(small[k], got[k]) for k in KEYS)


@pytest.mark.parametrize("family,one", CASES)
def test_no_sharing_gives_the_same_bits(gpu_device, family, one):
    am, sd, cfg, f, lens, texts, row_utt, ids, n, want, got, stats, plan = group_scene(family, one)
    for workspace in ("generous", "minimum"):
        flat, flat_stats = device_align_rows(am, f, lens, row_utt, ids, n, one, workspace=workspace, share=False)
        assert flat_stats == (stats[1], stats[1]) and all(same_bits(flat[k], got[k]) for k in KEYS)


@pytest.mark.parametrize("family,one", CASES)
def test_identity_map_equals_align(gpu_device, family, one):
    am, sd, cfg = greedy_scene(family)[:3]
    lens, counts = [7, 0, 4, 1, 6], [3, 0, 4, 2, 0]
    f, texts = random_case(am, cfg, lens, counts, 8)
    ids, n = R.pack(texts, 4)
    want = device_align(am, f, lens, ids, n, one)
    got, stats = device_align_rows(am, f, lens, list(range(5)), ids, n, one)
    assert all(same_bits(got[k], want[k]) for k in KEYS) and stats[0] == stats[1] > 0


@pytest.mark.parametrize("family,one,T", [("nemo", False, 3), ("k2", True, 301)])
def test_more_cells_than_dp_threads(gpu_device, family, one, T):
    am, sd, cfg = greedy_scene(family)[:3]
    f, (long_text,) = random_case(am, cfg, [T], [300], 10)
    (p, q), V = labels(cfg, 2, seed=1)
    other = long_text[:290] + [p if long_text[290 + k] != p else q for k in range(10)]
    texts, row_utt = [long_text, other, long_text[:295]], [0, 0, 0]
    ids, n = R.pack(texts, 300)
    # (T = 301: 3 x 301 x 301 cells through the serial C checker would take this case beyond its few seconds; rs_rnnt_align, which
    #  the rows are compared with there, equals the checker by tests/test_gpu_rnnt_align.py — the hardware is not the reason)
    want = replicated(am, sd, f, [T], row_utt, ids, n, one, checker=T == 3)
    got, stats = device_align_rows(am, f, [T], row_utt, ids, n, one)
    plan = RR.plan(row_utt, [T], texts, V, cfg.blank_id, one)
    assert plan["m"] == [0, 290, 295] and plan["donor"] == [-1, 0, 0] and stats == plan["stats"]
    assert_rows(got, want, row_utt, n)
    assert np.isfinite(got["loglik"]).all()
    small = device_align_rows(am, f, [T], row_utt, ids, n, one, workspace="minimum")[0] if T == 3 else got
    assert all(same_bits(small[k], got[k]) for k in KEYS)


@pytest.mark.parametrize("shape", ["nemo-3001", "k2-10720"])
def test_real_output_widths(gpu_device, shape):
    if shape == "nemo-3001":
        am, sd, cfg, _ = build("nemo", WIDE2)
    else:
        am, sd, cfg, _ = build("k2", ZIPFORMER_TINY.with_(vocab_size=10720, decoder_dim=512, joiner_dim=512).validate())
    one = R.is_k2(cfg)
    f, (t0,) = random_case(am, cfg, [4], [3], 2)
    (p, q), V = labels(cfg, 2, seed=3)
    texts, row_utt = [t0, t0[:2] + [p if t0[2] != p else q], t0[:1]], [0, 0, 0]
    ids, n = R.pack(texts, 3)
    want = replicated(am, sd, f, [4], row_utt, ids, n, one)
    got, stats = device_align_rows(am, f, [4], row_utt, ids, n, one)
    assert_rows(got, want, row_utt, n)
    assert stats == RR.plan(row_utt, [4], texts, V, cfg.blank_id, one)["stats"] == (4 * 4 + 4 * 2 + 4 * 1, 4 * 4 + 4 * 4 + 4 * 2)
    small = device_align_rows(am, f, [4], row_utt, ids, n, one, workspace="minimum")[0]
    assert all(same_bits(small[k], got[k]) for k in KEYS)


def test_row_utt_errors_write_nothing(gpu_device):
    am, sd, cfg, f, lens, texts, row_utt, ids, n, want, good, stats, plan = group_scene("nemo", False)
    untouched = lambda got: all((got[k] == (-9 if k == "frames" else 7.0)).all() for k in KEYS)      # noqa: E731
    for bad in ([0, 0, 0, -1, 0, 0, 0, 1, 2, 2, 3],         # an utterance >= B
                [0, 0, 0, -1, 0, 0, 0, 1, 2, 2, -2],        # below -1
                [0, 0, 0, -1, 0, 0, 1, 0, 2, 2, 2]):        # a decrease
        got, _ = device_align_rows(am, f, lens, bad, ids, n, False, want_code=capi.RS_EINVAL)
        assert untouched(got), bad
    many_ids, many_n = np.repeat(ids[:1], 65, 0), np.repeat(n[:1], 65)
    got, _ = device_align_rows(am, f, lens, [0] * 65, many_ids, many_n, False, want_code=capi.RS_EINVAL)
    assert untouched(got)
    got, st = device_align_rows(am, f, lens, [0] * 64, many_ids[:64], many_n[:64], False)             # 64 rows are fine
    assert st == (9 * 5 + 63 * 9, 64 * 9 * 5) and all(got["loglik"][r].tobytes() == good["loglik"][0].tobytes() for r in range(64))


def test_a_bad_row_is_no_donor(gpu_device):
    am, sd, cfg, f, lens, texts, row_utt, ids, n, want, good, stats, plan = group_scene("nemo", False)
    bad_ids = ids.copy()
    bad_ids[0, 1] = cfg.blank_id                            # row 0 gave columns to rows 1, 4 and 5
    got, _ = device_align_rows(am, f, lens, row_utt, bad_ids, n, False, want_code=capi.RS_EINVAL)
    assert np.isnan(got["loglik"][0]) and np.isnan(got["best"][0]) and (got["frames"][0, :4] == -1).all() and np.isnan(got["logp"][0, :4]).all()
    assert got["frames"][0, 4] == -9 and got["logp"][0, 4] == 7.0
    others = [r for r in range(len(row_utt)) if r != 0]
    keep = {k: np.delete(got[k], 0, 0) for k in KEYS}
    assert_rows(keep, {k: np.delete(want[k], 0, 0) for k in KEYS}, [row_utt[r] for r in others], n[others])


def test_argument_errors_come_before_any_launch(gpu_device):
    am, sd, cfg, f, lens, texts, row_utt, ids, n, want, good, stats, plan = group_scene("nemo", False)
    B, Tp, _ = f.shape
    Rn, dev = 4, am.device
    z = lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)       # noqa: E731
    ll, best, frames, logp = torch.full((Rn,), 7.0, device=dev), torch.full((Rn,), 7.0, device=dev), z(Rn, 8) - 9, torch.full((Rn, 8), 7.0, device=dev)
    least = am.ctx.align_rows_workspace_bytes(B, Rn, Tp, 8)
    assert least >= am.ctx.align_workspace_bytes(Rn, Tp, 8)
    ws = torch.empty((least,), dtype=torch.uint8, device=dev)
    el = dev_i32(am, lens)
    args = lambda ctx, **kw: ctx.rnnt_align_rows(f, el, B, Tp, z(Rn), z(Rn, 8), z(Rn), ll, best, frames, logp, ws, 0, **kw)   # noqa: E731
    with pytest.raises(capi.RsError, match="workspace") as e:
        args(am.ctx, ws_bytes=least - 1)
    assert e.value.code == capi.RS_EINVAL
    for other in (capi.Context(AVSR_TINY, 0), capi.Context(TINY, 0)):   # an AV-HuBERT context; a context that was never finalized
        with pytest.raises(RuntimeError):
            other.align_rows_workspace_bytes(B, Rn, Tp, 8)
        with pytest.raises(capi.RsError) as e:
            args(other)
        assert e.value.code == capi.RS_EINVAL
        other.close()
    lib, h = am.ctx.lib, am.ctx._h
    p = lambda t: t.data_ptr()                                          # noqa: E731
    full = (p(f), p(el), B, Tp, p(z(Rn)), Rn, p(z(Rn, 8)), p(z(Rn)), 8, 0, p(ll), p(best), p(frames), p(logp), None, p(ws), least, None)
    for at, value in ((2, -1), (3, -1), (5, -1), (8, -1), (9, 4), (8, capi.ALIGN_U_CAP_MAX + 1), (0, None), (4, None), (10, None), (15, None),
                      (2, 0)):
        bad = list(full)
        bad[at] = value
        assert lib.rs_rnnt_align_rows(h, *bad) == capi.RS_EINVAL, (at, value)
    assert lib.rs_rnnt_align_rows_workspace_bytes(h, B, Rn, Tp, capi.ALIGN_U_CAP_MAX + 1) == 0
    assert lib.rs_rnnt_align_rows_workspace_bytes(h, 0, Rn, Tp, 8) == 0 and lib.rs_rnnt_align_rows_workspace_bytes(h, B, 0, Tp, 8) == 0
    assert lib.rs_rnnt_token_scores_rows(h, p(f), p(el), B, Tp, None, Rn, p(z(Rn, 8)), p(z(Rn, 8)), p(z(Rn)), 8, 0, p(logp), None, p(ws), least,
                                         None) == capi.RS_EINVAL
    torch.cuda.synchronize()
    assert (ll == 7.0).all() and (frames == -9).all() and (logp == 7.0).all()              # nothing was written
    assert args(am.ctx) == (4 * 9, 4 * 9)                   # four empty texts on utterance 0: one column each, nothing to share
    torch.cuda.synchronize()
    assert (frames == -9).all() and (logp == 7.0).all() and len(set(ll.cpu().numpy().tobytes()[i:i + 4] for i in range(0, 16, 4))) == 1


# ---- rs_rnnt_token_scores_rows ------------------------------------------------------------------------------------------------
def device_scores_rows(am, f, lens, row_utt, ids, frames, n, steps=False, workspace="generous", want_code=None):
    B, Tp, _ = f.shape
    Rn, u_cap = ids.shape
    logp = torch.full((Rn, u_cap), 7.0, dtype=torch.float32, device=am.device)
    top1 = torch.full((Rn, u_cap), -9, dtype=torch.int32, device=am.device)
    least = am.ctx.token_scores_rows_workspace_bytes(B, Rn, u_cap)
    ws = torch.empty((least if workspace == "minimum" else least + (64 << 20),), dtype=torch.uint8, device=am.device)
    args = (f, dev_i32(am, lens), B, Tp, dev_i32(am, row_utt), dev_i32(am, ids), dev_i32(am, frames), dev_i32(am, n), logp, top1, ws,
            torch.cuda.current_stream().cuda_stream)
    if want_code is None:
        am.ctx.rnnt_token_scores_rows(*args, frames_are_steps=steps)
    else:
        with pytest.raises(capi.RsError) as e:
            am.ctx.rnnt_token_scores_rows(*args, frames_are_steps=steps)
        assert e.value.code == want_code
    torch.cuda.synchronize()
    return logp.cpu().numpy(), top1.cpu().numpy()


@pytest.mark.parametrize("family,kind", [("nemo", "greedy"), ("espnet", "greedy"), ("k2", "greedy"), ("nemo", "alsd-steps")])
def test_token_scores_rows_equal_the_entry_on_replicated_frames(gpu_device, family, kind):
    am, sd, cfg, f, lens, rows = greedy_scene(family)
    steps = False
    if kind == "alsd-steps":
        rows, steps = device_beam_rows(family, am, cfg, f, lens)
        assert steps
    rich = sorted(range(len(rows)), key=lambda b: -len(rows[b][0]))
    assert len(rows[rich[1]][0]) >= 2
    # every utterance once, the two richest three times (whole, a prefix, whole), one skipped row inside a group
    row_utt, texts = [], []
    for b in range(len(rows)):
        i, fr = rows[b]
        row_utt.append(b), texts.append((i, fr))
        if b in rich[:2]:
            row_utt.append(-1), texts.append((i[:1], fr[:1]))
            row_utt.append(b), texts.append((i[:len(i) // 2], fr[:len(i) // 2]))
            row_utt.append(b), texts.append((i, fr))
    u_cap = max(len(t[0]) for t in texts)
    ids, n = R.pack([t[0] for t in texts], u_cap)
    frames, _ = R.pack([t[1] for t in texts], u_cap)
    fr_, lr_ = RR.replicate(f, lens, row_utt)
    n_live = np.where(np.asarray(row_utt) >= 0, n, 0).astype(np.int32)
    want_lp, want_t1 = device_scores(am, fr_, lr_, ids, frames, n_live, steps=steps)
    assert n_live.sum() > 32 and not np.isnan(want_lp[np.arange(u_cap)[None, :] < n_live[:, None]]).any()
    for workspace in ("generous", "minimum"):
        lp, t1 = device_scores_rows(am, f, lens, row_utt, ids, frames, n, steps=steps, workspace=workspace)
        assert same_bits(lp, want_lp) and same_bits(t1, want_t1)         # the skipped rows and the slots past n_ids hold 7.0 / -9 in both
    skipped = [r for r, u in enumerate(row_utt) if u < 0]
    assert skipped and (lp[skipped] == 7.0).all() and (t1[skipped] == -9).all()
    bad = list(row_utt)
    bad[-1] = len(rows)
    lp, t1 = device_scores_rows(am, f, lens, bad, ids, frames, n, steps=steps, want_code=capi.RS_EINVAL)
    assert (lp == 7.0).all() and (t1 == -9).all()


# ---- the public surface -------------------------------------------------------------------------------------------------------
def public_models(family):
    """(the package, its interface, a model with nbest = 3 alone, the same weights with rescore = "likelihood"), token scores on"""
    import importlib
    from reazonspeech_amd.espnet.asr.model import EspnetModel, synthetic_token_list
    from reazonspeech_amd.k2.asr.model import K2Model, synthetic_tokens
    from reazonspeech_amd.runtime.k2_weights import synthetic_state_dict_k2
    from reazonspeech_amd.runtime.weights_espnet import synthetic_state_dict_espnet
    pkg = importlib.import_module(f"reazonspeech_amd.{family}.asr")
    iface = importlib.import_module(f"reazonspeech_amd.{family}.asr.interface")
    if family == "nemo":
        kw = dict(device="cuda:0", config=TINY, decoding="alsd", beam_size=4, nbest=3, token_scores=True)
        return pkg, iface, pkg.load_model(**kw), pkg.load_model(rescore="likelihood", **kw)
    if family == "k2":
        sd, tok = synthetic_state_dict_k2(ZIPFORMER_TINY, 3), synthetic_tokens(ZIPFORMER_TINY.vocab_size, 3)
        kw = dict(device="cuda:0", decoding_method="modified_beam_search", nbest=3, token_scores=True)
        return pkg, iface, K2Model(ZIPFORMER_TINY, sd, tok, **kw), K2Model(ZIPFORMER_TINY, sd, tok, rescore="likelihood", **kw)
    sd, tok = synthetic_state_dict_espnet(ESPNET_TINY, 11, blank_bias=12.0, dec_gain=8.0), synthetic_token_list(ESPNET_TINY.vocab_size, 11)
    kw = dict(device="cuda:0", beam_size=6, nbest=3, token_scores=True)
    return pkg, iface, EspnetModel(ESPNET_TINY, sd, tok, **kw), EspnetModel(ESPNET_TINY, sd, tok, rescore="likelihood", **kw)


def public_lists(family, pkg, iface, model, audios, waves):
    """per audio the n-best list as [(token ids where the entry has them, the entry object, its text)] and the result's own ids,
    through the package's public call"""
    if family == "espnet":
        lists = model.recognize_batch(waves, nbest=3)
        return [[(ids, hyp, text) for text, _, ids, hyp in entries] for entries in lists], [entries[0][2] for entries in lists]
    res = pkg.transcribe_batch(model, audios, iface.TranscribeConfig(verbose=False))
    return [[(e.token_ids, e, e.text) for e in r.nbest] for r in res], [r.token_ids for r in res]


@pytest.mark.parametrize("family", FAMILIES)
def test_public_path(gpu_device, family):
    from reazonspeech_amd.runtime.synth import synthetic_batch
    pkg, iface, plain, model = public_models(family)
    assert (plain.rescore, model.rescore, model.nbest) == (None, "likelihood", 3)
    audio, lens = synthetic_batch(5, 2.0, seed=50, ragged=True, min_seconds=0.5)
    waves = [audio[b, :lens[b]] for b in range(5)]
    audios = [iface.AudioData(w, 16000) for w in waves]
    before, before_ids = public_lists(family, pkg, iface, plain, audios, waves)
    lists, own = public_lists(family, pkg, iface, model, audios, waves)
    moved = 0
    for k, (entries, searched) in enumerate(zip(lists, before)):
        assert 1 <= len(entries) == len(searched) and own[k] == entries[0][0]                     # entry 0 is the result
        ranks = [e.search_rank for _, e, _ in entries]
        assert sorted(ranks) == list(range(len(entries))) and [searched[r][2] for r in ranks] == [text for _, _, text in entries]
        lls = [e.log_likelihood for _, e, _ in entries]
        assert lls == sorted(lls, reverse=True) and all(x != y or a < b for (x, a), (y, b) in zip(zip(lls, ranks), zip(lls[1:], ranks[1:])))
        moved += ranks != sorted(ranks)
        for ids, e, _ in entries:
            want = pkg.align_text(model, audios[k], ids)
            assert (e.log_likelihood, e.alignment_log_prob, e.norm_log_likelihood) == (want.log_likelihood, want.alignment_log_prob, want.norm_log_likelihood)
            assert len(e.token_logprobs) == len(ids) and all(v <= 1e-6 for v in e.token_logprobs)   # every entry, not entry 0 alone
        first = next(e for _, e, _ in entries if e.search_rank == 0)                                # the search's own best: today's scores
        assert first.token_logprobs == searched[0][1].token_logprobs and all(e.token_logprobs is None for _, e, _ in searched[1:])
        scored = pkg.score_texts(model, audios[k], [ids for ids, _, _ in entries] + [[]])
        assert scored == [pkg.align_text(model, audios[k], ids) for ids, _, _ in entries] + [pkg.align_text(model, audios[k], [])]
    print(f"{family}: {moved} of {len(lists)} lists changed their order; lengths {[len(x) for x in lists]}")
    assert sum(len(x) for x in lists) > len(lists), RECHOOSE_LISTS
    both = pkg.score_texts_batch(model, audios[:2], [[ids for ids, _, _ in lists[0]], []])
    assert [r.log_likelihood for r in both[0]] == [e.log_likelihood for _, e, _ in lists[0]] and both[1] == []
    # the runtime entry: one encoder pass per utterance, the call's stats
    am = model if family == "nemo" else model.am
    prep = {"nemo": lambda: [np.ascontiguousarray(w, np.float32) for w in waves],
            "k2": lambda: [a.waveform for a in __import__("reazonspeech_amd.k2.asr.transcribe", fromlist=["x"])._prepare_batch(model, audios)],
            "espnet": lambda: [np.pad(np.asarray(w, np.float32), __import__("reazonspeech_amd.espnet.asr.transcribe", fromlist=["x"]).PADDING,
                                      mode="constant") for w in waves]}[family]()
    kw = {"one_per_frame": False} if family == "espnet" else {}
    cands = [[ids for ids, _, _ in entries] for entries in lists]
    got, stats = am.align_candidates(prep, cands, **kw)
    flat, flat_stats = am.align_candidates(prep, cands, share=False, max_batch=2, **kw)
    assert got == flat and flat_stats[0] == flat_stats[1] == stats[1] and stats[0] <= stats[1]
    assert [g.log_likelihood for g in got] == [[e.log_likelihood for _, e, _ in entries] for entries in lists]
    # every entry's token log-probabilities are what the existing entry gives for that hypothesis at its frames
    res = am.transcribe_waveforms(prep)
    buf = am.stage(prep)
    with torch.cuda.device(am.device):
        am.run_encoder(buf, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    f, el = buf.joint_enc[:len(prep)].contiguous(), buf.enc_lens.cpu().numpy()[:len(prep)]
    assert [[r[0] for r in rows] for rows in res.nbest] == [[ids for ids, _, _ in sorted(entries, key=lambda x: x[1].search_rank)] for entries in lists]
    for k in range(3):
        rows = [res.nbest[b][k][:2] if k < len(res.nbest[b]) else ([], []) for b in range(len(prep))]
        ids, n = R.pack([r[0] for r in rows], max(max(len(r[0]) for r in rows), 1))
        frames, _ = R.pack([r[1] for r in rows], ids.shape[1])
        lp, _ = device_scores(am, f, el, ids, frames, n)
        for b in range(len(prep)):
            if k < len(res.nbest[b]):
                assert res.rescored[b][k][2] == lp[b, :n[b]].tolist(), (k, b)
    # a batch beyond one call's bound is scored over several calls on the same projection: the same lists
    am.run_device(buf)
    torch.cuda.synchronize()
    one_utt = buf.nbest_n * buf.tp_max * (buf.nbest_bufs["ids"].shape[2] + 1)       # the lattice cells of one utterance's lists
    assert buf.rescored_n == 3 and buf.B == 5
    am.ALIGN_MAX_CELLS = 2 * one_utt                          # two utterances per call: three calls
    try:
        assert am.transcribe_waveforms(prep) == res
        am.ALIGN_MAX_CELLS = one_utt - 1
        with pytest.raises(ValueError, match="of one utterance"):
            am.transcribe_waveforms(prep)
    finally:
        del am.ALIGN_MAX_CELLS
    # rescore off: the objects of a model that never had it
    model.rescore = None
    off, off_ids = public_lists(family, pkg, iface, model, audios, waves)
    assert off_ids == before_ids
    if family == "espnet":
        assert [[(i, vars(h), t) for i, h, t in x] for x in off] == [[(i, vars(h), t) for i, h, t in x] for x in before]
    else:
        assert [[e for _, e, _ in x] for x in off] == [[e for _, e, _ in x] for x in before]
    if family != "nemo":                                    # (the nemo package's model is the runtime model: a plain attribute there)
        with pytest.raises(ValueError, match="must be None"):
            model.rescore = "best"


RECHOOSE_LISTS = "re-choose the inputs of this test: some list must hold more than one hypothesis"


def test_espnet_transcribe_batch_follows_the_reranked_best(gpu_device):
    """with rescore on, `transcribe_batch` (both segmentations, with and without token scores) returns what `transcribe` returns:
    the re-ranked best of every window, not the search's own; and the greedy fall-back's list of one is scored too"""
    import warnings
    from reazonspeech_amd.espnet.asr import transcribe as etr_api  # noqa: F401
    from reazonspeech_amd.runtime.synth import synthetic_batch
    pkg, iface, plain, model = public_models("espnet")
    etr = __import__("reazonspeech_amd.espnet.asr.transcribe", fromlist=["x"])
    audio, lens = synthetic_batch(5, 2.0, seed=50, ragged=True, min_seconds=0.5)
    waves = [audio[b, :lens[b]] for b in range(5)]
    audios = [iface.AudioData(w, 16000) for w in waves]
    conf = iface.TranscribeConfig(verbose=False)
    lists = model.recognize_batch(waves, nbest=3)
    moved = [b for b, entries in enumerate(lists) if entries[0][3].search_rank != 0]
    print(f"espnet: full likelihood moves another entry to the top in windows {moved} of 5")
    assert moved, RECHOOSE_LISTS + ", and full likelihood must change the best of one"
    assert model.recognize_batch(waves) == [entries[0][0] for entries in lists]
    texts, scored = model.recognize_batch_scored(waves)
    assert texts == [entries[0][0] for entries in lists]
    assert scored == [(entries[0][2], entries[0][3].token_logprobs) for entries in lists]
    for with_scores in (True, False):
        model.token_scores = with_scores
        single = [etr.transcribe(model, a, conf) for a in audios]
        assert [r.text for r in single] == [entries[0][0] for entries in lists]
        for mode in ("host", "device"):
            model.segmentation = mode
            assert etr.transcribe_batch(model, audios, conf) == single, (with_scores, mode)
        model.segmentation = "host"
    model.token_scores = True
    assert any(a.text != b.text for a, b in zip(single, etr.transcribe_batch(plain, audios, conf)))     # (it is the re-ranking that shows)
    # the greedy fall-back (every beam decode made to overflow): its list of one is scored, as align_text scores that text
    real = model.am.decode

    def overflowing(ctx, buf, ws, stream, max_pops=None, decoding=None, nbest=None):
        if decoding is None:
            raise capi.RsError(capi.RS_EOVERFLOW, "beam search: a frame needed more than max_pops")
        return real(ctx, buf, ws, stream, max_pops=max_pops, decoding=decoding, nbest=nbest)
    model.am.decode = overflowing
    try:
        with warnings.catch_warnings(record=True):
            warnings.simplefilter("always")
            fell = model.recognize_batch(waves, nbest=3)
            alone = model.recognize_batch(waves[:2], nbest=3, isolate_overflow=True)
            texts = model.recognize_batch(waves)
    finally:
        model.am.decode = real
    assert [len(x) for x in fell] == [1] * 5 and texts == [x[0][0] for x in fell]
    for k, ((_, _, ids, hyp),) in enumerate(fell):
        want = pkg.align_text(model, audios[k], ids)
        assert (hyp.log_likelihood, hyp.alignment_log_prob, hyp.search_rank) == (want.log_likelihood, want.alignment_log_prob, 0)
        assert hyp.token_logprobs is not None and len(hyp.token_logprobs) == len(ids) and np.isnan(hyp.score)
    assert [(x[0][2], x[0][3].log_likelihood) for x in alone] == [(x[0][2], x[0][3].log_likelihood) for x in fell[:2]]
    # a refused value leaves the model's option as it was
    with pytest.raises(ValueError, match="must be None"):
        model.recognize_batch(waves, nbest=3, rescore="best")
    with pytest.raises(ValueError, match="nbest >= 2"):
        model.recognize_batch(waves, nbest=1, rescore="likelihood")
    assert model.rescore == "likelihood"
    assert [[e[2] for e in x] for x in model.recognize_batch(waves, nbest=3, rescore=False)] == [[e[2] for e in x] for x in plain.recognize_batch(waves, nbest=3)]
    assert model.rescore == "likelihood"
