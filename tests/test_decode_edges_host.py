"""Every fixture of tests/decode_edges_ref.py reaches the edge it was built for — shown on the CPU oracle alone (oracle/rnnt_greedy.c,
oracle/k2_greedy.c), so that tests/test_gpu_decode_edges.py cannot pass vacuously:
  * tied / near-tied blocks: the expected winner is emitted at least 10 times and no other column of the block ever is (the block has
    at least N columns with bit-identical screening logits: the candidate count is a property of the weights, not of the kernel);
    for near-ties a float64 evaluation of the same logits confirms that the raised copy is strictly the largest of the block;
  * the cap binds: some frame carries exactly max_symbols labels, some utterance emits on its last frame;
  * ragged rows: more than B tokens, and the loop's schedule replayed from the oracle's frames crosses the planned live-row seams;
  * the numpy model of the screen's candidate test EXCLUDES the true winner of the small-activation fixtures when the threshold is
    formed as m - 2 eps, includes it on every other fixture, and includes it everywhere with the margin of screen_margin (k_rnnt.hip).
"""
import numpy as np
import pytest

import decode_edges_ref as de


tokens, check_block = de.tokens, de.check_block


# ---- candidate lists --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,knobs,kw", de.block_cases(), ids=[c[0] for c in de.block_cases()])
def test_block_winner_decides_emissions(name, knobs, kw):
    case = de.tied_block(**kw)
    cfg, sd, f, lens, rec = case
    res = de.oracle(case)
    check_block(case, res)
    # the oracle's decisions one by one, up to the second one the block wins: float64 ordering inside the block, and the screen model keeps the winner
    W, b = sd[de.JOUT + ".weight"], sd[de.JOUT + ".bias"]
    W64, b64 = W.double().numpy(), b.double().numpy()
    cols, win = rec["cols"], rec["winner"]
    rest = [c for c in cols if c != win]
    won = 0
    steps = (x for u in range(f.shape[0]) for x in de.walk(cfg, sd, f[u].numpy(), int(lens[u]), 40))
    for a, logits, k in steps:
        if won >= 2:
            break
        z64 = (W64[cols] * a.astype(np.float64)[None, :]).sum(1) + b64[cols]          # every row in the same summation order
        zw = float(z64[cols.index(win)])
        if rec["kind"] == "near":
            assert (a > 0).any() and zw > z64[[cols.index(c) for c in rest]].max(), "the raised copy is strictly the largest in float64"
            assert logits[win] > logits[rest].max(), "... and in the oracle's float32"
        else:
            assert np.all(logits[cols] == logits[win]) and np.all(z64 == zw), "an exact tie"
        if k != win:
            continue
        won += 1
        for form in ("m-2eps", "margin"):
            z, mask = de.screen_model(a, W, b, form)
            assert mask[win], form
            assert len(set(z[cols].tolist())) == 1 and mask[cols].all(), "the block's screening logits are bit-identical"
    assert won >= 2


@pytest.mark.parametrize("V", [512, 3072])
def test_all_columns_tied(V):
    case = de.all_tied(V)
    cfg, sd, f, lens, rec = case
    res = de.oracle(case)
    toks = tokens(res)
    assert set(toks) == {0} and len(toks) == int(lens.sum()) * cfg.max_symbols >= 10
    a, logits, k = next(de.walk(cfg, sd, f[int(np.argmax(lens.numpy()))].numpy(), int(lens.max()), 1))
    assert k == 0 and np.all(logits[:V - 1] == logits[0]) and logits[V - 1] < logits[0]
    for form in ("m-2eps", "margin"):
        assert de.screen_model(a, sd[de.JOUT + ".weight"], sd[de.JOUT + ".bias"], form)[1].all(), "all V columns are candidates"


def test_j640_near_tie():
    case = de.tied_block(V=3001, start=60, N=9, raised=68, wide=True, B=2, Tp=10)
    assert case[0].joint_hidden == 640
    check_block(case, de.oracle(case))


def test_other_families():
    check_block(de.k2_tied(), de.oracle(de.k2_tied()))
    assert de.k2_tied()[0].unk_id in de.k2_tied()[4]["cols"]
    check_block(de.espnet_tied(), de.oracle(de.espnet_tied()))
    assert de.espnet_tied()[0].blank_id == 0


# ---- small activation rows ----------------------------------------------------------------------------------------------------
SMALL = de.small_cases()


@pytest.mark.parametrize("name,build", SMALL, ids=[s[0] for s in SMALL])
def test_small_activation_defeats_the_first_threshold_only(name, build):
    case = build()
    cfg, sd, f, lens, rec = case
    res = de.oracle(case)
    toks = tokens(res)
    win, lose = rec["winner"], rec["loser"]
    assert set(toks) == {win} and len(toks) == int(lens.sum()) * cfg.max_symbols >= 10
    W, b = sd[de.JOUT + ".weight"], sd[de.JOUT + ".bias"]
    n = 0
    for a, logits, k in de.walk(cfg, sd, f[0].numpy(), int(lens[0]), 4):
        n += 1
        assert k == win
        z64 = W.double().numpy()[[win, lose]] @ a.astype(np.float64) + b.double().numpy()[[win, lose]]
        if rec["kind"] == "small_onehot":
            # a tie of the float32 logits: the float64 values differ by less than half an ulp of 8
            assert logits[win] == logits[lose] == 8.0 and win < lose
            assert z64[1] > z64[0] and np.float32(z64[1]) == np.float32(z64[0]) == 8.0
        else:
            assert logits[win] > logits[lose] and z64[0] > z64[1]
        z, mask = de.screen_model(a, W, b, "m-2eps")
        assert z[lose] > z[win], "the screening order is the other way round"
        if rec["kind"] == "small_pair" and rec["exp"] == -70:
            # ||a||^2 = 2^-139 is a float32 subnormal: the row norm survives exactly where subnormals do
            assert mask[win] and not de.screen_model(a, W, b, "m-2eps", ftz=True)[1][win]
        else:
            assert not mask[win], "m - 2 eps excludes the true winner"
            assert not de.screen_model(a, W, b, "m-2eps", ftz=True)[1][win]
        assert mask[lose]
        for ftz in (False, True):
            assert de.screen_model(a, W, b, "margin", ftz=ftz)[1][[win, lose]].all(), "screen_margin keeps both"
    assert n == 4


def test_straddling_pairs_are_searched_not_hard_coded():
    a_vals, w = de.find_straddling_pairs()
    f32 = np.float32
    for a in a_vals:
        assert f32(f32(f32(a) * f32(w)) + f32(8)) == 8.0
        assert f32(np.float64(de._bf16_np(a)) * np.float64(de._bf16_np(w))) + f32(8) > 8.0


# ---- the cap ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,Tp", [(5, 24), (40, 24), (100, 24), (5, 3)])
@pytest.mark.parametrize("ms", [1, 2, 3])
def test_cap_binds(ms, B, Tp):
    case = de.binding_cap(ms, B, Tp)
    cfg, sd, f, lens, rec = case
    res = de.oracle(case)
    assert cfg.max_symbols == ms and len(tokens(res)) > B
    per_frame = [np.bincount(r[1], minlength=int(n)) for r, n in zip(res, lens) if int(n) > 0]
    assert max(int(c.max()) for c in per_frame) == ms, "some frame carries exactly max_symbols labels"
    assert any(c[-1] > 0 for c in per_frame), "some utterance emits on its last frame"
    if Tp > 8:
        # inside a look-ahead window: a window of 8 frames holds a frame the cap ended
        chunks, _ = de.replay(res, lens.numpy(), ms, lookahead=True)
        assert any(la > 1 for _, la in chunks)


# ---- ragged rows ----------------------------------------------------------------------------------------------------------------
def seams_crossed(bounds, seam):
    return max(bounds) > seam >= min(bounds)


@pytest.mark.parametrize("V", de.SEAM_V)
def test_ragged_rows_at_every_verify_seam(V):
    case = de.ragged_rows(V, 9, 32 if V > 4000 else de.TP_MAX)
    cfg, sd, f, lens, rec = case
    res = de.oracle(case)
    assert cfg.n_logits == V and len(tokens(res)) > 9 and (lens == 0).sum() >= 2
    chunks, live = de.replay(res, lens.numpy(), cfg.max_symbols, lookahead=False)
    bounds = [r for r, _ in chunks]
    assert len(chunks) >= 3 and bounds == sorted(bounds, reverse=True), "two read-backs at least, each with fewer rows"
    assert seams_crossed(bounds, 8) or seams_crossed(bounds, 4), "the 4-row verify grid shrinks"


@pytest.mark.parametrize("B", [1, 4, 5, 31, 32, 33, 65])
def test_ragged_rows_screened_path(B):
    case = de.ragged_rows(64, B)
    cfg, sd, f, lens, rec = case
    res = de.oracle(case)
    assert len(tokens(res)) > B
    chunks, live = de.replay(res, lens.numpy(), cfg.max_symbols, lookahead=False)
    bounds = [r for r, _ in chunks]
    assert len(chunks) >= 3 and bounds[0] == B
    for seam in (32, 64):                   # the 32-row tiles of the screen kernel
        if B > seam:
            assert seams_crossed(bounds, seam), (seam, bounds)
    if B > 4:
        assert len({(r + 3) // 4 for r in bounds}) >= 2


def test_all_empty_batch():
    case = de.ragged_rows(64, 6, all_empty=True)
    assert int(case[3].sum()) == 0 and de.oracle(case) == [([], [])] * 6


@pytest.mark.parametrize("B", [16, 17, 32, 33, 64, 65, 128, 129])
def test_ragged_rows_reach_every_lookahead_depth(B):
    case = de.ragged_rows(64, B)
    cfg, sd, f, lens, rec = case
    res = de.oracle(case)
    assert len(tokens(res)) > B
    chunks, live = de.replay(res, lens.numpy(), cfg.max_symbols, lookahead=True)
    depths = [la for _, la in chunks]
    want = [la for la, lo in ((1, 128), (2, 64), (4, 32), (8, 0)) if B > lo]
    assert sorted(set(depths)) == sorted(want), (depths, want)          # every depth from B's own down to 8 rows
    assert depths == sorted(depths) and len(chunks) >= 3, "the depth only grows as rows finish; two read-backs at least"
    assert chunks[0] == (B, de.lookahead_depth(B))


def test_lookahead_depth_thresholds():
    assert [de.lookahead_depth(r) for r in (1, 16, 32, 33, 64, 65, 128, 129, 300)] == [8, 8, 8, 4, 4, 2, 2, 1, 1]
