"""Fixture builders for the greedy transducer loop (csrc/k_rnnt.hip rs_rnnt_greedy_impl): weights and inputs that REACH the seams of
its dispatch — the verify kernel chosen by the logit count, candidate lists of a guaranteed length, ties and near-ties across the
column ranges the waves of a verify kernel own, activation rows too small for the screen's threshold, a binding max_symbols, and
live-row counts that fall through every look-ahead depth and row tile.  No GPU: tests/test_decode_edges_host.py shows on
oracle/rnnt_greedy.c alone that each fixture reaches its edge; tests/test_gpu_decode_edges.py runs the device on the same fixtures.

Every builder returns (cfg, state_dict, f [B][Tp][J] float32, lens [B] int32, rec): the first four go to AsrModel + ctx.rnnt_greedy,
`rec` says what the case is meant to reach (the block's columns, the expected winner, ...).  Builders are cached: the GPU file's
parametrised cases and the host file share one build and one oracle run per fixture.

Also here: a replay of the loop's step schedule from the oracle's frames (`replay`), a walk of the oracle's decisions with the
activation row and the exact float32 logits of each (`walk`), and a numpy model of the screen's candidate test (`screen_model`).
"""
import ctypes
import functools
import math

import numpy as np
import torch

from reazonspeech_amd.runtime.config import TINY, WIDE2, ESPNET_TINY
from reazonspeech_amd.runtime.weights import synthetic_state_dict
from oracle import greedy as og

JOUT = "joint.joint_net.2"
TP_MAX = 48
# logit counts at which the verify kernel changes (<8> | <48> | wide<48> | <0>), with Vpad != V (1001) and the benchmark's 3001
SEAM_V = (64, 512, 513, 1001, 3001, 3072, 3073, 12288, 12289)


def rb(t):
    """round to bf16 and back (round to nearest even, as pack_bf16x4 and the host weight prep do)"""
    return t.to(torch.bfloat16).to(torch.float32)


def nemo_cfg(V, wide=False, **kw):
    """TINY (H = J = 128) or WIDE2 (H = J = 640: 20 k-steps, the register cap of the screen kernel) with V logits (blank = V - 1)"""
    return (WIDE2 if wide else TINY).with_(vocab_size=V - 1, **kw)


def blank_bias_for(V, J=128):
    """a blank offset at which random weights emit about one token per frame: measured with the oracle, the largest non-blank logit
    of a decision sits near 1.9 sqrt(2 ln V) (5.1 at V = 64, 7.6 at 3001, 8.9 at 12289) and the blank's own logit varies by +-2"""
    return 2.0 * math.sqrt(2.0 * math.log(V))


@functools.lru_cache(maxsize=None)
def _base_sd(cfg, seed, blank_bias):
    return synthetic_state_dict(cfg, seed, blank_bias=blank_bias)


def base_sd(cfg, seed, blank_bias):
    """a state dict whose joint tensors may be edited: the rest is shared with every other fixture of the configuration"""
    sd = dict(_base_sd(cfg, seed, float(blank_bias)))
    for k in (JOUT + ".weight", JOUT + ".bias", "joint.pred.weight", "joint.pred.bias"):
        sd[k] = sd[k].clone()
    return sd


def random_f(B, Tp, J, seed, scale=1.5):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((B, Tp, J), generator=g) * scale, g


def spread_lens(B, Tp, g, zeros=1):
    """lengths spread evenly over 0 .. Tp in a random row order: the live-row count falls steadily through the whole decode;
    `zeros` rows (at least) are empty when B > 1, one row is full"""
    if B == 1:
        return torch.tensor([Tp], dtype=torch.int32)
    lens = torch.round(torch.linspace(0, Tp, B)).to(torch.int32)
    lens[:min(zeros, B - 1)] = 0
    lens[-1] = Tp
    return lens[torch.randperm(B, generator=g)]


# ---- ragged rows ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ragged_rows(V, B, Tp=TP_MAX, seed=2, all_empty=False, blank_bias=None, J=None):
    """random weights and inputs as the existing decode tests use them; lengths spread over 0 .. Tp so the live-row count passes
    DOWNWARD through every seam below B (look-ahead depths at 32 / 64 / 128 rows, 32-row tiles, the 4-row verify grid) over several
    16-step read-backs; empty rows included, `all_empty`: every row empty.  J: another joint width (768: the screen is not usable)"""
    cfg = nemo_cfg(V, **({"joint_hidden": J} if J else {}))
    sd = base_sd(cfg, 11, blank_bias_for(V) if blank_bias is None else blank_bias)
    f, g = random_f(B, Tp, cfg.joint_hidden, seed)
    lens = spread_lens(B, Tp, g, zeros=2 if B >= 8 else 1)
    if all_empty:
        lens = torch.zeros((B,), dtype=torch.int32)
    return cfg, sd, f, lens, dict(kind="ragged", V=V, B=B)


# ---- tied and near-tied blocks ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tied_block(V, start, N, raised=None, B=4, Tp=16, seed=3, wide=False, boost=None):
    """N rows start .. start + N - 1 of the joint's output layer are copies of row `start` with one bias, raised so the block wins
    often.  The screening logits of the copies are bit-identical: when one is a candidate all are, so the candidate list holds at least
    N columns by construction.  Expected winner: the lowest column of the block.
    raised = a column (inside the block, or any other one, which then joins the block): the near-tie form, ReLU joints only.  The
    source row is first rounded to bf16-exact values; the raised copy gets every weight moved up by a relative 2^-12 (w + |w| 2^-12,
    exact in float32: 8 + 12 significant bits).  That is below bf16 resolution — its screening logit stays bit-identical to the
    others' — and since a = relu(..) >= 0 every product of its exact chain is >= the others': its exact logit is the largest of the
    block, strictly whenever the 2^-12 survives the final roundings (checked in float64 by the host test).  Expected winner: it."""
    cfg = nemo_cfg(V, wide=wide)
    J = cfg.joint_hidden
    bb = blank_bias_for(V, J)
    sd = base_sd(cfg, 11, bb)
    W, b = sd[JOUT + ".weight"], sd[JOUT + ".bias"]
    cols = sorted(set(range(start, start + N)) | ({raised} if raised is not None else set()))
    assert 0 <= cols[0] and cols[-1] < V
    src = W[start].clone()
    if raised is not None:
        src = rb(src)
    W[cols] = src
    b[cols] = float(bb - 0.5 if boost is None else boost)
    if raised is not None:
        up = src + src.abs() * 2.0 ** -12
        assert torch.equal(rb(up), src) and torch.equal((up.double() - src.double()), src.abs().double() * 2.0 ** -12)
        W[raised] = up
    f, g = random_f(B, Tp, J, seed)
    lens = torch.randint(Tp // 2, Tp + 1, (B,), generator=g, dtype=torch.int32)
    lens[0] = Tp
    winner = raised if raised is not None else cols[0]
    return cfg, sd, f, lens, dict(kind="near" if raised is not None else "tied", V=V, cols=cols, winner=winner, n_cand=len(cols))


@functools.lru_cache(maxsize=None)
def all_tied(V, B=5, Tp=6, seed=4):
    """every output row and bias equal, the blank's bias a little lower (2^-10, far inside the screen's margin): every decision is a
    V - 1 way exact tie that column 0 wins, and the candidate list holds all V columns — CAND_ROWS of rnnt_verify_kernel<48> at
    V = 3072, of <8> at V = 512."""
    cfg = nemo_cfg(V)
    sd = base_sd(cfg, 11, 0.0)
    W, b = sd[JOUT + ".weight"], sd[JOUT + ".bias"]
    W[:] = W[7].clone()
    b[:] = 0.25
    b[cfg.blank_id] = 0.25 - 2.0 ** -10
    f, g = random_f(B, Tp, cfg.joint_hidden, seed)
    lens = spread_lens(B, Tp, g)
    return cfg, sd, f, lens, dict(kind="all_tied", V=V, cols=list(range(V)), winner=0, n_cand=V)


# ---- small activation rows --------------------------------------------------------------------------------------------------
C_MARGIN = np.float32(0.01953125)          # 2 * 2^-7 * 1.25: the screen's 2 eps per unit of ||a|| max ||w_v||
WMAX_PAD = 1.0 + 2.0 ** -10                # runtime/weights.py screen_tensors
ANORM_PAD = np.float32(1.0001)             # rnnt_prep_kernel


def _bf16_np(x):
    return rb(torch.from_numpy(np.asarray(x, np.float32))).numpy()


def find_straddling_pairs(bias=8.0, wmax=1.0, seed=0, want=4, draws=400_000):
    """(a, w) with a one-hot activation a and weight w under bias `bias`, by the numpy model of the three roundings the screen's
    bound does not cover:  fl(fl(a w) + bias) == bias on the exact side,  fl(bf16(a) bf16(w) + bias) > bias on the screening side,
    and fl(m - fl(fl(c wmax) anorm)) == m for the threshold.  One w, `want` values of a."""
    rng = np.random.default_rng(seed)
    f32 = np.float32
    bias = f32(bias)
    a = rng.uniform(2e-6, 2e-5, draws).astype(f32)
    w = rng.uniform(0.05, 1.0, draws).astype(f32)

    def straddles(a, w):
        exact = (a * w).astype(f32) + bias                                       # one product, one add: both rounded to float32
        approx = (_bf16_np(a).astype(np.float64) * _bf16_np(w).astype(np.float64)).astype(f32) + bias
        anorm = np.sqrt((a * a).astype(f32)).astype(f32) * ANORM_PAD
        thr = approx - (f32(C_MARGIN * f32(wmax * WMAX_PAD)) * anorm).astype(f32)
        return (exact == bias) & (approx > bias) & (thr > bias)

    hit = np.nonzero(straddles(a, w))[0]
    assert len(hit) >= 1, "no straddling (a, w) pair among the draws"
    w0 = w[hit[0]]
    a_all = rng.uniform(2e-6, 2e-5, draws).astype(f32)
    a_hit = a_all[straddles(a_all, np.full_like(a_all, w0))]
    assert len(a_hit) >= want, "too few activations straddle with the chosen weight"
    return [float(x) for x in a_hit[:want]], float(w0)


def _silent_decoder(cfg, V, norm1_col, k_norm):
    """a decoder whose prediction vector is exactly zero and whose output layer is zero but for one row of norm 1 that never wins"""
    sd = base_sd(cfg, 11, 0.0)
    sd["joint.pred.weight"].zero_()
    sd["joint.pred.bias"].zero_()
    W, b = sd[JOUT + ".weight"], sd[JOUT + ".bias"]
    W.zero_()
    b.zero_()
    W[norm1_col, k_norm] = 1.0
    b[norm1_col] = -100.0
    return sd, W, b


@functools.lru_cache(maxsize=None)
def small_onehot(V, u, v, B=2, Tp=4):
    """the screen's threshold against final roundings it does not bound.  g = 0 exactly (zero joint.pred), f = -1 but for ONE element
    per frame, so a = relu(f + g) is one-hot with a value ~1e-5.  Column u has one weight w under it, column v < u a zero row, both
    the bias 8; another column holds a row of norm 1 (it fixes max ||w_v|| = 1) under a bias that never wins.  The exact float32
    logits tie at 8.0 (a w is below half an ulp of 8): the oracle returns v.  The screening logit of u rounds UP to 8 + ulp, and
    2 eps ~ 1.7e-7 is below half an ulp too, so m - 2 eps rounds back to m and a threshold formed that way drops v."""
    assert v < u < V - 1
    cfg = nemo_cfg(V)
    J, k, k_norm = cfg.joint_hidden, 37, 90
    norm1_col = next(c for c in (V // 2, V // 2 + 1, V // 2 + 2) if c not in (u, v))
    sd, W, b = _silent_decoder(cfg, V, norm1_col, k_norm)
    a_vals, w = find_straddling_pairs()
    W[u, k] = w
    b[u] = b[v] = 8.0
    f = torch.full((B, Tp, J), -1.0)
    for i in range(B * Tp):
        f[i // Tp, i % Tp, k] = a_vals[i % len(a_vals)]
    lens = torch.full((B,), Tp, dtype=torch.int32)
    return cfg, sd, f, lens, dict(kind="small_onehot", V=V, cols=[v, u], winner=v, loser=u, k=k, w=w, a_vals=a_vals)


@functools.lru_cache(maxsize=None)
def small_pair(V, u, v, exp=-70, B=2, Tp=4, seed=0):
    """||a||^2 underflowing in rnnt_prep_kernel.  g = 0, all biases zero, a has two elements 2^exp.  Columns u and v carry two weights
    each: exact order fl(p + q) of v ABOVE u, order of the bf16-rounded weights the other way round (sums of two 8-bit values scaled by
    a power of two: exact in any accumulation order, on both sides).  exp = -70: a^2 = 2^-140 is a float32 SUBNORMAL — ||a|| survives
    only where subnormals do; exp = -80: a^2 = 2^-160 is zero in any mode.  With anorm = 0 the margin is zero and only u is evaluated."""
    assert v != u and max(u, v) < V - 1
    cfg = nemo_cfg(V)
    J, k1, k2, k_norm = cfg.joint_hidden, 0, 1, 90
    norm1_col = next(c for c in (V // 2, V // 2 + 1, V // 2 + 2) if c not in (u, v))
    sd, W, b = _silent_decoder(cfg, V, norm1_col, k_norm)
    b[norm1_col] = 0.0                               # its product with a is exactly 0: it ties the empty rows below u and v
    rng = np.random.default_rng(seed)
    f32 = np.float32
    found = None
    for _ in range(100_000):
        p, q = rng.uniform(0.05, 1.0, 2).astype(f32)
        r, s = (f32(p * f32(1 + rng.uniform(-1, 1) * 2.0 ** -9)), f32(q * f32(1 + rng.uniform(-1, 1) * 2.0 ** -9)))
        ev, eu = f32(p + q), f32(r + s)
        av, au = _bf16_np([p, q]).astype(np.float64).sum(), _bf16_np([r, s]).astype(np.float64).sum()
        if ev > eu and au > av:
            found = (p, q, r, s)
            break
    assert found is not None, "no pair of rows whose bf16 order inverts the exact order"
    p, q, r, s = found
    W[v, k1], W[v, k2] = float(p), float(q)
    W[u, k1], W[u, k2] = float(r), float(s)
    f = torch.full((B, Tp, J), -1.0)
    f[:, :, k1] = 2.0 ** exp
    f[:, :, k2] = 2.0 ** exp
    lens = torch.full((B,), Tp, dtype=torch.int32)
    return cfg, sd, f, lens, dict(kind="small_pair", V=V, cols=sorted((u, v)), winner=v, loser=u, exp=exp)


# ---- binding max_symbols ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def binding_cap(max_symbols, B, Tp=24, seed=6, V=64):
    """a NEGATIVE blank offset: most frames emit until max_symbols stops them, and utterances emit on their last frame"""
    cfg = nemo_cfg(V, max_symbols=max_symbols)
    sd = base_sd(cfg, 11, -2.0)
    f, g = random_f(B, Tp, cfg.joint_hidden, seed)
    lens = spread_lens(B, Tp, g)
    case = (cfg, sd, f, lens, dict(kind="cap", max_symbols=max_symbols, B=B))
    per_frame = [np.bincount(r[1], minlength=int(n)) for r, n in zip(oracle(case), lens) if int(n) > 0]
    assert max(int(c.max()) for c in per_frame) == max_symbols, "no frame carries exactly max_symbols labels"
    assert any(c[-1] > 0 for c in per_frame), "no utterance emits on its last frame"
    return case


# ---- the other two families ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def k2_tied(B=3, Tp=40, seed=8):
    """Zipformer family: stateless decoder, tanh joiner, V = 10720 (rnnt_verify_wide_kernel<48>): a tied block {1, 2 = <unk>, 3} and
    3070 .. 3074 (both sides of the wave seam at 3072).  Expected winner: 1; <unk> is inside the block and must not matter."""
    from reazonspeech_amd.runtime.k2_config import ZIPFORMER_TINY
    from reazonspeech_amd.runtime.k2_weights import synthetic_state_dict_k2
    cfg = ZIPFORMER_TINY.with_(vocab_size=10720)
    assert cfg.unk_id == 2 and cfg.blank_id == 0
    sd = dict(synthetic_state_dict_k2(cfg, 5))
    W, b = sd["joiner.output_linear.weight"].clone(), sd["joiner.output_linear.bias"].clone()
    cols = [1, 2, 3] + list(range(3070, 3075))
    W[cols] = W[1].clone()
    b[cfg.blank_id] = 16.0                 # (random tanh rows under the 6x output gain: the largest logit of a decision is ~15)
    b[cols] = 16.0
    sd["joiner.output_linear.weight"], sd["joiner.output_linear.bias"] = W, b
    f, g = random_f(B, Tp, cfg.joiner_dim, seed, scale=1.0)
    lens = torch.tensor([Tp, 0, Tp - 3][:B], dtype=torch.int32)
    return cfg, sd, f, lens, dict(kind="tied", V=cfg.vocab_size, cols=cols, winner=1, n_cand=len(cols))


@functools.lru_cache(maxsize=None)
def espnet_tied(B=4, Tp=24, seed=9):
    """ESPnet family: tanh joint, blank 0, one symbol per frame, V = 96 (rnnt_verify_kernel<8>): a tied block 40 .. 69 over the
    64-column chunk seam.  Expected winner: 40."""
    from reazonspeech_amd.runtime.weights_espnet import synthetic_state_dict_espnet
    cfg = ESPNET_TINY
    sd = dict(synthetic_state_dict_espnet(cfg, 3))
    W, b = sd["joint_network.lin_out.weight"].clone(), sd["joint_network.lin_out.bias"].clone()
    cols = list(range(40, 70))
    W[cols] = W[40].clone()
    b[cols] = b[cfg.blank_id] - 0.5
    sd["joint_network.lin_out.weight"], sd["joint_network.lin_out.bias"] = W, b
    f, g = random_f(B, Tp, cfg.joint_hidden, seed, scale=1.0)
    lens = spread_lens(B, Tp, g)
    return cfg, sd, f, lens, dict(kind="tied", V=cfg.n_logits, cols=cols, winner=40, n_cand=len(cols))


# ---- the oracle, once per fixture ---------------------------------------------------------------------------------------------
_ORACLE = {}


def oracle(case, u_max=None):
    """oracle/rnnt_greedy.c (k2_greedy.c for the Zipformer family) on a fixture, once per fixture and u_max"""
    cfg, sd, f, lens, rec = case
    key = (id(f), u_max)
    if key not in _ORACLE:
        fn = og.k2_greedy if getattr(cfg, "family", "") == "k2" else og.rnnt_greedy
        _ORACLE[key] = (fn(cfg, sd, f.numpy(), lens.numpy(), u_max=u_max), f)      # (f kept: its id stays unique)
    return _ORACLE[key][0]


# ---- the loop's schedule, replayed from the oracle's frames -------------------------------------------------------------------
def decisions(ids_frames, n_frames, max_symbols):
    """the utterance's decisions in order, True = a label: per frame its labels, then a blank unless max_symbols ended the frame"""
    per_frame = np.bincount(np.asarray(ids_frames[1], np.int64), minlength=n_frames) if n_frames else np.zeros((0,), np.int64)
    out = []
    for t in range(n_frames):
        out += [True] * int(per_frame[t])
        if per_frame[t] < max_symbols:
            out.append(False)
    return out


def lookahead_depth(rows):
    la = 1
    while la < 8 and 2 * la * max(rows, 1) <= 256:
        la *= 2
    return la


def replay(result, lens, max_symbols, lookahead, chunk=16):
    """rs_rnnt_greedy_impl's schedule for a batch whose decisions are the oracle's: per 16-step chunk the row bound read back from the
    device and the look-ahead depth chosen from it -> [(rows, la)] and the live-row count before every step.  A step takes one decision
    per live row; with look-ahead la it takes up to la of them, ending after the first label (rnnt_finalize_la_kernel)."""
    todo = [decisions(result[b], int(lens[b]), max_symbols) for b in range(len(lens))]
    pos = [0] * len(todo)
    chunks, live_counts = [], []
    rows = len(todo)
    while True:
        live = [b for b in range(len(todo)) if pos[b] < len(todo[b])]
        if chunks:
            rows = len(live)
        if not live:
            break
        la = lookahead_depth(rows) if lookahead else 1
        chunks.append((rows, la))
        for _ in range(chunk):
            live = [b for b in range(len(todo)) if pos[b] < len(todo[b])]
            live_counts.append(len(live))
            for b in live:
                for _j in range(la):
                    if pos[b] >= len(todo[b]):
                        break
                    pos[b] += 1
                    if todo[b][pos[b] - 1]:
                        break
    return chunks, live_counts


# ---- the oracle's decisions one by one (ReLU joint) -----------------------------------------------------------------------------
def walk(cfg, sd, f_row, n_frames, max_decisions):
    """the first decisions of one utterance from the oracle's own C pieces (rs_oracle_lstm_step, rs_oracle_dot,
    rs_oracle_joint_argmax): yields (a = relu(f_t + g) float32 [J], exact float32 logits [V], argmax)"""
    L = og.lib()
    L.rs_oracle_set_joint_act(0)
    L.rs_oracle_joint_argmax.restype = ctypes.c_int
    arr = og.decoder_arrays(cfg, sd)
    H, J, V, NL = cfg.pred_hidden, cfg.joint_hidden, cfg.n_logits, cfg.pred_layers
    fp = og._fp
    h, c = np.zeros((NL, H), np.float32), np.zeros((NL, H), np.float32)
    g, logits = np.zeros((J,), np.float32), np.zeros((V,), np.float32)
    token, t, sym, need, done = cfg.blank_id, 0, 0, True, 0
    f_row = np.ascontiguousarray(f_row, np.float32)
    while t < n_frames and done < max_decisions:
        if need:
            x = np.ascontiguousarray(arr["embed"][token])
            hn, cn = np.zeros_like(h), np.zeros_like(c)
            for l in range(NL):
                L.rs_oracle_lstm_step(fp(x), fp(h[l]), fp(c[l]), fp(arr["lstm_w"][l]), fp(arr["lstm_b"][l]), H, fp(hn[l]), fp(cn[l]))
                x = hn[l]
            h, c = hn, cn
            top = np.ascontiguousarray(h[NL - 1])
            for j in range(J):
                g[j] = np.float32(L.rs_oracle_dot(fp(top), fp(arr["Wp"][j]), H)) + arr["bp"][j]
            need = False
        k = L.rs_oracle_joint_argmax(fp(f_row[t]), fp(g), fp(arr["Wo"]), fp(arr["bo"]), J, V, fp(logits))
        yield np.maximum(f_row[t] + g, np.float32(0)), logits.copy(), int(k)
        done += 1
        if k == cfg.blank_id:
            t, sym = t + 1, 0
        else:
            token, need, sym = k, True, sym + 1
            if sym >= cfg.max_symbols:
                t, sym = t + 1, 0


# ---- numpy model of the screen's candidate test ---------------------------------------------------------------------------------
def screen_model(a, W, b, form="m-2eps", ftz=False):
    """candidates of one row under the screen: z~ = fl(bf16(a) . bf16(w_v) + b_v) (the dot product rounded once: exact for the
    small-activation fixtures, within the bound's own slack otherwise) and the candidate test in float32.
    form "m-2eps": thr = fl(m - fl(fl(c wmax) anorm)), anorm = fl(fl(sqrt(ss)) 1.0001) — the threshold as first built;
    form "margin": fl(m - z~) <= fl(2^-21 |m| + fl(fl(c wmax) anorm)), anorm = fl(fl(sqrt(ss)) 1.0001 + 2^-55) (screen_margin).
    ftz: squares below the smallest normal float32 count as zero in ss (a device mode that flushes subnormals).  -> (z~, mask)"""
    f32 = np.float32
    a = np.asarray(a, f32)
    W = W.numpy() if isinstance(W, torch.Tensor) else W
    b = b.numpy() if isinstance(b, torch.Tensor) else b
    z = (_bf16_np(W).astype(np.float64) @ _bf16_np(a).astype(np.float64)).astype(f32) + b.astype(f32)
    sq = (a * a).astype(f32)
    if ftz:
        sq = np.where(sq < np.finfo(f32).tiny, f32(0), sq)
    ss = f32(0)
    for x in sq[sq != 0]:
        ss = f32(ss + x)
    wmax = f32(float(np.sqrt((W.astype(np.float64) ** 2).sum(1)).max()) * WMAX_PAD)
    m = z.max()
    if form == "m-2eps":
        anorm = f32(f32(np.sqrt(ss)) * ANORM_PAD)
        thr = f32(m - f32(f32(C_MARGIN * wmax) * anorm))
        return z, z >= thr
    assert form == "margin"
    anorm = f32(f32(f32(np.sqrt(ss)) * ANORM_PAD) + f32(2.0 ** -55))
    margin = f32(f32(f32(2.0 ** -21) * np.abs(m)) + f32(f32(C_MARGIN * wmax) * anorm))
    return z, (m - z).astype(f32) <= margin


# ---- the case tables both test files run ------------------------------------------------------------------------------------------
def block_cases():
    """[(id, knobs, builder kwargs)] of the candidate-list table: every placement as an exact tie and as near-ties with the raised copy
    first in the block, last in it, or alone beyond the seam the block ends at"""
    out = []

    def add(tag, knobs, V, start, N, raised_list):
        out.append((f"{tag}-V{V}-s{start}-N{N}-tied", knobs, dict(V=V, start=start, N=N)))
        for r in raised_list:
            out.append((f"{tag}-V{V}-s{start}-N{N}-raised{r}", knobs, dict(V=V, start=start, N=N, raised=r)))

    # rnnt_verify_kernel<48>: more than one 8-wide pass, more than one 64-column chunk, hundreds; the ragged last chunk with V - 1
    add("v48", {}, 3001, 60, 9, [60, 68, 200])
    add("v48", {}, 3001, 100, 65, [100, 164])
    add("v48", {}, 3001, 1000, 600, [1000, 1599])
    add("v48", {}, 3001, 2992, 9, [2992, 2999])
    # rnnt_verify_kernel<0>: more than one VER_CAP = 1024 batch; the raised copy in the first, a middle and the last batch
    add("v0", {}, 12289, 500, 1100, [500, 1599])
    add("v0", {}, 12289, 6000, 2100, [7050, 8099])
    # the column ranges of the four waves of a wide verify kernel
    for seam in (3072, 6144, 9216):
        add("w48", {}, 12288, seam - 4, 9, [seam + 4, seam + 40])
    for seam in (768, 1536, 2304):
        add("w12", {"RS_VERIFY_WIDE": 1}, 3001, seam - 4, 9, [seam + 4, seam + 40])
    return out


def small_cases():
    """[(id, builder)] of the small-activation fixtures: V = 1001 (rnnt_verify_kernel<48>, rnnt_verify_wide_kernel<12> under
    $RS_VERIFY_WIDE: u and v in different waves' 768 columns) and V = 12288 (rnnt_verify_wide_kernel<48>: different 3072s)"""
    return [("onehot-V1001", lambda: small_onehot(1001, 900, 100)), ("onehot-V12288", lambda: small_onehot(12288, 9300, 100)),
            ("pair70-V1001", lambda: small_pair(1001, 900, 100, -70)), ("pair70-V12288", lambda: small_pair(12288, 100, 9300, -70)),
            ("pair80-V1001", lambda: small_pair(1001, 100, 900, -80)), ("pair80-V12288", lambda: small_pair(12288, 9300, 100, -80))]


def tokens(res):
    return [t for r in res for t in r[0]]


def check_block(case, res, at_least=10):
    """the oracle's result shows the block deciding emissions: its expected winner at least `at_least` times, no other column of it"""
    rec = case[4]
    toks = tokens(res)
    others = set(rec["cols"]) - {rec["winner"]}
    assert toks.count(rec["winner"]) >= at_least, (rec["winner"], toks.count(rec["winner"]))
    assert not others & set(toks), sorted(others & set(toks))
    assert rec["n_cand"] == len(rec["cols"]) >= 2
