#!/usr/bin/env python
"""bench.py — RTFx of the MI355X FastConformer-RNNT path (BASELINE.json metric).

    python bench.py --gpus 1 --steps 10 --warmup 3
    python bench.py --gpus 1 --steps 10 --warmup 3 --full
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

`--dump-outputs DIR` writes what the last timed step computed (dump_outputs) to DIR/*.npy: with the same arguments the inputs
and weights are the same seeded ones from run to run, so two builds can be compared output for output.

A plain run does only what the headline figure needs: set up, warm up, time the steps, dump the outputs if asked, and
print the line — `value`, `ms_per_step`, the step intervals, `config` and the GEMM `roofline` of the timed steps, which
costs no run of its own.  Everything described below that takes runs of its own (the PCIe-inclusive and host-boundary
rates, the sequential-schedule GEMM figures, `cpu_baseline`, `parity`, `configs`) is added by `--full`; the `--no-*`
switches trim a `--full` run.

One "step" = one pass of the whole hot path (log-mel front-end -> 24-layer FastConformer encoder
-> joint projection -> batched greedy RNN-T decode) over one batch of 256 synthetic 10 s
utterances per GPU.  `value` follows the bench contract: inputs already resident in HBM when the timed region
starts.  With `--full` the same JSON line carries what SURVEY.md §8(d) defines — the host-to-host rate through the
PUBLIC boundary: `value_host_to_ids` (AsrModel.transcribe_waveforms: host float32 lists -> token ids, H2D / D2H,
sorting, staging and the pipeline fill and drain inside the clock) and `value_transcribe_batch` (the same through
`transcribe_batch`, text post-processing included) — and `configs`: BASELINE configs[1] (B = 32), the ragged set of
§8(d) (lengths U(2 s, 10 s), seed 1235), the reference checkpoint's real decode strategy (ALSD beam 4) and the
limited-context attention variant the shipped model is believed to use ([128, 128] + 1 global token).
Weak scaling: every rank processes its own 256 utterances (BASELINE.json configs[2]: 2048 = 8 x 256); with N > 1
every step ends with the one collective of the path, an RCCL all_gather of that step's hypotheses, issued from the
decode worker as soon as the batch is decoded.  Rank 0 prints ONE JSON line, which also carries `roofline`
(dominant kernel class, HIP events on the launch stream, per GEMM shape in `roofline.per_shape`), `cpu_baseline` (the CPU
oracle on a bounded sample) and `parity`:
  * `fp32_mode`: ALL 256 rows of the timed batch through `precision="fp32"` (float32 end to end, what the reference
    computes) against the committed float32-oracle golden of every row (tests/golden/bench_fp32.npz) — ids / frames identity
    count, joint-projection error;
  * `bf16_audit_all_rows`: the throughput mode on ALL 256 rows audited against the parity mode (every greedy-id difference
    must start at a decision whose margin is below the Lipschitz bound of the measured difference: oracle/audit.py);
  * rows 0..7 against the CPU leg's own outputs (encoder error, alone == inside the batch, decode kernels bit-exact).
`value` is the bench contract's figure (inputs resident in HBM); SURVEY §8(d)'s figure — host float32 in, TranscribeResult
out through the public `transcribe_batch` — is `value_transcribe_batch` in the same line (`value_definition` says which is which).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from reazonspeech_amd.runtime import capi                                  # noqa: E402
from reazonspeech_amd.runtime.config import FASTCONFORMER_619M, TINY        # noqa: E402
from reazonspeech_amd.runtime.model import AsrModel                         # noqa: E402
from reazonspeech_amd.runtime.synth import synthetic_batch                  # noqa: E402
from reazonspeech_amd.runtime.tokenizer import SyntheticTokenizer           # noqa: E402
from reazonspeech_amd.runtime.weights import synthetic_state_dict           # noqa: E402
from reazonspeech_amd.runtime import dist as rdist                          # noqa: E402

MFMA_BF16_PEAK_TFLOPS = 2500.0     # MI355X dense bf16 (guides/MI355X_MICROARCH.md)
HBM_PEAK_TBPS = 8.0                # HBM3E (same guide)


def algorithmic_gflop_per_utt(cfg, tp, mean_tokens):
    """SURVEY.md §8(d) work model, evaluated for this config / T' / measured U"""
    d, f, c = cfg.d_model, cfg.ff_dim, cfg.sub_channels
    lin = 2 * (2 * d * f * 2) + 4 * 2 * d * d + 2 * d * 2 * d + 2 * d * d          # per frame per layer
    att = 3 * 2 * tp * d                                                              # ac + bd + pv per frame
    dw = 2 * cfg.conv_kernel * d
    enc = cfg.n_layers * tp * (lin + att + dw)
    t1, t2 = 4 * tp, 2 * tp
    sub = 2 * (t1 * 40 * c * 9 + t2 * 20 * c * 9 + t2 * 20 * c * c + tp * 10 * c * 9 + tp * 10 * c * c
               + tp * c * 10 * d)
    jenc = 2 * tp * d * cfg.joint_hidden
    H, J, V = cfg.pred_hidden, cfg.joint_hidden, cfg.n_logits
    dec = (tp + mean_tokens) * 2 * J * V + mean_tokens * (cfg.pred_layers * 2 * 4 * H * 2 * H + 2 * H * J)
    fe = 8 * tp * (5 * 512 * 9 + 3 * 257 + 2 * 600)
    return (enc + sub + jenc + dec + fe) / 1e9


def cpu_baseline(cfg, sd, audio, lens, seconds_budget=20.0, max_utt=8):
    """The reference's own CPU transcribe() cannot run here (NeMo absent, no checkpoint —
    BASELINE.md §4); timed instead: the repo's CPU oracle (fp32 torch + C greedy), driven like the
    reference — one utterance per call, 0.5 s padding — on the host cores of this node."""
    try:
        from oracle import model as om, greedy as og
    except Exception as e:                      # oracle is optional infrastructure for this leg
        return {"value": None, "unit": "x real-time", "cores": 0, "kind": "port", "sample": f"unavailable: {e}"}, []
    threads = torch.get_num_threads()
    done, audio_s = 0, 0.0
    outputs = []                                 # (joint_enc f32 [T', J], enc f32 [T', d], ids, frames) per utterance
    t0 = time.perf_counter()
    for b in range(min(max_utt, audio.shape[0])):
        n = int(lens[b])
        wav = np.pad(audio[b, :n], 8000)
        taps = {}
        f, el = om.forward_to_joint(cfg, sd, torch.from_numpy(wav)[None], torch.tensor([len(wav)]), "fp32", taps)
        hyp = og.rnnt_greedy(cfg, sd, f.numpy(), el.numpy())[0]
        outputs.append((f[0, :int(el[0])], taps["enc"][0, :int(el[0])], hyp[0], hyp[1]))
        done += 1
        audio_s += n / 16000.0
        if time.perf_counter() - t0 > seconds_budget:
            break
    dt = time.perf_counter() - t0
    return {"value": round(audio_s / dt, 3), "unit": "x real-time", "cores": threads, "kind": "port",
            "sample": f"{done} utterance(s) x {audio_s / max(done, 1):g} s, one per call (batch_size=1), fp32 torch CPU "
                      f"oracle + C greedy, {dt:.1f} s wall"}, outputs


def edit_distance(a, b):
    prev = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        cur = [i]
        for j, y in enumerate(b, 1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (x != y)))
        prev = cur
    return prev[-1]


def parity_vs_cpu_leg(model, cfg, sd, buf256, audio, lens, outputs):
    """The CPU leg's outputs are the checker of the same utterances through the HIP path AS THE BENCHMARK RUNS THEM:
    rows 0 .. k-1 of the resident B = 256 batch (`buf256` holds the same audio as the CPU leg), i.e. the tile heights
    and launch geometry of the timed region.  Reported: encoder output / joint projection error against the fp32
    oracle; whether the same utterances run ALONE (B = 1 each) give the same bits as inside the batch; greedy ids
    against the oracle's end-to-end ids with a flip audit (every difference must start at a decision whose oracle
    margin is below the Lipschitz bound of the measured encoder difference: oracle/audit.py); and the decode kernels
    alone — C greedy on the HIP joint projection — which must agree bit for bit."""
    from oracle import greedy as og, audit
    k = len(outputs)
    if k == 0:
        return None
    B = buf256.B
    enc = torch.zeros((B, buf256.tp_max, cfg.d_model), dtype=torch.float32, device=model.device)
    model.run_device(buf256, want_enc=enc)
    torch.cuda.synchronize()
    got = model.collect(buf256)
    enc_rows, f_rows = enc[:k].cpu(), buf256.joint_enc[:k].cpu()
    del enc
    # the same utterances alone: one launch chain each, tiny-M tiles
    alone_bits = True
    for b in range(k):
        one = model.stage([audio[b, :int(lens[b])]])
        e1 = torch.zeros((1, one.tp_max, cfg.d_model), dtype=torch.float32, device=model.device)
        model.run_device(one, want_enc=e1)
        torch.cuda.synchronize()
        r1 = model.collect(one)
        n = r1.enc_lens[0]
        alone_bits &= bool(torch.equal(e1[0, :n].cpu(), enc_rows[b, :n]) and torch.equal(one.joint_enc[0, :n].cpu(), f_rows[b, :n])
                           and r1.ids[0] == got.ids[b] and r1.frames[0] == got.frames[b])
    e_max = e_sum = j_max = j_sum = cnt_e = cnt_j = 0.0
    exact = dist = ref_tokens = 0
    audits, equal = [], []
    for b, (f_ref, enc_ref, ids_ref, frames_ref) in enumerate(outputs):
        n = f_ref.shape[0]
        assert got.enc_lens[b] == n, (got.enc_lens[b], n)
        de, dj = (enc_rows[b, :n] - enc_ref).abs(), (f_rows[b, :n] - f_ref).abs()
        e_max, j_max = max(e_max, de.max().item()), max(j_max, dj.max().item())
        e_sum, j_sum, cnt_e, cnt_j = e_sum + de.sum().item(), j_sum + dj.sum().item(), cnt_e + de.numel(), cnt_j + dj.numel()
        equal.append(got.ids[b] == ids_ref)
        exact += int(equal[-1])
        dist += edit_distance(got.ids[b], ids_ref)
        ref_tokens += len(ids_ref)
        audits.append(audit.flip_audit(cfg, sd, f_ref.numpy(), f_rows[b, :n].numpy(), n, got.ids[b], got.frames[b]))
    same = og.rnnt_greedy(cfg, sd, f_rows.numpy(), np.asarray(got.enc_lens[:k], np.int32))
    bit_exact = all(got.ids[b] == same[b][0] and got.frames[b] == same[b][1] for b in range(k))
    return {"utterances": k, "rows": f"0..{k - 1} of the resident B = {B} batch (the timed configuration's launch geometry)",
            "checker": "fp32 CPU oracle (cpu_baseline leg), same audio",
            "encoder_max_err": round(e_max, 4), "encoder_mean_err": round(e_sum / cnt_e, 5),
            "joint_enc_max_err": round(j_max, 4), "joint_enc_mean_err": round(j_sum / cnt_j, 5),
            "alone_equals_inside_batch_bits": alone_bits,
            "greedy_ids_exact_match": f"{exact}/{k}",
            "token_agreement": round(1.0 - dist / max(ref_tokens, 1), 4), "reference_tokens": ref_tokens,
            "flip_audit": audit.summarize(audits, equal),
            "decode_bit_exact_given_same_joint_enc": bool(bit_exact)}


def fp32_mode_parity(model, cfg, sd, buf256, audio, lens):
    """The float32 PARITY MODE (load_model(precision="fp32"): float32 weights / activations / arithmetic end to end, what the
    reference computes) on ALL rows of the benchmark batch against the committed float32-oracle golden
    (tests/golden/bench_fp32.npz: the CPU oracle run end to end on every row, one utterance per call), and the bf16
    throughput mode audited on ALL rows against the parity mode's joint projection (oracle/audit.py, float64 on the GPU)."""
    import hashlib
    from oracle import audit
    path = os.path.join(ROOT, "tests", "golden", "bench_fp32.npz")
    gold = np.load(path)
    if hashlib.sha256(audio.tobytes()).digest() != bytes(gold["equal_audio_sha256"].tolist()):
        return {"error": "the resident batch is not the golden's batch (seed / rank / --seconds differ)"}
    rows = int(gold["rows"])
    off = gold["equal_offsets"]
    g_ids = [gold["equal_ids"][off[b]:off[b + 1]].tolist() for b in range(rows)]
    g_frames = [gold["equal_frames"][off[b]:off[b + 1]].tolist() for b in range(rows)]
    t0 = time.perf_counter()
    m32 = AsrModel(cfg, sd, SyntheticTokenizer(cfg.vocab_size), device=str(model.device), precision="fp32")
    b32 = m32.stage([audio[b, :int(lens[b])] for b in range(audio.shape[0])], buf=m32.new_buffers(audio.shape[0], audio.shape[1]))
    m32.run_device(b32)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    m32.run_device(b32)
    torch.cuda.synchronize()
    ms32 = (time.perf_counter() - t1) * 1e3
    got32 = m32.collect(b32)
    g = torch.Generator().manual_seed(int(gold["proj_seed"]))
    R = (torch.randn((cfg.joint_hidden, 8), generator=g, dtype=torch.float32) / cfg.joint_hidden ** 0.5).to(model.device)
    proj = (b32.joint_enc @ R).cpu().numpy()
    perr = max(float(np.abs(proj[b, :got32.enc_lens[b]] - gold["equal_proj"][b, :got32.enc_lens[b]]).max()) for b in range(rows))
    ferr = max(float((b32.joint_enc[b, :got32.enc_lens[b]].cpu() - torch.from_numpy(gold["equal_f_rows"][b, :got32.enc_lens[b]])).abs().max())
               for b in range(2))
    exact = [got32.ids[b] == g_ids[b] and got32.frames[b] == g_frames[b] for b in range(rows)]
    near = [int(b) for b in np.nonzero(gold["equal_min_margin"] < float(gold["near_tie"]))[0]]
    out = {"fp32_mode": {"rows": rows, "ids_exact": f"{sum(exact)}/{rows}",
                         "checker": "tests/golden/bench_fp32.npz: float32 CPU oracle end to end on every row (committed; generator "
                                    "tests/golden/make_bench_golden.py)",
                         "enc_lens_equal": got32.enc_lens[:rows] == gold["equal_enc_lens"].tolist(),
                         "joint_proj_fingerprint_max_err_all_rows": round(perr, 7), "joint_enc_max_err_rows_0_1": round(ferr, 7),
                         "rows_differing": [b for b in range(rows) if not exact[b]],
                         "golden_rows_with_a_margin_below_1e-3": len(near), "golden_min_margin": float(gold["equal_min_margin"].min()),
                         "decisions": int(gold["equal_n_decisions"].sum()),
                         "ms_per_batch_of_256": round(ms32, 1), "rtfx": round(float(lens.sum()) / 16000.0 / (ms32 * 1e-3), 1),
                         "load_and_first_run_s": round(t1 - t0, 1)}}
    # throughput mode, every row, against the parity mode's projection of the same rows
    model.run_device(buf256)
    torch.cuda.synchronize()
    got16 = model.collect(buf256)
    f16 = buf256.joint_enc
    dj = max(float((f16[b, :got16.enc_lens[b]] - b32.joint_enc[b, :got16.enc_lens[b]]).abs().max()) for b in range(rows))
    audits = audit.flip_audit_batch(cfg, sd, b32.joint_enc[:rows], f16[:rows], got16.enc_lens[:rows], got16.ids[:rows],
                                    got16.frames[:rows], device=model.device)
    equal = [got16.ids[b] == g_ids[b] and got16.frames[b] == g_frames[b] for b in range(rows)]
    s = audit.summarize(audits, equal)
    bound_ok = all(fl["margin_ref"] <= fl["bound"] * (1 + 1e-9) + 1e-12 for a in audits for fl in a["flips"])
    ref_tokens = sum(len(x) for x in g_ids)
    dist = sum(edit_distance(got16.ids[b], g_ids[b]) for b in range(rows) if not equal[b])
    s.update(rows=rows, reference="the float32 parity mode's joint projection of the same rows (pinned to the oracle golden above)",
             ids_exact_vs_fp32_oracle=f"{sum(equal)}/{rows}", token_agreement=round(1.0 - dist / max(ref_tokens, 1), 4),
             joint_enc_max_diff_vs_fp32_mode=round(dj, 4), every_flip_obeys_the_lipschitz_bound=bool(bound_ok))
    out["bf16_audit_all_rows"] = s
    del m32, b32
    torch.cuda.empty_cache()
    # precision="fp32x3": the float32 mode with every float32 product of its GEMMs formed from three bf16 matrix-core terms (csrc/k_f32.hip X3)
    # — not an IEEE chain; a mode of its own, held to the same golden
    try:
        mx = AsrModel(cfg, sd, SyntheticTokenizer(cfg.vocab_size), device=str(model.device), precision="fp32x3")
        bx = mx.stage([audio[b, :int(lens[b])] for b in range(audio.shape[0])], buf=mx.new_buffers(audio.shape[0], audio.shape[1]))
        mx.run_device(bx)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        mx.run_device(bx)
        torch.cuda.synchronize()
        msx = (time.perf_counter() - t1) * 1e3
        gotx = mx.collect(bx)
        projx = (bx.joint_enc @ R).cpu().numpy()
        perrx = max(float(np.abs(projx[b, :gotx.enc_lens[b]] - gold["equal_proj"][b, :gotx.enc_lens[b]]).max()) for b in range(rows))
        exactx = [gotx.ids[b] == g_ids[b] and gotx.frames[b] == g_frames[b] for b in range(rows)]
        out["fp32x3_mode"] = {"what": "float32 weights / activations / accumulation; each float32 product of the GEMMs = hi.hi + hi.lo + lo.hi of a bf16 hi / lo "
                                      "split (16 mantissa bits per operand) on v_mfma_f32_16x16x32_bf16; same golden as fp32_mode",
                              "rows": rows, "ids_exact": f"{sum(exactx)}/{rows}", "rows_differing": [b for b in range(rows) if not exactx[b]],
                              "rows_differing_that_are_near_ties_of_the_golden": [b for b in range(rows) if not exactx[b] and b in near],
                              "joint_proj_fingerprint_max_err_all_rows": round(perrx, 7),
                              "ms_per_batch_of_256": round(msx, 1), "rtfx": round(float(lens.sum()) / 16000.0 / (msx * 1e-3), 1)}
        del mx, bx
        torch.cuda.empty_cache()
    except Exception as e:
        out["fp32x3_mode"] = {"error": repr(e)}
    return out


def per_shape_roofline(launches):
    """group the per-launch HIP-event records of the GEMM class by shape -> TF/s and fraction of the dense bf16 peak"""
    names = {(4096, 1024): "ffn_up", (3072, 1024): "qkv", (1024, 4096): "ffn_down", (2048, 1024): "pw1_glu", (640, 1024): "joint_enc",
             (256, 256): "sub_pw", (1024, 2560): "sub_out"}
    agg = {}
    for M, N, K, flags, flops, ms in launches:
        if ms <= 0:
            continue
        key = names.get((N, K), f"n{N}_k{K}")
        if (N, K) == (1024, 1024):
            key = "att_out_pw2" if flags & capi.GEMM_RESIDUAL else "pos_proj"
        a = agg.setdefault(key, {"launches": 0, "ms": 0.0, "flops": 0.0, "bytes": 0.0, "M": M, "N": N, "K": K})
        a["launches"] += 1
        a["ms"] += ms
        a["flops"] += flops
        # algorithmic bytes of the launch: A + W (bf16) + the output (bf16, GLU halves it, f32) + the f32 residual read once
        out_b = 4.0 * M * N if flags & (capi.GEMM_OUT_F32 | capi.GEMM_RESIDUAL) else (1.0 * M * N if flags & capi.GEMM_GLU else 2.0 * M * N)
        a["bytes"] += 2.0 * M * K + 2.0 * N * K + out_b + (4.0 * M * N if flags & capi.GEMM_RESIDUAL else 0.0)
    out = {}
    for key, a in sorted(agg.items(), key=lambda kv: -kv[1]["ms"]):
        tf = a["flops"] / (a["ms"] * 1e-3) / 1e12
        tbs = a["bytes"] / (a["ms"] * 1e-3) / 1e12
        # a shape is priced against the roofline it is closer to: a K = 256 product of 1.4 M rows moves its operands at HBM rate
        # long before it fills the matrix cores
        out[key] = {"M": a["M"], "N": a["N"], "K": a["K"], "launches": a["launches"], "avg_us": round(a["ms"] / a["launches"] * 1e3, 1),
                    "tflops": round(tf, 1), "frac": round(tf / MFMA_BF16_PEAK_TFLOPS, 4),
                    "algorithmic_tb_per_s": round(tbs, 2), "hbm_frac": round(tbs / HBM_PEAK_TBPS, 3),
                    "bound": "hbm" if tbs / HBM_PEAK_TBPS > tf / MFMA_BF16_PEAK_TFLOPS else "mfma"}
    return out


def decode_family_check(model, buf):
    """The pipeline's decode kernel family at this batch size (screened joint + narrow tiles with two decode lanes)
    against the exact-joint / wide-tile family on the SAME joint-encoder tensor of a whole benchmark batch: the ids and
    emission frames must be identical (the C oracle pins the families at B <= 37 in tests/; this is the same property
    at the benchmark batch, where the oracle would take minutes)."""
    ctx = model.ctx
    stream = torch.cuda.current_stream().cuda_stream
    got = []
    try:
        for screen, narrow in ((1, 1), (0, 0)):
            ctx.set_option("decode_screen", screen)
            ctx.set_option("decode_narrow", narrow)
            model.decode(ctx, buf, buf.ws, stream)
            torch.cuda.synchronize()
            r = model.collect(buf)
            got.append((r.ids, r.frames))
    finally:
        model._decode_policy(ctx, buf.B, pipelined=False)
    return {"batch": buf.B, "families": "screened joint + narrow tiles vs exact joint + wide tiles",
            "ids_and_frames_identical": got[0] == got[1], "tokens": sum(len(x) for x in got[0][0])}


def timed_pipeline(model, bufs, steps, warmup, dec_streams):
    """RTFx-style short run of resident batches through the pipeline -> seconds for `steps` steps"""
    model.run_pipelined(bufs, warmup, dec_streams=dec_streams)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    model.run_pipelined(bufs, steps, dec_streams=dec_streams)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


DUMP_BYTES = 48 << 20               # --dump-outputs: budget of the joint-encoder sample (the whole dump stays under 64 MB)


def dump_outputs(path, model, buf):
    """--dump-outputs: what the timed path handed back for its last step's batch (`buf`), one .npy per array — ids / frames
    [B][U] padded with -1, n_ids, enc_lens (and ALSD scores) in float64, and the joint-encoder projection of a fixed seeded
    sample of rows in float32, zero past each row's length (rows listed in joint_enc_rows)."""
    os.makedirs(path, exist_ok=True)
    got = model.collect(buf)
    B = buf.B
    n = np.asarray([len(x) for x in got.ids])
    ids, frames = np.full((B, max(int(n.max()), 1)), -1.0), np.full((B, max(int(n.max()), 1)), -1.0)
    for b in range(B):
        ids[b, :n[b]], frames[b, :n[b]] = got.ids[b], got.frames[b]
    arrays = {"ids": ids, "frames": frames, "n_ids": n.astype(np.float64), "enc_lens": np.asarray(got.enc_lens, np.float64)}
    if got.scores is not None:
        arrays["scores"] = np.asarray(got.scores, np.float64)
    k = max(1, min(B, 32, DUMP_BYTES // (buf.tp_max * buf.joint_enc.shape[2] * 4)))
    rows = np.sort(np.random.default_rng(0).choice(B, size=k, replace=False))
    je = buf.joint_enc[torch.from_numpy(rows).to(buf.joint_enc.device)].cpu().numpy().astype(np.float32)
    for i, b in enumerate(rows):
        je[i, got.enc_lens[b]:] = 0.0
    arrays["joint_enc_rows"], arrays["joint_enc"] = rows.astype(np.float64), je
    for name, a in arrays.items():
        np.save(os.path.join(path, name + ".npy"), a)


def resident_sets(model, batch, seconds, n_sets, seed0):
    bufs, lens_all, host = [], [], []
    for k in range(n_sets):
        audio, lens = synthetic_batch(batch, seconds, seed=seed0 + 1000 * k)
        b = model.stage([audio[i, :lens[i]] for i in range(batch)], buf=model.new_buffers(batch, int(seconds * 16000)))
        torch.cuda.synchronize()
        bufs.append(b)
        lens_all.append(lens)
        host.append((audio, lens))
    return bufs, lens_all, host


def extra_configs(model, cfg, sd, args, host_sets):
    """The other configurations the survey names, each a short run inside this one process (they are reported in the
    `configs` object, never as `value`)."""
    out = {}
    n_sets = len(host_sets)
    # BASELINE configs[1]: batch 32 x 10 s on one GPU
    try:
        # (three decode lanes were tried for this decode-bound size and lose: 14.1 vs 12.1 ms/step, profiles/r03e_bench.json)
        bufs32, lens32, _ = resident_sets(model, 32, args.seconds, n_sets, 4321)
        dt = timed_pipeline(model, bufs32, 30, 5, args.dec_streams)
        out["b32"] = {"workload": "32 x 10 s per step (BASELINE configs[1]), HBM-resident, pipelined",
                      "value": round(sum(float(lens32[i % n_sets].sum()) for i in range(30)) / 16000.0 / dt, 1),
                      "ms_per_step": round(dt / 30 * 1e3, 3)}
        del bufs32
    except Exception as e:
        out["b32"] = {"error": repr(e)}
    # the reference's own call pattern: ONE utterance per transcribe() (batch_size=1, transcribe.py:48-50), host to host
    try:
        wave = host_sets[0][0][0, :int(host_sets[0][1][0])]
        model.transcribe_waveforms([wave])
        lat = []
        for _ in range(12):
            t0 = time.perf_counter()
            r1 = model.transcribe_waveforms([wave])
            lat.append(time.perf_counter() - t0)
        lat.sort()
        out["b1_latency"] = {"workload": f"one {len(wave) / 16000.0:g} s utterance per call (the reference's batch_size=1), host float32 -> token ids",
                             "latency_ms_median": round(lat[len(lat) // 2] * 1e3, 2), "latency_ms_min": round(lat[0] * 1e3, 2),
                             "value": round(len(wave) / 16000.0 / lat[len(lat) // 2], 1), "tokens": len(r1.ids[0])}
    except Exception as e:
        out["b1_latency"] = {"error": repr(e)}
    # SURVEY §8(d) ragged set: lengths U(2 s, 10 s), seed 1235, through the host-to-host boundary (sorted, tight padding)
    try:
        n = 4 * args.batch
        audio, lens = synthetic_batch(n, args.seconds, seed=1235, ragged=True, min_seconds=2.0)
        waves = [audio[i, :lens[i]] for i in range(n)]
        model.transcribe_waveforms(waves[:2 * args.batch], max_batch=args.batch)      # warm the pool / kernels
        t0 = time.perf_counter()
        res = model.transcribe_waveforms(waves, max_batch=args.batch)
        dt = time.perf_counter() - t0
        out["ragged_u2_10"] = {"workload": f"{n} utterances, lengths U(2 s, 10 s) seed 1235, host float32 -> token ids "
                                           f"(length-sorted batches of {args.batch}, each padded to its own longest utterance)",
                               "value": round(float(lens.sum()) / 16000.0 / dt, 1), "wall_ms": round(dt * 1e3, 1),
                               "tokens": sum(len(x) for x in res.ids)}
        del audio, waves
    except Exception as e:
        out["ragged_u2_10"] = {"error": repr(e)}
    # the reference checkpoint's decode strategy (decode.py:29,38-41): ALSD, beam 4, on the synthetic recipe on which the search
    # behaves like on a trained model (profiles/r04zz_alsd_recipe_sweep.txt): a prediction network that weighs in the joint
    # (dec_gain 8) and peaked posteriors (out_gain 8, blank offset 53) -> tens of labels per utterance instead of the whole
    # 2 x T' label budget the flat random joint spent (311 labels per utterance in rounds 2-4).  The search still runs all
    # T' + budget alignment steps (a beam is never all-final in one step), so the time is per-step cost x 415.
    sd_alsd = synthetic_state_dict(cfg, 0, blank_bias=53.0, dec_gain=8.0, out_gain=8.0)
    for key, cfg2, what, sd2 in (
            ("alsd4", cfg.with_(decoding="alsd", beam_size=4), "ALSD beam-4 decode (max_target_len 2.0; synthetic recipe dec_gain 8 / out_gain 8 / "
             "blank offset 53: a trained model's label density)", sd_alsd),
            ("window_128_128_g1", cfg.with_(att_left=128, att_right=128, n_global=1),
             "limited-context attention [128, 128] + 1 global token (SURVEY row L5), greedy decode", sd)):
        try:
            m2 = AsrModel(cfg2, sd2, SyntheticTokenizer(cfg2.vocab_size), device=str(model.device))
            bufs2 = [m2.stage([a[i, :l[i]] for i in range(args.batch)], buf=m2.new_buffers(args.batch, int(args.seconds * 16000)))
                     for a, l in host_sets]
            torch.cuda.synchronize()
            steps = 8
            dt = timed_pipeline(m2, bufs2, steps, 3, args.dec_streams)
            out[key] = {"workload": f"{args.batch} x {args.seconds:g} s per step, {what}, HBM-resident, pipelined",
                        "value": round(sum(float(host_sets[i % n_sets][1].sum()) for i in range(steps)) / 16000.0 / dt, 1),
                        "ms_per_step": round(dt / steps * 1e3, 3)}
            if key.startswith("alsd"):
                n_lab = bufs2[0].n_ids.cpu().numpy()[:args.batch]
                out[key]["mean_tokens_per_utt"] = round(float(n_lab.mean()), 1)
                out[key]["max_tokens_per_utt"] = int(n_lab.max())
                try:                     # labels, alignment steps and float32 scores of the first rows against the C checker, bit for bit
                    from oracle import greedy as og
                    k = 2
                    m2.run_device(bufs2[0])
                    torch.cuda.synchronize()
                    got = m2.collect(bufs2[0])
                    st = bufs2[0].frames.cpu().numpy()
                    nn = bufs2[0].n_ids.cpu().numpy()
                    want = og.rnnt_alsd(cfg2, sd2, bufs2[0].joint_enc[:k].cpu().numpy(), np.asarray(got.enc_lens[:k], np.int32), beam=4, max_target_len=2.0)
                    ok = all(got.ids[b] == want[b][0] and st[b, :nn[b]].tolist() == want[b][1] and np.float32(got.scores[b]) == np.float32(want[b][2]) for b in range(k))
                    out[key]["parity"] = {"rows": k, "checker": "oracle/rnnt_alsd.c on the device's joint projection (follows oracle/alsd.py; unpinned against NeMo)",
                                          "labels_steps_scores_bit_exact": bool(ok)}
                except Exception as e:
                    out[key]["parity"] = {"error": repr(e)}
            if key.startswith("window"):
                out[key]["parity"] = window_parity(m2, cfg2, sd, host_sets[0])
            del bufs2, m2
            torch.cuda.empty_cache()
        except Exception as e:
            out[key] = {"error": repr(e)}
    # BASELINE configs[0]'s model on the GPU: reazonspeech.espnet.asr Conformer-Transducer 120M — the same
    # kernels behind another front-end / subsampling / joint, one 20 s window's worth of work per utterance
    try:
        out["espnet_120m"] = espnet_config(model.device, args)
    except Exception as e:
        out["espnet_120m"] = {"error": repr(e)}
    try:
        out["espnet_120m_beam20"] = espnet_beam_config(model.device, args)
    except Exception as e:
        out["espnet_120m_beam20"] = {"error": repr(e)}
    # BASELINE configs[3]: reazonspeech.k2.asr, the Zipformer transducer behind sherpa-onnx in the reference
    try:
        out["k2_zipformer_159m"] = k2_config(model.device, args)
    except Exception as e:
        out["k2_zipformer_159m"] = {"error": repr(e)}
    # BASELINE configs[4]: reazonspeech.avsr, the AV-HuBERT audio-visual encoder-decoder, batch = 16 clips
    try:
        out["avsr_b16"] = avsr_config(model.device, args)
    except Exception as e:
        out["avsr_b16"] = {"error": repr(e)}
    return out


def espnet_parity(am, cfg, sd, buf256, first):
    """End-to-end id parity of the ESPnet family (pkg/espnet-asr/src/transcribe.py:69: `model(np.pad(samples, PADDING))[0][0]`)
    on ALL 256 rows of the timed batch against the committed float32-oracle golden (tests/golden/bench_espnet_fp32.npz:
    oracle/espnet.py run end to end on every row, one utterance per call): the float32 parity mode must reproduce ids and
    frames, the bf16 throughput mode is flip-audited against the parity mode's projection (oracle/audit.py)."""
    import hashlib
    from oracle import audit, greedy as og
    from reazonspeech_amd.espnet.asr.model import EspnetModel, synthetic_token_list, PADDING
    gold = np.load(os.path.join(ROOT, "tests", "golden", "bench_espnet_fp32.npz"))
    audio, lens = first
    if hashlib.sha256(audio.tobytes()).digest() != bytes(gold["audio_sha256"].tolist()):
        return {"error": "the resident batch is not the golden's batch (seed / rank / --seconds differ)"}
    rows = int(gold["rows"])
    off = gold["ids_offsets"]
    g_ids = [gold["ids"][off[b]:off[b + 1]].tolist() for b in range(rows)]
    g_frames = [gold["frames"][off[b]:off[b + 1]].tolist() for b in range(rows)]
    waves = [np.pad(audio[i, :lens[i]], PADDING) for i in range(audio.shape[0])]
    t0 = time.perf_counter()
    m32 = EspnetModel(cfg, sd, synthetic_token_list(cfg.vocab_size, 0), device=str(am.device), precision="fp32").am
    b32 = m32.stage(waves, buf=m32.new_buffers(len(waves), len(waves[0])))
    m32.run_device(b32)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    m32.run_device(b32)
    torch.cuda.synchronize()
    ms32 = (time.perf_counter() - t1) * 1e3
    got32 = m32.collect(b32)
    g = torch.Generator().manual_seed(int(gold["proj_seed"]))
    R = (torch.randn((cfg.joint_hidden, 8), generator=g, dtype=torch.float32) / cfg.joint_hidden ** 0.5).to(am.device)
    proj = (b32.joint_enc @ R).cpu().numpy()
    perr = max(float(np.abs(proj[b, :got32.enc_lens[b]] - gold["proj"][b, :got32.enc_lens[b]]).max()) for b in range(rows))
    exact = [got32.ids[b] == g_ids[b] and got32.frames[b] == g_frames[b] for b in range(rows)]
    out = {"checker": "tests/golden/bench_espnet_fp32.npz: oracle/espnet.py (float32 CPU restatement of the ESPnet2 model; unpinned against "
                      "ESPnet itself) end to end on every row; generator tests/golden/make_espnet_golden.py",
           "fp32_mode": {"rows": rows, "ids_exact": f"{sum(exact)}/{rows}", "enc_lens_equal": got32.enc_lens[:rows] == gold["enc_lens"].tolist(),
                         "joint_proj_fingerprint_max_err_all_rows": round(perr, 7), "rows_differing": [b for b in range(rows) if not exact[b]],
                         "golden_rows_with_a_margin_below_1e-3": int((gold["min_margin"] < float(gold["near_tie"])).sum()),
                         "decisions": int(gold["n_decisions"].sum()), "ms_per_batch_of_256": round(ms32, 1),
                         "rtfx": round(float(lens.sum()) / 16000.0 / (ms32 * 1e-3), 1), "load_and_first_run_s": round(t1 - t0, 1)}}
    # the bf16 throughput mode (the timed kernels) on the same rows, audited against the parity mode's projection
    am.run_device(buf256)
    torch.cuda.synchronize()
    got16 = am.collect(buf256)
    f16 = buf256.joint_enc
    dj = max(float((f16[b, :got16.enc_lens[b]] - b32.joint_enc[b, :got16.enc_lens[b]]).abs().max()) for b in range(rows))
    audits = audit.flip_audit_batch(cfg, sd, b32.joint_enc[:rows], f16[:rows], got16.enc_lens[:rows], got16.ids[:rows], got16.frames[:rows],
                                    device=am.device)
    equal = [got16.ids[b] == g_ids[b] and got16.frames[b] == g_frames[b] for b in range(rows)]
    s = audit.summarize(audits, equal)
    ref_tokens = sum(len(x) for x in g_ids)
    dist = sum(edit_distance(got16.ids[b], g_ids[b]) for b in range(rows) if not equal[b])
    same = og.rnnt_greedy(cfg, sd, f16[:8].cpu().numpy(), np.asarray(got16.enc_lens[:8], np.int32))
    s.update(rows=rows, ids_exact_vs_fp32_oracle=f"{sum(equal)}/{rows}", token_agreement=round(1.0 - dist / max(ref_tokens, 1), 4),
             joint_enc_max_diff_vs_fp32_mode=round(dj, 4),
             every_flip_obeys_the_lipschitz_bound=all(fl["margin_ref"] <= fl["bound"] * (1 + 1e-9) + 1e-12 for a in audits for fl in a["flips"]),
             decode_bit_exact_given_same_joint_enc_rows_0_7=got16.ids[:8] == [r[0] for r in same] and got16.frames[:8] == [r[1] for r in same])
    out["bf16_audit_all_rows"] = s
    del m32, b32
    torch.cuda.empty_cache()
    return out


def family_roofline(am, buf, utterances, top=8):
    """`roofline` object of another model family: one batch through the sequential schedule with the library's HIP-event
    profiler on the GEMM class (the MFMA-bound class of every family) -> achieved TFLOP/s of Σ 2·M·N·K over Σ launch durations,
    fraction of the dense bf16 peak, the `top` shapes by time, and the algorithmic GEMM work per utterance."""
    ctx = am.ctx
    am.run_device(buf)
    torch.cuda.synchronize()
    ctx.profile_enable(capi.PROF_GEMM)
    ctx.profile_reset()
    t0 = time.perf_counter()
    am.run_device(buf)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    g = ctx.profile_read(capi.PROF_GEMM)
    launches = ctx.profile_launches(capi.PROF_GEMM)
    ctx.profile_enable(0)
    if not g["launches"] or g["ms"] <= 0:
        return None
    achieved = g["flops"] / (g["ms"] * 1e-3) / 1e12
    shapes = per_shape_roofline(launches)
    return {"bound": "mfma", "kernel": "gemm_smf16_kernel (every dense contraction of this family's encoder)", "achieved": round(achieved, 1),
            "peak": MFMA_BF16_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": round(achieved / MFMA_BF16_PEAK_TFLOPS, 4), "traffic": None,
            "launches": int(g["launches"]), "avg_launch_us": round(g["ms"] / g["launches"] * 1e3, 2), "schedule": "sequential, one batch",
            "gemm_ms_per_batch": round(g["ms"], 2), "batch_ms_sequential": round(dt * 1e3, 2), "share_of_sequential_batch": round(g["ms"] / (dt * 1e3), 3),
            "algorithmic_gemm_gflop_per_utt": round(g["flops"] / utterances / 1e9, 2),
            "algorithmic_bytes_per_launch": round(g["bytes"] / g["launches"]),
            "per_shape": dict(list(shapes.items())[:top])}


def k2_parity(am, cfg, sd, buf256, waves, audio):
    """End-to-end id parity of the Zipformer family (pkg/k2-asr/src/transcribe.py:36-45: create_stream / accept_waveform /
    decode_stream -> tokens, timestamps) on ALL 256 rows of the timed batch against the committed float32-oracle golden
    (tests/golden/bench_k2_fp32.npz: oracle/zipformer.py, its own window / mel banks / position rows, run end to end on every
    row, one utterance per call): the float32 parity mode must reproduce ids and frames, the bf16 throughput mode is flip-audited
    against the parity mode's projection (oracle/audit.py: flip_audit_batch_k2)."""
    import hashlib
    from oracle import audit, greedy as og, zipformer as oz
    from reazonspeech_amd.k2.asr.model import K2Model, synthetic_tokens
    gold = np.load(os.path.join(ROOT, "tests", "golden", "bench_k2_fp32.npz"))
    if hashlib.sha256(audio.tobytes()).digest() != bytes(gold["audio_sha256"].tolist()):
        return {"error": "the resident batch is not the golden's batch (seed / rank / --seconds differ)"}
    rows = int(gold["rows"])
    off = gold["ids_offsets"]
    g_ids = [gold["ids"][off[b]:off[b + 1]].tolist() for b in range(rows)]
    g_frames = [gold["frames"][off[b]:off[b + 1]].tolist() for b in range(rows)]
    t0 = time.perf_counter()
    m32 = K2Model(cfg, sd, synthetic_tokens(cfg.vocab_size, 0), device=str(am.device), precision="fp32").am
    b32 = m32.stage(waves, buf=m32.new_buffers(len(waves), len(waves[0])))
    m32.run_device(b32)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    m32.run_device(b32)
    torch.cuda.synchronize()
    ms32 = (time.perf_counter() - t1) * 1e3
    got32 = m32.collect(b32)
    g = torch.Generator().manual_seed(int(gold["proj_seed"]))
    R = (torch.randn((cfg.joiner_dim, 8), generator=g, dtype=torch.float32) / cfg.joiner_dim ** 0.5).to(am.device)
    proj = (b32.joint_enc @ R).cpu().numpy()
    perr = max(float(np.abs(proj[b, :got32.enc_lens[b]] - gold["proj"][b, :got32.enc_lens[b]]).max()) for b in range(rows))
    exact = [got32.ids[b] == g_ids[b] and got32.frames[b] == g_frames[b] for b in range(rows)]
    secs = float(sum(len(w) for w in waves) - 2 * len(waves) * int(0.9 * 16000)) / 16000.0
    out = {"checker": "tests/golden/bench_k2_fp32.npz: oracle/zipformer.py (float32 CPU restatement of icefall's Zipformer2 transducer + sherpa-onnx's greedy "
                      "search, its own fbank / position tables; unpinned against icefall / sherpa-onnx themselves) end to end on every row; generator "
                      "tests/golden/make_k2_golden.py",
           "rows": rows, "ids_exact": f"{sum(exact)}/{rows}",
           "fp32_mode": {"rows": rows, "ids_exact": f"{sum(exact)}/{rows}", "enc_lens_equal": got32.enc_lens[:rows] == gold["enc_lens"].tolist(),
                         "joint_proj_fingerprint_max_err_all_rows": round(perr, 7), "rows_differing": [b for b in range(rows) if not exact[b]],
                         "golden_rows_with_a_margin_below_1e-3": int((gold["min_margin"] < float(gold["near_tie"])).sum()),
                         "decisions": int(gold["n_decisions"].sum()), "ms_per_batch_of_256": round(ms32, 1),
                         "rtfx": round(secs / (ms32 * 1e-3), 1), "load_and_first_run_s": round(t1 - t0, 1)}}
    # the bf16 throughput mode (the timed kernels) on the same rows, audited against the parity mode's projection
    am.run_device(buf256)
    torch.cuda.synchronize()
    got16 = am.collect(buf256)
    f16 = buf256.joint_enc
    dj = max(float((f16[b, :got16.enc_lens[b]] - b32.joint_enc[b, :got16.enc_lens[b]]).abs().max()) for b in range(rows))
    audits = audit.flip_audit_batch_k2(cfg, sd, b32.joint_enc[:rows], f16[:rows], got16.enc_lens[:rows], got16.ids[:rows], got16.frames[:rows], device=am.device)
    equal = [got16.ids[b] == g_ids[b] and got16.frames[b] == g_frames[b] for b in range(rows)]
    s = audit.summarize(audits, equal)
    ref_tokens = sum(len(x) for x in g_ids)
    dist = sum(edit_distance(got16.ids[b], g_ids[b]) for b in range(rows) if not equal[b])
    same = og.k2_greedy(cfg, sd, f16[:8].cpu().numpy(), np.asarray(got16.enc_lens[:8], np.int32))
    worst = mean = 0.0
    for b in range(2):                         # rows 0-1 (full 10 s rows of the timed batch) against the bf16-recipe oracle
        ref = oz.forward(cfg, sd, waves[b], "bf16")
        n = ref["joint_enc"].shape[0]
        e = (f16[b, :n].cpu() - ref["joint_enc"]).abs()
        worst, mean = max(worst, float(e.max())), max(mean, float(e.mean()))
    small = am.stage(waves[:1], buf=am.new_buffers(1, len(waves[0])))
    am.run_device(small)
    torch.cuda.synchronize()
    alone = am.collect(small)
    n0 = alone.enc_lens[0]
    s.update(rows=rows, ids_exact_vs_fp32_oracle=f"{sum(equal)}/{rows}", token_agreement=round(1.0 - dist / max(ref_tokens, 1), 4),
             joint_enc_max_diff_vs_fp32_mode=round(dj, 4),
             every_flip_obeys_the_lipschitz_bound=all(fl["margin_ref"] <= fl["bound"] * (1 + 1e-9) + 1e-12 for a in audits for fl in a["flips"]),
             decode_bit_exact_given_same_joint_enc_rows_0_7=got16.ids[:8] == [r[0] for r in same] and got16.frames[:8] == [r[1] for r in same],
             joint_enc_rows01_vs_bf16_recipe_oracle_max_err=round(worst, 4), joint_enc_rows01_vs_bf16_recipe_oracle_mean_err=round(mean, 5),
             alone_equals_inside_batch_bits=bool(torch.equal(small.joint_enc[0, :n0], f16[0, :n0])) and alone.ids[0] == got16.ids[0]
             and alone.frames[0] == got16.frames[0])
    out["bf16_audit_all_rows"] = s
    del m32, b32, small
    torch.cuda.empty_cache()
    return out


def k2_config(device, args, steps=10):
    """`reazonspeech.k2.asr` (pkg/k2-asr/src/huggingface.py:73-83, transcribe.py:24-39): 256 x 10 s utterances with the reference's
    0.9 s of padding on both sides through kaldi-style fbank + encoder_embed + the six Zipformer2 stacks + the stateless-decoder
    greedy search, HBM-resident and pipelined like the headline loop.  Parity (`k2_parity`): ALL 256 rows of the timed batch against
    the committed float32-oracle golden — the float32 parity mode's ids / frames, the bf16 mode flip-audited — plus rows 0-1 against
    the bf16-recipe oracle, decode bit-exact vs oracle/k2_greedy.c, batch invariance (an utterance alone == inside the batch, bits)."""
    from reazonspeech_amd.runtime.k2_config import ZIPFORMER_159M
    from reazonspeech_amd.runtime.k2_weights import synthetic_state_dict_k2
    from reazonspeech_amd.k2.asr.model import K2Model, synthetic_tokens
    cfg = ZIPFORMER_159M
    sd = synthetic_state_dict_k2(cfg, 0)
    km = K2Model(cfg, sd, synthetic_tokens(cfg.vocab_size, 0), device=str(device))
    am = km.am
    pad = int(0.9 * 16000)
    n_sets = max(1 + args.dec_streams, 3)
    bufs, secs = [], []
    for k in range(n_sets):
        audio, lens = synthetic_batch(args.batch, args.seconds, seed=4242 + 1000 * k)
        waves = [np.pad(audio[i, :lens[i]], pad) for i in range(args.batch)]
        bufs.append(am.stage(waves, buf=am.new_buffers(args.batch, len(waves[0]))))
        secs.append(float(lens.sum()) / 16000.0)
        if k == 0:
            first, first_audio = waves, audio
    torch.cuda.synchronize()
    dt = timed_pipeline(am, bufs, steps, 3, args.dec_streams)
    n_tok = bufs[0].n_ids.cpu().numpy()
    res = {"workload": f"{args.batch} x {args.seconds:g} s per step (+ 0.9 s of padding on both sides), icefall Zipformer2 transducer "
                       f"{cfg.n_params() / 1e6:.0f}M (6 stacks, 19 layers), stateless-decoder greedy search (one symbol per frame), HBM-resident, pipelined",
           "value": round(sum(secs[i % n_sets] for i in range(steps)) / dt, 1), "ms_per_step": round(dt / steps * 1e3, 3),
           "enc_frames": bufs[0].tp_max, "mean_tokens_per_utt": round(float(n_tok.mean()), 1)}
    try:
        res["roofline"] = family_roofline(am, bufs[0], args.batch)
    except Exception as e:
        res["roofline"] = {"error": repr(e)}
    try:
        res["parity"] = k2_parity(am, cfg, sd, bufs[0], first, first_audio)
    except Exception as e:
        res["parity"] = {"error": repr(e)}
    del bufs, km
    torch.cuda.empty_cache()
    return res


def avsr_config(device, args):
    """BASELINE configs[4] `reazonspeech.avsr`: the AV-HuBERT encoder-decoder (pkg/avsr/src/avhubert/; 161M parameters: Conv3d + ResNet-18
    video front-end, 12 x 768 HuBERT encoder, 6-layer Transformer decoder) on 16 clips of 10 s (250 frames at 25 Hz: four stacked log
    filterbank frames + one 88 x 88 mouth crop per frame), float32 like the reference.  Timed: `AVHubertModel.forward`
    (rs_avsr_encoder_forward) and `generate(num_beams=5, max_new_tokens=32)` (the README's call with a shorter token budget: random
    weights never emit eos).  Parity: the committed golden of THE REFERENCE ITSELF (tests/golden/avsr_ref_base.npz: the reference's own
    modules run on these weights and 16 ragged clips of <= 4 s) — encoder output, teacher-forced logits, greedy and beam-search ids."""
    import hashlib
    from reazonspeech_amd.runtime.avsr_config import AVSR_BASE
    from reazonspeech_amd.runtime.avsr_synth import synthetic_clips
    from reazonspeech_amd.runtime.avsr_weights import synthetic_state_dict_avsr
    from reazonspeech_amd.avsr import AVHubertForConditionalGeneration
    cfg = AVSR_BASE
    sd = synthetic_state_dict_avsr(cfg, 0)
    model = AVHubertForConditionalGeneration(cfg, sd, device=str(device), products="exact")

    def measure(products):
        model.dev.set_products(products)
        B, T, beams, new_tokens = 16, 250, 5, 32
        a, v, mask, _ = synthetic_clips(B, T, seed=4242)
        ad, vd, md = (torch.from_numpy(x).to(model.device) for x in (a, v[:, :, 0], mask))
        model.dev.encode(ad, vd, md)
        torch.cuda.synchronize()
        reps = 5
        t0 = time.perf_counter()
        for _ in range(reps):
            enc = model.dev.encode(ad, vd, md)
        torch.cuda.synchronize()
        enc_ms = (time.perf_counter() - t0) / reps * 1e3
        model.generate(input_values=ad, pixel_values=vd, padding_mask=md, num_beams=beams, max_new_tokens=4)
        t0 = time.perf_counter()
        seq = model.generate(input_values=ad, pixel_values=vd, padding_mask=md, num_beams=beams, max_new_tokens=new_tokens)
        torch.cuda.synchronize()
        gen_ms = (time.perf_counter() - t0) * 1e3
        secs = B * T / 25.0
        # algorithmic work of the encoder half: ResNet front-end + projections + encoder layers (2 x multiply-adds)
        d, f, L = cfg.encoder_embed_dim, cfg.encoder_ffn_embed_dim, cfg.encoder_layers
        h1, h2 = cfg.image_size // 2, cfg.image_size // 4
        per_frame = 2.0 * (h1 * h1 * 64 * 245 + h2 * h2 * (4 * 64 * 64 * 9) + (h2 // 2 + h2 % 2) ** 2 * (64 * 128 * 9 + 3 * 128 * 128 * 9 + 64 * 128)
                           + 36 * (128 * 256 * 9 + 3 * 256 * 256 * 9 + 128 * 256) + 9 * (256 * 512 * 9 + 3 * 512 * 512 * 9 + 256 * 512)
                           + 512 * d + 104 * d + 2 * d * d + d * (d // cfg.conv_pos_groups) * cfg.conv_pos + L * (4 * d * d + 2 * d * f + 2 * T * d))
        res = {"workload": f"{B} clips x {T / 25.0:g} s ({T} frames at 25 Hz: 104-dim stacked log filterbank + 88 x 88 mouth crop per frame), AV-HuBERT "
                           f"{cfg.n_params() / 1e6:.0f}M, float32 end to end like the reference; generate(num_beams={beams}, max_new_tokens={new_tokens})",
               "value": round(secs / ((gen_ms) * 1e-3), 1), "unit": "audio-visual seconds per wall second (encoder + beam search, one batch of 16)",
               "encoder_ms": round(enc_ms, 2), "generate_ms": round(gen_ms, 2), "value_encoder_only": round(secs / (enc_ms * 1e-3), 1),
               "generated_tokens_per_clip": int(seq.shape[1] - 1), "dtype": "f32",
               "algorithmic_gflop_per_clip_encoder": round(per_frame * T / 1e9, 1),
               "roofline": {"bound": "mfma", "kernel": "gemm_f32_kernel (v_mfma_f32_16x16x4_f32: every convolution patch product and Linear)",
                            "achieved": round(per_frame * T * B / (enc_ms * 1e-3) / 1e12, 2), "peak": 157.3, "unit": "TFLOP/s (encoder forward, algorithmic FLOPs / wall)",
                            "frac": round(per_frame * T * B / (enc_ms * 1e-3) / 1e12 / 157.3, 4), "traffic": None}}
        try:
            g = np.load(os.path.join(ROOT, "tests", "golden", "avsr_ref_base.npz"))
            Bg, Tg = int(g["clips"]), int(g["frames"])
            ga, gv, gm, _ = synthetic_clips(Bg, Tg, seed=int(g["input_seed"]), ragged=True, min_frames=max(8, Tg // 3))
            if hashlib.sha256(ga.tobytes() + gv.tobytes() + gm.tobytes()).digest() != bytes(g["input_sha256"].tolist()):
                raise RuntimeError("inputs drifted from the golden's")
            enc_g = model.dev.encode(ga, gv, gm).cpu()
            R = torch.randn((cfg.encoder_embed_dim, 8), generator=torch.Generator().manual_seed(int(g["proj_seed"]))) / cfg.encoder_embed_dim ** 0.5
            logits = model(input_values=ga, pixel_values=gv, padding_mask=gm, decoder_input_ids=g["greedy"][:, :-1]).logits.cpu()
            Rv = torch.randn((cfg.vocab_size, 8), generator=torch.Generator().manual_seed(int(g["proj_seed"]) + 1)) / cfg.vocab_size ** 0.5
            kb = int(g["beam_clips"])
            greedy = model.generate(input_values=ga, pixel_values=gv, padding_mask=gm, num_beams=1, max_new_tokens=int(g["new_tokens"]))
            bm = model.generate(input_values=ga[:kb], pixel_values=gv[:kb], padding_mask=gm[:kb], num_beams=int(g["beams"]), max_new_tokens=int(g["new_tokens"]),
                                return_dict_in_generate=True)
            res["parity"] = {"checker": "tests/golden/avsr_ref_base.npz: THE REFERENCE ITSELF (pkg/avsr/src/avhubert/*.py imported unchanged, float32 CPU) on these "
                                        "synthetic weights and 16 ragged clips; generator tests/golden/make_avsr_golden.py",
                             "clips": Bg, "frames": Tg,
                             "encoder_clip0_max_err": round(float((enc_g[0] - torch.from_numpy(g["enc"][0])).abs().max()), 7),
                             "encoder_fingerprint_max_err_all_clips": round(float(((enc_g @ R) - torch.from_numpy(g["enc_proj"])).abs().max()), 7),
                             "logits_clips01_max_err": round(float((logits[:2] - torch.from_numpy(g["logits"])).abs().max()), 6),
                             "logits_fingerprint_max_err_all_clips": round(float(((logits @ Rv) - torch.from_numpy(g["logits_proj"])).abs().max()), 6),
                             "greedy_ids_exact": f"{int((greedy.numpy() == g['greedy']).all(axis=1).sum())}/{Bg}",
                             "beam_ids_exact": f"{int((bm.sequences.numpy() == g['beam']).all(axis=1).sum())}/{kb}" if bm.sequences.shape == g["beam"].shape else "shape differs",
                             "beam_scores_max_err": round(float(np.abs(bm.sequences_scores.numpy() - g["beam_scores"]).max()), 7)}
        except Exception as e:
            res["parity"] = {"error": repr(e)}
        return res

    res = measure("exact")
    try:
        # the same model with every float32 product of the big GEMMs / convolutions formed from three bf16 matrix-core terms (csrc/k_f32.hip
        # X3; `products="x3"`): NOT the mode `value` is quoted on — its own timings and its own parity against the same golden
        x3 = measure("x3")
        res["bf16x3_products"] = {"what": "products=\"x3\": hi / lo bf16 split of both operands, hi.hi + hi.lo + lo.hi on v_mfma_f32_16x16x32_bf16, float32 accumulation "
                                          "(16 mantissa bits per operand; gfx950 has no tf32 / xf32 MFMA); storage, softmax, LayerNorm, decode-step GEMMs stay float32",
                                  "value": x3["value"], "encoder_ms": x3["encoder_ms"], "generate_ms": x3["generate_ms"],
                                  "encoder_tflops_algorithmic": x3["roofline"]["achieved"], "parity": x3.get("parity")}
    except Exception as e:
        res["bf16x3_products"] = {"error": repr(e)}
    model.dev.set_products("exact")
    del model
    torch.cuda.empty_cache()
    return res


def espnet_config(device, args):
    """`reazonspeech.espnet.asr` (pkg/espnet-asr/src/transcribe.py): 256 x 10 s utterances with the reference's (16000, 8000)
    padding through front-end + Conv2dSubsampling + 17 conformer blocks + transducer greedy search, HBM-resident and pipelined
    like the headline loop; parity of two utterances against the CPU oracle of that model (oracle/espnet.py)."""
    from reazonspeech_amd.runtime.config import ESPNET_CONFORMER_120M
    from reazonspeech_amd.runtime.weights_espnet import synthetic_state_dict_espnet
    from reazonspeech_amd.espnet.asr.model import EspnetModel, synthetic_token_list, PADDING
    cfg = ESPNET_CONFORMER_120M
    sd = synthetic_state_dict_espnet(cfg, 0)
    em = EspnetModel(cfg, sd, synthetic_token_list(cfg.vocab_size, 0), device=str(device))
    am = em.am
    n_sets = max(1 + args.dec_streams, 3)
    bufs, secs = [], []
    for k in range(n_sets):
        audio, lens = synthetic_batch(args.batch, args.seconds, seed=4242 + 1000 * k)
        waves = [np.pad(audio[i, :lens[i]], PADDING) for i in range(args.batch)]
        bufs.append(am.stage(waves, buf=am.new_buffers(args.batch, len(waves[0]))))
        secs.append(float(lens.sum()) / 16000.0)
        if k == 0:
            first = (audio, lens)
    torch.cuda.synchronize()
    steps = 10
    dt = timed_pipeline(am, bufs, steps, 3, args.dec_streams)
    n_tok = bufs[0].n_ids.cpu().numpy()
    res = {"workload": f"{args.batch} x {args.seconds:g} s per step (+ (16000, 8000) samples of padding each), ESPnet Conformer-Transducer "
                       f"{cfg.n_params() / 1e6:.0f}M, transducer greedy search (one symbol per frame), HBM-resident, pipelined",
           "value": round(sum(secs[i % n_sets] for i in range(steps)) / dt, 1), "ms_per_step": round(dt / steps * 1e3, 3),
           "enc_frames": bufs[0].tp_max, "mean_tokens_per_utt": round(float(n_tok.mean()), 1)}
    try:
        res["roofline"] = family_roofline(am, bufs[0], args.batch)
    except Exception as e:
        res["roofline"] = {"error": repr(e)}
    try:
        res["parity"] = espnet_parity(am, cfg, sd, bufs[0], first)
    except Exception as e:
        res["parity"] = {"error": repr(e)}
    del bufs, em
    torch.cuda.empty_cache()
    return res


def espnet_beam_config(device, args, beam=20, max_pops=640):
    """`reazonspeech.espnet.asr` with the decode the reference actually runs: Speech2Text's default transducer beam search
    (beam_size 20, score_norm; pkg/espnet-asr/src/transcribe.py:27-31) on the device (k_rnnt_beam.hip), pipelined behind the
    encoder like every other configuration.  The synthetic checkpoint is the one the beam-search tests use (dec_gain 8: an
    untrained joint in which the encoder dominates makes the default search extend a frame without end).  Parity: two
    utterances, first 64 frames, against oracle/espnet_beam.c on the same joint-encoder projection — labels, scores, pop counts."""
    from reazonspeech_amd.runtime.config import ESPNET_CONFORMER_120M
    from reazonspeech_amd.runtime.weights_espnet import synthetic_state_dict_espnet
    from reazonspeech_amd.espnet.asr.model import EspnetModel, synthetic_token_list, PADDING
    cfg = ESPNET_CONFORMER_120M
    sd = synthetic_state_dict_espnet(cfg, 0, blank_bias=16.0, dec_gain=8.0)
    em = EspnetModel(cfg, sd, synthetic_token_list(cfg.vocab_size, 0), device=str(device), beam_size=beam, max_pops=max_pops)
    am = em.am
    n_sets = max(1 + args.dec_streams, 3)
    bufs, secs = [], []
    for k in range(n_sets):
        audio, lens = synthetic_batch(args.batch, args.seconds, seed=4242 + 1000 * k)
        waves = [np.pad(audio[i, :lens[i]], PADDING) for i in range(args.batch)]
        bufs.append(am.stage(waves, buf=am.new_buffers(args.batch, len(waves[0]))))
        secs.append(float(lens.sum()) / 16000.0)
    torch.cuda.synchronize()
    steps = 4
    dt = timed_pipeline(am, bufs, steps, 2, args.dec_streams)
    pops = bufs[0].pops.cpu().numpy().astype(np.float64)
    frames = float(bufs[0].enc_lens.sum())
    res = {"workload": f"{args.batch} x {args.seconds:g} s per step (+ (16000, 8000) samples of padding each), ESPnet Conformer-Transducer "
                       f"{cfg.n_params() / 1e6:.0f}M, default transducer beam search, beam {beam}, score_norm (Speech2Text's defaults), "
                       f"HBM-resident, pipelined, {args.dec_streams} decode lane(s)",
           "value": round(sum(secs[i % n_sets] for i in range(steps)) / dt, 1), "ms_per_step": round(dt / steps * 1e3, 3),
           "enc_frames": bufs[0].tp_max, "mean_tokens_per_utt": round(float(bufs[0].n_ids.cpu().numpy().mean()), 1),
           "pops_per_frame": round(float(pops.sum() / max(frames, 1.0)), 2), "max_pops_per_utterance": int(pops.max())}
    try:
        from oracle import greedy as og
        b0 = bufs[0]
        k, T = 2, 64
        el = np.minimum(b0.enc_lens.cpu().numpy()[:k], T).astype(np.int32)
        f = b0.joint_enc[:k].cpu().numpy()
        want = og.espnet_beam(cfg, sd, f, el, beam=beam, max_pops=max_pops, out_cap=b0.u_max)
        dev = am.device
        sub = am.stage([np.zeros(16, np.float32)] * k)          # a k-row buffer set for the outputs
        je = torch.zeros((k, b0.tp_max, cfg.joint_hidden), dtype=torch.float32, device=dev)
        je.copy_(b0.joint_enc[:k])
        ids = torch.zeros((k, b0.u_max), dtype=torch.int32, device=dev)
        n_ids = torch.zeros((k,), dtype=torch.int32, device=dev)
        sc = torch.zeros((k,), dtype=torch.float32, device=dev)
        pp = torch.zeros((k,), dtype=torch.int32, device=dev)
        ws = torch.empty((am.ctx.beam_workspace_bytes(k, beam, b0.tp_max, max_pops),), dtype=torch.uint8, device=dev)
        am.ctx.rnnt_beam(je, torch.from_numpy(el).to(dev), k, b0.tp_max, beam, True, max_pops, ids, n_ids, sc, pp, ws,
                         torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        n = n_ids.cpu().numpy()
        got = [(ids[i, :n[i]].cpu().tolist(), float(sc[i]), int(pp[i])) for i in range(k)]
        res["parity"] = {"utterances": k, "frames": T, "checker": "oracle/espnet_beam.c (float32, fixed order; follows the torch restatement of "
                         "ESPnet's default_beam_search — unpinned against ESPnet itself)",
                         "labels_scores_pops_bit_exact": got == [(w[0], float(np.float32(w[1])), w[2]) for w in want],
                         "whole_utterances": "tests/test_gpu_espnet_fp32.py::test_120m_beam20_whole_utterances (-m gpu): 32 rows x 358 frames of "
                                             "this batch, device == C checker bit for bit and labels == the float64 restatement's committed "
                                             "golden (the C checker needs ~40 s of CPU per whole row: not repeated inside the bench)"}
        del sub
    except Exception as e:
        res["parity"] = {"error": repr(e)}
    del bufs, em
    torch.cuda.empty_cache()
    return res


def window_parity(model, cfg, sd, host_set, k=2):
    """limited-context attention at the benchmark geometry, ALL rows of a resident batch: the float32 parity mode with the same
    attention predicate is the reference (itself checked against the fp32 CPU oracle on `k` utterances: oracle/model.py
    attention_allowed), the throughput mode is compared with it row by row — joint-projection difference, ids identity
    count, flip audit (oracle/audit.py)."""
    from oracle import model as om, audit
    audio, lens = host_set
    B = audio.shape[0]
    waves = [audio[b, :int(lens[b])] for b in range(B)]
    buf = model.stage(waves, buf=model.new_buffers(B, audio.shape[1]))
    model.run_device(buf)
    torch.cuda.synchronize()
    got = model.collect(buf)
    m32 = AsrModel(cfg, sd, SyntheticTokenizer(cfg.vocab_size), device=str(model.device), precision="fp32")
    b32 = m32.stage(waves, buf=m32.new_buffers(B, audio.shape[1]))
    enc32 = torch.zeros((B, b32.tp_max, cfg.d_model), dtype=torch.float32, device=model.device)
    m32.run_device(b32, want_enc=enc32)
    torch.cuda.synchronize()
    got32 = m32.collect(b32)
    e_max = 0.0
    for b in range(k):
        wav = np.pad(audio[b, :int(lens[b])], 8000)
        taps = {}
        f, el = om.forward_to_joint(cfg, sd, torch.from_numpy(wav)[None], torch.tensor([len(wav)]), "fp32", taps)
        n = int(el[0])
        e_max = max(e_max, float((enc32[b, :n].cpu() - taps["enc"][0, :n]).abs().max()))
    dj = max(float((buf.joint_enc[b, :got.enc_lens[b]] - b32.joint_enc[b, :got.enc_lens[b]]).abs().max()) for b in range(B))
    audits = audit.flip_audit_batch(cfg, sd, b32.joint_enc, buf.joint_enc, got.enc_lens, got.ids, got.frames, device=model.device)
    equal = [got.ids[b] == got32.ids[b] and got.frames[b] == got32.frames[b] for b in range(B)]
    s = audit.summarize(audits, equal)
    out = {"rows": B, "reference": "float32 parity mode with the same attention predicate, same rows",
           "fp32_mode_encoder_max_err_vs_cpu_oracle": round(e_max, 7), "fp32_mode_rows_checked_against_cpu_oracle": k,
           "joint_enc_max_diff_vs_fp32_mode": round(dj, 4), "ids_exact_vs_fp32_mode": f"{sum(equal)}/{B}",
           "local_flips": s["local_flips"], "every_id_difference_starts_at_a_flip": s["every_id_difference_starts_at_a_flip"],
           "every_flip_obeys_the_lipschitz_bound": all(fl["margin_ref"] <= fl["bound"] * (1 + 1e-9) + 1e-12 for a in audits for fl in a["flips"]),
           "flip_margin_max": s.get("flip_margin_max")}
    del m32, b32, enc32
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256, help="utterances per GPU per step")
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--tiny", action="store_true", help="debug: 2-layer toy config (NOT a valid bench line)")
    ap.add_argument("--full", action="store_true",
                    help="after the headline figure, also everything that takes runs of its own: PCIe-inclusive and host-boundary "
                         "rates, sequential-schedule GEMM roofline, cpu_baseline, parity, configs (trimmed by the --no-* switches)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--no-fp32-parity", action="store_true", help="skip the float32-parity-mode pass over all 256 rows")
    ap.add_argument("--no-extra-configs", action="store_true", help="skip the `configs` object (B = 32, ragged, ALSD, windowed)")
    ap.add_argument("--api-batches", type=int, default=8,
                    help="batches of --batch utterances pushed through the public host-to-host boundary (8 x 256 = BASELINE configs[2]'s 2048)")
    ap.add_argument("--decoding", default="greedy_batch", choices=["greedy_batch", "alsd"],
                    help="decode strategy: the headline metric is greedy; alsd = the device beam search (extra line for profiles/)")
    ap.add_argument("--beam", type=int, default=4, help="beam size of --decoding alsd")
    ap.add_argument("--att-context", default="", help="left,right,n_global: limited-context attention (extra line for profiles/)")
    ap.add_argument("--buffer-sets", type=int, default=int(os.environ.get("RS_BUFFER_SETS", "4")),
                    help="resident batches the pipeline rotates through (at least 1 + decode streams)")
    ap.add_argument("--dec-streams", type=int, default=int(os.environ.get("RS_DEC_STREAMS", "2")),
                    help="decode consecutive batches on this many streams (n lanes need n + 1 resident batches)")
    ap.add_argument("--no-pipeline", action="store_true",
                    help="run encoder and decode of each batch back to back on one stream")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one computed to DIR/<name>.npy (rank 0)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus and world > 1:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    torch.cuda.set_device(local_rank)
    if world > 1:
        rdist.init("nccl")

    cfg = TINY if args.tiny else FASTCONFORMER_619M
    alsd = args.decoding == "alsd"
    if alsd:
        cfg = cfg.with_(decoding="alsd", beam_size=args.beam)
    if args.att_context:
        left, right, n_glob = (int(x) for x in args.att_context.split(","))
        cfg = cfg.with_(att_left=left, att_right=right, n_global=n_glob)
    t0 = time.time()
    # (--decoding alsd: the synthetic recipe with a trained model's label density, see extra_configs)
    sd = synthetic_state_dict(cfg, 0, blank_bias=53.0, dec_gain=8.0, out_gain=8.0) if alsd else synthetic_state_dict(cfg, seed=0)
    model = AsrModel(cfg, sd, SyntheticTokenizer(cfg.vocab_size), device=f"cuda:{local_rank}")
    # resident batches (different utterances): the pipelined path rotates through them
    n_sets = max(1 + args.dec_streams, args.buffer_sets)
    bufs, lens_all, host_sets = resident_sets(model, args.batch, args.seconds, n_sets, 1234 + 17 * rank)
    buf = bufs[0]
    audio0, lens0 = host_sets[0]
    setup_s = time.time() - t0
    pipelined = not args.no_pipeline

    step_done = []                  # host time at which each step's hypotheses were complete (and gathered)

    def after_decode(bf):
        # called on the decode worker right after batch i is decoded: this step's one collective
        if world > 1:
            rdist.gather_hypotheses(bf.ids, bf.frames, bf.n_ids)
            torch.cuda.current_stream().synchronize()
        step_done.append(time.perf_counter())

    # The GEMM roofline is measured live with a HIP event pair around every GEMM launch (rs_profile_enable).  The events
    # themselves cost ~1 ms per step (392 markers, each a dependency point in the encoder queue), so they are recorded on
    # every PROFILE_EVERY-th step of the timed region only: `roofline.launches` says how many launches that was.
    PROFILE_EVERY = 2
    prof_state = {"on": False, "steps": 0}

    def before_encoder(i):
        if not prof_state["on"]:
            return
        sample = i % PROFILE_EVERY == 0
        model.ctx.profile_enable(capi.PROF_GEMM if sample else 0)
        prof_state["steps"] += 1 if sample else 0

    def run_steps(n):
        if pipelined:
            model.run_pipelined(bufs, n, after_decode=after_decode, dec_streams=args.dec_streams, before_encoder=before_encoder)
        else:
            for i in range(n):
                before_encoder(i)
                model.run_device(bufs[i % n_sets])
                after_decode(bufs[i % n_sets])

    run_steps(args.warmup)
    prof = not args.no_profile
    if prof:
        model.ctx.profile_reset()
        prof_state["on"] = True
    rdist.barrier()
    torch.cuda.synchronize()
    step_done.clear()
    t0 = time.perf_counter()
    run_steps(args.steps)
    torch.cuda.synchronize()
    rdist.barrier()
    dt = time.perf_counter() - t0
    if world > 1:        # every rank's own clock (rank 0 reports the maximum): scripts/scale.sh lists them
        print(f"rank {rank}: {dt / args.steps * 1e3:.3f} ms/step over {args.steps} steps", file=sys.stderr, flush=True)
    prof_state["on"] = False
    gemm = model.ctx.profile_read(capi.PROF_GEMM) if prof else None
    gemm_launches = model.ctx.profile_launches(capi.PROF_GEMM) if prof else []
    model.ctx.profile_enable(0)
    dt = rdist.max_over_ranks(dt)
    if args.dump_outputs and rank == 0:     # before anything else runs on the resident batches: step i used bufs[i % n_sets]
        dump_outputs(args.dump_outputs, model, bufs[(args.steps - 1) % n_sets])
    # per-step completion intervals (steady state of the pipeline): median next to the mean
    marks = [t0] + list(step_done)
    intervals = sorted(b - a for a, b in zip(marks[1:-1], marks[2:])) if len(marks) > 3 else []
    median_ms = intervals[len(intervals) // 2] * 1e3 if intervals else None

    # PCIe-inclusive rate of the SAME resident-batch loop (never `value`): every batch is copied from pinned host
    # memory first and its hypotheses are copied back after decode
    dt_host = None
    if args.full and pipelined and world == 1:
        model.run_pipelined(bufs, 2, from_host=True, dec_streams=args.dec_streams)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        model.run_pipelined(bufs, args.steps, from_host=True, dec_streams=args.dec_streams)
        torch.cuda.synchronize()
        dt_host = time.perf_counter() - t1

    # SURVEY.md §8(d)'s metric through the PUBLIC boundary: a list of host float32 utterances in, token ids (and, second
    # figure, TranscribeResult text) out — sorting, pinned staging, H2D, the pipeline's fill and drain, D2H all inside
    api = None
    if args.full and world == 1 and not args.tiny and args.api_batches > 0:
        try:
            from reazonspeech_amd.nemo.asr import transcribe_batch, audio_from_numpy, TranscribeConfig
            waves = [host_sets[k % n_sets][0][i, :host_sets[k % n_sets][1][i]] for k in range(args.api_batches) for i in range(args.batch)]
            secs = sum(len(w) for w in waves) / 16000.0
            model.transcribe_waveforms(waves[:4 * args.batch], max_batch=args.batch)          # allocate the pool (4 sets), warm up
            runs = []
            for _ in range(3):
                t1 = time.perf_counter()
                res = model.transcribe_waveforms(waves, max_batch=args.batch)
                runs.append(time.perf_counter() - t1)
            audios = [audio_from_numpy(w, 16000) for w in waves]
            transcribe_batch(model, audios[:args.batch], TranscribeConfig(verbose=False))     # first call: fills the per-tokenizer piece-text cache
            runs_text = []
            for _ in range(3):
                t1 = time.perf_counter()
                texts = transcribe_batch(model, audios, TranscribeConfig(verbose=False))
                runs_text.append(time.perf_counter() - t1)
            runs_text.sort()
            dt_text = runs_text[len(runs_text) // 2]
            runs.sort()
            api = {"utterances": len(waves), "audio_seconds": round(secs, 1),
                   "value_host_to_ids": round(secs / runs[len(runs) // 2], 1), "wall_ms_runs": [round(r * 1e3, 1) for r in runs],
                   "value_transcribe_batch": round(secs / dt_text, 1), "wall_ms_transcribe_batch": round(dt_text * 1e3, 1),
                   "wall_ms_runs_transcribe_batch": [round(r * 1e3, 1) for r in runs_text],
                   "tokens": sum(len(x) for x in res.ids), "results": len(texts),
                   "what": "AsrModel.transcribe_waveforms / transcribe_batch on a host list: length sort, pinned staging by a "
                           "stager thread, H2D, 4 resident batches / 2 decode lanes, D2H; pipeline fill and drain included "
                           "(median of 3 for both)"}
            del audios, waves
        except Exception as e:               # the bench line must still be printed
            api = {"error": repr(e)}

    # the same GEMM launches without the decode stream next to them (sequential schedule, 2 steps): how much of the
    # in-pipeline figure is CU sharing with the decode kernels rather than the kernel itself
    gemm_seq = None
    if args.full and prof and pipelined and world == 1:
        model.ctx.profile_reset()
        model.ctx.profile_enable(capi.PROF_GEMM)
        for i in range(2):
            model.run_device(bufs[i % n_sets])
        torch.cuda.synchronize()
        gemm_seq = model.ctx.profile_read(capi.PROF_GEMM)
        model.ctx.profile_enable(0)

    n_ids = np.concatenate([b.n_ids.cpu().numpy() for b in bufs])
    mean_tokens = float(n_ids.mean())
    audio_seconds = sum(float(lens_all[i % n_sets].sum()) for i in range(args.steps)) / 16000.0 * world
    value = audio_seconds / dt

    if rank == 0:
        out = {
            "metric": f"RTFx (audio-sec/wall-sec), FastConformer-RNNT 619M batch={args.batch}"
                      + (f", ALSD beam {args.beam} decode" if alsd else ""),
            "value": round(value, 1), "unit": "x real-time", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(dt / args.steps * 1e3, 3),
            "ms_per_step_median": round(median_ms, 3) if median_ms else None,
            "step_intervals_ms": [round((b - a) * 1e3, 1) for a, b in zip(marks[:-1], marks[1:])],
            "higher_is_better": True,
            "value_device_resident": round(value, 1),      # = `value` under its explicit name (the bench contract's definition)
            "value_definition": "bench contract: whole-job RTFx with the step's inputs already resident in HBM.  SURVEY 8(d)'s "
                                "definition (host float32 -> TranscribeResult through the public transcribe_batch, H2D / D2H, "
                                "pipeline fill and drain inside the clock) is `value_transcribe_batch`; `value_host_to_ids` stops "
                                "at token ids (both measured by --full)",
            "scaling": "weak", "vs_baseline": None, "dtype": "bf16", "data": "synthetic",
            "config": {"workload": f"FastConformer-RNNT {cfg.n_params() / 1e6:.0f}M, {args.batch} x "
                                   f"{args.seconds:g} s utterances per GPU (+0.5 s pad each side), "
                                   + (f"ALSD beam-{args.beam} decode (max_target_len {cfg.alsd_max_target_len:g})" if alsd else "greedy decode") + ", "
                                   + (f"attention context [{cfg.att_left}, {cfg.att_right}] + {cfg.n_global} global, " if cfg.att_left >= 0 else "")
                                   + "random-init weights, inputs resident in HBM", "global_batch": args.batch * world,
                       "utterance_seconds": args.seconds, "parallelism": f"dp{world}",
                       "enc_frames": buf.tp_max, "resident_batches": n_sets, "mean_tokens_per_utt": round(mean_tokens, 1),
                       "max_tokens_per_utt": int(n_ids.max()),
                       "schedule": (f"2-stage pipeline: one encoder stream + {args.dec_streams} decode lane(s) on their own HIP streams "
                                    f"(encoder of batch i+{args.dec_streams} next to the decodes of the {args.dec_streams} batches before it)")
                                   if pipelined else "sequential"},
            "setup_s": round(setup_s, 1),
        }
        if dt_host:
            out["value_pcie_inclusive"] = round(audio_seconds / dt_host, 1)
            out["ms_per_step_pcie_inclusive"] = round(dt_host / args.steps * 1e3, 3)
        if api:
            out["host_boundary"] = api
            if "value_host_to_ids" in api:
                out["value_host_to_ids"] = api["value_host_to_ids"]
                out["value_transcribe_batch"] = api["value_transcribe_batch"]
        gf = algorithmic_gflop_per_utt(cfg, buf.tp_max, mean_tokens)
        out["algorithmic_tflops_whole_path"] = round(gf * args.batch * world * args.steps / dt / 1e3, 1)
        if gemm and gemm["launches"]:
            per_launch_ms = gemm["ms"] / gemm["launches"]
            achieved = gemm["flops"] / (gemm["ms"] * 1e-3) / 1e12
            traffic = mfma_busy = pmc_clock = None
            try:   # HBM bytes per launch from the committed PMC passes (cannot be collected in-process)
                with open(os.path.join(ROOT, "profiles", "gemm_traffic.json")) as fp:
                    pmc = json.load(fp)
                traffic, mfma_busy, pmc_clock = pmc["hbm_bytes_per_launch"], pmc.get("mfma_busy_pct"), pmc.get("clock_ghz")
            except Exception:
                pass
            out["roofline"] = {"bound": "mfma", "kernel": "gemm_smf16_kernel (every dense contraction of the encoder)",
                               "achieved": round(achieved, 1), "peak": MFMA_BF16_PEAK_TFLOPS, "unit": "TFLOP/s",
                               "frac": round(achieved / MFMA_BF16_PEAK_TFLOPS, 4), "traffic": traffic,
                               "traffic_unit": "HBM bytes per launch (PMC, profiles/gemm_traffic.json)",
                               "algorithmic_bytes_per_launch": round(gemm["bytes"] / gemm["launches"]),
                               "launches": gemm["launches"], "avg_launch_us": round(per_launch_ms * 1e3, 2),
                               "profiled_steps": f"{prof_state['steps']} of {args.steps} (every {PROFILE_EVERY}nd step of the timed region)",
                               "share_of_step": round(gemm["ms"] / max(prof_state["steps"], 1) / (dt / args.steps * 1e3), 3),
                               # committed PMC passes (sequential schedule): MFMA-pipe busy cycles at the clock the chip ran at
                               "mfma_busy_pct_pmc": mfma_busy, "clock_ghz_pmc": pmc_clock,
                               "pmc_source": "profiles/gemm_traffic.json — separate rocprofv3 --pmc passes of THIS tree's evidence run "
                                             "(scripts/evidence.sh), not collected by this process: `traffic`, `mfma_busy_pct_pmc` and "
                                             "`clock_ghz_pmc` are as old as that file says (`collected`)",
                               "pmc_collected": pmc.get("collected") if traffic else None,
                               "traffic_ratio": round(traffic / (gemm["bytes"] / gemm["launches"]), 3) if traffic else None,
                               # the same HIP-event records grouped by GEMM shape: the weakest shape is visible in the line
                               "per_shape": per_shape_roofline(gemm_launches)}
            if gemm_seq and gemm_seq["launches"]:
                seq = gemm_seq["flops"] / (gemm_seq["ms"] * 1e-3) / 1e12
                out["roofline"]["achieved_sequential_schedule"] = round(seq, 1)
                out["roofline"]["frac_sequential_schedule"] = round(seq / MFMA_BF16_PEAK_TFLOPS, 4)
        if args.full and world == 1 and not args.no_cpu_baseline and not alsd:     # the CPU leg and its parity check are the greedy path's
            budget, k = (5.0, 2) if args.tiny else (20.0, 8)
            out["cpu_baseline"], cpu_outputs = cpu_baseline(cfg, sd, audio0, lens0, seconds_budget=budget, max_utt=k)
            try:
                out["parity"] = parity_vs_cpu_leg(model, cfg, sd, bufs[0], audio0, lens0, cpu_outputs)
            except Exception as e:               # the bench line must still be printed
                out["parity"] = {"error": repr(e)}
        if args.full and world == 1 and not alsd and not args.tiny:
            if not isinstance(out.get("parity"), dict):
                out["parity"] = {}
            if not args.no_fp32_parity and not args.att_context:
                try:
                    out["parity"].update(fp32_mode_parity(model, cfg, sd, bufs[0], audio0, lens0))
                except Exception as e:           # the bench line must still be printed
                    out["parity"]["fp32_mode"] = {"error": repr(e)}
            try:
                out["parity"]["decode_families_whole_batch"] = decode_family_check(model, bufs[0])
            except Exception as e:               # the bench line must still be printed
                out["parity"]["decode_families_whole_batch"] = {"error": repr(e)}
        if args.full and world == 1 and not args.tiny and not args.no_extra_configs and not alsd and not args.att_context:
            out["configs"] = extra_configs(model, cfg, sd, args, host_sets)
        print(json.dumps(out), flush=True)
    rdist.shutdown()


if __name__ == "__main__":
    main()
