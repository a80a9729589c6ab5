"""What forced alignment (`AsrModel.align_waveforms`, rs_rnnt_align) costs, and that `transcribe_waveforms` did not move: synthetic
weights, the bench batch (256 x 10 s, seed 4242); the texts are the greedy result.

    python scripts/align_ab.py --parent-tree DIR [--configs nemo,espnet,k2] [--repeats 20] [--out profiles/align_ab.json]

DIR is a checkout of the parent commit with its library built (it runs under its own tree's Python, one process per run, like
scripts/token_scores_ab.py).  Per family three worker processes run one after the other — parent, this tree, parent again:
  transcribe_ms   median of `--repeats` timed `transcribe_waveforms` calls after `--warmup`; the ids and frames must be identical
                  (sha256), the medians are compared with the +-3 % the project sees between runs
In this tree's worker, after that:
  align_ms        median of `--align-repeats` `align_waveforms` calls on the same waveforms with the greedy ids as texts
  encoder_ms      front end + encoder alone (`run_encoder`, host clock around a stream synchronise)
  the brackets    one profiled call (rs_profile_read_launches, decode class): the plan, the prediction chain (LSTM families), the
                  lattice (row list, gather, exact float32 joint, pick; for the Zipformer family its decoder rows too), the DP
  lattice_tflops  2 x rows x joint_hidden x n_logits / lattice time, next to the 107 TF/s recorded for gemm_f32_kernel
  dp_us_per_diagonal   DP time / the longest utterance's diagonals (one workgroup per utterance: the longest one sets the time)
"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = ("nemo", "espnet", "k2")
GEMM_F32_TFLOPS = 107.0        # gemm_f32_kernel's recorded rate (README.md)


def make_model(name):
    import numpy as np
    from reazonspeech_amd.runtime.synth import synthetic_batch
    if name == "nemo":
        from reazonspeech_amd.runtime.config import FASTCONFORMER_619M as cfg
        from reazonspeech_amd.runtime.model import AsrModel
        from reazonspeech_amd.runtime.tokenizer import SyntheticTokenizer
        from reazonspeech_amd.runtime.weights import synthetic_state_dict
        am, pad = AsrModel(cfg, synthetic_state_dict(cfg, 0), SyntheticTokenizer(cfg.vocab_size), device="cuda:0"), 0
    elif name == "espnet":
        from reazonspeech_amd.runtime.config import ESPNET_CONFORMER_120M as cfg
        from reazonspeech_amd.runtime.weights_espnet import synthetic_state_dict_espnet
        from reazonspeech_amd.espnet.asr.model import EspnetModel, synthetic_token_list
        am, pad = EspnetModel(cfg, synthetic_state_dict_espnet(cfg, 0), synthetic_token_list(cfg.vocab_size, 0), device="cuda:0").am, 0
    else:
        from reazonspeech_amd.runtime.k2_config import ZIPFORMER_159M as cfg
        from reazonspeech_amd.runtime.k2_weights import synthetic_state_dict_k2
        from reazonspeech_amd.k2.asr.model import K2Model, synthetic_tokens
        am = K2Model(cfg, synthetic_state_dict_k2(cfg, 0), synthetic_tokens(cfg.vocab_size, 0), device="cuda:0").am
        pad = int(0.9 * 16000)
    return am, pad, np, synthetic_batch


def worker(args):
    sys.path.insert(0, args.tree)
    import torch
    import reazonspeech_amd
    assert os.path.realpath(os.path.dirname(os.path.dirname(reazonspeech_amd.__file__))) == os.path.realpath(args.tree), reazonspeech_amd.__file__
    am, pad, np, synthetic_batch = make_model(args.config)
    audio, lens = synthetic_batch(args.batch, args.seconds, seed=4242)
    waves = [np.pad(audio[i, :lens[i]], pad) for i in range(args.batch)]
    res = am.transcribe_waveforms(waves)
    torch.cuda.synchronize()
    out = {"sha256": hashlib.sha256(json.dumps([res.ids, res.frames]).encode()).hexdigest(), "tokens": sum(len(x) for x in res.ids)}
    times = []
    for i in range(args.warmup + args.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        am.transcribe_waveforms(waves)
        torch.cuda.synchronize()
        if i >= args.warmup:
            times.append((time.perf_counter() - t0) * 1e3)
    out["transcribe_ms"] = times
    if args.worker == "this":
        cfg = am.cfg
        one = cfg.max_symbols == 1
        texts = res.ids
        al = am.align_waveforms(waves, texts)                   # warm-up, and the figures of the alignment itself
        torch.cuda.synchronize()
        a_times = []
        for _ in range(args.align_repeats):
            t0 = time.perf_counter()
            am.align_waveforms(waves, texts)
            torch.cuda.synchronize()
            a_times.append((time.perf_counter() - t0) * 1e3)
        buf = am.stage(waves)
        stream = torch.cuda.current_stream().cuda_stream
        e_times = []
        for _ in range(args.align_repeats + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            am.run_encoder(buf, stream)
            torch.cuda.synchronize()
            e_times.append((time.perf_counter() - t0) * 1e3)
        am.ctx.profile_enable(8)
        am.ctx.profile_reset()
        am.align_waveforms(waves, texts)
        torch.cuda.synchronize()
        recs = am.ctx.profile_launches(8)
        am.ctx.profile_enable(0)
        names = ["plan", "lattice", "dp"] if len(recs) == 3 else ["plan", "prediction_chain", "lattice", "dp"]
        assert len(recs) == len(names), recs
        brackets = {k: round(r[5], 3) for k, r in zip(names, recs)}
        flops = recs[names.index("lattice")][4]
        V = cfg.n_logits
        rows = int(round(flops / (2.0 * cfg.joint_hidden * V)))
        feasible = [i for i in range(len(waves)) if al.feasible[i]]
        diagonals = max((al.enc_lens[i] + len(texts[i]) + (1 if one else 0) for i in feasible), default=0)
        tf = flops / (brackets["lattice"] * 1e-3) / 1e12 if brackets["lattice"] > 0 else None
        out["align"] = {"one_per_frame": bool(one), "align_ms": a_times, "encoder_ms": e_times[1:], "brackets_ms": brackets, "lattice_rows": rows,
                        "labels": sum(len(t) for t in texts), "longest_text": max(len(t) for t in texts), "enc_frames": max(al.enc_lens),
                        "feasible": len(feasible), "lattice_tflops": round(tf, 2) if tf else None,
                        "lattice_vs_gemm_f32": f"{tf:.1f} TF/s against {GEMM_F32_TFLOPS:g} TF/s of gemm_f32_kernel: {100.0 * tf / GEMM_F32_TFLOPS:.0f} %" if tf else None,
                        "longest_diagonals": int(diagonals), "dp_us_per_diagonal": round(1e3 * brackets["dp"] / diagonals, 3) if diagonals else None,
                        "mean_norm_loglik": float(np.mean([al.log_likelihood[i] / max(len(texts[i]), 1) for i in feasible])) if feasible else None,
                        "loglik_ge_best": all(al.log_likelihood[i] >= al.alignment_log_prob[i] for i in feasible)}
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree")
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--align-repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_ab.json"))
    ap.add_argument("--worker", choices=("parent", "this"))
    ap.add_argument("--config", choices=CONFIGS)
    ap.add_argument("--tree", default=ROOT)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    if not args.parent_tree:
        raise SystemExit("--parent-tree DIR: a built checkout of the parent commit")
    med = statistics.median
    result = {"setup": f"synthetic weights, {args.batch} x {args.seconds:g} s (seed 4242); transcribe: median of {args.repeats} timed runs after "
                       f"{args.warmup} warm-ups per process (parent, this tree, parent again); align: median of {args.align_repeats}; texts = the greedy ids"}
    if os.path.exists(args.out):                               # families measured in an earlier call stay
        with open(args.out) as fp:
            result.update({k: v for k, v in json.load(fp).items() if k in CONFIGS})
    for config in args.configs.split(","):
        got = {}
        for key, role, tree in (("parent_a", "parent", os.path.abspath(args.parent_tree)), ("this", "this", ROOT),
                                ("parent_b", "parent", os.path.abspath(args.parent_tree))):
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", role, "--config", config, "--tree", tree, "--repeats", str(args.repeats),
                   "--align-repeats", str(args.align_repeats), "--warmup", str(args.warmup), "--batch", str(args.batch), "--seconds", str(args.seconds)]
            out = subprocess.run(cmd, check=True, capture_output=True, text=True, cwd=tree, timeout=900).stdout
            got[key] = json.loads(next(line for line in out.splitlines() if line.startswith("RESULT "))[7:])
            print(f"{config} {key}: transcribe {med(got[key]['transcribe_ms']):.2f} ms", flush=True)
        pa, pb, th = (med(got[k]["transcribe_ms"]) for k in ("parent_a", "parent_b", "this"))
        parent = 0.5 * (pa + pb)
        entry = {"tokens": got["this"]["tokens"],
                 "same_ids_and_frames": got["parent_a"]["sha256"] == got["this"]["sha256"] == got["parent_b"]["sha256"],
                 "transcribe_ms": {"parent": [round(pa, 3), round(pb, 3)], "this": round(th, 3), "this_vs_parent_percent": round(100.0 * (th - parent) / parent, 2),
                                   "within_3_percent": abs(th - parent) <= 0.03 * parent}}
        a = got["this"]["align"]
        a["align_ms"], a["encoder_ms"] = round(med(a["align_ms"]), 3), round(med(a["encoder_ms"]), 3)
        entry["align"] = a
        result[config] = entry
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fp:
            json.dump(result, fp, indent=1)
            fp.write("\n")
        print(config, json.dumps(entry), flush=True)


if __name__ == "__main__":
    main()
