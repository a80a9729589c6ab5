"""What token log-probabilities (`token_scores=True`, rs_rnnt_token_scores) cost, and that the path without them did not move:
synthetic weights, 256 x 10 s (seed 4242) staged once in HBM.

    python scripts/token_scores_ab.py --parent-tree DIR [--configs nemo,espnet,k2,k2-mbs] [--rounds 2] [--repeats 6]
                                      [--out profiles/token_scores_ab.json]

DIR is a checkout of the parent commit with its library built (the parent's library lacks the two new exports, so it runs under
its own tree's Python, one process per run, like scripts/k2_hotwords_ab.py).  Configurations: nemo 619M greedy, espnet 120M
greedy, k2 159M greedy and modified beam search 4.  Per configuration and round three worker processes run one after the other —
parent, parent again, this tree — so the spread of repeating the parent against itself is measured in the same call as the
comparison.  Inside the worker of this tree scores off and on ALTERNATE run by run.  Timed, after `--warmup` runs per process
(host clock around calls that end in a stream synchronise), median over rounds x repeats >= 10 runs:
  decode_ms       `AsrModel.decode` (+ `AsrModel.score` when on) alone on the resident encoder projection
  transcribe_ms   `AsrModel.transcribe_waveforms` of the 256 host waveforms (staging, front end, encoder, decode, copy back)
Launch records (rs_profile_read_launches, all classes, one `run_device`) are counted in a separate untimed pass: with scores off
they must equal the parent's.  `off_inside_parent_spread`: the off median lies within the parent-vs-parent band
[min(parent medians) - spread, max(parent medians) + spread], spread = |parent A - parent B| per round, the largest taken."""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = ("nemo", "espnet", "k2", "k2-mbs")


def make_model(name, token_scores):
    import numpy as np
    from reazonspeech_amd.runtime.synth import synthetic_batch
    kw = {"token_scores": True} if token_scores is not None else {}      # (the parent tree has no such keyword)
    if name == "nemo":
        from reazonspeech_amd.runtime.config import FASTCONFORMER_619M as cfg
        from reazonspeech_amd.runtime.model import AsrModel
        from reazonspeech_amd.runtime.tokenizer import SyntheticTokenizer
        from reazonspeech_amd.runtime.weights import synthetic_state_dict
        am, pad = AsrModel(cfg, synthetic_state_dict(cfg, 0), SyntheticTokenizer(cfg.vocab_size), device="cuda:0", **kw), 0
    elif name == "espnet":
        from reazonspeech_amd.runtime.config import ESPNET_CONFORMER_120M as cfg
        from reazonspeech_amd.runtime.weights_espnet import synthetic_state_dict_espnet
        from reazonspeech_amd.espnet.asr.model import EspnetModel, synthetic_token_list
        am, pad = EspnetModel(cfg, synthetic_state_dict_espnet(cfg, 0), synthetic_token_list(cfg.vocab_size, 0), device="cuda:0", **kw).am, 0
    else:
        from reazonspeech_amd.runtime.k2_config import ZIPFORMER_159M as cfg
        from reazonspeech_amd.runtime.k2_weights import synthetic_state_dict_k2
        from reazonspeech_amd.k2.asr.model import K2Model, synthetic_tokens
        search = dict(decoding_method="modified_beam_search", max_active_paths=4) if name == "k2-mbs" else {}
        am = K2Model(cfg, synthetic_state_dict_k2(cfg, 0), synthetic_tokens(cfg.vocab_size, 0), device="cuda:0", **search, **kw).am
        pad = int(0.9 * 16000)
    return am, pad, np, synthetic_batch


def worker(args):
    sys.path.insert(0, args.tree)
    import torch
    import reazonspeech_amd
    assert os.path.realpath(os.path.dirname(os.path.dirname(reazonspeech_amd.__file__))) == os.path.realpath(args.tree), reazonspeech_amd.__file__
    this = args.worker == "this"
    am, pad, np, synthetic_batch = make_model(args.config, True if this else None)
    audio, lens = synthetic_batch(args.batch, args.seconds, seed=4242)
    waves = [np.pad(audio[i, :lens[i]], pad) for i in range(args.batch)]
    buf = am.stage(waves, buf=am.new_buffers(args.batch, len(waves[0])))
    stream = torch.cuda.current_stream().cuda_stream
    modes = ("off", "on") if this else ("off",)

    def set_mode(mode):
        if this:
            am.token_scores = mode == "on"

    digest, tokens = {}, {}
    for mode in modes:
        set_mode(mode)
        am.run_device(buf)                                      # the projection stays resident; also the first decode
        torch.cuda.synchronize()
        res = am.collect(buf)
        h = hashlib.sha256(json.dumps([res.ids, res.frames]).encode())
        digest[mode], tokens[mode] = h.hexdigest(), sum(len(x) for x in res.ids)
        if mode == "on":
            lp = [v for row in res.token_logprobs for v in row]
            tokens["mean_logprob"] = float(np.mean(lp)) if lp else None
    times = {m: {"decode": [], "transcribe": []} for m in modes}
    for i in range(args.warmup + args.repeats):
        for mode in modes:                                      # off and on alternate run by run
            set_mode(mode)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            am.decode(am.ctx, buf, buf.ws, stream)              # synchronises the stream itself
            if this:
                am.score(am.ctx, buf, stream)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            am.transcribe_waveforms(waves)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            if i >= args.warmup:
                times[mode]["decode"].append((t1 - t0) * 1e3)
                times[mode]["transcribe"].append((t2 - t1) * 1e3)
    launches = {}
    am.ctx.profile_enable(63)
    for mode in modes:                                          # untimed: the launch records of one whole pass, per class
        set_mode(mode)
        am.ctx.profile_reset()
        am.run_device(buf)
        torch.cuda.synchronize()
        launches[mode] = {str(k): len(am.ctx.profile_launches(k)) for k in (1, 2, 4, 8, 16, 32)}
    am.ctx.profile_enable(0)
    print("RESULT " + json.dumps(dict(times_ms=times, sha256=digest, tokens=tokens, launches=launches, enc_frames=int(buf.tp_max),
                                      u_cap=int(buf.ids.shape[1]))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree")
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "token_scores_ab.json"))
    ap.add_argument("--worker", choices=("parent", "this"))
    ap.add_argument("--config", choices=CONFIGS)
    ap.add_argument("--tree", default=ROOT)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    if not args.parent_tree:
        raise SystemExit("--parent-tree DIR: a built checkout of the parent commit")
    assert args.rounds * args.repeats >= 10, "at least 10 timed runs per variant"
    med = statistics.median
    result = {"setup": f"synthetic weights, {args.batch} x {args.seconds:g} s (seed 4242); median of {args.rounds} x {args.repeats} timed runs after "
                       f"{args.warmup} warm-ups per process; per round: parent, parent again, this tree (scores off / on alternating)"}
    if os.path.exists(args.out):                               # configurations measured in an earlier call stay
        with open(args.out) as fp:
            result.update({k: v for k, v in json.load(fp).items() if k in CONFIGS})
    for config in args.configs.split(","):
        runs = {k: {"decode": [], "transcribe": []} for k in ("parent_a", "parent_b", "off", "on")}
        spread = {"decode": 0.0, "transcribe": 0.0}
        meta = {}
        for r in range(args.rounds):
            round_med = {}
            for role, tree, key in (("parent", os.path.abspath(args.parent_tree), "parent_a"), ("parent", os.path.abspath(args.parent_tree), "parent_b"),
                                    ("this", ROOT, None)):
                cmd = [sys.executable, os.path.abspath(__file__), "--worker", role, "--config", config, "--tree", tree, "--repeats", str(args.repeats),
                       "--warmup", str(args.warmup), "--batch", str(args.batch), "--seconds", str(args.seconds)]
                out = subprocess.run(cmd, check=True, capture_output=True, text=True, cwd=tree, timeout=900).stdout
                res = json.loads(next(line for line in out.splitlines() if line.startswith("RESULT "))[7:])
                for mode, t in res["times_ms"].items():
                    k = key or mode
                    for what in ("decode", "transcribe"):
                        runs[k][what] += t[what]
                        round_med[(k, what)] = med(t[what])
                meta.setdefault(key or "this", res)
                print(f"{config} round {r} {key or 'this'}: " + ", ".join(f"{m} decode {med(t['decode']):.2f} transcribe {med(t['transcribe']):.2f} ms"
                                                                           for m, t in res["times_ms"].items()), flush=True)
            for what in spread:
                spread[what] = max(spread[what], abs(round_med[("parent_a", what)] - round_med[("parent_b", what)]))
        entry = {"enc_frames": meta["this"]["enc_frames"], "u_cap": meta["this"]["u_cap"], "tokens": meta["this"]["tokens"],
                 "same_ids_and_frames": len({meta["parent_a"]["sha256"]["off"], meta["this"]["sha256"]["off"], meta["this"]["sha256"]["on"]}) == 1,
                 "launch_records": {"parent": meta["parent_a"]["launches"]["off"], "off": meta["this"]["launches"]["off"], "on": meta["this"]["launches"]["on"]},
                 "off_launches_equal_parent": meta["parent_a"]["launches"]["off"] == meta["this"]["launches"]["off"]}
        for what in ("decode", "transcribe"):
            pa, pb, off, on = (med(runs[k][what]) for k in ("parent_a", "parent_b", "off", "on"))
            entry[what] = {"parent_ms": [round(pa, 3), round(pb, 3)], "parent_spread_ms": round(spread[what], 3), "off_ms": round(off, 3),
                           "on_ms": round(on, 3), "overhead_ms": round(on - off, 3), "overhead_percent": round(100.0 * (on - off) / off, 2),
                           "off_inside_parent_spread": min(pa, pb) - spread[what] <= off <= max(pa, pb) + spread[what],
                           "min_max_ms": {k: [round(min(v[what]), 3), round(max(v[what]), 3)] for k, v in runs.items()}}
        result[config] = entry
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fp:
            json.dump(result, fp, indent=1)
            fp.write("\n")
        print(config, json.dumps(entry), flush=True)


if __name__ == "__main__":
    main()
