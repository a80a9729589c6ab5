"""What hotwords cost in the modified beam search of reazonspeech.k2.asr, and that the plain search did not move: 159M Zipformer
(synthetic weights), 256 x 10 s + 0.9 s of padding (seed 4242) staged once in HBM, max_active_paths = 4.

    python scripts/k2_hotwords_ab.py --parent-tree DIR [--rounds 2] [--repeats 8] [--out profiles/k2_hotwords_ab.json]

DIR is a checkout of the parent commit with its library built.  Three numbers, each the median over all timed runs of
`AsrModel.decode` alone on the resident encoder projection (host clock around a call that ends in a stream synchronise; 3 warm-up
runs per process first):
  parent_plain_ms     the parent commit's modified_beam_search
  plain_ms            this commit without hotwords: the same kernel instantiations, so it must agree with the parent within the
                      spread between runs — if not, something leaked into the plain path.  `plain_same_results` = ids, frames and
                      scores equal the parent's
  hotwords_ms         this commit with one model-level graph of 1000 random phrases of 2 - 6 tokens on every utterance;
                      hotwords_extra_us_per_frame = (hotwords_ms - plain_ms) / encoder frames
Every variant runs in a process of its own (one worker per tree and round, the rounds alternating between the trees; inside the
worker of this tree the plain and the hotword runs alternate), so neither tree's runs all come before or after the other's."""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def worker(args):
    sys.path.insert(0, args.tree)
    import numpy as np
    import torch
    from reazonspeech_amd.runtime.k2_config import ZIPFORMER_159M
    from reazonspeech_amd.runtime.k2_weights import synthetic_state_dict_k2
    from reazonspeech_amd.runtime.synth import synthetic_batch
    from reazonspeech_amd.k2.asr.model import K2Model, synthetic_tokens
    import reazonspeech_amd
    assert os.path.realpath(os.path.dirname(os.path.dirname(reazonspeech_amd.__file__))) == os.path.realpath(args.tree), reazonspeech_amd.__file__
    cfg = ZIPFORMER_159M
    sd = synthetic_state_dict_k2(cfg, 0)
    kw = {}
    if args.worker == "this":
        rng = np.random.default_rng(1)
        kw["hotwords"] = [tuple(int(t) for t in rng.integers(3, cfg.vocab_size, size=int(rng.integers(2, 7)))) for _ in range(1000)]
    km = K2Model(cfg, sd, synthetic_tokens(cfg.vocab_size, 0), device="cuda:0", decoding_method="modified_beam_search", max_active_paths=4, **kw)
    am = km.am
    audio, lens = synthetic_batch(args.batch, args.seconds, seed=4242)
    waves = [np.pad(audio[i, :lens[i]], int(0.9 * 16000)) for i in range(args.batch)]
    variants = {"plain": am.stage(waves, buf=am.new_buffers(args.batch, len(waves[0])))}
    if args.worker == "this":
        plan = am.graph_plan([km.hotwords] * args.batch, args.batch)
        variants["hotwords"] = am.stage(waves, buf=am.new_buffers(args.batch, len(waves[0])), hotwords=plan)
    stream = torch.cuda.current_stream().cuda_stream
    times = {name: [] for name in variants}
    digest = {}
    for name, buf in variants.items():
        am.run_device(buf)                                     # the projection stays resident; also the first decode
        torch.cuda.synchronize()
        n = buf.n_ids.cpu().numpy()
        h = hashlib.sha256()
        for t in (n, buf.scores.cpu().numpy()) + tuple(x.cpu().numpy()[b, :n[b]] for x in (buf.ids, buf.frames) for b in range(args.batch)):
            h.update(np.ascontiguousarray(t).tobytes())
        digest[name] = (h.hexdigest(), int(n.sum()), int(buf.tp_max))
    for i in range(args.warmup + args.repeats):
        for name, buf in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            am.decode(am.ctx, buf, buf.ws, stream)             # synchronises the stream itself
            torch.cuda.synchronize()
            if i >= args.warmup:
                times[name].append((time.perf_counter() - t0) * 1e3)
    print("RESULT " + json.dumps({name: dict(times_ms=times[name], sha256=digest[name][0], tokens=digest[name][1], enc_frames=digest[name][2])
                                  for name in variants}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "k2_hotwords_ab.json"))
    ap.add_argument("--worker", choices=("parent", "this"))
    ap.add_argument("--tree", default=ROOT)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    if not args.parent_tree:
        raise SystemExit("--parent-tree DIR: a built checkout of the parent commit")
    assert args.rounds * args.repeats >= 10, "at least 10 timed runs per variant"
    runs = {"parent_plain": [], "plain": [], "hotwords": []}
    meta = {}
    for r in range(args.rounds):
        for role, tree in (("parent", os.path.abspath(args.parent_tree)), ("this", ROOT)):
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", role, "--tree", tree, "--repeats", str(args.repeats),
                   "--warmup", str(args.warmup), "--batch", str(args.batch), "--seconds", str(args.seconds)]
            out = subprocess.run(cmd, check=True, capture_output=True, text=True, cwd=tree).stdout
            res = json.loads(next(line for line in out.splitlines() if line.startswith("RESULT "))[7:])
            for name, v in res.items():
                key = "parent_plain" if role == "parent" else name
                runs[key] += v["times_ms"]
                meta.setdefault(key, v)
                assert (meta[key]["sha256"], meta[key]["tokens"]) == (v["sha256"], v["tokens"]), "results changed between rounds"
            print(f"round {r} {role}: " + ", ".join(f"{k} {statistics.median(v['times_ms']):.2f} ms" for k, v in res.items()), flush=True)
    med = {k: statistics.median(v) for k, v in runs.items()}
    frames = meta["plain"]["enc_frames"]
    result = {
        "setup": f"159M synthetic, {args.batch} x {args.seconds:g} s + 0.9 s padding, max_active_paths 4, AsrModel.decode on the resident projection; "
                 f"median of {args.rounds} x {args.repeats} timed runs after {args.warmup} warm-ups per process",
        "enc_frames": frames,
        "parent_plain_ms": round(med["parent_plain"], 3), "plain_ms": round(med["plain"], 3), "hotwords_ms": round(med["hotwords"], 3),
        "plain_over_parent": round(med["plain"] / med["parent_plain"], 4),
        "plain_same_results": meta["plain"]["sha256"] == meta["parent_plain"]["sha256"],
        "hotwords_phrases": 1000,
        "hotwords_extra_ms": round(med["hotwords"] - med["plain"], 3),
        "hotwords_extra_us_per_frame": round((med["hotwords"] - med["plain"]) / frames * 1e3, 3),
        "hotwords_change_results": meta["hotwords"]["sha256"] != meta["plain"]["sha256"],
        "tokens": {k: meta[k]["tokens"] for k in meta},
        "min_max_ms": {k: [round(min(v), 3), round(max(v), 3)] for k, v in runs.items()},
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fp:
        json.dump(result, fp, indent=1)
        fp.write("\n")
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
