"""What hotwords cost in the ALSD beam search of reazonspeech.nemo.asr, and that the plain search did not move: FastConformer-RNNT
619M (synthetic weights), 256 x 10 s (seed 4242) staged once in HBM, decoding="alsd", beam 4.

    python scripts/alsd_hotwords_ab.py --parent-tree DIR [--rounds 2] [--repeats 10] [--out profiles/alsd_hotwords_ab.json]

DIR is a checkout of the parent commit with its library built.  Three numbers, each the median over all timed runs of
`AsrModel.decode` alone on the resident encoder projection (host clock around a call that ends in a stream synchronise; 3 warm-up
runs per process first):
  parent_plain_ms     the parent commit's ALSD
  plain_ms            this commit without hotwords: the same kernel text, so it must agree with the parent within the spread
                      between runs — if not, something leaked into the plain path.  `plain_same_results` = ids, alignment steps
                      and scores equal the parent's
  hotwords_ms         this commit with one graph of 1000 random phrases of 2 - 6 tokens on every utterance;
                      hotwords_extra_us_per_step = (hotwords_ms - plain_ms) / alignment steps
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
    from reazonspeech_amd.runtime.config import FASTCONFORMER_619M
    from reazonspeech_amd.runtime.model import AsrModel
    from reazonspeech_amd.runtime.synth import synthetic_batch
    from reazonspeech_amd.runtime.tokenizer import SyntheticTokenizer
    from reazonspeech_amd.runtime.weights import synthetic_state_dict
    import reazonspeech_amd
    assert os.path.realpath(os.path.dirname(os.path.dirname(reazonspeech_amd.__file__))) == os.path.realpath(args.tree), reazonspeech_amd.__file__
    cfg = FASTCONFORMER_619M.with_(decoding="alsd", beam_size=4)
    am = AsrModel(cfg, synthetic_state_dict(cfg, 0), SyntheticTokenizer(cfg.vocab_size, 0), device="cuda:0")
    audio, lens = synthetic_batch(args.batch, args.seconds, seed=4242)
    waves = [audio[i, :lens[i]] for i in range(args.batch)]
    variants = {"plain": am.stage(waves, buf=am.new_buffers(args.batch, max(len(w) for w in waves)))}
    if args.worker == "this":
        from reazonspeech_amd.runtime import k2_hotwords
        rng = np.random.default_rng(1)
        phrases = [(tuple(int(t) for t in rng.integers(0, cfg.vocab_size, size=int(rng.integers(2, 7)))), 1.5) for _ in range(1000)]
        plan = am.graph_plan([k2_hotwords.build_graph(phrases)] * args.batch, args.batch)
        variants["hotwords"] = am.stage(waves, buf=am.new_buffers(args.batch, max(len(w) for w in waves)), hotwords=plan)
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
        el = buf.enc_lens.cpu().numpy()
        budget = [int(cfg.alsd_max_target_len * int(t)) if isinstance(cfg.alsd_max_target_len, float) else int(cfg.alsd_max_target_len) for t in el]
        digest[name] = (h.hexdigest(), int(n.sum()), int(max(int(t) + u for t, u in zip(el, budget))) + 1)
    for i in range(args.warmup + args.repeats):
        for name, buf in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            am.decode(am.ctx, buf, buf.ws, stream)             # synchronises the stream itself
            torch.cuda.synchronize()
            if i >= args.warmup:
                times[name].append((time.perf_counter() - t0) * 1e3)
    print("RESULT " + json.dumps({name: dict(times_ms=times[name], sha256=digest[name][0], tokens=digest[name][1], steps=digest[name][2])
                                  for name in variants}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "alsd_hotwords_ab.json"))
    ap.add_argument("--worker", choices=("parent", "this"))
    ap.add_argument("--tree", default=ROOT)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    if not args.parent_tree:
        raise SystemExit("--parent-tree DIR: a built checkout of the parent commit")
    assert args.rounds * args.repeats >= 20, "at least 20 timed runs per variant"
    runs = {"parent_plain": [], "plain": [], "hotwords": []}
    meta = {}
    for r in range(args.rounds):
        for role, tree in (("parent", os.path.abspath(args.parent_tree)), ("this", ROOT)):
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", role, "--tree", tree, "--repeats", str(args.repeats),
                   "--warmup", str(args.warmup), "--batch", str(args.batch), "--seconds", str(args.seconds)]
            out = subprocess.run(cmd, check=True, capture_output=True, text=True, cwd=tree, timeout=900).stdout
            res = json.loads(next(line for line in out.splitlines() if line.startswith("RESULT "))[7:])
            for name, v in res.items():
                key = "parent_plain" if role == "parent" else name
                runs[key] += v["times_ms"]
                meta.setdefault(key, v)
                assert (meta[key]["sha256"], meta[key]["tokens"]) == (v["sha256"], v["tokens"]), "results changed between rounds"
            print(f"round {r} {role}: " + ", ".join(f"{k} {statistics.median(v['times_ms']):.2f} ms" for k, v in res.items()), flush=True)
    med = {k: statistics.median(v) for k, v in runs.items()}
    steps = meta["plain"]["steps"]
    result = {
        "setup": f"619M synthetic, {args.batch} x {args.seconds:g} s, decoding alsd, beam 4, AsrModel.decode on the resident projection; "
                 f"median of {args.rounds} x {args.repeats} timed runs after {args.warmup} warm-ups per process",
        "alignment_steps": steps,
        "parent_plain_ms": round(med["parent_plain"], 3), "plain_ms": round(med["plain"], 3), "hotwords_ms": round(med["hotwords"], 3),
        "plain_over_parent": round(med["plain"] / med["parent_plain"], 4),
        "plain_same_results": meta["plain"]["sha256"] == meta["parent_plain"]["sha256"],
        "hotwords_phrases": 1000,
        "hotwords_extra_ms": round(med["hotwords"] - med["plain"], 3),
        "hotwords_extra_us_per_step": round((med["hotwords"] - med["plain"]) / steps * 1e3, 3),
        "hotwords_over_plain": round(med["hotwords"] / med["plain"], 4),
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
