"""What an n-gram LM costs in the ALSD beam search of reazonspeech.nemo.asr, and that the search without one did not move:
FastConformer-RNNT 619M (synthetic weights), 256 x 10 s (seed 4242) staged once in HBM, decoding="alsd", beam 4.

    python scripts/alsd_lm_ab.py --parent-tree DIR [--rounds 2] [--repeats 10] [--out profiles/alsd_lm_ab.json]

DIR is a checkout of the parent commit with its library built.  Three numbers, each the median over all timed runs of
`AsrModel.decode` alone on the resident encoder projection (host clock around a call that ends in a stream synchronise; 3 warm-up
runs per process first):
  parent_plain_ms     the parent commit's ALSD
  plain_ms            this commit without an LM: the same kernel text, so it must agree with the parent within the spread between
                      runs — if not, something leaked into the plain path.  `plain_same_results` = ids, alignment steps and scores
                      equal the parent's
  lm_ms               this commit with a synthetic order-4 LM (a unigram for every token, about 10^5 higher-order n-grams, prefix
                      closed) at alpha 0.3.  The LM changes what the search keeps, so the comparison that means something is per
                      alignment step: `*_us_per_step` = ms / alignment steps run, the steps estimated from the results as
                      max over utterances of (encoder frames + min(labels of the winner, label budget)) + 1 — a hypothesis is live
                      while its frame index is inside the utterance and the alignment budget lasts —, rounded up to the 16 steps
                      between two looks at the "finished" counter
Every variant runs in a process of its own (one worker per tree and round, the rounds alternating between the trees; inside the
worker of this tree the plain and the LM runs alternate), so neither tree's runs all come before or after the other's."""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def synthetic_lm(cfg, n_high=36000, order=4, seed=1):
    """every unigram, `n_high` random n-grams of full order over a skewed token distribution with all their prefixes (about 10^5
    higher-order n-grams in all), and `<s>`"""
    import numpy as np
    from reazonspeech_amd.runtime import ngram_lm
    rng = np.random.default_rng(seed)
    V = cfg.vocab_size
    p = 1.0 / np.arange(1, V + 1) ** 0.8
    p /= p.sum()
    tokens = rng.permutation(V)
    ent = {(int(t),): (-float(rng.integers(8, 48)) / 8.0, -float(rng.integers(0, 8)) / 8.0) for t in range(V)}
    ent[(ngram_lm.BOS,)] = (-99.0, -0.25)
    grams = tokens[rng.choice(V, size=(n_high, order), p=p)]
    for row in grams.tolist():
        for k in range(2, order + 1):
            ent.setdefault(tuple(row[:k]), (-float(rng.integers(1, 24)) / 8.0, -float(rng.integers(0, 8)) / 8.0 if k < order else 0.0))
    return ngram_lm.build(ent, cfg.vocab_size, cfg.blank_id, cfg.n_logits), len(ent) - V - 1


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
    extra = {}
    if args.worker == "this":
        lm, n_high = synthetic_lm(cfg)
        extra = dict(lm_nodes=lm.n_nodes, lm_higher_order=n_high)
        variants["lm"] = am.stage(waves, buf=am.new_buffers(args.batch, max(len(w) for w in waves)), ngram_lm=(lm, args.alpha))
        assert variants["lm"].lm is not None and variants["plain"].lm is None
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
        mtl = cfg.alsd_max_target_len
        budget = [int(mtl * int(t)) if isinstance(mtl, float) else int(mtl) for t in el]
        steps = int(max(int(t) + min(int(u), bud) for t, u, bud in zip(el, n, budget))) + 1
        digest[name] = (h.hexdigest(), int(n.sum()), (steps + 15) // 16 * 16)
    for i in range(args.warmup + args.repeats):
        for name, buf in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            am.decode(am.ctx, buf, buf.ws, stream)             # synchronises the stream itself
            torch.cuda.synchronize()
            if i >= args.warmup:
                times[name].append((time.perf_counter() - t0) * 1e3)
    print("RESULT " + json.dumps({name: dict(times_ms=times[name], sha256=digest[name][0], tokens=digest[name][1], steps=digest[name][2], **extra)
                                  for name in variants}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--alpha", type=float, default=0.3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "alsd_lm_ab.json"))
    ap.add_argument("--worker", choices=("parent", "this"))
    ap.add_argument("--tree", default=ROOT)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    if not args.parent_tree:
        raise SystemExit("--parent-tree DIR: a built checkout of the parent commit")
    assert args.rounds * args.repeats >= 20, "at least 20 timed runs per variant"
    runs = {"parent_plain": [], "plain": [], "lm": []}
    meta = {}
    for r in range(args.rounds):
        for role, tree in (("parent", os.path.abspath(args.parent_tree)), ("this", ROOT)):
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", role, "--tree", tree, "--repeats", str(args.repeats),
                   "--warmup", str(args.warmup), "--batch", str(args.batch), "--seconds", str(args.seconds), "--alpha", str(args.alpha)]
            out = subprocess.run(cmd, check=True, capture_output=True, text=True, cwd=tree, timeout=900).stdout
            res = json.loads(next(line for line in out.splitlines() if line.startswith("RESULT "))[7:])
            for name, v in res.items():
                key = "parent_plain" if role == "parent" else name
                runs[key] += v["times_ms"]
                meta.setdefault(key, v)
                assert (meta[key]["sha256"], meta[key]["tokens"]) == (v["sha256"], v["tokens"]), "results changed between rounds"
            print(f"round {r} {role}: " + ", ".join(f"{k} {statistics.median(v['times_ms']):.2f} ms" for k, v in res.items()), flush=True)
    med = {k: statistics.median(v) for k, v in runs.items()}
    per_step = {k: med[k] / meta[k]["steps"] * 1e3 for k in ("plain", "lm")}
    result = {
        "setup": f"619M synthetic, {args.batch} x {args.seconds:g} s, decoding alsd, beam 4, AsrModel.decode on the resident projection; "
                 f"median of {args.rounds} x {args.repeats} timed runs after {args.warmup} warm-ups per process",
        "parent_plain_ms": round(med["parent_plain"], 3), "plain_ms": round(med["plain"], 3), "lm_ms": round(med["lm"], 3),
        "plain_over_parent": round(med["plain"] / med["parent_plain"], 4),
        "plain_same_results": meta["plain"]["sha256"] == meta["parent_plain"]["sha256"],
        "lm": {"order": 4, "alpha": args.alpha, "nodes": meta["lm"]["lm_nodes"], "higher_order_ngrams": meta["lm"]["lm_higher_order"]},
        "alignment_steps": {k: meta[k]["steps"] for k in ("plain", "lm")},
        "plain_us_per_step": round(per_step["plain"], 3), "lm_us_per_step": round(per_step["lm"], 3),
        "lm_per_step_over_plain": round(per_step["lm"] / per_step["plain"], 4),
        "lm_over_plain": round(med["lm"] / med["plain"], 4),
        "lm_changes_results": meta["lm"]["sha256"] != meta["plain"]["sha256"],
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
