"""What an n-gram LM costs in the modified beam search of reazonspeech.k2.asr, and that the search without one did not move: 159M
Zipformer (synthetic weights), 256 x 10 s + 0.9 s of padding (seed 4242) staged once in HBM, max_active_paths = 4.

    python scripts/k2_lm_ab.py --parent-tree DIR [--rounds 2] [--repeats 10] [--out profiles/k2_lm_ab.json]

DIR is a checkout of the parent commit with its library built.  Four numbers, each the median over all timed runs of
`AsrModel.decode` alone on the resident encoder projection (host clock around a call that ends in a stream synchronise; 3 warm-up
runs per process first):
  parent_plain_ms     (a) the parent commit's modified_beam_search
  plain_ms            (b) this commit without an LM: the plain kernel instantiations, so it must agree with the parent within the
                      spread between runs.  `plain_same_results` = ids, frames and scores equal the parent's
  lm_ms               (c) this commit with a synthetic order-4 LM at alpha 0.3: every unigram, every n-gram of what the plain search
                      emits on this batch and random higher-order n-grams around those tokens up to about 100k
  lm_hotwords_ms      (d) (c) plus the graph of 1000 random phrases of scripts/k2_hotwords_ab.py on every utterance
(c) and (d) are records, not pass/fail lines; the LM changes what the search keeps (`tokens`), so their times are not the cost of
the walks alone.  *_extra_us_per_frame = (variant - plain_ms) / encoder frames.
Every tree runs in a process of its own (one worker per tree and round, the rounds alternating between the trees; inside the worker
of this tree the variants alternate), so neither tree's runs all come before or after the other's."""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALPHA = 0.3


def synthetic_lm(cfg, seqs, n_high, order=4, seed=1):
    """{(ids...): (log10 p, log10 backoff)}: every unigram, `<s>`, every n-gram of `seqs`, and random n-grams around their tokens"""
    import numpy as np
    from reazonspeech_amd.runtime.ngram_lm import BOS
    rng = np.random.default_rng(seed)
    vocab = np.asarray([t for t in range(cfg.vocab_size) if t not in (cfg.blank_id, cfg.unk_id)])
    ent = {(int(t),): (-float(rng.integers(8, 40)) / 8.0, -float(rng.integers(0, 8)) / 8.0) for t in vocab}
    ent[(BOS,)] = (-99.0, -0.25)
    n0 = len(ent)
    for y in seqs:
        y = (BOS,) + tuple(int(t) for t in y)
        for k in range(len(y)):
            for m in range(2, min(order, len(y) - k) + 1):
                ent.setdefault(y[k:k + m], (-float(rng.integers(0, 8)) / 8.0, -float(rng.integers(0, 8)) / 8.0 if m < order else 0.0))
    seen = np.asarray(sorted({int(t) for y in seqs for t in y})) if seqs else vocab
    while len(ent) - n0 < n_high:
        n = int(rng.integers(2, order + 1))
        near = rng.random(n) < 0.7
        words = tuple(int(a if c else b) for a, b, c in zip(rng.choice(seen, n), rng.choice(vocab, n), near))
        for k in range(2, n + 1):
            ent.setdefault(words[:k], (-float(rng.integers(0, 24)) / 8.0, -float(rng.integers(0, 8)) / 8.0 if k < order else 0.0))
    return ent


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
    km = K2Model(cfg, sd, synthetic_tokens(cfg.vocab_size, 0), device="cuda:0", decoding_method="modified_beam_search", max_active_paths=4)
    am = km.am
    audio, lens = synthetic_batch(args.batch, args.seconds, seed=4242)
    waves = [np.pad(audio[i, :lens[i]], int(0.9 * 16000)) for i in range(args.batch)]
    new = lambda: am.new_buffers(args.batch, len(waves[0]))                # noqa: E731
    variants = {"plain": am.stage(waves, buf=new())}
    stream = torch.cuda.current_stream().cuda_stream
    digest, extra = {}, {}

    def first_run(name, buf):
        am.run_device(buf)                                     # the projection stays resident; also the first decode
        torch.cuda.synchronize()
        n = buf.n_ids.cpu().numpy()
        ids = [buf.ids.cpu().numpy()[b, :n[b]] for b in range(args.batch)]
        h = hashlib.sha256()
        for t in [n, buf.scores.cpu().numpy()] + ids + [buf.frames.cpu().numpy()[b, :n[b]] for b in range(args.batch)]:
            h.update(np.ascontiguousarray(t).tobytes())
        digest[name] = (h.hexdigest(), int(n.sum()), int(buf.tp_max))
        return ids

    plain_ids = first_run("plain", variants["plain"])
    if args.worker == "this":
        from reazonspeech_amd.runtime import ngram_lm
        lm = ngram_lm.build(synthetic_lm(cfg, [y.tolist() for y in plain_ids], args.ngrams), cfg.vocab_size, cfg.blank_id)
        extra = dict(lm_nodes=lm.n_nodes, lm_children=lm.n_children, lm_order=lm.order)
        rng = np.random.default_rng(1)
        graph = km.hotword_graph([tuple(int(t) for t in rng.integers(3, cfg.vocab_size, size=int(rng.integers(2, 7)))) for _ in range(1000)])
        variants["lm"] = am.stage(waves, buf=new(), ngram_lm=(lm, ALPHA))
        variants["lm_hotwords"] = am.stage(waves, buf=new(), hotwords=am.graph_plan([graph] * args.batch, args.batch), ngram_lm=(lm, ALPHA))
        for name in ("lm", "lm_hotwords"):
            first_run(name, variants[name])
    times = {name: [] for name in variants}
    for i in range(args.warmup + args.repeats):
        for name, buf in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            am.decode(am.ctx, buf, buf.ws, stream)             # synchronises the stream itself
            torch.cuda.synchronize()
            if i >= args.warmup:
                times[name].append((time.perf_counter() - t0) * 1e3)
    print("RESULT " + json.dumps({name: dict(times_ms=times[name], sha256=digest[name][0], tokens=digest[name][1], enc_frames=digest[name][2],
                                             **extra) for name in variants}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--ngrams", type=int, default=100000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "k2_lm_ab.json"))
    ap.add_argument("--worker", choices=("parent", "this"))
    ap.add_argument("--tree", default=ROOT)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    if not args.parent_tree:
        raise SystemExit("--parent-tree DIR: a built checkout of the parent commit")
    assert args.rounds * args.repeats >= 20, "at least 20 timed runs per variant"
    runs = {"parent_plain": [], "plain": [], "lm": [], "lm_hotwords": []}
    meta = {}
    for r in range(args.rounds):
        for role, tree in (("parent", os.path.abspath(args.parent_tree)), ("this", ROOT)):
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", role, "--tree", tree, "--repeats", str(args.repeats),
                   "--warmup", str(args.warmup), "--batch", str(args.batch), "--seconds", str(args.seconds), "--ngrams", str(args.ngrams)]
            out = subprocess.run(cmd, check=True, capture_output=True, text=True, cwd=tree, timeout=900).stdout
            res = json.loads(next(line for line in out.splitlines() if line.startswith("RESULT "))[7:])
            for name, v in res.items():
                key = "parent_plain" if role == "parent" else name
                runs[key] += v["times_ms"]
                meta.setdefault(key, v)
                assert (meta[key]["sha256"], meta[key]["tokens"]) == (v["sha256"], v["tokens"]), "results changed between rounds"
            print(f"round {r} {role}: " + ", ".join(f"{k} {statistics.median(v['times_ms']):.2f} ms" for k, v in res.items()), flush=True)
    med = {k: statistics.median(v) for k, v in runs.items()}
    frames = meta["plain"]["enc_frames"]
    per_frame = lambda k: round((med[k] - med["plain"]) / frames * 1e3, 3)     # noqa: E731
    result = {
        "setup": f"159M synthetic, {args.batch} x {args.seconds:g} s + 0.9 s padding, max_active_paths 4, AsrModel.decode on the resident projection; "
                 f"median of {args.rounds} x {args.repeats} timed runs after {args.warmup} warm-ups per process",
        "enc_frames": frames,
        "parent_plain_ms": round(med["parent_plain"], 3), "plain_ms": round(med["plain"], 3), "lm_ms": round(med["lm"], 3),
        "lm_hotwords_ms": round(med["lm_hotwords"], 3),
        "plain_over_parent": round(med["plain"] / med["parent_plain"], 4),
        "plain_same_results": meta["plain"]["sha256"] == meta["parent_plain"]["sha256"],
        "lm": {k: meta["lm"][k] for k in ("lm_nodes", "lm_children", "lm_order")}, "lm_alpha": ALPHA, "hotwords_phrases": 1000,
        "lm_extra_ms": round(med["lm"] - med["plain"], 3), "lm_extra_us_per_frame": per_frame("lm"),
        "lm_hotwords_extra_ms": round(med["lm_hotwords"] - med["plain"], 3), "lm_hotwords_extra_us_per_frame": per_frame("lm_hotwords"),
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
