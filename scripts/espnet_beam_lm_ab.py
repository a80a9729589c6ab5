"""What an n-gram LM and hotwords cost in the default beam search of reazonspeech.espnet.asr, and that the search without them did not
move: 120M Conformer-Transducer (synthetic weights, blank bias 16, dec_gain 8), 256 x 10 s + (16000, 8000) samples of padding (seed
1234: the batch of scripts/espnet_beam_bench.py) staged once in HBM, beam 20, max_pops 640.

    python scripts/espnet_beam_lm_ab.py --parent-tree DIR [--rounds 2] [--repeats 10] [--out profiles/espnet_beam_lm_ab.json]

DIR is a checkout of the parent commit with its library built.  Each number is the median over all timed runs of the search alone
on the resident encoder projection (host clock around a call that ends in a stream synchronise; 3 warm-up runs per process first):
  parent_plain_ms     (a) the parent commit's rs_rnnt_beam
  plain_ms            (b) this commit through the same entry: the plain kernel instantiations.  `plain_same_results` = ids, frames,
                      scores and pops equal the parent's.  `parent_spread` = (max - min) / median of the parent's per-process medians:
                      the criterion for (b) against (a) is that spread, measured here, not a fixed percentage
  lm_ms               (c) this commit with a synthetic order-4 LM at alpha 0.3: every unigram, every n-gram of what the plain search
                      emits on this batch and random higher-order n-grams around those labels up to about 100k
  lm_hotwords_ms      (d) (c) plus a graph of 1000 random phrases (score 1.5) on every utterance
(c) and (d) are records, not pass/fail lines; the terms change what the search keeps (`labels`, `pops`), so their times are NOT the
cost of the walks alone.  The worker passes no new keyword for the plain search, so it also runs on the parent.
Every tree runs in a process of its own (one worker per tree and round, the rounds alternating between the trees; inside the worker of
this tree the variants alternate), so neither tree's runs all come before or after the other's.  With $RS_BEAM_TRACE=1 the step
kernel prints its phase split per call (stderr), which shows whether the per-pop state reads landed in the pop loop."""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALPHA, BEAM = 0.3, 20


def synthetic_lm(n_logits, blank, seqs, n_high, order=4, seed=1):
    """{(ids...): (log10 p, log10 backoff)}: every unigram, `<s>`, every n-gram of `seqs`, and random n-grams around their labels"""
    import numpy as np
    from reazonspeech_amd.runtime.ngram_lm import BOS
    rng = np.random.default_rng(seed)
    vocab = np.asarray([t for t in range(n_logits) if t != blank])
    ent = {(int(t),): (-float(rng.integers(8, 40)) / 8.0, -float(rng.integers(0, 8)) / 8.0) for t in vocab}
    ent[(BOS,)] = (-99.0, -0.25)
    n0 = len(ent)
    for y in seqs:
        y = (BOS,) + tuple(int(t) for t in y)
        for k in range(len(y)):
            for m in range(2, min(order, len(y) - k) + 1):
                ent.setdefault(y[k:k + m], (-float(rng.integers(0, 8)) / 8.0, -float(rng.integers(0, 8)) / 8.0 if m < order else 0.0))
    seen = np.asarray(sorted({int(t) for y in seqs for t in y})) if any(len(y) for y in seqs) else vocab
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
    import reazonspeech_amd
    assert os.path.realpath(os.path.dirname(os.path.dirname(reazonspeech_amd.__file__))) == os.path.realpath(args.tree), reazonspeech_amd.__file__
    from reazonspeech_amd.runtime.config import ESPNET_CONFORMER_120M as cfg
    from reazonspeech_amd.runtime.weights_espnet import synthetic_state_dict_espnet
    from reazonspeech_amd.runtime.synth import synthetic_batch
    from reazonspeech_amd.espnet.asr.model import EspnetModel, synthetic_token_list
    am = EspnetModel(cfg, synthetic_state_dict_espnet(cfg, 0, blank_bias=16.0, dec_gain=8.0), synthetic_token_list(cfg.vocab_size, 0), device="cuda:0").am
    audio, lens = synthetic_batch(args.batch, args.seconds, seed=1234)
    waves = [np.pad(audio[i, :lens[i]], (16000, 8000)) for i in range(args.batch)]
    buf = am.stage(waves, buf=am.new_buffers(args.batch, len(waves[0])))
    am.run_device(buf)                                         # front end and encoder: the projection stays resident
    torch.cuda.synchronize()
    ctx, dev, B, Tp = am.ctx, am.device, buf.B, buf.tp_max
    stream = torch.cuda.current_stream().cuda_stream
    cap = 2 * Tp + 16
    out = dict(ids=torch.zeros((B, cap), dtype=torch.int32, device=dev), frames=torch.zeros((B, cap), dtype=torch.int32, device=dev),
               n_ids=torch.zeros((B,), dtype=torch.int32, device=dev), scores=torch.zeros((B,), dtype=torch.float32, device=dev),
               pops=torch.zeros((B,), dtype=torch.int32, device=dev))

    def search(ws, **tables):
        ctx.rnnt_beam(buf.joint_enc, buf.enc_lens, B, Tp, BEAM, True, args.max_pops, out["ids"], out["n_ids"], out["scores"], out["pops"], ws,
                      stream, frames=out["frames"], **tables)

    def digest():
        torch.cuda.synchronize()
        n = out["n_ids"].cpu().numpy()
        ids = [out["ids"].cpu().numpy()[b, :n[b]] for b in range(B)]
        h = hashlib.sha256()
        for t in [n, out["scores"].cpu().numpy(), out["pops"].cpu().numpy()] + ids + [out["frames"].cpu().numpy()[b, :n[b]] for b in range(B)]:
            h.update(np.ascontiguousarray(t).tobytes())
        return (h.hexdigest(), int(n.sum()), int(out["pops"].sum().item())), ids

    plain_ws = torch.empty((ctx.beam_workspace_bytes(B, BEAM, Tp, args.max_pops),), dtype=torch.uint8, device=dev)
    variants = {"plain": lambda: search(plain_ws)}
    variants["plain"]()
    digests, extra = {}, {}
    digests["plain"], plain_ids = digest()
    if args.worker == "this":
        from reazonspeech_amd.runtime import k2_hotwords, ngram_lm
        from reazonspeech_amd.runtime.model import _HotwordSet, _NgramSet
        lm = ngram_lm.build(synthetic_lm(cfg.n_logits, cfg.blank_id, [y.tolist() for y in plain_ids], args.ngrams), cfg.n_logits, cfg.blank_id)
        extra = dict(lm_nodes=lm.n_nodes, lm_children=lm.n_children, lm_order=lm.order)
        rng = np.random.default_rng(1)
        graph = k2_hotwords.build_graph([(tuple(int(t) for t in rng.integers(2, cfg.vocab_size - 1, size=int(rng.integers(2, 7)))), 1.5) for _ in range(1000)])
        ns, hw = _NgramSet(lm, dev), _HotwordSet([graph], dev)
        graph_of = torch.zeros((B,), dtype=torch.int32, device=dev)
        fused_ws = torch.empty((ctx.beam_workspace_bytes(B, BEAM, Tp, args.max_pops, hotwords=True, lm=True),), dtype=torch.uint8, device=dev)
        variants["lm"] = lambda: search(fused_ws, lm=ns.struct, lm_alpha=ALPHA)
        variants["lm_hotwords"] = lambda: search(fused_ws, lm=ns.struct, lm_alpha=ALPHA, hotwords=hw.struct, graph_of=graph_of)
        for name in ("lm", "lm_hotwords"):
            variants[name]()
            digests[name], _ = digest()
    times = {name: [] for name in variants}
    for i in range(args.warmup + args.repeats):
        for name, run in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run()                                              # synchronises the stream itself
            torch.cuda.synchronize()
            if i >= args.warmup:
                times[name].append((time.perf_counter() - t0) * 1e3)
    print("RESULT " + json.dumps({name: dict(times_ms=times[name], sha256=digests[name][0], labels=digests[name][1], pops=digests[name][2],
                                             enc_frames=int(Tp), **extra) for name in variants}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--max-pops", type=int, default=640)
    ap.add_argument("--ngrams", type=int, default=100000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "espnet_beam_lm_ab.json"))
    ap.add_argument("--worker", choices=("parent", "this"))
    ap.add_argument("--tree", default=ROOT)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    if not args.parent_tree:
        raise SystemExit("--parent-tree DIR: a built checkout of the parent commit")
    assert args.rounds * args.repeats >= 20, "at least 20 timed runs per variant"
    runs = {"parent_plain": [], "plain": [], "lm": [], "lm_hotwords": []}
    meta, parent_medians = {}, []
    for r in range(args.rounds):
        for role, tree in (("parent", os.path.abspath(args.parent_tree)), ("this", ROOT)):
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", role, "--tree", tree, "--repeats", str(args.repeats), "--warmup", str(args.warmup),
                   "--batch", str(args.batch), "--seconds", str(args.seconds), "--max-pops", str(args.max_pops), "--ngrams", str(args.ngrams)]
            out = subprocess.run(cmd, check=True, capture_output=True, text=True, cwd=tree, timeout=900).stdout
            res = json.loads(next(line for line in out.splitlines() if line.startswith("RESULT "))[7:])
            for name, v in res.items():
                key = "parent_plain" if role == "parent" else name
                runs[key] += v["times_ms"]
                meta.setdefault(key, v)
                assert (meta[key]["sha256"], meta[key]["labels"]) == (v["sha256"], v["labels"]), "results changed between rounds"
            if role == "parent":
                parent_medians.append(statistics.median(res["plain"]["times_ms"]))
            print(f"round {r} {role}: " + ", ".join(f"{k} {statistics.median(v['times_ms']):.2f} ms" for k, v in res.items()), flush=True)
    med = {k: statistics.median(v) for k, v in runs.items()}
    result = {
        "setup": f"120M synthetic, {args.batch} x {args.seconds:g} s + (16000, 8000) padding, beam {BEAM}, max_pops {args.max_pops}, the search alone on the "
                 f"resident projection; median of {args.rounds} x {args.repeats} timed runs after {args.warmup} warm-ups per process",
        "enc_frames": meta["plain"]["enc_frames"],
        "parent_plain_ms": round(med["parent_plain"], 3), "plain_ms": round(med["plain"], 3), "lm_ms": round(med["lm"], 3),
        "lm_hotwords_ms": round(med["lm_hotwords"], 3),
        "plain_over_parent": round(med["plain"] / med["parent_plain"], 4),
        "parent_spread": round((max(parent_medians) - min(parent_medians)) / med["parent_plain"], 4),
        "parent_min_max_ms": [round(min(runs["parent_plain"]), 3), round(max(runs["parent_plain"]), 3)],
        "plain_same_results": meta["plain"]["sha256"] == meta["parent_plain"]["sha256"],
        "lm": {k: meta["lm"][k] for k in ("lm_nodes", "lm_children", "lm_order")}, "lm_alpha": ALPHA, "hotwords_phrases": 1000,
        "lm_changes_results": meta["lm"]["sha256"] != meta["plain"]["sha256"],
        "labels": {k: meta[k]["labels"] for k in meta}, "pops": {k: meta[k]["pops"] for k in meta},
        "min_max_ms": {k: [round(min(v), 3), round(max(v), 3)] for k, v in runs.items()},
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fp:
        json.dump(result, fp, indent=1)
        fp.write("\n")
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
