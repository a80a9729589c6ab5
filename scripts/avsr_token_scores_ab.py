"""What recording the per-token scores costs generate(search="device"): the bench's avsr configuration (AVSR_BASE, 16 clips x 250 frames,
num_beams=5, 32 new tokens), three variants, written to profiles/avsr_token_scores_ab.json.

    python scripts/avsr_token_scores_ab.py ab --parent-tree DIR [--rounds 2] [--calls 12]

  parent        the parent commit: a checkout of it at DIR with its library built (git worktree add DIR HEAD~1; python -m
                reazonspeech_amd.build there); generate(**inputs, num_beams=5, max_new_tokens=32)
  off           this tree, the same call: nothing is recorded, rs_avsr_generate_opts runs
  on            this tree, return_dict_in_generate=True: rs_avsr_generate_scored, no dump
  on_dump       ... and output_scores=True: with the step_scores dump and the `scores` tuple

Every variant is timed in processes of its own (the two trees cannot share one), `rounds` processes per tree, alternating between
the trees; each process warms every variant it has up with two calls and then times `calls` calls per variant, alternating between
them, each ended by a device synchronise.  Reported per variant: the median and the extremes over all rounds x calls timed calls, the
ratio to `parent`, and whether the ids equal the parent's.  `parent` and `off` run the same kernels: their ratio shows the
run-to-run spread the other two ratios have to be read against.

    python scripts/avsr_token_scores_ab.py measure TREE calls     # one process: JSON on the last line of stdout
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
B, T, BEAMS, NEW_TOKENS = 16, 250, 5, 32
VARIANTS = {"off": {}, "on": dict(return_dict_in_generate=True), "on_dump": dict(return_dict_in_generate=True, output_scores=True)}
PARENT = {"parent": {}}


def measure(tree, calls):
    tree = os.path.abspath(tree)
    sys.path.insert(0, tree)
    import numpy as np
    import torch
    import reazonspeech_amd
    assert os.path.dirname(os.path.dirname(os.path.abspath(reazonspeech_amd.__file__))) == tree, "the package was imported from another tree"
    from reazonspeech_amd.avsr import synthetic_model
    from reazonspeech_amd.runtime.avsr_config import AVSR_BASE
    from reazonspeech_amd.runtime.avsr_synth import synthetic_clips
    m = synthetic_model(AVSR_BASE, 0, device="cuda:0", search="device")
    a, v, mask, _ = synthetic_clips(B, T, seed=4242)
    kw = dict(input_values=torch.from_numpy(a).to(m.device), pixel_values=torch.from_numpy(v[:, :, 0]).to(m.device), padding_mask=torch.from_numpy(mask).to(m.device),
              num_beams=BEAMS, max_new_tokens=NEW_TOKENS)
    variants = VARIANTS if hasattr(m, "compute_transition_scores") else PARENT

    def call(opts):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = m.generate(**kw, **opts)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    ms, ids = {k: [] for k in variants}, {}
    for k, o in variants.items():
        call(o), call(o)
    for _ in range(calls):
        for k, o in variants.items():
            t, out = call(o)
            ms[k].append(t)
            seq = out.sequences if hasattr(out, "sequences") else out
            ids[k] = hashlib.sha256(np.ascontiguousarray(seq.numpy().astype(np.int64)).tobytes()).hexdigest()
    print(json.dumps({"ms": ms, "ids_sha256": ids, "device": torch.cuda.get_device_name(0)}))


def ab(parent_tree, rounds, calls, out_path):
    ms, ids, device = {}, {}, None
    for _ in range(rounds):
        for tree in (parent_tree, ROOT):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "measure", tree, str(calls)], capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                raise SystemExit(f"measuring {tree} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
            got = json.loads(r.stdout.strip().splitlines()[-1])
            device = got["device"]
            for k, t in got["ms"].items():
                ms.setdefault(k, []).extend(t)
                assert ids.setdefault(k, got["ids_sha256"][k]) == got["ids_sha256"][k], f"{k}: ids differ between two processes"
    base = statistics.median(ms["parent"])
    res = {"workload": f"AVSR_BASE, {B} clips x {T} frames, generate(num_beams={BEAMS}, max_new_tokens={NEW_TOKENS}, search='device'), encoder included",
           "device": device, "timed_calls_per_variant": rounds * calls, "method": "median of wall-clock ms per call ended by a device synchronise; "
           f"{rounds} processes per tree alternating between the trees, variants alternating inside a process, two warm-up calls each",
           "variants": {}}
    for k in ("parent", "off", "on", "on_dump"):
        res["variants"][k] = {"median_ms": round(statistics.median(ms[k]), 3), "min_ms": round(min(ms[k]), 3), "max_ms": round(max(ms[k]), 3),
                              "ratio_to_parent": round(statistics.median(ms[k]) / base, 4), "ids_equal_parent": ids[k] == ids["parent"]}
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res, indent=1))
    if not all(v["ids_equal_parent"] for v in res["variants"].values()):
        raise SystemExit("ids differ from the parent's")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="mode", required=True)
    p = sub.add_parser("ab")
    p.add_argument("--parent-tree", required=True)
    p.add_argument("--rounds", type=int, default=2)
    p.add_argument("--calls", type=int, default=12)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "avsr_token_scores_ab.json"))
    p = sub.add_parser("measure")
    p.add_argument("tree")
    p.add_argument("calls", type=int)
    args = ap.parse_args()
    if args.mode == "ab":
        ab(args.parent_tree, args.rounds, args.calls, args.out)
    else:
        measure(args.tree, args.calls)
