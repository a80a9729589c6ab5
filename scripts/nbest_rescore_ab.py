"""What n-best rescoring by full likelihood (`AsrModel.rescore`, rs_rnnt_align_rows) costs, how much of the lattice the entries of a
synthetic n-best list share, and that the paths without it did not move: synthetic weights, the bench batch (256 x 10 s, seed 4242),
every family with its beam search (nemo ALSD beam 4; espnet default beam search, beam 20, max_pops 640, blank bias 16, dec_gain 8;
k2 modified beam search, 4 paths).

    python scripts/nbest_rescore_ab.py --parent-tree DIR [--configs nemo,espnet,k2] [--repeats 10] [--out profiles/nbest_rescore_ab.json]

DIR is a checkout of the parent commit with its library built (it runs under its own tree's Python, one process per run, like
scripts/align_ab.py).  Per family three worker processes run one after the other — parent, this tree, parent again — and each times
  transcribe_ms   `transcribe_waveforms(waves)`                     ids, frames and scores must be identical (sha256)
  nbest4_ms       `transcribe_waveforms(waves, nbest=4)`            the lists must be identical
  align_ms        `align_waveforms(waves, the search's ids)`        frames and the bits of the likelihoods must be identical
as medians of `--repeats` calls after `--warmup`; the medians are compared with the +-3 % the project sees between runs.
In this tree's worker, after that, with `rescore = "likelihood"` and nbest = 4:
  rescore_ms      `transcribe_waveforms(waves, nbest=4)` with the rescoring step on, against nbest4_ms of the same process
  stats           the call's (lattice rows computed, lattice rows there are without sharing), and the lists' lengths
  brackets        one profiled rs_rnnt_align_rows call on the resident lists with sharing and one with RS_ALIGN_NO_SHARING
                  (rs_profile_read_launches, decode class): the plan, the prediction chain (LSTM families), the lattice, the DP;
                  and that both give the same bits
Nothing is fixed in advance: what is measured is written down, also where sharing does not pay.
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


def make_model(name):
    import numpy as np
    from reazonspeech_amd.runtime.synth import synthetic_batch
    if name == "nemo":
        from reazonspeech_amd.runtime.config import FASTCONFORMER_619M
        from reazonspeech_amd.runtime.model import AsrModel
        from reazonspeech_amd.runtime.tokenizer import SyntheticTokenizer
        from reazonspeech_amd.runtime.weights import synthetic_state_dict
        cfg = FASTCONFORMER_619M.with_(decoding="alsd", beam_size=4)
        am, pad, seed = AsrModel(cfg, synthetic_state_dict(cfg, 0), SyntheticTokenizer(cfg.vocab_size, 0), device="cuda:0"), 0, 4242
    elif name == "espnet":
        from reazonspeech_amd.runtime.config import ESPNET_CONFORMER_120M as cfg
        from reazonspeech_amd.runtime.weights_espnet import synthetic_state_dict_espnet
        from reazonspeech_amd.espnet.asr.model import EspnetModel, synthetic_token_list
        am = EspnetModel(cfg, synthetic_state_dict_espnet(cfg, 0, blank_bias=16.0, dec_gain=8.0), synthetic_token_list(cfg.vocab_size, 0),
                         device="cuda:0", beam_size=20, max_pops=640).am
        pad, seed = (16000, 8000), 1234
    else:
        from reazonspeech_amd.runtime.k2_config import ZIPFORMER_159M as cfg
        from reazonspeech_amd.runtime.k2_weights import synthetic_state_dict_k2
        from reazonspeech_amd.k2.asr.model import K2Model, synthetic_tokens
        am = K2Model(cfg, synthetic_state_dict_k2(cfg, 0), synthetic_tokens(cfg.vocab_size, 0), device="cuda:0",
                     decoding_method="modified_beam_search", max_active_paths=4).am
        pad, seed = int(0.9 * 16000), 4242
    return am, pad, seed, np, synthetic_batch


def bits(values):
    import struct
    return [struct.pack("<f", v).hex() for v in values]


def timed(fn, warmup, repeats):
    import torch
    times = []
    for i in range(warmup + repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= warmup:
            times.append((time.perf_counter() - t0) * 1e3)
    return times


def worker(args):
    sys.path.insert(0, args.tree)
    import torch
    import reazonspeech_amd
    assert os.path.realpath(os.path.dirname(os.path.dirname(reazonspeech_amd.__file__))) == os.path.realpath(args.tree), reazonspeech_amd.__file__
    am, pad, seed, np, synthetic_batch = make_model(args.config)
    audio, lens = synthetic_batch(args.batch, args.seconds, seed=seed)
    waves = [np.pad(audio[i, :lens[i]], pad) for i in range(args.batch)]
    sha = lambda obj: hashlib.sha256(json.dumps(obj).encode()).hexdigest()      # noqa: E731
    one = None if args.config != "espnet" else False
    res = am.transcribe_waveforms(waves)
    lists = am.transcribe_waveforms(waves, nbest=4)
    al = am.align_waveforms(waves, res.ids, one_per_frame=one)
    out = {"tokens": sum(len(x) for x in res.ids),
           "sha_transcribe": sha([res.ids, res.frames, bits(res.scores)]),
           "sha_nbest4": sha([[(y, fr, bits([s, n])) for y, fr, s, n in rows] for rows in lists.nbest]),
           "sha_align": sha([al.frames, bits(al.log_likelihood), bits(al.alignment_log_prob), [bits(x) for x in al.token_logprobs]]),
           "transcribe_ms": timed(lambda: am.transcribe_waveforms(waves), args.warmup, args.repeats),
           "nbest4_ms": timed(lambda: am.transcribe_waveforms(waves, nbest=4), args.warmup, args.repeats),
           "align_ms": timed(lambda: am.align_waveforms(waves, res.ids, one_per_frame=one), 1, args.align_repeats)}
    if args.worker == "this":
        am.nbest, am.rescore = 4, "likelihood"
        scored = am.transcribe_waveforms(waves)
        assert [[r[:2] for r in rows] for rows in scored.nbest] == [[r[:2] for r in rows] for rows in lists.nbest]
        r = {"rescore_ms": timed(lambda: am.transcribe_waveforms(waves), args.warmup, args.repeats),
             "list_lengths": {str(k): sum(len(rows) == k for rows in scored.nbest) for k in range(5)},
             "lists_whose_best_changes": sum(max(range(len(rows)), key=lambda k: (rows[k][0], -k)) != 0 for rows in scored.rescored if rows)}
        buf = am.stage(waves)
        am.run_device(buf)
        torch.cuda.synchronize()
        rb, nb = buf.rescore_bufs, buf.nbest_bufs
        B, n, u_cap = buf.B, buf.nbest_n, nb["ids"].shape[2]
        r["stats"] = {"rows_computed": rb["stats"][0], "rows_without_sharing": rb["stats"][1],
                      "computed_percent": round(100.0 * rb["stats"][0] / max(rb["stats"][1], 1), 2)}
        stream = torch.cuda.current_stream().cuda_stream
        topo = bool(am.cfg.max_symbols == 1 and am.cfg.decoding == "modified_beam_search")
        got = {}
        for share in (True, False):
            outs = [torch.zeros_like(rb[k]) for k in ("loglik", "best", "frames", "logp")]
            call = lambda: am.ctx.rnnt_align_rows(buf.joint_enc, buf.enc_lens, B, buf.tp_max, rb["row_utt"], nb["ids"].view(B * n, u_cap),      # noqa: E731
                                                  nb["n_ids"].view(B * n), *outs, rb["ws"], stream, one_per_frame=topo, share=share)
            call()
            ms = timed(call, 1, args.align_repeats)
            am.ctx.profile_enable(8)
            am.ctx.profile_reset()
            stats = call()
            torch.cuda.synchronize()
            recs = am.ctx.profile_launches(8)
            am.ctx.profile_enable(0)
            names = ["plan", "lattice", "dp"] if len(recs) == 3 else ["plan", "prediction_chain", "lattice", "dp"]
            assert len(recs) == len(names), recs
            key = "sharing" if share else "no_sharing"
            r[key] = {"call_ms": round(statistics.median(ms), 3), "brackets_ms": {k: round(x[5], 3) for k, x in zip(names, recs)}, "stats": list(stats)}
            live = (rb["row_utt"] >= 0).cpu().numpy()
            got[share] = [o.cpu().numpy()[live].tobytes() for o in outs[:2]]
        r["same_bits_with_and_without_sharing"] = got[True] == got[False]
        out["rescore"] = r
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree")
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--align-repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nbest_rescore_ab.json"))
    ap.add_argument("--worker", choices=("parent", "this"))
    ap.add_argument("--config", choices=CONFIGS)
    ap.add_argument("--tree", default=ROOT)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    if not args.parent_tree:
        raise SystemExit("--parent-tree DIR: a built checkout of the parent commit")
    med = statistics.median
    result = {"setup": f"synthetic weights, {args.batch} x {args.seconds:g} s; medians of {args.repeats} timed runs after {args.warmup} warm-ups per "
                       f"process (parent, this tree, parent again), align and the bracket calls: median of {args.align_repeats}; nemo ALSD beam 4, "
                       "espnet beam 20 / max_pops 640, k2 modified beam search 4 paths; lists of nbest = 4"}
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
        entry = {"tokens": got["this"]["tokens"]}
        for what in ("transcribe", "nbest4", "align"):
            pa, pb, th = (med(got[k][what + "_ms"]) for k in ("parent_a", "parent_b", "this"))
            parent = 0.5 * (pa + pb)
            entry[what] = {"identical": got["parent_a"]["sha_" + what] == got["this"]["sha_" + what] == got["parent_b"]["sha_" + what],
                           "parent_ms": [round(pa, 3), round(pb, 3)], "this_ms": round(th, 3),
                           "this_vs_parent_percent": round(100.0 * (th - parent) / parent, 2), "within_3_percent": abs(th - parent) <= 0.03 * parent}
        r = got["this"]["rescore"]
        r["rescore_ms"] = round(med(r["rescore_ms"]), 3)
        r["rescore_minus_nbest4_ms"] = round(r["rescore_ms"] - entry["nbest4"]["this_ms"], 3)
        entry["rescore"] = r
        result[config] = entry
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fp:
            json.dump(result, fp, indent=1)
            fp.write("\n")
        print(config, json.dumps(entry), flush=True)


if __name__ == "__main__":
    main()
