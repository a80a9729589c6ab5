"""The decoding methods of reazonspeech.k2.asr side by side: sherpa-onnx's greedy_search and modified_beam_search on the 159M
Zipformer (synthetic weights), the benchmark batch (256 x 10 s + 0.9 s of padding, seed 4242) staged once in HBM.

    python scripts/k2_decode_methods.py [--methods greedy,mbs4] [--repeats 20] [--steps 6] [--batch 256]

One JSON line per method:
  decode_ms        AsrModel.decode alone on the resident encoder projection (warm-up, then the median of --repeats runs)
  pipelined_ms     the whole step (front-end + encoder + decode) through run_pipelined with the schedule bench.k2_config uses
                   (max(1 + dec_streams, 3) resident batches, 2 decode lanes), per batch;  rtfx = audio seconds / that
For "mbsK" also the arithmetic floor of the search, decode_ms as a multiple of it and of nothing else measured here:
  floor_ms = frames x (2 B K J V flop at --f32-tflops, the exact-f32 MFMA rate the joint tiles reach) + logits traffic
             (write + read of B K V floats per frame at --hbm-tbs)
"greedy" passes no new keyword, so the script also runs on a checkout that predates the beam search."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from reazonspeech_amd.runtime.k2_config import ZIPFORMER_159M                 # noqa: E402
from reazonspeech_amd.runtime.k2_weights import synthetic_state_dict_k2       # noqa: E402
from reazonspeech_amd.runtime.synth import synthetic_batch                    # noqa: E402
from reazonspeech_amd.k2.asr.model import K2Model, synthetic_tokens           # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--methods", default="greedy,mbs4")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--dec-streams", type=int, default=2)
    ap.add_argument("--f32-tflops", type=float, default=0.0, help="exact-f32 MFMA rate of the joint tiles for the floor (0: no floor)")
    ap.add_argument("--hbm-tbs", type=float, default=4.0, help="HBM rate for the floor's logits traffic, TB/s")
    args = ap.parse_args()
    cfg = ZIPFORMER_159M
    sd = synthetic_state_dict_k2(cfg, 0)
    pad = int(0.9 * 16000)
    n_sets = max(1 + args.dec_streams, 3)
    batches, secs = [], []
    for k in range(n_sets):
        audio, lens = synthetic_batch(args.batch, args.seconds, seed=4242 + 1000 * k)
        batches.append([np.pad(audio[i, :lens[i]], pad) for i in range(args.batch)])
        secs.append(float(lens.sum()) / 16000.0)
    for method in args.methods.split(","):
        kw = {}
        if method.startswith("mbs"):
            kw = dict(decoding_method="modified_beam_search", max_active_paths=int(method[3:] or 4))
        elif method != "greedy":
            raise SystemExit(f"unknown method {method!r}: greedy or mbsK")
        km = K2Model(cfg, sd, synthetic_tokens(cfg.vocab_size, 0), device="cuda:0", **kw)
        am = km.am
        bufs = [am.stage(w, buf=am.new_buffers(args.batch, len(w[0]))) for w in batches]
        buf = bufs[0]
        am.run_device(buf)                                    # projection of batch 0 resident; also the decode's warm-up
        torch.cuda.synchronize()
        stream = torch.cuda.current_stream().cuda_stream
        times = []
        for i in range(args.warmup + args.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            am.decode(am.ctx, buf, buf.ws, stream)            # synchronises the stream itself
            torch.cuda.synchronize()
            if i >= args.warmup:
                times.append((time.perf_counter() - t0) * 1e3)
        n_tok = float(buf.n_ids.float().mean())
        am.run_pipelined(bufs, args.warmup, dec_streams=args.dec_streams)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        am.run_pipelined(bufs, args.steps, dec_streams=args.dec_streams)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        out = {"method": method, "batch": args.batch, "enc_frames": int(buf.tp_max), "mean_tokens_per_utt": round(n_tok, 1),
               "decode_ms": round(statistics.median(times), 2), "decode_ms_min": round(min(times), 2), "decode_ms_max": round(max(times), 2),
               "pipelined_ms": round(dt / args.steps * 1e3, 2),
               "rtfx": round(sum(secs[i % n_sets] for i in range(args.steps)) / dt, 1)}
        if kw and args.f32_tflops > 0:
            K = kw["max_active_paths"]
            flop = 2.0 * args.batch * K * cfg.joiner_dim * cfg.vocab_size * buf.tp_max
            traffic = 2.0 * 4.0 * args.batch * K * cfg.vocab_size * buf.tp_max
            floor = flop / (args.f32_tflops * 1e12) * 1e3 + traffic / (args.hbm_tbs * 1e12) * 1e3
            out.update(floor_ms=round(floor, 2), joint_tflop=round(flop / 1e12, 2), logits_gb=round(traffic / 1e9, 1),
                       decode_over_floor=round(out["decode_ms"] / floor, 2))
        print(json.dumps(out), flush=True)
        del bufs, buf, km, am
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
