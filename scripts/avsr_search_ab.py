"""generate() with the search on the host (generation.py) against the search on the device (csrc/k_avsr_search.hip), one process,
AVSR_BASE, 16 clips x 250 frames: num_beams 5 at max_new_tokens 32 and 256, num_beams 1 at 256.  The two are alternated after a
warm-up; the encoder alone is timed too, so that the per-token figure is (call - encoder) / tokens.

    python scripts/avsr_search_ab.py [reps] > profiles/<name>.txt"""
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.getcwd())
from reazonspeech_amd.avsr import AVHubertForConditionalGeneration          # noqa: E402
from reazonspeech_amd.runtime.avsr_config import AVSR_BASE                  # noqa: E402
from reazonspeech_amd.runtime.avsr_synth import synthetic_clips             # noqa: E402
from reazonspeech_amd.runtime.avsr_weights import synthetic_state_dict_avsr  # noqa: E402


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    B, T = 16, 250
    sd = synthetic_state_dict_avsr(AVSR_BASE, 0)
    models = {s: AVHubertForConditionalGeneration(AVSR_BASE, sd, device="cuda:0", search=s) for s in ("host", "device")}
    a, v, mask, _ = synthetic_clips(B, T, seed=1, ragged=True, min_frames=T // 3)
    kw = dict(input_values=a, pixel_values=v, padding_mask=mask)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    enc_ms = {}
    for s, m in models.items():
        timed(lambda: m.avhubert(**kw))
        enc_ms[s] = statistics.median(timed(lambda: m.avhubert(**kw))[0] for _ in range(reps))
    print(f"# AVSR_BASE, {B} clips x {T} frames (ragged), {reps} alternated repetitions after one warm-up call each; {torch.cuda.get_device_name(0)}")
    print(f"# encoder alone: median {enc_ms['host']:.1f} ms (host model) {enc_ms['device']:.1f} ms (device model)")
    print(f"{'beams':>5} {'new_tokens':>10} {'search':>7} {'call_ms':>9} {'min_ms':>9} {'tokens':>7} {'ms_per_token':>13}")
    for beams, n_new in ((5, 32), (5, 256), (1, 256)):
        ts, outs = {"host": [], "device": []}, {}
        for s, m in models.items():
            timed(lambda: m.generate(**kw, num_beams=beams, max_new_tokens=n_new))
        for _ in range(reps):
            for s, m in models.items():
                ms, outs[s] = timed(lambda: m.generate(**kw, num_beams=beams, max_new_tokens=n_new))
                ts[s].append(ms)
        same = bool(torch.equal(outs["host"], outs["device"]))
        for s in ("host", "device"):
            med, tokens = statistics.median(ts[s]), outs[s].shape[1] - 1
            print(f"{beams:>5} {n_new:>10} {s:>7} {med:>9.1f} {min(ts[s]):>9.1f} {tokens:>7} {(med - enc_ms[s]) / tokens:>13.3f}")
        print(f"#   ids equal: {same}; device / host call time {statistics.median(ts['device']) / statistics.median(ts['host']):.3f}")


if __name__ == "__main__":
    main()
