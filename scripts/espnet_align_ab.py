"""`transcribe_batch` WITH segments, `segmentation="host"` against `"device"`, one process: the 120M synthetic ESPnet model and
the benchmark's batch of 256 x 10 s synthetic utterances.  After one warm-up call per mode the two are alternated; each call is
synchronised and the median is reported.  One more `align_batch` call runs under the per-class HIP-event profile: the align
kernel is the only launch of the decode class in it, the second encoder pass is everything else.

    python scripts/espnet_align_ab.py [--batch=256] [--reps=5] > profiles/espnet_align_ab.json      (one JSON line)
"""
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from reazonspeech_amd.runtime import capi                                    # noqa: E402
from reazonspeech_amd.runtime.config import ESPNET_CONFORMER_120M            # noqa: E402
from reazonspeech_amd.runtime.synth import synthetic_batch                   # noqa: E402
from reazonspeech_amd.runtime.weights_espnet import synthetic_state_dict_espnet  # noqa: E402
from reazonspeech_amd.espnet.asr.model import EspnetModel, synthetic_token_list   # noqa: E402
from reazonspeech_amd.espnet.asr import interface                            # noqa: E402
from reazonspeech_amd.espnet.asr.transcribe import transcribe_batch          # noqa: E402


def arg(name, default):
    return ([int(a.split("=")[1]) for a in sys.argv[1:] if a.startswith(f"--{name}=")] or [default])[0]


def main():
    B, reps = arg("batch", 256), max(arg("reps", 5), 5)
    cfg = ESPNET_CONFORMER_120M
    model = EspnetModel(cfg, synthetic_state_dict_espnet(cfg, 0), synthetic_token_list(cfg.vocab_size, 0), device="cuda:0")
    audio, lens = synthetic_batch(B, 10.0, seed=1234)
    waves = [audio[b, :int(lens[b])] for b in range(B)]
    audios = [interface.AudioData(w, 16000) for w in waves]
    seconds = float(lens.sum()) / 16000.0

    def timed(mode):
        model.segmentation = mode
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = transcribe_batch(model, audios)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    times, outs = {"host": [], "device": []}, {}
    for mode in times:
        timed(mode)                                              # warm-up: buffers, first launches
    for _ in range(reps):
        for mode in times:
            ms, outs[mode] = timed(mode)
            times[mode].append(ms)
    model.segmentation = "host"
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    texts = model.recognize_batch(waves)
    torch.cuda.synchronize()
    recognise_ms = (time.perf_counter() - t0) * 1e3

    classes = {"gemm": capi.PROF_GEMM, "attention": capi.PROF_ATTN, "frontend": capi.PROF_FRONTEND, "decode": capi.PROF_DECODE,
               "elementwise": capi.PROF_ELEMENTWISE, "subsample": capi.PROF_SUBSAMPLE}
    ctx = model.am.ctx
    ctx.profile_reset()
    ctx.profile_enable(sum(classes.values()))
    timings = model.align_batch(waves, texts)
    torch.cuda.synchronize()
    prof = {k: ctx.profile_read(v)["ms"] for k, v in classes.items()}
    ctx.profile_enable(0)

    med = {m: statistics.median(t) for m, t in times.items()}
    print(json.dumps({
        "workload": f"espnet 120M synthetic, transcribe_batch with segments, {B} x 10 s (seed 1234), greedy search",
        "device": torch.cuda.get_device_name(0), "reps": reps, "audio_seconds": seconds,
        "host_ms": round(med["host"], 2), "device_ms": round(med["device"], 2),
        "host_ms_all": [round(t, 1) for t in times["host"]], "device_ms_all": [round(t, 2) for t in times["device"]],
        "speedup": round(med["host"] / med["device"], 2),
        "rtfx_host": round(seconds / (med["host"] / 1e3), 1), "rtfx_device": round(seconds / (med["device"] / 1e3), 1),
        "recognise_only_ms": round(recognise_ms, 2),
        "align_kernel_ms": round(prof["decode"], 3),
        "second_encoder_pass_ms": round(sum(v for k, v in prof.items() if k != "decode"), 3),
        "second_encoder_pass_by_class_ms": {k: round(v, 3) for k, v in prof.items() if k != "decode"},
        "results_equal": outs["host"] == outs["device"],
        "aligned_utterances": sum(t is not None for t in timings),
        "aligned_characters": sum(len(t) for t in timings if t is not None),
    }))


if __name__ == "__main__":
    main()
