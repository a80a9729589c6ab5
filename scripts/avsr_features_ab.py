"""`AVHubertFeatureExtractor(features="host")` against `features="device"` next to the model's own times, one process:
`configs.avsr_b16` — the 161M synthetic AV-HuBERT, 16 clips x 10 s of synthetic raw input (160 000 samples of noise at 16 kHz and
250 uint8 mouth crops of 96 x 96 at 25 fps per clip).

Per path, after one warm-up call, alternating the two paths, medians of --reps calls (host clock around work that ends in a device
synchronise; the host extractor's calls take longer: --host-reps):
  extractor_ms   `processor(raw_audio=..., raw_video=...)`: host = numpy on the calling thread, the result on the host;
                 device = staging, upload and the two launches, the result on the device
  upload_ms      host: the three float32 numpy results to the device as `AvsrDevice._dev` does it (pageable memory);
                 device: the raw buffers (flat float32 samples, flat uint8 crops) through pinned memory — the part of extractor_ms
                 that is staging and copy — and, beside it, the two launches alone by HIP events on resident buffers (kernels_ms)
  encoder_ms     `model.avhubert(**inputs)` on that path's extractor output (numpy for host, device tensors for device)
  generate_ms    `model.generate(**inputs, num_beams=5, max_new_tokens=32)`, per search mode ("host", "device")
  end_to_end_ms  raw clips -> token ids on the host: extractor + generate in one timed call, per search mode
and once: whether both paths' `pixel_values` are equal, the largest difference of their `input_values`, and the bounded audio cases
of tests/test_gpu_avsr_features.py (device and float32-CPU error against the host path, maxima and rms).

    python scripts/avsr_features_ab.py [--reps=20] [--host-reps=5] > profiles/avsr_features_ab.json      (one JSON line)
"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))
from reazonspeech_amd.avsr import AVHubertFeatureExtractor, AVHubertProcessor, synthetic_model      # noqa: E402
from reazonspeech_amd.runtime import avsr_features as af                                           # noqa: E402
from reazonspeech_amd.runtime.avsr_config import AVSR_BASE                                         # noqa: E402

B, SECONDS, FPS, SIDE = 16, 10.0, 25, 96
BEAMS, NEW_TOKENS = 5, 32
DEV = "cuda:0"


def arg(name, default, kind=int):
    return ([kind(a.split("=")[1]) for a in sys.argv[1:] if a.startswith(f"--{name}=")] or [default])[0]


def spread(v):
    q = np.percentile(v, [25, 75])
    return {"median": statistics.median(v), "p25": float(q[0]), "p75": float(q[1]), "min": min(v), "max": max(v), "reps": len(v)}


def make_inputs():
    rng = np.random.default_rng(4242)
    audio = [(0.1 * rng.standard_normal(int(SECONDS * 16000))).astype(np.float32) for _ in range(B)]
    video = [rng.integers(0, 256, size=(int(SECONDS * FPS), SIDE, SIDE), dtype=np.uint8) for _ in range(B)]
    return audio, video


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def upload_host_result(model, feats):
    return [model.dev._dev(feats[k]) for k in ("input_values", "pixel_values", "padding_mask")]


def upload_raw(audio, video):
    dev = torch.device(DEV)
    return (af._pinned(torch, audio, torch.float32, np.float32).to(dev, non_blocking=True),
            af._pinned(torch, video, torch.uint8, np.uint8).to(dev, non_blocking=True))


def kernels_alone(audio, video, reps):
    """the two launches by HIP events on buffers that are already on the device"""
    fe = AVHubertFeatureExtractor()
    p = af.plan(fe, audio, video)
    dev = torch.device(DEV)
    a, v = upload_raw(p.audio, p.groups[0].frames)
    tw, fb_idx, fb_w = af.device_tables(dev)
    off, ln = torch.from_numpy(p.row_off).to(dev), torch.from_numpy(p.row_len).to(dev)
    idx, lut = torch.from_numpy(p.groups[0].frame_idx).to(dev), torch.from_numpy(p.lut).to(dev)
    iv = torch.empty((p.B, p.T_out, 104), device=dev)
    pv = torch.empty((p.B, p.T_out, p.crop, p.crop), device=dev)
    g = p.groups[0]
    stream = torch.cuda.current_stream(dev).cuda_stream
    ms = {"logfbank": [], "pixels": []}
    for r in range(reps + 1):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        af.logfbank(0, a, off, ln, p.B, p.T_out, p.stack, True, tw, fb_idx, fb_w, iv, stream)
        e[1].record()
        af.pixels(0, v, g.n_frames, g.H, g.W, g.channels, idx, p.T_out, p.B, p.T_out, p.crop, g.top, g.left, lut, pv, stream)
        e[2].record()
        torch.cuda.synchronize()
        if r:                                        # the first round loads the code objects
            ms["logfbank"].append(e[0].elapsed_time(e[1]))
            ms["pixels"].append(e[1].elapsed_time(e[2]))
    out_bytes = iv.numel() * 4 + pv.numel() * 4
    in_bytes = a.numel() * 4 + v.numel()
    return {"logfbank_ms": spread(ms["logfbank"]), "pixels_ms": spread(ms["pixels"]), "bytes_in": in_bytes, "bytes_out": out_bytes}


def main():
    reps, host_reps = arg("reps", 20), arg("host-reps", 5)
    audio, video = make_inputs()
    model = synthetic_model(AVSR_BASE, seed=0, device=DEV)
    procs = {"host": AVHubertProcessor(AVHubertFeatureExtractor(features="host")),
             "device": AVHubertProcessor(AVHubertFeatureExtractor(features="device", device=DEV))}
    n = {"host": host_reps, "device": reps}
    searches = ("host", "device")
    out = {"script": "scripts/avsr_features_ab.py", "gpu": torch.cuda.get_device_name(0), "config": "avsr_b16", "batch": B, "seconds": SECONDS,
           "frames": f"{int(SECONDS * FPS)} x {SIDE} x {SIDE} uint8", "num_beams": BEAMS, "max_new_tokens": NEW_TOKENS, "products": getattr(model.dev, "products", "exact"),
           "paths": {}}
    feats = {k: p(raw_audio=audio, raw_video=video) for k, p in procs.items()}           # warm-up of both extractors
    ms = {k: {"extractor_ms": [], "upload_ms": [], "encoder_ms": [], **{f"generate_ms[{s}]": [] for s in searches},
              **{f"end_to_end_ms[{s}]": [] for s in searches}} for k in procs}
    ids = {}
    for k in procs:                                                                      # warm-up of the model on both kinds of input
        model.avhubert(**feats[k])
        for s in searches:
            model.search = s
            ids[(k, s)] = model.generate(**feats[k], num_beams=BEAMS, max_new_tokens=NEW_TOKENS)
        upload_host_result(model, feats["host"]) if k == "host" else upload_raw(audio, video)
    for r in range(max(n.values())):
        for k, p in procs.items():
            if r >= n[k]:
                continue
            t, f = clock(lambda: p(raw_audio=audio, raw_video=video))
            ms[k]["extractor_ms"].append(t)
            ms[k]["upload_ms"].append(clock((lambda: upload_host_result(model, f)) if k == "host" else (lambda: upload_raw(audio, video)))[0])
            ms[k]["encoder_ms"].append(clock(lambda: model.avhubert(**f))[0])
            for s in searches:
                model.search = s
                ms[k][f"generate_ms[{s}]"].append(clock(lambda: model.generate(**f, num_beams=BEAMS, max_new_tokens=NEW_TOKENS))[0])
                ms[k][f"end_to_end_ms[{s}]"].append(clock(lambda: model.generate(**p(raw_audio=audio, raw_video=video), num_beams=BEAMS,
                                                                                 max_new_tokens=NEW_TOKENS))[0])
    for k in procs:
        out["paths"][k] = {name: spread(v) for name, v in ms[k].items()}
    out["paths"]["device"]["kernels_alone"] = kernels_alone(audio, video, reps)
    h, d = feats["host"], {k: v.cpu().numpy() for k, v in feats["device"].items()}
    out["same_results"] = {
        "pixel_values_equal": bool(np.array_equal(h["pixel_values"], d["pixel_values"])),
        "padding_mask_equal": bool(np.array_equal(h["padding_mask"], d["padding_mask"])),
        "input_values_max_abs_diff": float(np.abs(h["input_values"].astype(np.float64) - d["input_values"]).max()),
        "ids_equal": {s: bool(torch.equal(ids[("host", s)], ids[("device", s)])) for s in searches},
        "upload_bytes": {"host": int(sum(h[k].nbytes for k in h)), "device": int(sum(a.nbytes for a in audio) + sum(v.nbytes for v in video))}}
    import test_gpu_avsr_features as t                                                    # the bounded audio cases, as the test measures them
    out["audio_error_vs_host64"] = {}
    for length in t.BOUNDED_LENGTHS:
        dmax, drms, cmax, crms = t.bounded_case(length)
        out["audio_error_vs_host64"][str(length)] = {"device_max": dmax, "device_rms": drms, "cpu32_max": cmax, "cpu32_rms": crms,
                                                      "allowed_max": t.FACTOR * cmax}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
