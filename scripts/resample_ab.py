"""`load_model(resample="host")` against `resample="device"` on input that is not 16 kHz mono, one process: the 619M synthetic
NeMo model, 256 x 10 s, as 16 kHz mono (the control: neither option touches it), 48 kHz stereo and 44.1 kHz mono.

Per input and option, after one warm-up call: milliseconds per `transcribe_batch` (host clock around the call, which ends with the
results on the host), alternating the two options, median of --reps calls (the host option's calls on the resampled inputs take
seconds each: --host-reps sets their count; the control's calls take 0.1 s: --control-reps, 100 by default).  Per resampled input, in a run of its own and in the same repeat: the
rs_resample launch alone by HIP events, and the host-to-device copy of its input timed twice, from pageable memory (what
`resample_batch` does today) and from pinned memory (the fastest the copy can be: the harder comparison), medians of --reps; the
launch's FLOP/s and bytes/s from the counts the algorithm needs (two per tap and output after the channels were averaged; the input
read once and the output written once) against the larger of FLOPs / 157.3 TF/s and bytes / 6.29 TB/s; how many of the 256 rows
give the same token ids under both options (informational: the inputs differ at float32 rounding — and by the filter when soxr is
installed — and bf16-mode flips are near-ties); and the largest error of the device rows against the float64 closed form on 2048
random outputs, with its bound.

Two conditions are reported as met / not met: the launch is shorter than the host-to-device copy of its own input (the verdict
is taken against the PINNED copy; the pageable one is reported beside it, both with their GB/s), and — given
--parent=<the control's ms per transcribe_batch measured by this script on the parent commit, same box> — the control is within
3 % of it.  On a tree without the option (the parent commit) the script measures the control only.

    python scripts/resample_ab.py [--reps=20] [--host-reps=20] [--control-reps=100] [--parent=MS] > profiles/resample_ab.json      (one JSON line)
"""
import inspect
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from reazonspeech_amd.runtime.synth import synthetic_batch                   # noqa: E402
from reazonspeech_amd.nemo.asr import load_model, interface                  # noqa: E402
from reazonspeech_amd.nemo.asr.transcribe import transcribe_batch            # noqa: E402

B, SECONDS = 256, 10.0
QUIET = interface.TranscribeConfig(verbose=False)
PEAK_FLOPS, PEAK_BYTES = 157.3e12, 6.29e12          # float32 vector peak, measured HBM copy rate of one MI355X


def arg(name, default, kind=int):
    return ([kind(a.split("=")[1]) for a in sys.argv[1:] if a.startswith(f"--{name}=")] or [default])[0]


def make_inputs(rate, channels):
    audio, lens = synthetic_batch(B, SECONDS, seed=1234, samplerate=rate)
    rows = [audio[b, :lens[b]] for b in range(B)]
    if channels == 2:                                # a second microphone: the same speech a little later and quieter
        rows = [np.stack([r, np.float32(0.8) * np.roll(r, 7)]) for r in rows]
    return [interface.AudioData(r, rate) for r in rows]


def spread(v):
    q = np.percentile(v, [25, 75])
    return {"median": statistics.median(v), "p25": float(q[0]), "p75": float(q[1]), "min": min(v), "max": max(v), "reps": len(v)}


def timed(model, audios):
    t0 = time.perf_counter()
    res = transcribe_batch(model, audios, QUIET)
    return (time.perf_counter() - t0) * 1e3, [[s.token_id for s in r.subwords] for r in res]


def main():
    reps, host_reps, parent_ms = arg("reps", 20), arg("host-reps", 20), arg("parent", 0.0, float)
    control_reps = arg("control-reps", max(reps, 100))          # a control call is 0.1 s: 20 of them are too short a window for a 3 % verdict
    if "resample" in inspect.signature(load_model).parameters:
        models = {opt: load_model(device="cuda:0", synthetic=True, resample=opt) for opt in ("host", "device")}
    else:                                            # the parent commit: no such option
        models = {"host": load_model(device="cuda:0", synthetic=True)}
    out = {"script": "scripts/resample_ab.py", "gpu": torch.cuda.get_device_name(0), "batch": B, "seconds": SECONDS, "reps": reps,
           "host_reps": host_reps, "control_reps": control_reps, "options": list(models), "inputs": {}}
    cases = [("16k_mono_control", 16000, 1)] + ([("48k_stereo", 48000, 2), ("44k1_mono", 44100, 1)] if "device" in models else [])
    for name, rate, channels in cases:
        audios = make_inputs(rate, channels)
        n = {opt: (control_reps if rate == 16000 else reps if opt == "device" else host_reps) for opt in models}
        ms, ids = {opt: [] for opt in models}, {}
        for opt, m in models.items():                # warm-up: buffers, code objects, the plan and its table
            ids[opt] = timed(m, audios)[1]
        for k in range(max(n.values())):             # alternate the options
            for opt, m in models.items():
                if k < n[opt]:
                    ms[opt].append(timed(m, audios)[0])
                    if ms[opt][-1] > 5e3:
                        print(f"[resample_ab] {name} {opt} call {k}: {ms[opt][-1]:.0f} ms", file=sys.stderr, flush=True)
        row = {"rate": rate, "channels": channels,
               "transcribe_batch_ms": {opt: spread(v) for opt, v in ms.items()},
               "rtfx": {opt: B * SECONDS / (statistics.median(v) * 1e-3) for opt, v in ms.items()}}
        if "device" in models:
            row["rows_with_identical_ids"] = sum(a == b for a, b in zip(ids["host"], ids["device"]))
            row["speedup_host_over_device"] = row["transcribe_batch_ms"]["host"]["median"] / row["transcribe_batch_ms"]["device"]["median"]
        if rate != 16000 or channels != 1:
            row["rs_resample"] = launch_alone(models["device"], audios, rate, channels, reps)
        out["inputs"][name] = row
        print(f"[resample_ab] {name}: " + json.dumps(row["transcribe_batch_ms"]), file=sys.stderr, flush=True)
    control = out["inputs"]["16k_mono_control"]["transcribe_batch_ms"]
    out["conditions"] = {}
    if "device" in models:
        out["conditions"]["kernel_shorter_than_its_h2d"] = {
            k: {"verdict": "met" if v["rs_resample"]["kernel_ms"] < v["rs_resample"]["h2d_pinned_ms"] else "not met",
                "basis": "the host-to-device copy from PINNED memory", "kernel_ms": v["rs_resample"]["kernel_ms"],
                "h2d_pinned_ms": v["rs_resample"]["h2d_pinned_ms"], "h2d_pinned_gb_per_s": v["rs_resample"]["h2d_pinned_gb_per_s"],
                "h2d_pageable_ms": v["rs_resample"]["h2d_pageable_ms"], "h2d_pageable_gb_per_s": v["rs_resample"]["h2d_pageable_gb_per_s"]}
            for k, v in out["inputs"].items() if "rs_resample" in v}
    if parent_ms > 0:
        worst = max(abs(v["median"] / parent_ms - 1.0) for v in control.values())
        out["conditions"]["control_within_3_percent_of_parent"] = {"parent_ms": parent_ms, "worst_relative_difference": worst,
                                                                   "verdict": "met" if worst <= 0.03 else "not met"}
    else:
        out["conditions"]["control_within_3_percent_of_parent"] = "not measured: no --parent figure given"
    print(json.dumps(out))


def launch_alone(model, audios, rate, channels, reps):
    """the launch and the two copies of its input by HIP events, medians; the counts; the error against the closed form"""
    from reazonspeech_amd.runtime import resample as rs
    pl = rs.plan(rate)
    waves = [a.waveform for a in audios]
    host, offs, lens = rs.pack_rows(waves, channels)
    pinned = torch.from_numpy(host).pin_memory()
    n_outs = [rs.n_out(n, pl.up, pl.down) for n in lens]
    pitch = (max(n_outs) + 63) // 64 * 64
    dev = model.device
    kernel, pageable, pin = [], [], []
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream()
        x = torch.empty(host.shape, dtype=torch.float32, device=dev)
        row_off, row_len = torch.tensor(offs, dtype=torch.int64).to(dev), torch.tensor(lens, dtype=torch.int32).to(dev)
        out = torch.empty((len(waves), pitch), dtype=torch.float32, device=dev)
        out_lens = torch.empty((len(waves),), dtype=torch.int32, device=dev)
        table = model.resample_table(rate, pl)
        for _ in range(reps + 1):                    # the first repeat is the warm-up
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
            ev[0].record(stream)
            x.copy_(torch.from_numpy(host))
            ev[1].record(stream)
            torch.cuda.synchronize()
            ev[2].record(stream)
            x.copy_(pinned, non_blocking=True)
            ev[3].record(stream)
            ev[4].record(stream)
            model.ctx.resample(x, row_off, row_len, len(waves), channels, table, pl.up, pl.down, pl.numtaps, out, 0, out_lens,
                               stream.cuda_stream)
            ev[5].record(stream)
            torch.cuda.synchronize()
            pageable.append(ev[0].elapsed_time(ev[1]))
            pin.append(ev[2].elapsed_time(ev[3]))
            kernel.append(ev[4].elapsed_time(ev[5]))
        h_out = out.cpu().numpy()
        assert out_lens.cpu().tolist() == n_outs
    rows = [h_out[b, :n] for b, n in enumerate(n_outs)]
    kernel_ms, pageable_ms, pinned_ms = (statistics.median(v[1:]) for v in (kernel, pageable, pin))
    n_out = sum(n_outs)
    flops = 2.0 * -(-pl.numtaps // pl.up) * n_out
    nbytes = host.nbytes + n_out * 4
    floor_ms = max(flops / PEAK_FLOPS, nbytes / PEAK_BYTES) * 1e3
    rng = np.random.default_rng(5)
    worst, worst_bound, sq, count = 0.0, 0.0, 0.0, 0
    for b in rng.integers(0, len(rows), 8):
        pick = rng.integers(0, len(rows[b]), 256)
        y, mag = rs.reference(waves[b], rate, pick)
        err = np.abs(rows[b][pick].astype(np.float64) - y)
        sq, count = sq + float((err ** 2).sum()), count + len(err)
        k = int(np.argmax(err))
        if err[k] > worst:
            worst, worst_bound = float(err[k]), float(rs.error_bound(y, mag, rate, channels)[k])
    return {"up": pl.up, "down": pl.down, "numtaps": pl.numtaps, "kernel_ms": kernel_ms, "kernel_ms_min_max": [min(kernel[1:]), max(kernel[1:])],
            "input_bytes": host.nbytes, "h2d_pageable_ms": pageable_ms, "h2d_pageable_gb_per_s": host.nbytes / (pageable_ms * 1e-3) / 1e9,
            "h2d_pinned_ms": pinned_ms, "h2d_pinned_gb_per_s": host.nbytes / (pinned_ms * 1e-3) / 1e9,
            "flops": flops, "bytes": nbytes,
            "tflops_per_s": flops / (kernel_ms * 1e-3) / 1e12, "gb_per_s": nbytes / (kernel_ms * 1e-3) / 1e9,
            "floor_ms": floor_ms, "floor_is": "flops" if flops / PEAK_FLOPS > nbytes / PEAK_BYTES else "bytes",
            "share_of_floor": floor_ms / kernel_ms, "rms_error_vs_float64": (sq / count) ** 0.5, "max_abs_error_vs_float64": worst,
            "its_bound": worst_bound}


if __name__ == "__main__":
    main()
