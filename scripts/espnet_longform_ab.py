"""Long recordings WITH segments, three ways, one process: the 120M synthetic ESPnet model with the greedy search on (a) one
recording of 600 s and (b) 16 recordings of 120 s.  Per input: `transcribe` per recording with `segmentation="host"`, `transcribe`
per recording with `segmentation="device"` (what a user of long audio had before `transcribe_batch` took long recordings), and
`transcribe_batch` with `segmentation="device"` (cut points in lockstep through rs_ctc_find_blank, all pieces recognised and
aligned as one pool).  After one warm-up call per way the three are alternated; each call is synchronised and the median is
reported, with the encoder passes of one call counted per phase (blank finder / recognition / alignment) as calls x windows.

The token list is the synthetic one with '<unk>' and ',' replaced by two more kanji: a recognised text that holds a character
the aligner leaves out of its ground truth ('<unk>' is five characters no token spells, ',' is one of ctc-segmentation's excluded
characters) has more characters than timings, and the segment loop then raises IndexError — in the reference as in every way
timed here — which random weights run into within a few hundred windows.

The cuts of this run come from the synthetic CTC head, whose blank posterior is above the blank finder's threshold on about
half of the frames whatever the audio holds: the pieces are shorter than real speech would give (their count is in the
output), so the figures say nothing about the statistics of real cuts.

    python scripts/espnet_longform_ab.py [--reps=3] > profiles/espnet_longform_ab.json      (one JSON line)
"""
import importlib
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from reazonspeech_amd.runtime.config import ESPNET_CONFORMER_120M            # noqa: E402
from reazonspeech_amd.runtime.synth import synthetic_batch                   # noqa: E402
from reazonspeech_amd.runtime.weights_espnet import synthetic_state_dict_espnet  # noqa: E402
from reazonspeech_amd.espnet.asr.model import EspnetModel, synthetic_token_list   # noqa: E402
from reazonspeech_amd.espnet.asr import interface                            # noqa: E402

etr = importlib.import_module("reazonspeech_amd.espnet.asr.transcribe")
QUIET = interface.TranscribeConfig(verbose=False)
WAYS = ("transcribe_host", "transcribe_device", "transcribe_batch_device")


def arg(name, default):
    return ([int(a.split("=")[1]) for a in sys.argv[1:] if a.startswith(f"--{name}=")] or [default])[0]


class PassCounter:
    """counts the encoder passes of the model by phase.  The phase of a pass is what is registered as the CTC output while it
    runs (nothing: recognition; the blank column: blank finder; the posteriors: alignment), except that the host blank finder
    also registers the posteriors — it is told apart by being inside `find_blank`."""

    def __init__(self, model):
        self.model, self.inside_find_blank, self.counts = model, False, None
        ctx = model.am.ctx
        encoder, find_blank = ctx.encoder, etr.find_blank

        def counted_encoder(feats, n_frames, B, *rest):
            if self.counts is not None:
                probs, col = getattr(ctx, "_ctc", (None, None))
                phase = "blank" if (self.inside_find_blank or col is not None) else ("align" if probs is not None else "recognise")
                self.counts[phase]["passes"] += 1
                self.counts[phase]["windows"] += int(B)
            return encoder(feats, n_frames, B, *rest)

        def counted_find_blank(*a, **k):
            self.inside_find_blank = True
            try:
                return find_blank(*a, **k)
            finally:
                self.inside_find_blank = False

        ctx.encoder, etr.find_blank = counted_encoder, counted_find_blank

    def start(self):
        self.counts = {p: {"passes": 0, "windows": 0} for p in ("blank", "recognise", "align")}

    def stop(self):
        counts, self.counts = self.counts, None
        return counts


def run(model, way, audios):
    model.segmentation = "host" if way == "transcribe_host" else "device"
    if way == "transcribe_batch_device":
        return etr.transcribe_batch(model, audios)
    return [etr.transcribe(model, a, QUIET) for a in audios]


def measure(model, counter, label, audios, reps):
    def timed(way):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = run(model, way, audios)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    times, outs, passes = {w: [] for w in WAYS}, {}, {}
    for way in WAYS:                                             # warm-up (buffers, first launches) with the passes counted
        counter.start()
        timed(way)
        passes[way] = counter.stop()
    for _ in range(reps):
        for way in WAYS:
            ms, outs[way] = timed(way)
            times[way].append(ms)
    med = {w: statistics.median(t) for w, t in times.items()}
    seconds = sum(len(a.waveform) for a in audios) / 16000.0
    return {
        "input": label, "audio_seconds": seconds,
        "pieces": passes["transcribe_batch_device"]["recognise"]["windows"],
        "segments": sum(len(r.segments) for r in outs["transcribe_host"]),
        "ms": {w: round(med[w], 2) for w in WAYS}, "ms_all": {w: [round(t, 1) for t in times[w]] for w in WAYS},
        "rtfx": {w: round(seconds / (med[w] / 1e3), 1) for w in WAYS},
        "encoder_passes": passes,
        "speedup_over_transcribe_host": round(med["transcribe_host"] / med["transcribe_batch_device"], 2),
        "speedup_over_transcribe_device": round(med["transcribe_device"] / med["transcribe_batch_device"], 2),
        "results_equal": outs["transcribe_host"] == outs["transcribe_device"] == outs["transcribe_batch_device"],
    }


def main():
    reps = max(arg("reps", 3), 3)
    cfg = ESPNET_CONFORMER_120M
    spare = iter(chr(0x4E00 + 8192 + k) for k in range(2))          # past the pool synthetic_token_list draws from
    tokens = [next(spare) if t in ("<unk>", ",") else t for t in synthetic_token_list(cfg.vocab_size, 0)]
    model = EspnetModel(cfg, synthetic_state_dict_espnet(cfg, 0), tokens, device="cuda:0")
    counter = PassCounter(model)
    one = [interface.AudioData(synthetic_batch(1, 600.0, seed=1234)[0][0], 16000)]
    audio, _ = synthetic_batch(16, 120.0, seed=4321)
    many = [interface.AudioData(audio[b], 16000) for b in range(16)]
    print(json.dumps({
        "workload": "espnet 120M synthetic, long recordings with segments, greedy search; the cuts come from the synthetic CTC head "
                    "(blank above the threshold on about half of the frames), not from pauses in speech",
        "device": torch.cuda.get_device_name(0), "reps": reps,
        "inputs": [measure(model, counter, "1 x 600 s", one, reps), measure(model, counter, "16 x 120 s", many, reps)],
    }))


if __name__ == "__main__":
    main()
