"""generate(search="device") with neutral options against the options of rs_avsr_search_opts, one process, AVSR_BASE, 16 clips x 250
frames, 256 new tokens: the cost of the <true> selection kernels (csrc/k_avsr_search.hip) per token.

    python scripts/avsr_search_opts_ab.py ab [reps] > profiles/<name>.txt
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o trace -- python scripts/avsr_search_opts_ab.py run CASE
    python scripts/avsr_search_opts_ab.py stats OUT/**/trace_kernel_stats.csv       # the search kernels' lines of a trace

CASE: neutral | ngram3_rep12 | nret5 | es_true.  The synthetic weights never emit eos, so every call runs all 256 steps and the cases
differ by the selection launch alone (early_stopping=True therefore never stops early here: it times the second stop word)."""
import csv
import os
import statistics
import sys
import time

CASES = {
    "neutral": {},
    "ngram3_rep12": dict(no_repeat_ngram_size=3, repetition_penalty=1.2),
    "nret5": dict(num_return_sequences=5),
    "es_true": dict(early_stopping=True),
}
B, T, N = 16, 250, 256


def setup():
    import torch
    sys.path.insert(0, os.getcwd())
    from reazonspeech_amd.avsr import synthetic_model
    from reazonspeech_amd.runtime.avsr_config import AVSR_BASE
    from reazonspeech_amd.runtime.avsr_synth import synthetic_clips
    m = synthetic_model(AVSR_BASE, 0, device="cuda:0", search="device")
    a, v, mask, _ = synthetic_clips(B, T, seed=1, ragged=True, min_frames=T // 3)
    return torch, m, dict(input_values=a, pixel_values=v, padding_mask=mask)


def ab(reps):
    torch, m, kw = setup()

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    timed(lambda: m.avhubert(**kw))
    enc_ms = statistics.median(timed(lambda: m.avhubert(**kw))[0] for _ in range(reps))
    print(f"# AVSR_BASE, {B} clips x {T} frames (ragged), search='device', {reps} alternated repetitions after one warm-up call each; {torch.cuda.get_device_name(0)}")
    print(f"# encoder alone: median {enc_ms:.1f} ms")
    print(f"{'beams':>5} {'case':>13} {'call_ms':>9} {'min_ms':>9} {'rows':>5} {'tokens':>7} {'ms_per_token':>13} {'vs_neutral':>11}")
    for beams in (5, 1):
        cases = {k: o for k, o in CASES.items() if beams > 1 or k in ("neutral", "ngram3_rep12")}
        ts, outs = {k: [] for k in cases}, {}
        for k, o in cases.items():
            timed(lambda: m.generate(**kw, num_beams=beams, max_new_tokens=N, **o))
        for _ in range(reps):
            for k, o in cases.items():
                ms, outs[k] = timed(lambda: m.generate(**kw, num_beams=beams, max_new_tokens=N, **o))
                ts[k].append(ms)
        base = statistics.median(ts["neutral"])
        for k in cases:
            med, tokens = statistics.median(ts[k]), outs[k].shape[1] - 1
            print(f"{beams:>5} {k:>13} {med:>9.1f} {min(ts[k]):>9.1f} {outs[k].shape[0]:>5} {tokens:>7} {(med - enc_ms) / tokens:>13.3f} {med / base:>11.3f}")


def run(case):
    torch, m, kw = setup()
    for _ in range(2):
        out = m.generate(**kw, num_beams=5, max_new_tokens=N, **CASES[case])
        torch.cuda.synchronize()
    print(f"generate(search='device', {CASES[case]}) ->", tuple(out.shape))


def stats(path):
    for r in csv.DictReader(open(path, newline="")):
        if "avsr_beam_step" in r["Name"] or "avsr_greedy_step" in r["Name"] or "avsr_search_" in r["Name"]:
            name = r["Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
            print(f"{name:45s} calls {r['Calls']:>6}  average {float(r['AverageNs']) / 1e3:8.2f} us  total {float(r['TotalDurationNs']) / 1e6:8.2f} ms")


if __name__ == "__main__":
    mode = sys.argv[1]
    if mode == "ab":
        ab(int(sys.argv[2]) if len(sys.argv) > 2 else 5)
    elif mode == "run":
        run(sys.argv[2])
    else:
        stats(sys.argv[2])
