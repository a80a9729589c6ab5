"""Kernel trace of generate(search="device"): which kernels run between the encoder's end and the end of generate().

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o trace -- python scripts/avsr_search_trace.py run
    python scripts/avsr_search_trace.py check OUT/**/trace_kernel_trace.csv > profiles/<name>.txt

`check` takes the last generate() of the trace: from the last encoder attention kernel (avsr_attn_mfma_kernel runs only in the
encoder; the rest of the last encoder layer follows it) to avsr_search_finish_kernel, lists the kernels in that window and fails if
one of them is a torch kernel (at::native)."""
import csv
import os
import sys


def run():
    import torch
    sys.path.insert(0, os.getcwd())
    from reazonspeech_amd.avsr import synthetic_model
    from reazonspeech_amd.runtime.avsr_config import AVSR_BASE
    from reazonspeech_amd.runtime.avsr_synth import synthetic_clips
    m = synthetic_model(AVSR_BASE, 0, device="cuda:0", search="device")
    a, v, mask, _ = synthetic_clips(16, 250, seed=1, ragged=True, min_frames=83)
    for _ in range(2):                       # the second call is the one `check` reads
        out = m.generate(input_values=a, pixel_values=v, padding_mask=mask, num_beams=5, max_new_tokens=32)
        torch.cuda.synchronize()
    print("generate(search='device') ->", tuple(out.shape))


def check(path):
    rows = list(csv.DictReader(open(path, newline="")))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    names = [r["Kernel_Name"] for r in rows]
    last = max(i for i, n in enumerate(names) if "avsr_search_finish_kernel" in n)
    init = max(i for i, n in enumerate(names[:last]) if "avsr_search_init_kernel" in n)
    enc_end = max(i for i, n in enumerate(names[:init]) if "avsr_attn_mfma_kernel" in n)
    window = names[enc_end + 1:last + 1]
    counts = {}
    for n in window:
        short = n.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
        counts[short] = counts.get(short, 0) + 1
    span = (int(rows[last]["End_Timestamp"]) - int(rows[enc_end]["End_Timestamp"])) / 1e6
    busy = sum(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rows[enc_end + 1:last + 1]) / 1e6
    print(f"# {path}: last generate(search='device'), from the encoder's last attention kernel to avsr_search_finish_kernel")
    print(f"# {len(window)} kernels, {span:.2f} ms span, {busy:.2f} ms busy (the window still holds the rest of the last encoder layer: 3 GEMMs, 2 LayerNorms)")
    for n, c in sorted(counts.items(), key=lambda kv: -kv[1]):
        print(f"{c:>6}  {n}")
    torch_kernels = sorted({n for n in window if "at::native" in n or "at::cuda" in n})
    print(f"# torch kernels in the window: {len(torch_kernels)}")
    for n in torch_kernels:
        print("#   ", n[:160])
    return 1 if torch_kernels else 0


if __name__ == "__main__":
    sys.exit(run() if sys.argv[1] == "run" else check(sys.argv[2]))
