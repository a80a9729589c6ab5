"""Every workspace query of the library for the tiny configuration of each family, as one JSON object on stdout.

    python scripts/workspace_sizes.py > sizes.json

The ladder is fixed: B in {1, 3, 32, 256}, lengths 0.5 s, 10 s and 20 s (avsr: 12, 250 and 500 frames of 25 fps video), and the
search parameters of tests/test_gpu_workspace.py.  Run on two commits, the two tables show what a change to a layout does to the
sizes a caller is told (profiles/workspace_sizes_ab.json).  Needs a GPU only because a context cannot be made without one."""
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from reazonspeech_amd.avsr import AVHubertForConditionalGeneration                                       # noqa: E402
from reazonspeech_amd.espnet.asr.model import EspnetModel, synthetic_token_list                         # noqa: E402
from reazonspeech_amd.k2.asr.model import K2Model, synthetic_tokens                                     # noqa: E402
from reazonspeech_amd.runtime.avsr_config import AVSR_TINY                                               # noqa: E402
from reazonspeech_amd.runtime.avsr_weights import synthetic_state_dict_avsr                              # noqa: E402
from reazonspeech_amd.runtime.config import ESPNET_TINY, TINY                                            # noqa: E402
from reazonspeech_amd.runtime.k2_config import ZIPFORMER_TINY                                            # noqa: E402
from reazonspeech_amd.runtime.k2_weights import synthetic_state_dict_k2                                  # noqa: E402
from reazonspeech_amd.runtime.model import AsrModel                                                      # noqa: E402
from reazonspeech_amd.runtime.tokenizer import SyntheticTokenizer                                        # noqa: E402
from reazonspeech_amd.runtime.weights import synthetic_state_dict                                        # noqa: E402
from reazonspeech_amd.runtime.weights_espnet import synthetic_state_dict_espnet                          # noqa: E402

BATCHES = (1, 3, 32, 256)
SECONDS = (0.5, 10.0, 20.0)
AVSR_FRAMES = (12, 250, 500)


def contexts(precision):
    nemo = AsrModel(TINY, synthetic_state_dict(TINY, 0), SyntheticTokenizer(TINY.vocab_size), device="cuda:0", precision=precision)
    espnet = EspnetModel(ESPNET_TINY, synthetic_state_dict_espnet(ESPNET_TINY, 3), synthetic_token_list(ESPNET_TINY.vocab_size, 3), device="cuda:0",
                         precision=precision).am
    k2 = K2Model(ZIPFORMER_TINY, synthetic_state_dict_k2(ZIPFORMER_TINY, 3), synthetic_tokens(ZIPFORMER_TINY.vocab_size, 3), device="cuda:0",
                 precision=precision).am
    return {"nemo": nemo, "espnet": espnet, "k2": k2}


def main():
    out = {}
    keep = []
    for precision in ("bf16", "fp32"):
        for family, am in contexts(precision).items():
            keep.append(am)
            ctx = am.ctx
            for B in BATCHES:
                for s in SECONDS:
                    n = int(s * 16000)
                    at = f"B={B} s={s}"
                    out[f"{family} {precision} rs_workspace_bytes {at}"] = ctx.workspace_bytes(B, n)
                    if precision != "bf16":
                        continue
                    tp = max(ctx.enc_frames(max(ctx.mel_frames(n), 1)), 1)
                    if family == "nemo":
                        out[f"nemo alsd beam=4 {at}"] = ctx.alsd_workspace_bytes(B, 4, tp, 1.0)
                    if family == "espnet":
                        out[f"espnet beam beam=3 {at}"] = ctx.beam_workspace_bytes(B, 3, tp, 0)
                        out[f"espnet ctc_align c_max=64 S=4 {at}"] = ctx.ctc_align_workspace_bytes(B, tp, 64, 4)
                    if family == "k2":
                        out[f"k2 mbs K=4 {at}"] = ctx.mbs_workspace_bytes(B, 4, tp, tp)
    dev = AVHubertForConditionalGeneration(AVSR_TINY, synthetic_state_dict_avsr(AVSR_TINY, 0), device="cuda:0").dev
    lib, h = dev.ctx.lib, dev.ctx._h
    for B in BATCHES:
        for T in AVSR_FRAMES:
            at = f"B={B} T={T}"
            out[f"avsr encoder {at}"] = int(lib.rs_avsr_workspace_bytes(h, B, T))
            out[f"avsr decoder_state beams=2 max_len=9 {at}"] = int(lib.rs_avsr_decoder_state_bytes(h, B, T, 2, 9))
            # the search state's optional pieces: go2 with early_stopping=True; the marks where an options kernel runs (the n-gram ban) and
            # beams x vocabulary exceeds the 32768-byte LDS share: never at AVSR_TINY's 61 tokens, so 8 beams over 5000 tokens as well
            for ngram, es in ((0, False), (2, False), (2, True)):
                so = dev.search_opts(no_repeat_ngram_size=ngram, early_stopping=es)
                opts = f"ngram={ngram}" + (" es=1" if es else "")
                out[f"avsr search_state beams=2 max_len=9 {opts} {at}"] = int(
                    lib.rs_avsr_search_state_bytes_opts(h, B, 2, 9, AVSR_TINY.vocab_size, ctypes.byref(so)))
                out[f"avsr generate beams=2 max_len=9 {opts} {at}"] = int(lib.rs_avsr_generate_state_bytes_opts(h, B, T, 2, 9, ctypes.byref(so)))
                if T == AVSR_FRAMES[0]:                                       # (the search state does not depend on T)
                    out[f"avsr search_state beams=8 max_len=9 vocab=5000 {opts} B={B}"] = int(lib.rs_avsr_search_state_bytes_opts(h, B, 8, 9, 5000, ctypes.byref(so)))
    print(json.dumps(out, indent=0, sort_keys=True))


if __name__ == "__main__":
    main()
