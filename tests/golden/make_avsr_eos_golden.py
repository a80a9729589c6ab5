"""Generate tests/golden/avsr_ref_eos.npz — generate() of the REFERENCE ITSELF (pkg/avsr/src/avhubert/modeling_avhubert.py through
transformers' GenerationMixin) on weights that DO emit eos.  Run in the BUILD container (CPU; the reference tree must be present):

    python tests/golden/make_avsr_eos_golden.py

The other avsr goldens (make_avsr_golden.py) contain no eos token: random weights never emit it, so the finished-slot half of beam
search (the K finished slots, the length penalty, the "cannot improve" early stop) and greedy's pad filling are not exercised by
them.  The recipe here (tests/avsr_search_ref.py: eos_recipe / EOS_RECIPE) raises every eos logit by alpha:

    AVSR_TINY, synthetic_state_dict_avsr(cfg, 0), decoder.layer_norm.bias += alpha * e / (e . e) with e = lm_head.weight[eos_token_id]
    synthetic_clips(6, 24, seed=11, ragged=True, min_frames=8); num_beams 3; max_new_tokens 24; use_cache=False as make_avsr_golden.py

and two values of alpha are stored (alpha <= 4: almost nothing ends early; alpha >= 7: everything ends within ten tokens):
  alpha 5.5   one clip runs to the length limit, the others end by eos at different lengths
  alpha 6.5   every beam result ends by eos, so the output is narrower than 1 + max_new_tokens (the search itself still runs to the
              limit: no clip stops improving earlier; the stop before the limit is covered at alpha 7.5 against oracle/avsr.py in
              tests/test_avsr_search_host.py); every greedy row emits eos
These properties are asserted below.  They are conditions on the recipe, not measurements: if a torch / transformers version breaks
them, move alpha inside (5, 7) until they hold and say so here.

Stored: alphas, weight_seed, input_seed, clips, frames, lens, beams, new_tokens, input_sha256, and per alpha (suffix _a55 / _a65)
beam (sequences int32), beam_scores (sequences_scores float32), greedy (sequences int32).
"""
import hashlib
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

from reazonspeech_amd.runtime.avsr_config import AVSR_TINY                             # noqa: E402
from reazonspeech_amd.runtime.avsr_synth import synthetic_clips                        # noqa: E402
from oracle import _ref_avsr as ra                                                     # noqa: E402
from avsr_search_ref import EOS_ALPHAS, EOS_RECIPE, eos_recipe                         # noqa: E402


def suffix(alpha):
    return f"_a{int(round(alpha * 10))}"


def lengths(seq, eos):
    """per row: tokens up to and including the first eos after the prompt, or the full width"""
    out = []
    for row in seq.tolist():
        out.append(row.index(eos, 1) + 1 if eos in row[1:] else len(row))
    return out


def main():
    r, cfg = EOS_RECIPE, AVSR_TINY
    a, v, mask, lens = synthetic_clips(r["clips"], r["frames"], seed=r["seed"], ragged=True, min_frames=r["min_frames"])
    kw = dict(input_values=torch.from_numpy(a), pixel_values=torch.from_numpy(v), padding_mask=torch.from_numpy(mask))
    h = hashlib.sha256(a.tobytes() + v.tobytes() + mask.tobytes()).digest()
    N, K = r["max_new_tokens"], r["num_beams"]
    store = {"alphas": np.asarray(EOS_ALPHAS, np.float64), "weight_seed": np.int64(r["weights_seed"]), "input_seed": np.int64(r["seed"]),
             "clips": np.int64(r["clips"]), "frames": np.int64(r["frames"]), "lens": lens, "beams": np.int64(K), "new_tokens": np.int64(N),
             "input_sha256": np.frombuffer(h, np.uint8)}
    for alpha in EOS_ALPHAS:
        model = ra.build(cfg, eos_recipe(cfg, alpha, r["weights_seed"]))
        t0 = time.time()
        with torch.no_grad():
            greedy = model.generate(**kw, num_beams=1, do_sample=False, max_new_tokens=N, use_cache=False)
            out = model.generate(**kw, num_beams=K, do_sample=False, max_new_tokens=N, use_cache=False, return_dict_in_generate=True, output_scores=True)
        bl, gl = lengths(out.sequences, cfg.eos_token_id), lengths(greedy, cfg.eos_token_id)
        print(f"[alpha {alpha}] {time.time() - t0:.1f} s: beam width {out.sequences.shape[1]} lengths {bl} scores {out.sequences_scores.tolist()}; "
              f"greedy width {greedy.shape[1]} lengths {gl}", flush=True)
        s = suffix(alpha)
        store["beam" + s] = out.sequences.numpy().astype(np.int32)
        store["beam_scores" + s] = out.sequences_scores.numpy().astype(np.float32)
        store["greedy" + s] = greedy.numpy().astype(np.int32)
        if alpha == EOS_ALPHAS[0]:
            assert max(bl) == 1 + N, "alpha 5.5: one clip must reach the length limit"
            assert sum(n < 1 + N for n in bl) >= 4, "alpha 5.5: at least four clips must end by eos before the limit"
        else:
            assert out.sequences.shape[1] < 1 + N, "alpha 6.5: every beam result must end by eos before the length limit"
    path = os.path.join(HERE, "avsr_ref_eos.npz")
    np.savez_compressed(path, **store)
    print("wrote", path, os.path.getsize(path), "bytes", flush=True)


if __name__ == "__main__":
    main()
