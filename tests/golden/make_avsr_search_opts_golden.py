"""Generate tests/golden/avsr_ref_search_opts.npz — generate() of the REFERENCE ITSELF (pkg/avsr/src/avhubert/modeling_avhubert.py
through transformers' GenerationMixin) with the options that shape the search.  Run in the BUILD container (CPU; the reference tree
must be present):

    python tests/golden/make_avsr_search_opts_golden.py

The recipe is make_avsr_eos_golden.py's (tests/avsr_search_ref.py: eos_recipe / EOS_RECIPE — AVSR_TINY, 6 ragged clips, num_beams 3,
max_new_tokens 24, use_cache=False); the cases are tests/avsr_search_opts_ref.py's CASES, beam search plus greedy where the option
applies (early_stopping and num_return_sequences are beam-search options):

  rep13     repetition_penalty=1.3           alpha 5.5
  ngram2    no_repeat_ngram_size=2           alpha 5.5
  ngram3    no_repeat_ngram_size=3           alpha 5.5
  min8      min_new_tokens=8                 alpha 6.5: at 5.5 the beam results are longer than 8 tokens anyway and do not change
  es_true   early_stopping=True              alpha 5.5
  never     early_stopping="never"           alpha 6.5, length_penalty 2.0: with length_penalty 1.0 (and 0.5) the result equals
                                             early_stopping=False's at alpha 5.5, 6.5 and 7.5; at 2.0 four of the six clips differ
  nret3     num_return_sequences=3           alpha 5.5
  combined  repetition_penalty=1.2, no_repeat_ngram_size=2, min_new_tokens=6, num_return_sequences=2, early_stopping=True   alpha 5.5

CONDITION, asserted below: every stored result differs from the no-option result of the same alpha, length_penalty and search on at
least one clip (for num_return_sequences: has more rows).  A case that does not differ pins nothing; if a torch / transformers
version breaks the condition, move that case's alpha within (5, 8) or its length_penalty and say so here.

Stored: transformers_version, input_sha256, clips, beams, new_tokens, weight_seed, input_seed, and per case NAME: NAME_alpha,
NAME_length_penalty, NAME_beam (sequences int32), NAME_beam_scores (sequences_scores float32), and NAME_greedy where it applies.
"""
import hashlib
import multiprocessing
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

from reazonspeech_amd.runtime.avsr_config import AVSR_TINY                             # noqa: E402
from reazonspeech_amd.runtime.avsr_synth import synthetic_clips                        # noqa: E402
from avsr_search_ref import EOS_RECIPE, eos_recipe                                     # noqa: E402
from avsr_search_opts_ref import CASES                                                 # noqa: E402


def inputs():
    r = EOS_RECIPE
    return synthetic_clips(r["clips"], r["frames"], seed=r["seed"], ragged=True, min_frames=r["min_frames"])


def run(job):
    """one generate() of the reference -> (job, sequences, scores or None, seconds)"""
    import torch
    from oracle import _ref_avsr as ra
    torch.set_num_threads(2)
    name, alpha, lp, search, opts = job
    r, cfg = EOS_RECIPE, AVSR_TINY
    a, v, mask, _ = inputs()
    kw = dict(input_values=torch.from_numpy(a), pixel_values=torch.from_numpy(v), padding_mask=torch.from_numpy(mask))
    model = ra.build(cfg, eos_recipe(cfg, alpha, r["weights_seed"]))
    t0 = time.time()
    with torch.no_grad():
        if search == "greedy":
            seq = model.generate(**kw, num_beams=1, do_sample=False, max_new_tokens=r["max_new_tokens"], use_cache=False, **opts)
            return job, seq.numpy().astype(np.int32), None, time.time() - t0
        out = model.generate(**kw, num_beams=r["num_beams"], do_sample=False, max_new_tokens=r["max_new_tokens"], use_cache=False, length_penalty=lp,
                             return_dict_in_generate=True, output_scores=True, **opts)
    return job, out.sequences.numpy().astype(np.int32), out.sequences_scores.numpy().astype(np.float32), time.time() - t0


def differs(x, y):
    return x.shape != y.shape or not np.array_equal(x, y)


def main():
    import transformers
    r = EOS_RECIPE
    a, v, mask, lens = inputs()
    h = hashlib.sha256(a.tobytes() + v.tobytes() + mask.tobytes()).digest()
    jobs = []
    for name, (alpha, lp, opts, searches) in CASES.items():
        for search in searches:
            jobs.append((name, alpha, lp if search == "beam" else 1.0, search, opts))
            base = ("baseline", alpha, lp if search == "beam" else 1.0, search, {})
            if base not in jobs:
                jobs.append(base)
    with multiprocessing.get_context("spawn").Pool(4) as pool:
        done = {}
        for job, seq, scores, dt in pool.imap_unordered(run, jobs):
            print(f"{job[0]:9s} alpha {job[1]} length_penalty {job[2]} {job[3]:6s} {dt:5.1f} s  shape {seq.shape}", flush=True)
            done[job[:4]] = (seq, scores)
    store = {"transformers_version": np.asarray(transformers.__version__), "input_sha256": np.frombuffer(h, np.uint8), "clips": np.int64(r["clips"]),
             "beams": np.int64(r["num_beams"]), "new_tokens": np.int64(r["max_new_tokens"]), "weight_seed": np.int64(r["weights_seed"]),
             "input_seed": np.int64(r["seed"])}
    for name, (alpha, lp, opts, searches) in CASES.items():
        store[name + "_alpha"], store[name + "_length_penalty"] = np.float64(alpha), np.float64(lp)
        for search in searches:
            lpj = lp if search == "beam" else 1.0
            seq, scores = done[(name, alpha, lpj, search)]
            base = done[("baseline", alpha, lpj, search)][0]
            assert differs(seq, base), f"{name} / {search}: equal to the no-option result: the case pins nothing"
            n = int(opts.get("num_return_sequences", 1))
            assert seq.shape[0] == r["clips"] * n
            store[f"{name}_{search}"] = seq
            if search == "beam":
                store[name + "_beam_scores"] = scores
    path = os.path.join(HERE, "avsr_ref_search_opts.npz")
    np.savez_compressed(path, **store)
    print("wrote", path, os.path.getsize(path), "bytes", flush=True)


if __name__ == "__main__":
    main()
