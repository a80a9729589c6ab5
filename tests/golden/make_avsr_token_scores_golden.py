"""Generate tests/golden/avsr_ref_token_scores.npz — what generate(..., return_dict_in_generate=True, output_scores=True) of the
REFERENCE ITSELF (pkg/avsr/src/avhubert/modeling_avhubert.py through transformers' GenerationMixin) returns beside the ids:
`scores`, `beam_indices` and compute_transition_scores().  Run in the BUILD container (CPU; the reference tree must be present):

    python tests/golden/make_avsr_token_scores_golden.py

The recipe is make_avsr_eos_golden.py's (tests/avsr_search_ref.py: eos_recipe / EOS_RECIPE — AVSR_TINY, 6 ragged clips, num_beams 3,
max_new_tokens 24, use_cache=False), alpha 5.5 for every case (no condition below asked for another value).  Cases:

  beam      num_beams 3, no option                       + the whole `scores` tuple
  greedy    num_beams 1, no option                       + the whole `scores` tuple
  combined  avsr_search_opts_ref.CASES["combined"]       (repetition_penalty, no_repeat_ngram_size, min_new_tokens, 2 sequences, early_stopping)
  nret3     avsr_search_opts_ref.CASES["nret3"]          (3 sequences per clip)

CONDITIONS, asserted below; if a torch / transformers version breaks one, move alpha within (5, 8) and say so here:
  - some returned hypothesis has non-constant beam_indices (it re-parented)
  - one beam-baseline hypothesis ends by eos before the length limit and one reaches max_new_tokens
  - in `combined` the normalised and the unnormalised transition scores differ by more than 1e-3 on some token

Stored: transformers_version, input_sha256, alpha, clips, beams, new_tokens, and per case NAME: NAME_sequences int32, NAME_transition /
NAME_transition_norm float32 (compute_transition_scores with normalize_logits False / True), for the beam cases NAME_sequences_scores
float32 and NAME_beam_indices int32, for the two baselines NAME_scores float32 [steps][rows][vocab].  Only arrays of numbers.
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

ALPHA = 5.5
TOL = 1e-3
JOBS = {"beam": ("beam", {}), "greedy": ("greedy", {}), "combined": ("beam", CASES["combined"][2]), "nret3": ("beam", CASES["nret3"][2])}


def inputs():
    r = EOS_RECIPE
    return synthetic_clips(r["clips"], r["frames"], seed=r["seed"], ragged=True, min_frames=r["min_frames"])


def run(name):
    """one generate() of the reference -> (name, dict of arrays, seconds)"""
    import torch
    from oracle import _ref_avsr as ra
    torch.set_num_threads(2)
    search, opts = JOBS[name]
    r, cfg = EOS_RECIPE, AVSR_TINY
    a, v, mask, _ = inputs()
    kw = dict(input_values=torch.from_numpy(a), pixel_values=torch.from_numpy(v), padding_mask=torch.from_numpy(mask))
    model = ra.build(cfg, eos_recipe(cfg, ALPHA, r["weights_seed"]))
    t0 = time.time()
    with torch.no_grad():
        out = model.generate(**kw, num_beams=1 if search == "greedy" else r["num_beams"], do_sample=False, max_new_tokens=r["max_new_tokens"],
                             use_cache=False, return_dict_in_generate=True, output_scores=True, **opts)
        bi = getattr(out, "beam_indices", None)
        assert (bi is None) == (search == "greedy")
        got = {"sequences": out.sequences.numpy().astype(np.int32)}
        for key, norm in (("transition", False), ("transition_norm", True)):
            got[key] = model.compute_transition_scores(out.sequences, out.scores, bi, normalize_logits=norm).numpy().astype(np.float32)
        if bi is not None:
            got["beam_indices"] = bi.numpy().astype(np.int32)
            got["sequences_scores"] = out.sequences_scores.numpy().astype(np.float32)
        if not opts:
            got["scores"] = np.stack([s.numpy().astype(np.float32) for s in out.scores])
    return name, got, time.time() - t0


def main():
    import transformers
    r = EOS_RECIPE
    a, v, mask, _ = inputs()
    h = hashlib.sha256(a.tobytes() + v.tobytes() + mask.tobytes()).digest()
    with multiprocessing.get_context("spawn").Pool(4) as pool:
        done = {}
        for name, got, dt in pool.imap_unordered(run, list(JOBS)):
            print(f"{name:9s} {dt:5.1f} s  " + "  ".join(f"{k} {v_.shape}" for k, v_ in got.items()), flush=True)
            done[name] = got
    N, eos = r["max_new_tokens"], AVSR_TINY.eos_token_id
    # the conditions
    reparented = False
    for name in ("beam", "combined", "nret3"):
        for row in done[name]["beam_indices"]:
            live = row[row >= 0]
            reparented |= live.size > 1 and bool((live != live[0]).any())
    assert reparented, "no returned hypothesis re-parented: beam_indices would pin nothing"
    glen = (done["beam"]["beam_indices"] >= 0).sum(axis=1)
    print("beam baseline generated lengths", glen.tolist(), flush=True)
    seq = done["beam"]["sequences"]
    assert any(g < N and seq[i, g] == eos for i, g in enumerate(glen)), "no hypothesis ends by eos before the limit"
    assert (glen == N).any(), "no hypothesis reaches max_new_tokens"
    live = done["combined"]["beam_indices"] >= 0
    gap = np.abs(done["combined"]["transition"] - done["combined"]["transition_norm"])[live]
    print(f"combined: normalised vs unnormalised transition scores differ by up to {float(gap.max()):.3f}", flush=True)
    assert float(gap.max()) > TOL, "normalize_logits changes nothing in `combined`"
    # what the reference documents of its own output: the mean transition score is sequences_scores (length_penalty 1)
    for name in ("beam", "combined", "nret3"):
        d = done[name]
        n = (d["beam_indices"] >= 0).sum(axis=1)
        assert np.abs(d["transition"].sum(axis=1) / n - d["sequences_scores"]).max() <= 1e-4, name
    store = {"transformers_version": np.asarray(transformers.__version__), "input_sha256": np.frombuffer(h, np.uint8), "alpha": np.float64(ALPHA),
             "clips": np.int64(r["clips"]), "beams": np.int64(r["num_beams"]), "new_tokens": np.int64(N)}
    for name, got in done.items():
        for key, arr in got.items():
            store[f"{name}_{key}"] = arr
    path = os.path.join(HERE, "avsr_ref_token_scores.npz")
    np.savez_compressed(path, **store)
    print("wrote", path, os.path.getsize(path), "bytes", flush=True)


if __name__ == "__main__":
    main()
