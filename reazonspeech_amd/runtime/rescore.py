"""N-best rescoring by full likelihood, the host side the three packages share (`AsrModel.rescore`, runtime/model.py: the lists are
scored on the device by rs_rnnt_align_rows; here they are re-ranked).  The search's own ranking is not touched: `search_rank`
keeps it."""
import math

KEYS = ("likelihood", "norm_likelihood")


def check(rescore, nbest, beam_search, who="rescore"):
    """the `rescore=` keyword of a load_model -> None or the key; ValueError before anything is loaded"""
    if rescore is None or rescore is False:
        return None
    if rescore not in KEYS:
        raise ValueError(f"{who} must be None, 'likelihood' or 'norm_likelihood', not {rescore!r}")
    if not beam_search or not (isinstance(nbest, int) and not isinstance(nbest, bool) and nbest >= 2):
        raise ValueError(f"{who}={rescore!r} re-ranks an n-best list: it needs a beam search and nbest >= 2")
    return rescore


def norm(log_likelihood, n_tokens):
    return log_likelihood / max(int(n_tokens), 1)


def order(log_likelihoods, lengths, key):
    """positions of a list's entries by the chosen key, descending; ties (and entries without a likelihood: NaN counts as -inf)
    keep the search's order"""
    if key not in KEYS:
        raise ValueError(f"rescore key must be 'likelihood' or 'norm_likelihood', not {key!r}")
    vals = [ll if key == "likelihood" else norm(ll, n) for ll, n in zip(log_likelihoods, lengths)]
    vals = [-math.inf if v != v else v for v in vals]
    return sorted(range(len(vals)), key=lambda k: -vals[k])      # (sorted is stable)
