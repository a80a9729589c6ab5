"""Helpers of the rows-per-utterance alignment tests (tests/test_rnnt_align_rows_host.py, tests/test_gpu_rnnt_align_rows.py).  TEST
INFRASTRUCTURE.

  plan(...)          the sharing rule of rs_rnnt_align_rows (include/rs_asr.h) restated in plain Python from its text: which rows
                     have a lattice, m, donor, the lattice rows each row owns, and the two numbers of `stats`.
  replicate(...)     the batch of R utterances whose row r is a copy of utterance row_utt[r]: what the guarantee compares against.
"""
import numpy as np

MAX_ROWS_PER_UTT = 64
OK, BAD_UTT, DECREASE, GROUP = 0, 1, 2, 4


def check_row_utt(row_utt, B):
    """0, or the OR of what is wrong: an entry below -1 or >= B, a decrease among the non-negative entries, a group above the cap"""
    err, last, count = 0, None, {}
    for v in (int(x) for x in row_utt):
        if v == -1:
            continue
        if v < -1 or v >= B:
            err |= BAD_UTT
            continue
        if last is not None and v < last:
            err |= DECREASE
        last = v if last is None else max(last, v)
        count[v] = count.get(v, 0) + 1
    if any(c > MAX_ROWS_PER_UTT for c in count.values()):
        err |= GROUP
    return err


def plan(row_utt, T, texts, V, blank, one, u_cap=None, counts=None):
    """row_utt [R], T [B] frames per utterance, texts [R] label lists (counts: n_ids where it differs from len, for bad rows) ->
    dict(err; lat_u, m, donor, owned [R]; stats (computed, without sharing))"""
    R, B = len(row_utt), len(T)
    u_cap = u_cap if u_cap is not None else max([len(t) for t in texts] + [1])
    counts = [len(t) for t in texts] if counts is None else list(counts)
    err = check_row_utt(row_utt, B)
    if err:
        return dict(err=err)
    lat_u = []
    for r in range(R):
        utt, n = int(row_utt[r]), counts[r]
        if utt < 0:
            lat_u.append(-1)
            continue
        bad = n < 0 or n > u_cap or any(i < 0 or i >= V or i == blank for i in texts[r][:n])
        frames = max(int(T[utt]), 0)
        lat_u.append(n if not bad and frames > 0 and not (one and n > frames) else -1)
    m, donor, owned, full = [0] * R, [-1] * R, [0] * R, 0
    for r in range(R):
        if lat_u[r] < 0:
            continue
        best, first = 0, -1
        for q in range(r):                                  # the earlier rows of the same utterance that have a lattice, in order
            if row_utt[q] != row_utt[r] or lat_u[q] < 0:
                continue
            a, b = texts[r][:lat_u[r]], texts[q][:lat_u[q]]
            c = 0
            while c < min(len(a), len(b)) and a[c] == b[c]:
                c += 1
            if c > best:                                    # strictly more: the FIRST row that attains the greatest stays
                best, first = c, q
        m[r], donor[r] = best, first
        frames = int(T[row_utt[r]])
        owned[r] = frames * (lat_u[r] + 1 - best)
        full += frames * (lat_u[r] + 1)
    return dict(err=0, lat_u=lat_u, m=m, donor=donor, owned=owned, stats=(sum(owned), full))


def replicate(f, lens, row_utt):
    """f torch [B][Tp][J], lens [B] -> (f [R][Tp][J], lens [R]) with row r = utterance row_utt[r] (a skipped row: utterance 0, length 0)"""
    idx = [max(int(u), 0) for u in row_utt]
    return f[idx].contiguous(), [int(lens[u]) if int(row_utt[r]) >= 0 else 0 for r, u in enumerate(idx)]
