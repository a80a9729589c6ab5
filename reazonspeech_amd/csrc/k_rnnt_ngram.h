// k_rnnt_ngram.h — the device walk over a backoff n-gram language model (include/rs_asr.h: rs_ngram), for the searches that fuse an
// LM into their scores: ALSD (k_rnnt_alsd.hip, rs_rnnt_alsd_lm) and the modified beam search (k_rnnt_mbs.hip, rs_rnnt_mbs_lm).  It
// holds the walk only and includes nothing of a search: both compile the same text, so a step gives both the same bits.
//
// The model is read-only flat arrays: a forward trie over token ids with sorted child lists (a child is found by bisection), a link
// from every node to the longest proper suffix of its words that the model has, and the backoff weight paid on that link.  Most
// walks end at the unigrams, and the root can have thousands of children: the last level is one load of root_child[token], not a
// bisection.  THESE GPUS ARE SHARED, so the walk cannot spin or read out of bounds whatever the table holds: every loop is counted (a
// suffix link strictly lowers the level in a valid table, so order + 1 backoff steps suffice and that is the bound; a bisection
// halves an interval of < 2^31 entries, 32 steps), a node or child index outside the table is replaced by the root (node 0) before it
// is used, and a token outside root_child counts as "not found" — a corrupt table can give a wrong score, nothing else.
// rs_ngram_check (rs_ngram_check.h) refuses such tables on the host before upload.
// Float32 order of one step (compile with -ffp-contract=off):
//   acc = 0; every backoff step: acc = acc + backoff[n];   found: lp = acc + logp[c];   not found: lp = acc + unk_logp
#pragma once
#include "k_rnnt_common.h"

namespace {

__device__ __forceinline__ int lm_node(const rs_ngram& g, int n) { return (n >= 0 && n < g.n_nodes) ? n : 0; }

// the child of node n (valid) on token tok, or -1: bisection of the node's sorted token list, at most 32 steps
__device__ __forceinline__ int lm_child(const rs_ngram& g, int n, int tok) {
    int lo = g.child_begin[n], hi = g.child_begin[n + 1];
    if (lo < 0) lo = 0;
    if (hi > g.n_children) hi = g.n_children;
    for (int it = 0; it < 32 && lo < hi; ++it) {
        const int mid = lo + ((hi - lo) >> 1);
        const int ct = g.child_tok[mid];
        if (ct == tok) { const int c = g.child_node[mid]; return (c > 0 && c < g.n_nodes) ? c : -1; }
        if (ct < tok) lo = mid + 1; else hi = mid;
    }
    return -1;
}

// (state, tok) -> log-probability of tok after the state's words, next state.  Every index is made valid before use.
__device__ float lm_step(const rs_ngram& g, int state, int tok, int* next) {
    int n = lm_node(g, state);
    float acc = 0.0f;
    int c = -1;
    for (int it = 0; it <= g.order; ++it) {
        if (n == 0) {
            if (tok >= 0 && tok < g.n_logits) { const int r = g.root_child[tok]; c = (r > 0 && r < g.n_nodes) ? r : -1; }
        } else {
            c = lm_child(g, n, tok);
        }
        if (c >= 0 || n == 0) break;
        acc = acc + g.backoff[n];
        n = lm_node(g, g.suffix[n]);
    }
    if (c < 0) { *next = 0; return acc + g.unk_logp; }
    *next = g.level[c] < g.order ? c : lm_node(g, g.suffix[c]);
    return acc + g.logp[c];
}

}  // namespace
