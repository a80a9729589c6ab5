// rs_ngram_check.h — is a table (HOST pointers) an n-gram model the device walk may be given?  Host only, plain C++: no HIP include.
// The walk (k_rnnt_ngram.h) is safe on any table; a table that fails here would give scores nobody meant.  rs_api.hip exports this as
// rs_ngram_check; tests/ngram_host_main.cpp builds it alone, also under AddressSanitizer + UBSan.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdio.h>

#include "../../include/rs_asr.h"

enum { RS_NGRAM_MAX_ORDER = 8 };

inline int rs_ngram_check_table(const rs_ngram_host* t, char* msg, size_t msg_bytes) {
    auto fail = [&](const char* fmt, long long a, long long b, long long c) {
        if (msg && msg_bytes) snprintf(msg, msg_bytes, fmt, a, b, c);
        return (int)RS_EINVAL;
    };
    if (msg && msg_bytes) msg[0] = 0;
    if (!t) return fail("ngram: null table", 0, 0, 0);
    if (t->n_nodes < 0 || t->n_children < 0 || t->n_logits < 0) return fail("ngram: negative count", 0, 0, 0);
    if (t->n_nodes == 0) return RS_OK;                                     // no model
    if (t->order < 1 || t->order > RS_NGRAM_MAX_ORDER) return fail("ngram: order %lld outside 1..%lld", t->order, RS_NGRAM_MAX_ORDER, 0);
    if (!t->child_begin || !t->logp || !t->backoff || !t->suffix || !t->level || (t->n_logits > 0 && !t->root_child) ||
        (t->n_children > 0 && (!t->child_tok || !t->child_node)))
        return fail("ngram: null array", 0, 0, 0);
    const int N = t->n_nodes, C = t->n_children, V = t->n_logits;
    if (!isfinite(t->unk_logp)) return fail("ngram: unk_logp is not finite", 0, 0, 0);
    if (t->child_begin[0] != 0 || t->child_begin[N] != C) return fail("ngram: child_begin must run from 0 to n_children=%lld", C, 0, 0);
    if (t->level[0] != 0 || t->suffix[0] != 0) return fail("ngram: the root (node 0) must have level 0 and itself as suffix", 0, 0, 0);
    if (t->start < 0 || t->start >= N || (t->start != 0 && t->level[t->start] != 1))
        return fail("ngram: start=%lld is neither the root nor a level-1 node", t->start, 0, 0);
    for (int n = 0; n < N; ++n) {
        const int lo = t->child_begin[n], hi = t->child_begin[n + 1];
        if (lo < 0 || hi < lo || hi > C) return fail("ngram: child_begin[%lld..] = %lld, %lld is not an ascending range of the children", n, lo, hi);
        if (t->level[n] < 0 || t->level[n] > t->order) return fail("ngram: level[%lld]=%lld outside 0..order=%lld", n, t->level[n], t->order);
        if (!isfinite(t->logp[n]) || !isfinite(t->backoff[n])) return fail("ngram: node %lld has a value that is not finite", n, 0, 0);
        const int s = t->suffix[n];
        if (s < 0 || s >= N) return fail("ngram: suffix[%lld]=%lld outside the %lld nodes", n, s, N);
        if (n > 0 && t->level[s] >= t->level[n]) return fail("ngram: suffix[%lld]=%lld does not lower the level (%lld)", n, s, t->level[n]);
        for (int c = lo; c < hi; ++c) {
            const int k = t->child_node[c];
            if (k <= 0 || k >= N) return fail("ngram: child_node[%lld]=%lld outside the nodes 1..%lld", c, k, N - 1);
            if (t->level[k] != t->level[n] + 1) return fail("ngram: child %lld of node %lld is not one level below it", k, n, 0);
            if (t->child_tok[c] < 0 || t->child_tok[c] >= V) return fail("ngram: child_tok[%lld]=%lld outside the %lld logits", c, t->child_tok[c], V);
            if (c > lo && t->child_tok[c] <= t->child_tok[c - 1]) return fail("ngram: the children of node %lld are not sorted ascending (entry %lld)", n, c, 0);
        }
    }
    // root_child[v] is the root's child on v, and every child of the root is in it
    int listed = 0;
    for (int v = 0; v < V; ++v) {
        const int r = t->root_child[v];
        if (r == -1) continue;
        if (r <= 0 || r >= N || t->level[r] != 1) return fail("ngram: root_child[%lld]=%lld is not a level-1 node", v, r, 0);
        int found = -1;
        for (int lo = t->child_begin[0], hi = t->child_begin[1]; lo < hi;) {
            const int mid = lo + ((hi - lo) >> 1);
            if (t->child_tok[mid] == v) { found = t->child_node[mid]; break; }
            if (t->child_tok[mid] < v) lo = mid + 1; else hi = mid;
        }
        if (found != r) return fail("ngram: root_child[%lld]=%lld is not the root's child on that token", v, r, 0);
        ++listed;
    }
    if (listed != t->child_begin[1]) return fail("ngram: the root has %lld children but root_child lists %lld", t->child_begin[1], listed, 0);
    return RS_OK;
}
