// k_rnnt_hotwords.h — the device walk over the context graphs of a call (include/rs_asr.h: rs_hotwords), shared by the searches that
// bias towards hotwords: the modified beam search (k_rnnt_mbs.hip, rs_rnnt_mbs_hotwords) and ALSD (k_rnnt_alsd.hip,
// rs_rnnt_alsd_hotwords).  Both compile this text, so a step gives both the same bits.
//
// The graph is read-only flat arrays, all graphs of the call concatenated.  A root can have thousands of children: a child is found
// by bisection of the node's sorted token list.  THESE GPUS ARE SHARED, so the walk cannot spin or read out of bounds whatever the
// table holds: every loop is counted (a fail step strictly lowers the level in a valid table, so max_level + 1 fail steps suffice
// and that is the bound; a bisection halves an interval of < 2^31 entries, 32 steps), and a node or child index outside the table is
// replaced by the root before it is used — a corrupt table can give a wrong bonus, nothing else.  rs_hotwords_check (rs_api.hip)
// refuses such tables on the host before upload.
// Float32 order of one step (compile with -ffp-contract=off):
//   child hit:  score = token_score[n];       otherwise:  score = node_score[n] - node_score[state]
//   non-strict exit (output_score[n] != 0):  delta = (score + out) - node_score[n];     otherwise:  delta = score + output_score[n]
#pragma once
#include "k_rnnt_common.h"

namespace {

struct RnntNoHw {};      // the kernel argument of a search's plain form
struct RnntHw {          // the graphs of a call (include/rs_asr.h rs_hotwords; device pointers) and each utterance's graph
    rs_hotwords g;
    const int32_t* graph_of;   // [B], -1 = none
};

// root of utterance b's graph, or -1 when it has none (an index outside the table counts as none)
__device__ __forceinline__ int hw_root(const RnntHw& hw, int b) {
    const int gi = hw.graph_of[b];
    if (gi < 0 || gi >= hw.g.n_graphs) return -1;
    const int r = hw.g.graph_root[gi];
    return (r >= 0 && r < hw.g.n_nodes) ? r : -1;
}
__device__ __forceinline__ int hw_node(const rs_hotwords& g, int n, int root) { return (n >= 0 && n < g.n_nodes) ? n : root; }

// the child of node n (valid) on token tok, or -1: bisection of the node's sorted token list, at most 32 steps
__device__ __forceinline__ int hw_child(const rs_hotwords& g, int n, int tok, int root) {
    int lo = g.child_begin[n], hi = g.child_begin[n + 1];
    if (lo < 0) lo = 0;
    if (hi > g.n_children) hi = g.n_children;
    for (int it = 0; it < 32 && lo < hi; ++it) {
        const int mid = lo + ((hi - lo) >> 1);
        const int ct = g.child_tok[mid];
        if (ct == tok) return hw_node(g, g.child_node[mid], root);
        if (ct < tok) lo = mid + 1; else hi = mid;
    }
    return -1;
}

// ForwardOneStep(strict_mode = false): (state, tok) -> delta, next state.  `root` is valid; every index is made valid before use.
__device__ float hw_step(const rs_hotwords& g, int root, int state, int tok, int* next) {
    state = hw_node(g, state, root);
    int n = hw_child(g, state, tok, root);
    float score;
    if (n >= 0) {
        score = g.token_score[n];
    } else {
        n = hw_node(g, g.fail[state], root);
        int c = hw_child(g, n, tok, root);
        for (int it = 0; it <= g.max_level && c < 0 && n != root; ++it) {
            n = hw_node(g, g.fail[n], root);
            c = hw_child(g, n, tok, root);
        }
        if (c >= 0) n = c;
        score = g.node_score[n] - g.node_score[state];
    }
    const float os = g.output_score[n];
    if (os != 0.0f) {
        const int o = g.output[n];
        const float out = g.is_end[n] ? g.node_score[n] : ((o >= 0 && o < g.n_nodes) ? g.node_score[o] : g.node_score[n]);
        *next = root;
        return (score + out) - g.node_score[n];
    }
    *next = n;
    return score + os;
}

}  // namespace
