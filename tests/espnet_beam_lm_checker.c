/*
 * espnet_beam_lm_checker.c — CPU restatement of reazonspeech_amd/csrc/k_rnnt_beam.hip in ALL its forms: rs_rnnt_beam (plain),
 * rs_rnnt_beam_nbest (the ranked list) and rs_rnnt_beam_lm (hotwords, an n-gram LM, or both, with or without the list), in the
 * device's float32 evaluation order.  TEST INFRASTRUCTURE, built by tests/checker_lib.py with the flags of oracle/build.py and linked
 * against the oracle library.  Without a graph and without an LM it must equal oracle/espnet_beam.c (nbest = 0) and
 * tests/espnet_beam_nbest_checker.c (nbest >= 1) bit for bit (tests/test_espnet_beam_lm_host.py holds it to that); folding the three
 * into one checker is left for later.
 *
 * The search is the text of tests/espnet_beam_nbest_checker.c (pops, kept list, end-of-frame test, survivors ascending by score with
 * ties in kept order, the ranked list) with the rule of include/rs_asr.h (rs_rnnt_beam_lm) added.  Every hypothesis carries a context
 * state (a node of its utterance's graph; the utterance has one when graph_of[b] >= 0) and an LM state; the start hypothesis stands
 * at the graph's root and at lm->start.  A pop of a hypothesis with score hs, context state c and LM state s:
 *     the beam_k best labels are picked by raw logit, no term inside;
 *     blank extension: kept with hs + logp(blank), c, s;
 *     label extension v:   sc = hs + logp(v);   with a graph: (delta, c') = hw_step(c, v), sc = sc + delta;
 *                          with an LM: (lp, s') = lm_step(s, v), sc = sc + (alpha * lp), the product rounded first;
 *                          opened with sc, c', s' — the open list ranks sc (pop order, end-of-frame test).
 *   hw_step: tests/k2_mbs_lm_checker.c's (ForwardOneStep, strict_mode = false);  lm_step: the same file's (backoff walk).
 * After the last frame the survivors stay in the kept list's order (ascending by score BEFORE Finalize); each gets
 * sc = sc + (-node_score(c)) when its utterance has a graph (Finalize); then norm = sc / (float)len(yseq) (or sc), and the ranking of
 * rs_rnnt_beam_nbest.  No end-of-sentence term.  lm == NULL, no nodes or alpha == 0: no LM statement runs; hw == NULL, graph_of ==
 * NULL or no graphs: no hotword statement runs.
 *
 * nbest == 0: the one result of rs_rnnt_beam (entry 0 of the ranking) in ids / frames [B][out_cap], n_ids / scores / norm_scores
 * [B]; nbest >= 1: the lists [B][nbest][...].  n_hyps [B] as rs_rnnt_beam_nbest states (nbest == 0: 1, or 0 after an overflow).
 * Counters per utterance:
 *   nb_counters[b][0..5]   [0] length of the kept list after the last frame, [1] pairs of entries of the returned list with equal
 *                          label sequences, [2] equal norms met while ranking, [3] 1 if ranking by score alone gives another order,
 *                          [4] pops whose hypothesis tied with another open one on the score (the lower position went first),
 *                          [5] 1 if ranking the scores BEFORE Finalize gives another order than the one returned
 *   hw_counters[b][0..2]   [0] child hits, [1] fail transitions, [2] non-strict exits (a phrase completed);  finalize_total[b]: the
 *                          sum of the Finalize terms of the survivors
 *   lm_counters[b][0..13]  the layout of tests/k2_mbs_lm_checker.c: [1..8] hits by level, [9] backoffs, [10] unknown tokens, [11]
 *                          full-order pops, [13] walks
 *
 * `inject` (may be NULL): the hand-built cases replace prediction network and joint by a table — the logits of frame t for a
 * hypothesis whose last label is u (the blank at the start) are inject[(t V + u) V .. + V]; the weights are then not read.
 */
#include <stdlib.h>
#include <string.h>

#include "rnnt_math.h"

void rs_oracle_lstm_step(const float* x, const float* h, const float* c, const float* W, const float* bias, int H,
                         float* h_out, float* c_out);
int rs_oracle_joint_argmax(const float* f, const float* g, const float* Wo, const float* bo, int J, int V,
                           float* logits_out);
float rs_oracle_dot(const float* a, const float* w, int K);
float rs_oracle_lse(const float* z, int V);

#define LM_COUNTERS 14
#define NB_COUNTERS 6

typedef struct {
    float score;
    int node;      /* label-trie node of the whole sequence when tok < 0, of the sequence without its last label otherwise */
    int tok;       /* last label not yet in the trie, or -1 */
    int len;       /* len(yseq): labels + the leading blank */
    int state;     /* index of the prediction-net state stored BEFORE the last label */
    int alive;
    int ctx;       /* node of the context graph after the whole sequence */
    int lm;        /* node of the language model after the whole sequence */
} bhyp_t;

typedef struct { int parent, tok, t; } node_t;

typedef struct { float* v; int n, cap, width; } pool_t;     /* states: h [L][H] then c [L][H] */

/* the flat tables, as the ctypes drivers of tests/k2_mbs_lm_ref.py fill them */
typedef struct {
    const int32_t *child_begin, *child_tok, *child_node, *fail, *output, *is_end;
    const float *token_score, *node_score, *output_score;
    const int32_t* graph_root;
    int32_t n_graphs;
} hw_table;

typedef struct {
    const int32_t *child_begin, *child_tok, *child_node, *root_child, *suffix, *level;
    const float *logp, *backoff;
    int32_t n_nodes, order, start;
    float unk_logp;
} lm_table;

static int pool_push(pool_t* p, const float* h, const float* c, int LH) {
    if (p->n == p->cap) {
        p->cap = p->cap ? 2 * p->cap : 64;
        p->v = (float*)realloc(p->v, sizeof(float) * (size_t)p->cap * p->width);
    }
    memcpy(p->v + (size_t)p->n * p->width, h, sizeof(float) * LH);
    memcpy(p->v + (size_t)p->n * p->width + LH, c, sizeof(float) * LH);
    return p->n++;
}

static int same_labels(const node_t* nodes, int a, int la, int b, int lb) {
    if (la != lb) return 0;
    while (a != b) {
        if (a < 0 || b < 0 || nodes[a].tok != nodes[b].tok) return 0;
        a = nodes[a].parent; b = nodes[b].parent;
    }
    return 1;
}

static int hw_child(const hw_table* g, int n, int tok) {
    for (int c = g->child_begin[n]; c < g->child_begin[n + 1]; ++c)
        if (g->child_tok[c] == tok) return g->child_node[c];
    return -1;
}

static float hw_step(const hw_table* g, int root, int state, int tok, int* next, int32_t* counters) {
    int n = hw_child(g, state, tok);
    float score;
    if (n >= 0) {
        score = g->token_score[n];
        counters[0] += 1;
    } else {
        n = g->fail[state];
        while (hw_child(g, n, tok) < 0 && n != root) n = g->fail[n];
        const int c = hw_child(g, n, tok);
        if (c >= 0) n = c;
        score = g->node_score[n] - g->node_score[state];
        if (state != root) counters[1] += 1;
    }
    if (g->output_score[n] != 0.0f) {
        const int o = g->output[n];
        const float out = g->is_end[n] ? g->node_score[n] : (o >= 0 ? g->node_score[o] : g->node_score[n]);
        *next = root;
        counters[2] += 1;
        return (score + out) - g->node_score[n];
    }
    *next = n;
    return score + g->output_score[n];
}

static int lm_child(const lm_table* g, int n, int tok) {
    for (int c = g->child_begin[n]; c < g->child_begin[n + 1]; ++c)
        if (g->child_tok[c] == tok) return g->child_node[c];
    return -1;
}

static float lm_step(const lm_table* g, int state, int tok, int* next, int32_t* cnt) {
    int n = state, c = -1;
    float acc = 0.0f;
    cnt[13] += 1;
    for (int it = 0; it <= g->order; ++it) {
        c = n == 0 ? g->root_child[tok] : lm_child(g, n, tok);
        if (c >= 0 || n == 0) break;
        acc = acc + g->backoff[n];
        n = g->suffix[n];
        cnt[9] += 1;
    }
    if (c < 0) { cnt[10] += 1; *next = 0; return acc + g->unk_logp; }
    cnt[g->level[c]] += 1;
    if (g->level[c] < g->order) *next = c;
    else { *next = g->suffix[c]; cnt[11] += 1; }
    return acc + g->logp[c];
}

/* f [B][Tp][J] (joint.enc output).  N = max(nbest, 1): ids / frames [B][N][out_cap] (frames may be NULL), n_ids / scores /
 * norm_scores [B][N], n_hyps / pops [B].  Returns 0, -5 on overflow (max_pops per frame / out_cap), -1 for an nbest outside 0..8 or
 * above the beam. */
int rs_espnet_beam_lm_checker(const float* f, const int32_t* enc_lens, int B, int Tp, int J, int H, int L, int V, int blank,
                              const float* embed, const float* const* lstm_w, const float* const* lstm_b, const float* Wp,
                              const float* bp, const float* Wo, const float* bo, const float* inject, int beam, int score_norm, int max_pops,
                              int nbest, int out_cap, int32_t* ids, int32_t* frames, int32_t* n_ids, float* scores, float* norm_scores,
                              int32_t* n_hyps, int32_t* pops, int32_t* nb_counters /* [B][NB_COUNTERS] */, const hw_table* hw,
                              const int32_t* graph_of, int32_t* hw_counters /* [B][3] */, float* finalize_total /* [B] */,
                              const lm_table* lm, float lm_alpha, int32_t* lm_counters /* [B][LM_COUNTERS] */) {
    int overflow = 0;
    if (nbest < 0 || nbest > 8 || nbest > (beam < V ? beam : V)) return -1;
    const int N = nbest > 0 ? nbest : 1;
    const int use_lm = lm != NULL && lm->n_nodes > 0 && lm_alpha != 0.0f;
    const int use_hw = hw != NULL && graph_of != NULL && hw->n_graphs > 0;
    if (beam > V) beam = V;
    const int beam_k = beam < V - 1 ? beam : V - 1;
    const int LH = L * H;
    float* z = (float*)malloc(sizeof(float) * V);
    float* g = (float*)malloc(sizeof(float) * (J > 0 ? J : 1));
    float* hn = (float*)malloc(sizeof(float) * (LH > 0 ? LH : 1));
    float* cn = (float*)malloc(sizeof(float) * (LH > 0 ? LH : 1));
    for (int b = 0; b < B; ++b) {
        const int T = enc_lens[b];
        const int gi = use_hw ? graph_of[b] : -1;
        const int root = (gi >= 0 && gi < hw->n_graphs) ? hw->graph_root[gi] : -1;
        int32_t* hcnt = hw_counters + 3 * b;
        int32_t* lcnt = lm_counters + LM_COUNTERS * b;
        int32_t* nc = nb_counters + NB_COUNTERS * b;
        hcnt[0] = hcnt[1] = hcnt[2] = 0;
        for (int k = 0; k < LM_COUNTERS; ++k) lcnt[k] = 0;
        for (int k = 0; k < NB_COUNTERS; ++k) nc[k] = 0;
        finalize_total[b] = 0.0f;
        int n_nodes = 1, cap_nodes = 1024;
        node_t* nodes = (node_t*)malloc(sizeof(node_t) * cap_nodes);
        nodes[0].parent = -1; nodes[0].tok = blank; nodes[0].t = -1;
        pool_t pool[2] = {{NULL, 0, 0, 2 * LH}, {NULL, 0, 0, 2 * LH}};
        int cur = 0;
        memset(hn, 0, sizeof(float) * LH); memset(cn, 0, sizeof(float) * LH);
        pool_push(&pool[0], hn, cn, LH);
        const int cap_h = max_pops * (beam_k + 1) + 1;
        bhyp_t* hyps = (bhyp_t*)malloc(sizeof(bhyp_t) * cap_h);
        bhyp_t* kept = (bhyp_t*)malloc(sizeof(bhyp_t) * (max_pops + 1));
        int n_kept = 1, n_pops_total = 0, failed = 0;
        kept[0] = (bhyp_t){0.0f, 0, -1, 1, 0, 1, root < 0 ? 0 : root,
                           use_lm ? ((lm->start >= 0 && lm->start < lm->n_nodes) ? lm->start : 0) : 0};
        for (int t = 0; t < T && !failed; ++t) {
            int n_h = n_kept;
            memcpy(hyps, kept, sizeof(bhyp_t) * n_kept);
            n_kept = 0;
            int n_pop = 0;
            for (;;) {
                if (n_pop == max_pops) { failed = 1; break; }
                int mi = -1;
                for (int i = 0; i < n_h; ++i) if (hyps[i].alive && (mi < 0 || hyps[i].score > hyps[mi].score)) mi = i;
                for (int i = 0; i < n_h; ++i) if (i != mi && hyps[i].alive && hyps[i].score == hyps[mi].score) { nc[4] += 1; break; }
                bhyp_t mh = hyps[mi];
                hyps[mi].alive = 0;
                ++n_pop; ++n_pops_total;
                if (mh.tok >= 0) {                                     /* its sequence enters the trie now */
                    if (n_nodes == cap_nodes) { cap_nodes *= 2; nodes = (node_t*)realloc(nodes, sizeof(node_t) * cap_nodes); }
                    nodes[n_nodes].parent = mh.node; nodes[n_nodes].tok = mh.tok; nodes[n_nodes].t = t;
                    mh.node = n_nodes++; mh.tok = -1;
                }
                if (!inject) {
                    const float* sv = pool[cur].v + (size_t)mh.state * 2 * LH;
                    const float* x = embed + (size_t)nodes[mh.node].tok * H;
                    for (int l = 0; l < L; ++l) {
                        rs_oracle_lstm_step(x, sv + l * H, sv + LH + l * H, lstm_w[l], lstm_b[l], H, hn + l * H, cn + l * H);
                        x = hn + l * H;
                    }
                    for (int j = 0; j < J; ++j) g[j] = rs_oracle_dot(hn + (L - 1) * H, Wp + (size_t)j * H, H) + bp[j];
                }
                const int after = pool_push(&pool[cur], hn, cn, LH);
                if (inject) memcpy(z, inject + ((size_t)t * V + nodes[mh.node].tok) * V, sizeof(float) * V);
                else rs_oracle_joint_argmax(f + ((size_t)b * Tp + t) * J, g, Wo, bo, J, V, z);
                const float lse = rs_oracle_lse(z, V);
                kept[n_kept] = mh;                                     /* the blank extension keeps both states */
                kept[n_kept].score = mh.score + (z[blank] - lse);
                kept[n_kept].alive = 1;
                ++n_kept;
                float pz = INFINITY; int pv = -1;
                for (int j = 0; j < beam_k; ++j) {                     /* the beam_k best labels by raw logit: no term inside */
                    float bz = -INFINITY; int bv = -1;
                    for (int v = 0; v < V; ++v) {
                        if (v == blank) continue;
                        if (!(z[v] < pz || (z[v] == pz && v > pv))) continue;
                        if (bv < 0 || z[v] > bz) { bz = z[v]; bv = v; }
                    }
                    if (bv < 0) break;
                    float sc = mh.score + (bz - lse);
                    int nctx = 0, nlm = 0;
                    if (root >= 0) {
                        const float delta = hw_step(hw, root, mh.ctx, bv, &nctx, hcnt);
                        sc = sc + delta;
                    }
                    if (use_lm) {
                        const float lp = lm_step(lm, mh.lm, bv, &nlm, lcnt);
                        sc = sc + (lm_alpha * lp);
                    }
                    hyps[n_h++] = (bhyp_t){sc, mh.node, bv, mh.len + 1, after, 1, nctx, nlm};
                    pz = bz; pv = bv;
                }
                float hmax = -INFINITY;
                for (int i = 0; i < n_h; ++i) if (hyps[i].alive && hyps[i].score > hmax) hmax = hyps[i].score;
                int n_good = 0;
                for (int i = 0; i < n_kept; ++i) if (kept[i].score > hmax) ++n_good;
                if (n_good >= beam) {
                    bhyp_t* out = hyps;                             /* hyps is dead from here: reuse it as the sort buffer */
                    pool[cur ^ 1].n = 0;
                    int n_out = 0;
                    for (int i = 0; i < n_kept; ++i) {
                        if (!(kept[i].score > hmax)) continue;
                        int rank = 0;
                        for (int o = 0; o < n_kept; ++o) {
                            if (!(kept[o].score > hmax)) continue;
                            if (kept[o].score < kept[i].score || (kept[o].score == kept[i].score && o < i)) ++rank;
                        }
                        out[rank] = kept[i];
                        ++n_out;
                    }
                    for (int i = 0; i < n_out; ++i) {
                        const float* s0 = pool[cur].v + (size_t)out[i].state * 2 * LH;
                        out[i].state = pool_push(&pool[cur ^ 1], s0, s0 + LH, LH);
                    }
                    memcpy(kept, out, sizeof(bhyp_t) * n_out);
                    n_kept = n_out;
                    cur ^= 1;
                    break;
                }
            }
        }
        pops[b] = n_pops_total;
        nc[0] = failed ? 0 : n_kept;
        for (int r = 0; r < N; ++r) { n_ids[(size_t)b * N + r] = 0; scores[(size_t)b * N + r] = 0.0f; norm_scores[(size_t)b * N + r] = 0.0f; }
        n_hyps[b] = 0;
        if (failed) overflow = 1;
        else {
            /* Finalize, on the kept list's order (which the scores BEFORE it gave) */
            float* before = (float*)malloc(sizeof(float) * n_kept);
            for (int i = 0; i < n_kept; ++i) {
                before[i] = kept[i].score;
                if (root >= 0 && T > 0) {
                    const float delta = -hw->node_score[kept[i].ctx];
                    kept[i].score = kept[i].score + delta;
                    finalize_total[b] = finalize_total[b] + delta;
                }
            }
            char* taken = (char*)calloc(n_kept, 1);
            char* taken0 = (char*)calloc(n_kept, 1);
            char* taken1 = (char*)calloc(n_kept, 1);
            int* order = (int*)malloc(sizeof(int) * n_kept);
            for (int r = 0; r < n_kept; ++r) {                       /* the whole order, for the counters; the first N ranks are written */
                int pick = -1, pick0 = -1, pick1 = -1;
                float pn = 0.0f, pn1 = 0.0f;
                for (int i = 0; i < n_kept; ++i) {
                    const float norm = score_norm ? kept[i].score / (float)kept[i].len : kept[i].score;
                    const float norm1 = score_norm ? before[i] / (float)kept[i].len : before[i];
                    if (!taken[i] && (pick < 0 || norm > pn)) { pick = i; pn = norm; }
                    if (!taken0[i] && (pick0 < 0 || kept[i].score > kept[pick0].score)) pick0 = i;
                    if (!taken1[i] && (pick1 < 0 || norm1 > pn1)) { pick1 = i; pn1 = norm1; }
                }
                taken[pick] = 1; taken0[pick0] = 1; taken1[pick1] = 1;
                order[r] = pick;
                if (pick != pick0) nc[3] = 1;
                if (pick != pick1) nc[5] = 1;
                if (r >= N) continue;
                for (int i = 0; i < n_kept; ++i)
                    if (!taken[i] && (score_norm ? kept[i].score / (float)kept[i].len : kept[i].score) == pn) nc[2] += 1;
                for (int q = 0; q < r; ++q)
                    if (same_labels(nodes, kept[order[q]].node, kept[order[q]].len, kept[pick].node, kept[pick].len)) nc[1] += 1;
                const size_t e = (size_t)b * N + r;
                const int n = kept[pick].len - 1;
                scores[e] = kept[pick].score;
                norm_scores[e] = pn;
                n_hyps[b] += 1;
                if (n > out_cap) { overflow = 1; continue; }
                int node = kept[pick].node;                          /* survivors are always in the trie */
                for (int q = n - 1; q >= 0; --q) {
                    ids[e * out_cap + q] = nodes[node].tok;
                    if (frames) frames[e * out_cap + q] = nodes[node].t;
                    node = nodes[node].parent;
                }
                n_ids[e] = n;
            }
            free(taken); free(taken0); free(taken1); free(order); free(before);
        }
        free(nodes); free(pool[0].v); free(pool[1].v); free(hyps); free(kept);
    }
    free(z); free(g); free(hn); free(cn);
    return overflow ? -5 : 0;
}
