/*
 * k2_mbs_nbest_checker.c — CPU restatement of reazonspeech_amd/csrc/k_rnnt_mbs.hip with the ranked list of rs_rnnt_mbs_nbest, all
 * forms (plain, hotwords, n-gram LM, both), in the device's float32 evaluation order.  TEST INFRASTRUCTURE, built by
 * tests/checker_lib.py with the flags of oracle/build.py and linked against the oracle library.  The search is the text of
 * tests/k2_mbs_lm_checker.c (which states it in full); with nbest = 1 it must equal that checker bit for bit
 * (tests/test_nbest_host.py holds it to that); folding the two into one checker is left for later.
 *
 * The list (include/rs_asr.h rs_rnnt_mbs_nbest): the candidates are the entries of the set the last frame leaves, after merging and
 * after the hotword Finalize, in the order of entry; norm = log_prob / (float)(n + 2) with length_norm, else log_prob; rank r takes
 * the greatest norm among those not yet ranked, of equal norms the one that entered first (strict `>` while walking in the order of
 * entry).  n_hyps = min(nbest, size of the last set); an utterance without frames has n_hyps = 0.  Entries past n_hyps: n_ids = 0.
 * nb_counters per utterance [0..3]: [0] size of the last set, [1] equal norms met while ranking (a remaining entry equal to the one
 * picked), [2] merges in the last frame, [3] 1 if ranking by the norms BEFORE Finalize gives another order than after it.
 *
 * `inject` (may be NULL): the hand-built cases replace decoder and joiner by a table — logits of frame t for a hypothesis whose
 * last token is u (the blank at the start) are inject[(t V + u) V .. + V]; the weights are then not read.
 */
#include <stdlib.h>
#include <string.h>

#include "rnnt_math.h"

float rs_oracle_dot(const float* a, const float* w, int K);
int rs_oracle_joint_argmax(const float* f, const float* g, const float* Wo, const float* bo, int J, int V, float* logits_out);
void rs_oracle_k2_decoder(const float* embed, const float* conv_w, int D, int t0, int t1, float* h);

#define MBS_MAX_K 8
#define MBS_THREADS 256
#define LM_COUNTERS 14

typedef struct {
    int n;          /* tokens after the context */
    int t0, t1;     /* the last two entries of ys */
    float lp;
    int ctx;        /* node of the context graph */
    int lm;         /* node of the language model */
    int32_t* y;     /* [cap] */
    int32_t* fr;    /* [cap] */
    float* g;       /* [J] decoder_proj(decoder(t0, t1)) */
} hyp_t;

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

static float lse_sum(const float* x, int V, float m) {
    float part[MBS_THREADS], tmp[64];
    for (int i = 0; i < MBS_THREADS; ++i) {
        float s = 0.0f;
        for (int v = i; v < V; v += MBS_THREADS) s = s + rs_expf(x[v] - m);
        part[i] = s;
    }
    float wsum[MBS_THREADS / 64];
    for (int w = 0; w < MBS_THREADS / 64; ++w) {
        float* a = part + 64 * w;
        for (int off = 32; off > 0; off >>= 1) {
            for (int l = 0; l < 64; ++l) tmp[l] = a[l] + a[l ^ off];
            memcpy(a, tmp, sizeof tmp);
        }
        wsum[w] = a[0];
    }
    return ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

static int hw_child(const hw_table* g, int n, int tok) {
    for (int c = g->child_begin[n]; c < g->child_begin[n + 1]; ++c)
        if (g->child_tok[c] == tok) return g->child_node[c];
    return -1;
}

/* counters: [0] child hits, [1] fail transitions, [2] non-strict exits */
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

static void hyp_alloc(hyp_t* h, int cap, int J) {
    h->y = (int32_t*)malloc(sizeof(int32_t) * cap);
    h->fr = (int32_t*)malloc(sizeof(int32_t) * cap);
    h->g = (float*)malloc(sizeof(float) * (J > 0 ? J : 1));
}
static void hyp_free(hyp_t* h) { free(h->y); free(h->fr); free(h->g); }

static void hyp_decoder(hyp_t* h, const float* embed, const float* conv_w, const float* Wp, const float* bp, int D, int J, float* hdec) {
    rs_oracle_k2_decoder(embed, conv_w, D, h->t0, h->t1, hdec);
    for (int j = 0; j < J; ++j) h->g[j] = rs_oracle_dot(hdec, Wp + (size_t)j * D, D) + bp[j];
}

/* final_* (may be NULL): the last set of every utterance, in the order of entry — final_n [B], final_len / final_lp / final_lm
 * [B][8], final_y [B][8][out_cap].  hw (may be NULL, or n_graphs 0) with graph_of [B] (may be NULL); lm (may be NULL) with alpha.
 * Returns 0, or -5 if a result has more than out_cap tokens. */
int rs_k2_mbs_nbest_checker(const float* f, const int32_t* enc_lens, int B, int Tp, int J, int D, int V, int blank, int unk,
                         const float* embed, const float* conv_w, const float* Wp, const float* bp, const float* Wo, const float* bo,
                         const float* inject, int K, float blank_penalty, int length_norm, int nbest, int out_cap, int32_t* ids /* [B][nbest][out_cap] */,
                         int32_t* frames, int32_t* n_ids /* [B][nbest] */, float* scores, float* norm_scores, int32_t* n_hyps /* [B] */,
                         int32_t* nb_counters /* [B][4] */, int32_t* merges, int32_t* final_n, int32_t* final_len, float* final_lp,
                         int32_t* final_lm, int32_t* final_y, const hw_table* hw, const int32_t* graph_of,
                         int32_t* hw_counters /* [B][3] */, float* finalize_total /* [B] */, const lm_table* lm, float lm_alpha,
                         int32_t* lm_counters /* [B][LM_COUNTERS] */) {
    if (K < 1 || K > MBS_MAX_K || nbest < 1 || nbest > 8 || nbest > K) return -1;
    const int use_lm = lm != NULL && lm->n_nodes > 0 && lm_alpha != 0.0f;
    const int use_hw = hw != NULL && graph_of != NULL && hw->n_graphs > 0;
    int overflow = 0;
    const int cap = Tp > 0 ? Tp : 1;
    hyp_t set[2][MBS_MAX_K];
    for (int s = 0; s < 2; ++s) for (int k = 0; k < MBS_MAX_K; ++k) hyp_alloc(&set[s][k], cap, J);
    float* lpv = (float*)malloc(sizeof(float) * (size_t)K * V);
    float* hdec = (float*)malloc(sizeof(float) * (D > 0 ? D : 1));
    for (int b = 0; b < B; ++b) {
        int cur = 0, H = 1, n_merge = 0, last_merge = 0;
        const int T = enc_lens[b];
        const int gi = use_hw ? graph_of[b] : -1;
        const int root = (gi >= 0 && gi < hw->n_graphs) ? hw->graph_root[gi] : -1;
        int32_t* hcnt = hw_counters + 3 * b;
        int32_t* lcnt = lm_counters + LM_COUNTERS * b;
        hcnt[0] = hcnt[1] = hcnt[2] = 0;
        for (int k = 0; k < LM_COUNTERS; ++k) lcnt[k] = 0;
        finalize_total[b] = 0.0f;
        {
            hyp_t* h0 = &set[0][0];
            h0->n = 0; h0->t0 = -1; h0->t1 = blank; h0->lp = 0.0f;
            h0->ctx = root < 0 ? 0 : root;
            h0->lm = use_lm ? ((lm->start >= 0 && lm->start < lm->n_nodes) ? lm->start : 0) : 0;
            if (!inject) hyp_decoder(h0, embed, conv_w, Wp, bp, D, J, hdec);
        }
        for (int t = 0; t < T; ++t) {
            hyp_t* old = set[cur];
            hyp_t* nw = set[cur ^ 1];
            for (int h = 0; h < H; ++h) {
                float* x = lpv + (size_t)h * V;
                if (inject) memcpy(x, inject + ((size_t)t * V + old[h].t1) * V, sizeof(float) * V);
                else rs_oracle_joint_argmax(f + ((size_t)b * Tp + t) * J, old[h].g, Wo, bo, J, V, x);
                if (blank_penalty > 0.0f) x[blank] = x[blank] - blank_penalty;
                float m = -INFINITY;
                for (int v = 0; v < V; ++v) if (x[v] > m) m = x[v];
                const float lg = rs_logf(lse_sum(x, V, m));
                for (int v = 0; v < V; ++v) x[v] = ((x[v] - m) - lg) + old[h].lp;
            }
            /* the K best by (value desc, flat index asc): no bonus, no LM term */
            int sel[MBS_MAX_K], n_cand = 0;
            const int total = H * V;
            for (int j = 0; j < K && j < total; ++j) {
                int best = -1;
                for (int c = 0; c < total; ++c) {
                    int taken = 0;
                    for (int q = 0; q < n_cand; ++q) taken |= sel[q] == c;
                    if (taken) continue;
                    if (best < 0 || lpv[c] > lpv[best]) best = c;
                }
                sel[n_cand++] = best;
            }
            /* every candidate is scored whole before any merge: the hotword step, then the LM step */
            float clp[MBS_MAX_K];
            int cctx[MBS_MAX_K], clm[MBS_MAX_K];
            for (int j = 0; j < n_cand; ++j) {
                const int h = sel[j] / V, v = sel[j] - h * V;
                clp[j] = lpv[sel[j]];
                cctx[j] = old[h].ctx;
                clm[j] = old[h].lm;
                if (v == blank || v == unk) continue;
                if (root >= 0) {
                    int nx = root;
                    const float delta = hw_step(hw, root, old[h].ctx, v, &nx, hcnt);
                    clp[j] = clp[j] + delta;
                    cctx[j] = nx;
                }
                if (use_lm) {
                    int ln = 0;
                    const float l = lm_step(lm, old[h].lm, v, &ln, lcnt);
                    clp[j] = clp[j] + (lm_alpha * l);
                    clm[j] = ln;
                }
            }
            int nn = 0;
            const int merge_before = n_merge;
            for (int j = 0; j < n_cand; ++j) {
                const int h = sel[j] / V, v = sel[j] - h * V;
                const int tok = (v != blank && v != unk) ? v : -1;
                const int n = old[h].n + (tok >= 0 ? 1 : 0);
                const float lp = clp[j];
                int merged = 0;
                for (int e = 0; e < nn && !merged; ++e) {
                    if (nw[e].n != n) continue;
                    int same = 1;
                    for (int q = 0; q < n && same; ++q) same = nw[e].y[q] == (q < old[h].n ? old[h].y[q] : tok);
                    if (!same) continue;
                    nw[e].lp = rs_logaddexpf(nw[e].lp, lp);
                    if (use_lm && nw[e].lm != clm[j]) lcnt[12] += 1;
                    merged = 1;
                    n_merge += 1;
                }
                if (merged) continue;
                hyp_t* d = &nw[nn++];
                memcpy(d->y, old[h].y, sizeof(int32_t) * old[h].n);
                memcpy(d->fr, old[h].fr, sizeof(int32_t) * old[h].n);
                d->n = n; d->lp = lp; d->t0 = old[h].t0; d->t1 = old[h].t1; d->ctx = cctx[j]; d->lm = clm[j];
                if (tok >= 0) {
                    d->y[n - 1] = tok; d->fr[n - 1] = t;
                    d->t0 = old[h].t1; d->t1 = tok;
                    if (!inject) hyp_decoder(d, embed, conv_w, Wp, bp, D, J, hdec);
                } else if (!inject) {
                    memcpy(d->g, old[h].g, sizeof(float) * J);
                }
            }
            cur ^= 1;
            H = nn;
            last_merge = n_merge - merge_before;
        }
        hyp_t* fin = set[cur];
        float before[MBS_MAX_K], norm[MBS_MAX_K];
        for (int k = 0; k < H; ++k) before[k] = length_norm ? fin[k].lp / (float)(fin[k].n + 2) : fin[k].lp;
        if (root >= 0 && T > 0)
            for (int k = 0; k < H; ++k) {                    /* Finalize */
                const float delta = -hw->node_score[fin[k].ctx];
                fin[k].lp = fin[k].lp + delta;
                finalize_total[b] = finalize_total[b] + delta;
                fin[k].ctx = root;
            }
        for (int k = 0; k < H; ++k) norm[k] = length_norm ? fin[k].lp / (float)(fin[k].n + 2) : fin[k].lp;
        int32_t* nc = nb_counters + 4 * b;
        nc[0] = T > 0 ? H : 0; nc[1] = 0; nc[2] = T > 0 ? last_merge : 0; nc[3] = 0;
        for (int r = 0; r < nbest; ++r) n_ids[(size_t)b * nbest + r] = 0;
        n_hyps[b] = 0;
        if (T > 0) {
            int taken[MBS_MAX_K] = {0}, taken0[MBS_MAX_K] = {0};
            for (int r = 0; r < H; ++r) {                    /* the whole order, for the counters; the first nbest ranks are written */
                int pick = -1, pick0 = -1;
                for (int k = 0; k < H; ++k) {
                    if (!taken[k] && (pick < 0 || norm[k] > norm[pick])) pick = k;
                    if (!taken0[k] && (pick0 < 0 || before[k] > before[pick0])) pick0 = k;
                }
                taken[pick] = 1; taken0[pick0] = 1;
                if (pick != pick0) nc[3] = 1;
                if (r >= nbest) continue;
                for (int k = 0; k < H; ++k) if (!taken[k] && norm[k] == norm[pick]) nc[1] += 1;
                const size_t e = (size_t)b * nbest + r;
                int n = fin[pick].n;
                if (n > out_cap) { n = out_cap; overflow = 1; }
                memcpy(ids + e * out_cap, fin[pick].y, sizeof(int32_t) * n);
                memcpy(frames + e * out_cap, fin[pick].fr, sizeof(int32_t) * n);
                n_ids[e] = n; scores[e] = fin[pick].lp; norm_scores[e] = norm[pick];
                n_hyps[b] += 1;
            }
        }
        merges[b] = n_merge;
        if (final_n) {
            final_n[b] = H;
            for (int k = 0; k < H; ++k) {
                final_len[b * MBS_MAX_K + k] = fin[k].n;
                final_lp[b * MBS_MAX_K + k] = fin[k].lp;
                final_lm[b * MBS_MAX_K + k] = fin[k].lm;
                const int m = fin[k].n < out_cap ? fin[k].n : out_cap;
                memcpy(final_y + ((size_t)b * MBS_MAX_K + k) * out_cap, fin[k].y, sizeof(int32_t) * m);
            }
        }
    }
    for (int s = 0; s < 2; ++s) for (int k = 0; k < MBS_MAX_K; ++k) hyp_free(&set[s][k]);
    free(lpv); free(hdec);
    return overflow ? -5 : 0;
}
