/*
 * k2_mbs_checker.c — CPU restatement of reazonspeech_amd/csrc/k_rnnt_mbs.hip (rs_rnnt_mbs, rs_rnnt_mbs_hotwords): sherpa-onnx's
 * modified_beam_search over icefall's stateless decoder and tanh joiner, without and with hotwords (contextual biasing), in the
 * device's float32 evaluation order.  The one modified-beam-search checker of the tests.  TEST INFRASTRUCTURE, built by
 * tests/checker_lib.py with the flags of oracle/build.py and linked against the oracle library, whose routines compute the decoder
 * (rs_oracle_k2_decoder), decoder_proj (rs_oracle_dot) and the joint logits (rs_oracle_joint_argmax with logits_out; the caller
 * sets the joint activation to tanh) — this file holds the search only.
 *
 * [UPSTREAM, not vendored; PARITY UNPINNED] OfflineTransducerModifiedBeamSearchDecoder::Decode without LM, Hypotheses::Add,
 * GetMostProbable(length_norm).  Per utterance: one starting hypothesis ys = [-1, blank], log_prob 0; per frame t, for the H <= K
 * hypotheses of the set: logits[h] (blank logit - blank_penalty when the penalty is > 0),
 * lp[h][v] = ((logits[h][v] - max) - log(sum)) + log_prob[h]; the K largest of the H V values (equal values: the lower flat
 * index h V + v first) in descending order: copy h, append v / t unless v is the blank or <unk>, log_prob = lp[h][v]; a
 * hypothesis whose token sequence equals one already in the new set is merged into it (rs_logaddexpf(old, new), first
 * tokens / timestamps stay).  Winner: the largest log_prob / (float)(tokens + 2) (or log_prob without length normalisation);
 * equal scores: the one that entered the last set first.
 *
 * The log-softmax reduction, written down: the device's selection kernel has 256 threads = 4 waves of 64; thread i owns the
 * columns v = i + 256 q.
 *   max      exact in any order
 *   s_i      = chain over q ascending of s = s + rs_expf(x[i + 256 q] - max), from 0   (0 for a thread without columns)
 *   wave w   : lanes l = 0..63 hold s_(64 w + l); for off = 32, 16, 8, 4, 2, 1: every lane l takes s_l + s_(l xor off); lane 0
 *              is the wave's sum
 *   sum      = ((wave0 + wave1) + wave2) + wave3
 *
 * Hotwords.  [UPSTREAM, not vendored; PARITY UNPINNED] ContextGraph::ForwardOneStep(strict_mode = false) and Finalize as Decode uses
 * them; the specification is in include/rs_asr.h (rs_rnnt_mbs_hotwords).  The graph arrives as the flat table the device reads (all
 * graphs concatenated; graph_of[b] = -1, or no table: the utterance has none and none of the statements below runs for it).  Every
 * hypothesis carries a node; the K best are selected WITHOUT bonus; each selected candidate that appends a label v walks once,
 * before the merge:
 *   state has a child n on v:  score = token_score[n]
 *   else: n = fail[state]; while n has no child on v and n is not the root: n = fail[n]; n = its child on v if any;
 *         score = node_score[n] - node_score[state]
 *   output_score[n] != 0:  out = is_end[n] ? node_score[n] : output[n] >= 0 ? node_score[output[n]] : node_score[n];
 *                          delta = (score + out) - node_score[n]; next = root                        (the non-strict exit)
 *   else:                  delta = score + output_score[n]; next = n
 *   log_prob = lp + delta.  A merged candidate adds its log_prob (bonus inside) by rs_logaddexpf; the first entry's state stays.
 * After the last frame: log_prob = log_prob + (-node_score[state]) for every entry of the final set, then the winner.
 * Counters per utterance (how the batch exercised the graph): child hits, fail transitions (steps that left `state` through its
 * fail link), non-strict exits, and the sum of the Finalize deltas over the final set.
 */
#include <stdlib.h>
#include <string.h>

#include "rnnt_math.h"

float rs_oracle_dot(const float* a, const float* w, int K);
int rs_oracle_joint_argmax(const float* f, const float* g, const float* Wo, const float* bo, int J, int V, float* logits_out);
void rs_oracle_k2_decoder(const float* embed, const float* conv_w, int D, int t0, int t1, float* h);

#define MBS_MAX_K 8
#define MBS_THREADS 256

typedef struct {
    int n;          /* tokens after the context */
    int t0, t1;     /* the last two entries of ys */
    float lp;
    int ctx;        /* node of the context graph */
    int32_t* y;     /* [cap] */
    int32_t* fr;    /* [cap] */
    float* g;       /* [J] decoder_proj(decoder(t0, t1)) */
} hyp_t;

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

typedef struct {
    const int32_t *child_begin, *child_tok, *child_node, *fail, *output, *is_end;
    const float *token_score, *node_score, *output_score;
} hw_table;

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

static void hyp_alloc(hyp_t* h, int cap, int J) {
    h->y = (int32_t*)malloc(sizeof(int32_t) * cap);
    h->fr = (int32_t*)malloc(sizeof(int32_t) * cap);
    h->g = (float*)malloc(sizeof(float) * J);
}
static void hyp_free(hyp_t* h) { free(h->y); free(h->fr); free(h->g); }

/* final_* (may be NULL): the last set of every utterance, in the order of entry — final_n [B], final_len / final_lp [B][8],
 * final_y [B][8][out_cap].  Returns 0, or -5 if a result has more than out_cap tokens. */
int rs_k2_mbs_checker(const float* f, const int32_t* enc_lens, int B, int Tp, int J, int D, int V, int blank, int unk,
                      const float* embed, const float* conv_w, const float* Wp, const float* bp, const float* Wo, const float* bo,
                      int K, float blank_penalty, int length_norm, int out_cap, int32_t* ids, int32_t* frames, int32_t* n_ids,
                      float* scores, int32_t* merges, int32_t* final_n, int32_t* final_len, float* final_lp, int32_t* final_y,
                      const int32_t* child_begin, const int32_t* child_tok, const int32_t* child_node, const int32_t* hw_fail,
                      const int32_t* hw_output, const int32_t* is_end, const float* token_score, const float* node_score,
                      const float* output_score, const int32_t* graph_root, int n_graphs, const int32_t* graph_of,
                      int32_t* hw_counters /* [B][3] */, float* finalize_total /* [B] */) {
    const hw_table G = {child_begin, child_tok, child_node, hw_fail, hw_output, is_end, token_score, node_score, output_score};
    if (K < 1 || K > MBS_MAX_K) return -1;
    int overflow = 0;
    const int cap = Tp > 0 ? Tp : 1;
    hyp_t set[2][MBS_MAX_K];
    for (int s = 0; s < 2; ++s) for (int k = 0; k < MBS_MAX_K; ++k) hyp_alloc(&set[s][k], cap, J);
    float* lpv = (float*)malloc(sizeof(float) * (size_t)K * V);
    float* hdec = (float*)malloc(sizeof(float) * D);
    for (int b = 0; b < B; ++b) {
        int cur = 0, H = 1, n_merge = 0;
        const int T = enc_lens[b];
        const int gi = graph_of ? graph_of[b] : -1;
        const int root = (gi >= 0 && gi < n_graphs) ? graph_root[gi] : -1;
        hw_counters[3 * b] = hw_counters[3 * b + 1] = hw_counters[3 * b + 2] = 0;
        finalize_total[b] = 0.0f;
        set[0][0].ctx = root < 0 ? 0 : root;
        {
            hyp_t* h0 = &set[0][0];
            h0->n = 0; h0->t0 = -1; h0->t1 = blank; h0->lp = 0.0f;
            rs_oracle_k2_decoder(embed, conv_w, D, h0->t0, h0->t1, hdec);
            for (int j = 0; j < J; ++j) h0->g[j] = rs_oracle_dot(hdec, Wp + (size_t)j * D, D) + bp[j];
        }
        for (int t = 0; t < T; ++t) {
            hyp_t* old = set[cur];
            hyp_t* nw = set[cur ^ 1];
            for (int h = 0; h < H; ++h) {
                float* x = lpv + (size_t)h * V;
                rs_oracle_joint_argmax(f + ((size_t)b * Tp + t) * J, old[h].g, Wo, bo, J, V, x);
                if (blank_penalty > 0.0f) x[blank] = x[blank] - blank_penalty;
                float m = -INFINITY;
                for (int v = 0; v < V; ++v) if (x[v] > m) m = x[v];
                const float lg = rs_logf(lse_sum(x, V, m));
                for (int v = 0; v < V; ++v) x[v] = ((x[v] - m) - lg) + old[h].lp;
            }
            /* the K best by (value desc, flat index asc) */
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
            /* hotwords: every candidate walks before any merge */
            float clp[MBS_MAX_K];
            int cctx[MBS_MAX_K];
            for (int j = 0; j < n_cand; ++j) {
                const int h = sel[j] / V, v = sel[j] - h * V;
                clp[j] = lpv[sel[j]];
                cctx[j] = old[h].ctx;
                if (root >= 0 && v != blank && v != unk) {
                    int nx = root;
                    const float delta = hw_step(&G, root, old[h].ctx, v, &nx, hw_counters + 3 * b);
                    clp[j] = clp[j] + delta;
                    cctx[j] = nx;
                }
            }
            int nn = 0;
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
                    merged = 1;
                    n_merge += 1;
                }
                if (merged) continue;
                hyp_t* d = &nw[nn++];
                memcpy(d->y, old[h].y, sizeof(int32_t) * old[h].n);
                memcpy(d->fr, old[h].fr, sizeof(int32_t) * old[h].n);
                d->n = n; d->lp = lp; d->t0 = old[h].t0; d->t1 = old[h].t1; d->ctx = cctx[j];
                if (tok >= 0) {
                    d->y[n - 1] = tok; d->fr[n - 1] = t;
                    d->t0 = old[h].t1; d->t1 = tok;
                    rs_oracle_k2_decoder(embed, conv_w, D, d->t0, d->t1, hdec);
                    for (int j2 = 0; j2 < J; ++j2) d->g[j2] = rs_oracle_dot(hdec, Wp + (size_t)j2 * D, D) + bp[j2];
                } else {
                    memcpy(d->g, old[h].g, sizeof(float) * J);
                }
            }
            cur ^= 1;
            H = nn;
        }
        hyp_t* fin = set[cur];
        if (root >= 0 && T > 0)
            for (int k = 0; k < H; ++k) {                    /* Finalize */
                const float delta = -node_score[fin[k].ctx];
                fin[k].lp = fin[k].lp + delta;
                finalize_total[b] = finalize_total[b] + delta;
                fin[k].ctx = root;
            }
        int win = 0;
        float win_norm = 0.0f;
        for (int k = 0; k < H; ++k) {
            const float norm = length_norm ? fin[k].lp / (float)(fin[k].n + 2) : fin[k].lp;
            if (k == 0 || norm > win_norm) { win = k; win_norm = norm; }
        }
        int n = fin[win].n;
        if (n > out_cap) { n = out_cap; overflow = 1; }
        memcpy(ids + (size_t)b * out_cap, fin[win].y, sizeof(int32_t) * n);
        memcpy(frames + (size_t)b * out_cap, fin[win].fr, sizeof(int32_t) * n);
        n_ids[b] = n;
        scores[b] = fin[win].lp;
        merges[b] = n_merge;
        if (final_n) {
            final_n[b] = H;
            for (int k = 0; k < H; ++k) {
                final_len[b * MBS_MAX_K + k] = fin[k].n;
                final_lp[b * MBS_MAX_K + k] = fin[k].lp;
                const int m = fin[k].n < out_cap ? fin[k].n : out_cap;
                memcpy(final_y + ((size_t)b * MBS_MAX_K + k) * out_cap, fin[k].y, sizeof(int32_t) * m);
            }
        }
    }
    for (int s = 0; s < 2; ++s) for (int k = 0; k < MBS_MAX_K; ++k) hyp_free(&set[s][k]);
    free(lpv); free(hdec);
    return overflow ? -5 : 0;
}
