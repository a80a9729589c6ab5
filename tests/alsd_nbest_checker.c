/*
 * alsd_nbest_checker.c — CPU restatement of reazonspeech_amd/csrc/k_rnnt_alsd.hip with the ranked list of rs_rnnt_alsd_nbest, all
 * forms (plain, hotwords, n-gram LM, both; merge on and off), in the device's float32 evaluation order.  TEST INFRASTRUCTURE, built by
 * tests/checker_lib.py with the flags of oracle/build.py and linked against the oracle library.  The search is the text of
 * tests/alsd_checker.c (which states it in full); with nbest = 1 it must equal that checker bit for bit (tests/test_nbest_alsd_host.py
 * holds it to that); folding the two into one checker is left for later.
 *
 * The list (include/rs_asr.h rs_rnnt_alsd_nbest) stands in place of the single best finished hypothesis.  A hypothesis finishes when
 * it takes the blank at its utterance's last frame; its score is read after the step's recombination, then Finalize under hotwords;
 * norm = sc / (float)(n + 1) with score_norm, else sc.  Offered in beam-slot order within a step:
 *   1. an entry with the same labels (it can only have entered in this step): the greater norm stays, the first on a tie;
 *   2. the candidate enters below every entry whose norm is >= its own; a full list drops its last entry (or refuses a candidate
 *      that would be last).
 * Nothing finished (budget spent, no frames): every beam entry is offered the same way, after Finalize.  n_hyps = entries.
 * nb_counters per utterance [0..6]: [0] hypotheses offered, [1] evictions from the tail + candidates refused by a full list,
 * [2] offers that met an entry with equal labels, [3] of those, the ones whose greater norm replaced the entry, [4] candidates that
 * entered directly below an entry of EQUAL norm from an EARLIER step, [5] 1 if nothing finished (the budget exit), [6] 1 if ranking
 * the final entries by their norms BEFORE Finalize gives another order.
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

#define MAX_BEAM 8

#define LM_COUNTERS 14

typedef struct {
    int n;          /* labels emitted */
    float score;
    int state;      /* node of the context graph */
    int lm;         /* node of the language model */
    int* y;         /* [cap] */
    int* steps;     /* [cap] alignment index of each label */
    float* h;       /* [L][H] */
    float* c;
    float* g;       /* [J] */
} hyp_t;

typedef struct { float score; int parent; int tok; int state; int lm; } cand_t;

typedef struct {
    const int32_t *child_begin, *child_tok, *child_node, *root_child, *suffix, *level;
    const float *logp, *backoff;
    int order;
    float unk_logp;
} lm_table;

static int lm_child(const lm_table* g, int n, int tok) {
    for (int c = g->child_begin[n]; c < g->child_begin[n + 1]; ++c)
        if (g->child_tok[c] == tok) return g->child_node[c];
    return -1;
}

static float lm_step(const lm_table* g, int state, int tok, int* next, int32_t* cnt) {
    int n = state, c = -1;
    float acc = 0.0f;
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

typedef struct {
    const int32_t *child_begin, *child_tok, *child_node, *fail, *output, *is_end;
    const float *token_score, *node_score, *output_score;
} hw_table;

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

static hyp_t* hyps_new(int n, int cap, int L, int H, int J) {
    hyp_t* a = (hyp_t*)calloc(n, sizeof(hyp_t));
    for (int i = 0; i < n; ++i) {
        a[i].y = (int*)malloc(sizeof(int) * (cap + 1));
        a[i].steps = (int*)malloc(sizeof(int) * (cap + 1));
        a[i].h = (float*)malloc(sizeof(float) * L * H);
        a[i].c = (float*)malloc(sizeof(float) * L * H);
        a[i].g = (float*)malloc(sizeof(float) * J);
    }
    return a;
}
static void hyps_free(hyp_t* a, int n) {
    for (int i = 0; i < n; ++i) { free(a[i].y); free(a[i].steps); free(a[i].h); free(a[i].c); free(a[i].g); }
    free(a);
}

static int cand_len(const hyp_t* cur, const cand_t* c) { return cur[c->parent].n + (c->tok >= 0); }
static int cand_label(const hyp_t* cur, const cand_t* c, int q) { return q < cur[c->parent].n ? cur[c->parent].y[q] : c->tok; }
static int cand_equal(const hyp_t* cur, const cand_t* a, const cand_t* b) {
    const int n = cand_len(cur, a);
    if (n != cand_len(cur, b)) return 0;
    for (int q = 0; q < n; ++q) if (cand_label(cur, a, q) != cand_label(cur, b, q)) return 0;
    return 1;
}

static void pred_step(const float* x, const hyp_t* p, hyp_t* q, int L, int H, int J, const float* const* lstm_w,
                      const float* const* lstm_b, const float* Wp, const float* bp, const float* h0, const float* c0) {
    for (int l = 0; l < L; ++l) {
        rs_oracle_lstm_step(x, (p ? p->h : h0) + l * H, (p ? p->c : c0) + l * H, lstm_w[l], lstm_b[l], H, q->h + l * H, q->c + l * H);
        x = q->h + l * H;
    }
    for (int j = 0; j < J; ++j) q->g[j] = rs_oracle_dot(q->h + (L - 1) * H, Wp + (size_t)j * H, H) + bp[j];
}

/* beam_* (may be NULL): the beam as the search left it — beam_n [B], beam_len / beam_state [B][8], beam_score [B][8],
 * beam_y [B][8][out_cap].  Returns 0, -1 for a bad beam size, -5 when a result did not fit out_cap (it is truncated). */
typedef struct { int n, step; float score, norm, before; int *y, *steps; } nb_entry;

/* offer a hypothesis to the list `e[0 .. *cnt - 1]` (best first, at most nbest); `step`: the alignment step of the offer */
static void nb_offer(nb_entry* e, int* cnt, int nbest, const int* y, const int* steps, int n, float sc, float norm, float before, int step,
                     int32_t* nc) {
    nc[0] += 1;
    for (int r = 0; r < *cnt; ++r) {
        if (e[r].n != n || memcmp(e[r].y, y, sizeof(int) * n) != 0) continue;
        nc[2] += 1;
        if (!(norm > e[r].norm)) return;
        nc[3] += 1;
        nb_entry gone = e[r];
        for (int k = r; k + 1 < *cnt; ++k) e[k] = e[k + 1];
        e[*cnt - 1] = gone;                                   /* (keeps its buffers for reuse) */
        *cnt -= 1;
        break;
    }
    int pos = 0;
    for (int r = 0; r < *cnt; ++r) if (e[r].norm >= norm) ++pos;
    if (pos >= nbest) { nc[1] += 1; return; }
    if (*cnt == nbest) { nc[1] += 1; *cnt -= 1; }             /* the tail leaves */
    nb_entry slot = e[*cnt];                                  /* a free record (its buffers) */
    for (int k = *cnt; k > pos; --k) e[k] = e[k - 1];
    e[pos] = slot;
    e[pos].n = n; e[pos].step = step; e[pos].score = sc; e[pos].norm = norm; e[pos].before = before;
    memcpy(e[pos].y, y, sizeof(int) * n);
    memcpy(e[pos].steps, steps, sizeof(int) * n);
    *cnt += 1;
    if (pos > 0 && e[pos - 1].norm == norm && e[pos - 1].step < step) nc[4] += 1;
}

int rs_alsd_nbest_checker(const float* f, const int32_t* enc_lens, int B, int Tp, int J, int H, int L, int V, int blank,
                             const float* embed, const float* const* lstm_w, const float* const* lstm_b, const float* Wp,
                             const float* bp, const float* Wo, const float* bo, int beam, const int32_t* u_max, int score_norm,
                             int merge, int nbest, int out_cap, int32_t* ids /* [B][nbest][out_cap] */, int32_t* steps,
                             int32_t* n_ids /* [B][nbest] */, float* scores, float* norm_scores, int32_t* n_hyps /* [B] */,
                             int32_t* nb_counters /* [B][7] */,
                             const int32_t* child_begin, const int32_t* child_tok, const int32_t* child_node, const int32_t* hw_fail,
                             const int32_t* hw_output, const int32_t* is_end, const float* token_score, const float* node_score,
                             const float* output_score, const int32_t* graph_root, int n_graphs, const int32_t* graph_of,
                             int32_t* hw_counters /* [B][6] */, float* finalize /* [B] */, const float* inject,
                             int32_t* beam_n, int32_t* beam_len, int32_t* beam_state, float* beam_score, int32_t* beam_y,
                             const int32_t* lm_child_begin, const int32_t* lm_child_tok, const int32_t* lm_child_node,
                             const int32_t* lm_root_child, const float* lm_logp, const float* lm_backoff, const int32_t* lm_suffix,
                             const int32_t* lm_level, int lm_nodes, int lm_order, int lm_start, float lm_unk_logp, float lm_alpha,
                             int32_t* lm_counters /* [B][LM_COUNTERS] */, int32_t* beam_lm /* [B][8], may be NULL */) {
    const lm_table M = {lm_child_begin, lm_child_tok, lm_child_node, lm_root_child, lm_suffix, lm_level, lm_logp, lm_backoff, lm_order, lm_unk_logp};
    const int use_lm = lm_nodes > 0 && lm_alpha != 0.0f;
    const hw_table G = {child_begin, child_tok, child_node, hw_fail, hw_output, is_end, token_score, node_score, output_score};
    int overflow = 0;
    if (beam > V - 1) beam = V - 1;
    if (beam < 1 || beam > MAX_BEAM || nbest < 1 || nbest > 8 || nbest > beam) return -1;
    float* z = (float*)malloc(sizeof(float) * V);
    float* hn = (float*)calloc((size_t)L * H, sizeof(float));
    float* cn = (float*)calloc((size_t)L * H, sizeof(float));
    cand_t cands[MAX_BEAM * (MAX_BEAM + 1)], sel[MAX_BEAM];
    int sel_src[MAX_BEAM], dup[MAX_BEAM];
    for (int b = 0; b < B; ++b) {
        const int T = enc_lens[b], n_steps = T + u_max[b];
        const int cap = n_steps > 0 ? n_steps : 1;
        const int gi = graph_of ? graph_of[b] : -1;
        const int root = (gi >= 0 && gi < n_graphs) ? graph_root[gi] : -1;
        int32_t* cnt = hw_counters + 6 * b;
        for (int k = 0; k < 6; ++k) cnt[k] = 0;
        int32_t* lcnt = lm_counters + LM_COUNTERS * b;
        for (int k = 0; k < LM_COUNTERS; ++k) lcnt[k] = 0;
        finalize[b] = 0.0f;
        hyp_t* cur = hyps_new(beam, cap, L, H, J);
        hyp_t* nxt = hyps_new(beam, cap, L, H, J);
        nb_entry list[9];
        int n_list = 0;
        for (int k = 0; k < 9; ++k) { list[k].y = (int*)malloc(sizeof(int) * (cap + 1)); list[k].steps = (int*)malloc(sizeof(int) * (cap + 1)); }
        int32_t* nc = nb_counters + 7 * b;
        for (int k = 0; k < 7; ++k) nc[k] = 0;
        int n_cur = 1;
        cur[0].n = 0; cur[0].score = 0.0f; cur[0].state = root < 0 ? 0 : root; cur[0].lm = use_lm ? lm_start : 0;
        if (!inject) pred_step(embed + (size_t)blank * H, NULL, &cur[0], L, H, J, lstm_w, lstm_b, Wp, bp, hn, cn);
        for (int i = 0; i < n_steps; ++i) {
            int n_c = 0, any_live = 0;
            for (int s = 0; s < n_cur; ++s) {
                const int t = i - cur[s].n;
                if (t > T - 1) continue;
                any_live = 1;
                if (inject) memcpy(z, inject + ((size_t)t * V + (cur[s].n ? cur[s].y[cur[s].n - 1] + 1 : 0)) * V, sizeof(float) * V);
                else rs_oracle_joint_argmax(f + ((size_t)b * Tp + t) * J, cur[s].g, Wo, bo, J, V, z);
                const float lse = rs_oracle_lse(z, V);
                cands[n_c].score = cur[s].score + (z[blank] - lse);
                cands[n_c].parent = s; cands[n_c].tok = -1; cands[n_c].state = cur[s].state; cands[n_c].lm = cur[s].lm;
                ++n_c;
                float pz = INFINITY; int pv = -1;          /* previous pick in the (z desc, v asc) order */
                for (int j = 0; j < beam; ++j) {
                    float bz = -INFINITY; int bv = -1;
                    for (int v = 0; v < V; ++v) {
                        if (v == blank) continue;
                        if (!(z[v] < pz || (z[v] == pz && v > pv))) continue;
                        if (bv < 0 || z[v] > bz) { bz = z[v]; bv = v; }
                    }
                    if (bv < 0) break;
                    float sc = cur[s].score + (bz - lse);
                    int nx = 0;
                    if (root >= 0) {
                        const float delta = hw_step(&G, root, cur[s].state, bv, &nx, cnt);
                        sc = sc + delta;
                    }
                    int ln = 0;
                    if (use_lm) {
                        const float lp = lm_step(&M, cur[s].lm, bv, &ln, lcnt);
                        sc = sc + (lm_alpha * lp);
                    }
                    cands[n_c].score = sc;
                    cands[n_c].parent = s; cands[n_c].tok = bv; cands[n_c].state = nx; cands[n_c].lm = ln;
                    ++n_c;
                    pz = bz; pv = bv;
                }
            }
            if (!any_live) break;
            /* the `beam` best candidates by their boosted scores, ties in expansion order */
            int n_sel = 0;
            for (int c = 0; c < n_c; ++c) {
                int rank = 0;
                for (int o = 0; o < n_c; ++o)
                    if (cands[o].score > cands[c].score || (cands[o].score == cands[c].score && o < c)) ++rank;
                if (rank < beam) { sel[rank] = cands[c]; sel_src[rank] = c; if (rank + 1 > n_sel) n_sel = rank + 1; }
            }
            /* recombination: the first occurrence's labels, steps and state stay */
            for (int j = 0; j < n_sel; ++j) {
                dup[j] = 0;
                for (int k = 0; k < j; ++k)
                    if (!dup[k] && cand_equal(cur, &sel[k], &sel[j])) {
                        sel[k].score = rs_logaddexpf(sel[k].score, sel[j].score);
                        dup[j] = 1;
                        cnt[4] += 1;
                        if (root >= 0 && sel[k].state != sel[j].state) cnt[5] += 1;
                        lcnt[12] += 1;
                        if (use_lm && sel[k].lm != sel[j].lm) lcnt[13] += 1;
                        break;
                    }
            }
            /* finished hypotheses: blank taken at the last frame (score after recombination, then Finalize) */
            for (int c = 0; c < n_c; ++c) {
                if (cands[c].tok >= 0 || i - cur[cands[c].parent].n != T - 1) continue;
                float sc = cands[c].score;
                for (int j = 0; j < n_sel; ++j) if (sel_src[j] == c) sc = sel[j].score;
                float delta = 0.0f;
                if (root >= 0) {
                    delta = -node_score[cands[c].state];
                    sc = sc + delta;
                    if (delta != 0.0f) cnt[3] += 1;
                }
                const hyp_t* p = &cur[cands[c].parent];
                const float norm = score_norm ? sc / (float)(p->n + 1) : sc;
                const float raw = sc - delta;
                nb_offer(list, &n_list, nbest, p->y, p->steps, p->n, sc, norm, score_norm ? raw / (float)(p->n + 1) : raw, i, nc);
            }
            /* the new beam */
            int n_nxt = 0;
            for (int j = 0; j < n_sel; ++j) {
                if (merge && dup[j]) continue;
                const hyp_t* p = &cur[sel[j].parent];
                hyp_t* q = &nxt[n_nxt++];
                q->n = p->n; q->score = sel[j].score; q->state = root >= 0 ? sel[j].state : 0; q->lm = sel[j].lm;
                memcpy(q->y, p->y, sizeof(int) * p->n);
                memcpy(q->steps, p->steps, sizeof(int) * p->n);
                if (sel[j].tok < 0) {
                    memcpy(q->h, p->h, sizeof(float) * L * H);
                    memcpy(q->c, p->c, sizeof(float) * L * H);
                    memcpy(q->g, p->g, sizeof(float) * J);
                } else {
                    q->y[q->n] = sel[j].tok; q->steps[q->n] = i; q->n += 1;
                    if (!inject) pred_step(embed + (size_t)sel[j].tok * H, p, q, L, H, J, lstm_w, lstm_b, Wp, bp, NULL, NULL);
                }
            }
            hyp_t* tmp = cur; cur = nxt; nxt = tmp;
            n_cur = n_nxt;
        }
        if (n_list == 0) {                                      /* nothing finished: the beam's entries, after Finalize */
            nc[5] = 1;
            for (int s = 0; s < n_cur; ++s) {
                float sc = cur[s].score, delta = 0.0f;
                if (root >= 0) {
                    delta = -node_score[cur[s].state];
                    sc = sc + delta;
                    if (delta != 0.0f) cnt[3] += 1;
                }
                const float norm = score_norm ? sc / (float)(cur[s].n + 1) : sc;
                nb_offer(list, &n_list, nbest, cur[s].y, cur[s].steps, cur[s].n, sc, norm, score_norm ? cur[s].score / (float)(cur[s].n + 1) : cur[s].score,
                         n_steps, nc);
            }
        }
        for (int r = 0; r + 1 < n_list; ++r) if (list[r].before < list[r + 1].before) nc[6] = 1;
        n_hyps[b] = n_list;
        for (int r = 0; r < nbest; ++r) {
            const size_t e = (size_t)b * nbest + r;
            n_ids[e] = 0; scores[e] = 0.0f; norm_scores[e] = 0.0f;
            if (r >= n_list) continue;
            int n = list[r].n;
            if (n > out_cap) { n = out_cap; overflow = 1; }
            for (int q = 0; q < n; ++q) { ids[e * out_cap + q] = list[r].y[q]; steps[e * out_cap + q] = list[r].steps[q]; }
            n_ids[e] = n; scores[e] = list[r].score; norm_scores[e] = list[r].norm;
        }
        finalize[b] = n_list ? list[0].score - (score_norm ? list[0].before * (float)(list[0].n + 1) : list[0].before) : 0.0f;
        if (beam_n) {
            beam_n[b] = n_cur;
            for (int k = 0; k < n_cur; ++k) {
                beam_len[b * MAX_BEAM + k] = cur[k].n;
                beam_state[b * MAX_BEAM + k] = cur[k].state;
                if (beam_lm) beam_lm[b * MAX_BEAM + k] = cur[k].lm;
                beam_score[b * MAX_BEAM + k] = cur[k].score;
                const int m = cur[k].n < out_cap ? cur[k].n : out_cap;
                for (int q = 0; q < m; ++q) beam_y[((size_t)b * MAX_BEAM + k) * out_cap + q] = cur[k].y[q];
            }
        }
        hyps_free(cur, beam); hyps_free(nxt, beam);
        for (int k = 0; k < 9; ++k) { free(list[k].y); free(list[k].steps); }
    }
    free(z); free(hn); free(cn);
    return overflow ? -5 : 0;
}
