/*
 * espnet_beam_nbest_checker.c — CPU restatement of reazonspeech_amd/csrc/k_rnnt_beam.hip with the ranked list of rs_rnnt_beam_nbest:
 * ESPnet's "default" transducer beam search followed by upstream's sort_nbest(kept_hyps)[:nbest], in the device's float32 evaluation
 * order.  TEST INFRASTRUCTURE, built by tests/checker_lib.py with the flags of oracle/build.py and linked against the oracle library.
 * The search is the text of oracle/espnet_beam.c (which states it in full: pops, kept list, end-of-frame test, survivors ascending by
 * score with ties in kept order); with nbest = 1 it must equal that checker bit for bit (tests/test_nbest_espnet_host.py holds it to
 * that); folding the two into one checker is left for later.
 *
 * The list (include/rs_asr.h rs_rnnt_beam_nbest): the candidates are ALL hypotheses kept after the last frame, in the kept list's
 * order; norm = score / (float)len(yseq) with score_norm (yseq counts the leading blank), else score; the list is sorted by norm
 * descending and stable in that order — rank r takes the first maximum (strict `>` while walking the list) among those not yet
 * ranked.  Equal label sequences are NOT removed.  n_hyps = min(nbest, kept); an utterance without frames keeps the start hypothesis
 * alone (n_hyps 1, no labels, score 0); one that overflowed max_pops has n_hyps 0.  An entry with more than out_cap labels returns
 * n_ids 0 (and -5).  Entries past n_hyps: n_ids 0.
 * nb_counters per utterance [0..3]: [0] length of the kept list after the last frame, [1] pairs of entries of the RETURNED list
 * with equal label sequences, [2] equal norms met while ranking (a remaining entry equal to the one picked), [3] 1 if ranking by
 * score alone gives another order than ranking by norm.
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

typedef struct {
    float score;
    int node;      /* label-trie node of the whole sequence when tok < 0, of the sequence without its last label otherwise */
    int tok;       /* last label not yet in the trie, or -1 */
    int len;       /* len(yseq): labels + the leading blank */
    int state;     /* index of the prediction-net state stored BEFORE the last label */
    int alive;
} bhyp_t;

typedef struct { int parent, tok, t; } node_t;   /* t: the frame at which the label was appended (its hypothesis was opened AND popped there) */

typedef struct { float* v; int n, cap, width; } pool_t;     /* states: h [L][H] then c [L][H] */

static int pool_push(pool_t* p, const float* h, const float* c, int LH) {
    if (p->n == p->cap) {
        p->cap = p->cap ? 2 * p->cap : 64;
        p->v = (float*)realloc(p->v, sizeof(float) * (size_t)p->cap * p->width);
    }
    memcpy(p->v + (size_t)p->n * p->width, h, sizeof(float) * LH);
    memcpy(p->v + (size_t)p->n * p->width + LH, c, sizeof(float) * LH);
    return p->n++;
}

/* do two kept hypotheses spell the same labels?  The trie makes a node per POP, not per sequence: the same labels reached along
 * two alignments are two chains of nodes, compared label by label up to the root (or to a shared ancestor). */
static int same_labels(const node_t* nodes, int a, int la, int b, int lb) {
    if (la != lb) return 0;
    while (a != b) {
        if (a < 0 || b < 0 || nodes[a].tok != nodes[b].tok) return 0;
        a = nodes[a].parent; b = nodes[b].parent;
    }
    return 1;
}

/* f [B][Tp][J] (joint.enc output).  Outputs per utterance the ranked list: ids [B][nbest][out_cap] (without the leading blank),
 * frames likewise (may be NULL: the frame each label was appended at), n_ids / scores / norm_scores [B][nbest], n_hyps [B], pops [B]
 * (prediction-net evaluations spent) and nb_counters [B][4].  Returns 0, -5 on overflow (max_pops per frame / out_cap), -1 for an
 * nbest outside 1..8 or above the beam. */
int rs_espnet_beam_nbest_checker(const float* f, const int32_t* enc_lens, int B, int Tp, int J, int H, int L, int V, int blank,
                          const float* embed, const float* const* lstm_w, const float* const* lstm_b, const float* Wp,
                          const float* bp, const float* Wo, const float* bo, const float* inject, int beam, int score_norm, int max_pops,
                          int nbest, int out_cap, int32_t* ids /* [B][nbest][out_cap] */, int32_t* frames, int32_t* n_ids /* [B][nbest] */,
                          float* scores, float* norm_scores, int32_t* n_hyps /* [B] */, int32_t* pops, int32_t* nb_counters /* [B][4] */) {
    int overflow = 0;
    if (nbest < 1 || nbest > 8 || nbest > (beam < V ? beam : V)) return -1;
    if (beam > V) beam = V;
    const int beam_k = beam < V - 1 ? beam : V - 1;
    const int LH = L * H;
    float* z = (float*)malloc(sizeof(float) * V);
    float* g = (float*)malloc(sizeof(float) * J);
    float* hn = (float*)malloc(sizeof(float) * LH);
    float* cn = (float*)malloc(sizeof(float) * LH);
    for (int b = 0; b < B; ++b) {
        const int T = enc_lens[b];
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
        kept[0] = (bhyp_t){0.0f, 0, -1, 1, 0, 1};
        for (int t = 0; t < T && !failed; ++t) {
            /* hyps <- kept (already ordered), states stay in pool[cur] */
            int n_h = n_kept;
            memcpy(hyps, kept, sizeof(bhyp_t) * n_kept);
            n_kept = 0;
            int n_pop = 0;
            for (;;) {
                if (n_pop == max_pops) { failed = 1; break; }
                int mi = -1;
                for (int i = 0; i < n_h; ++i) if (hyps[i].alive && (mi < 0 || hyps[i].score > hyps[mi].score)) mi = i;
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
                kept[n_kept] = mh;
                kept[n_kept].score = mh.score + (z[blank] - lse);
                kept[n_kept].alive = 1;
                ++n_kept;
                float pz = INFINITY; int pv = -1;
                for (int j = 0; j < beam_k; ++j) {
                    float bz = -INFINITY; int bv = -1;
                    for (int v = 0; v < V; ++v) {
                        if (v == blank) continue;
                        if (!(z[v] < pz || (z[v] == pz && v > pv))) continue;
                        if (bv < 0 || z[v] > bz) { bz = z[v]; bv = v; }
                    }
                    if (bv < 0) break;
                    hyps[n_h++] = (bhyp_t){mh.score + (bz - lse), mh.node, bv, mh.len + 1, after, 1};
                    pz = bz; pv = bv;
                }
                float hmax = -INFINITY;
                for (int i = 0; i < n_h; ++i) if (hyps[i].alive && hyps[i].score > hmax) hmax = hyps[i].score;
                int n_good = 0;
                for (int i = 0; i < n_kept; ++i) if (kept[i].score > hmax) ++n_good;
                if (n_good >= beam) {
                    /* survivors ascending by score, ties in kept order; their states move to the other pool */
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
        int32_t* nc = nb_counters + 4 * b;
        nc[0] = failed ? 0 : n_kept; nc[1] = nc[2] = nc[3] = 0;
        for (int r = 0; r < nbest; ++r) { n_ids[(size_t)b * nbest + r] = 0; scores[(size_t)b * nbest + r] = 0.0f; norm_scores[(size_t)b * nbest + r] = 0.0f; }
        n_hyps[b] = 0;
        if (failed) overflow = 1;
        else {
            char* taken = (char*)calloc(n_kept, 1);
            char* taken0 = (char*)calloc(n_kept, 1);
            int* order = (int*)malloc(sizeof(int) * n_kept);
            for (int r = 0; r < n_kept; ++r) {                       /* the whole order, for the counters; the first nbest ranks are written */
                int pick = -1, pick0 = -1;
                float pn = 0.0f;
                for (int i = 0; i < n_kept; ++i) {
                    const float norm = score_norm ? kept[i].score / (float)kept[i].len : kept[i].score;
                    if (!taken[i] && (pick < 0 || norm > pn)) { pick = i; pn = norm; }
                    if (!taken0[i] && (pick0 < 0 || kept[i].score > kept[pick0].score)) pick0 = i;
                }
                taken[pick] = 1; taken0[pick0] = 1;
                order[r] = pick;
                if (pick != pick0) nc[3] = 1;
                if (r >= nbest) continue;
                for (int i = 0; i < n_kept; ++i)
                    if (!taken[i] && (score_norm ? kept[i].score / (float)kept[i].len : kept[i].score) == pn) nc[2] += 1;
                for (int q = 0; q < r; ++q)
                    if (same_labels(nodes, kept[order[q]].node, kept[order[q]].len, kept[pick].node, kept[pick].len)) nc[1] += 1;
                const size_t e = (size_t)b * nbest + r;
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
            free(taken); free(taken0); free(order);
        }
        free(nodes); free(pool[0].v); free(pool[1].v); free(hyps); free(kept);
    }
    free(z); free(g); free(hn); free(cn);
    return overflow ? -5 : 0;
}
