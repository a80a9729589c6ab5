/*
 * avsr_search_checker.c — TEST INFRASTRUCTURE.  One step of the two searches of csrc/k_avsr_search.hip (transformers'
 * GenerationMixin._sample without sampling and ._beam_search, as reazonspeech_amd/avsr/generation.py states them) restated for
 * the CPU in the device's float32 order over a logits array.  State comes in and goes out, so the caller drives it step by step
 * (tests/avsr_search_ref.py).  Compile with -ffp-contract=off; rs_expf / rs_logf are oracle/rnnt_math.h's.
 *
 * log_softmax of a row: m = max x; S: "thread" t of 256 adds rs_expf(x[v] - m) over v = t, t + 256, ... in increasing v, the 256
 * partial sums are combined by a binary tree (stride 128 .. 1: p[t] += p[t + stride]); logp[v] = ((x[v] - m) - rs_logf(S)) + run.
 * Top 2K: value descending, then flat index k V + v ascending.  Equal running / finished scores: the earlier position.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#include "rnnt_math.h"

#define NT 256
#define MAXK 8
#define NEG (-1.0e9f)

/* greedy: logits [B][Vp]; seq [B][max_len], unfinished [B], lengths [B] in / out; tokens [B] out.
 * returns the number of rows still unfinished after the step (0: the search stops) */
int rs_avsr_checker_greedy_step(const float* logits, int B, int V, int Vp, int step, int max_len, int eos, int pad, int32_t* seq,
                                int32_t* unfinished, int32_t* lengths, int32_t* tokens) {
    int left = 0;
    for (int b = 0; b < B; ++b) {
        const float* row = logits + (size_t)b * Vp;
        int bi = 0;
        float best = -INFINITY;
        for (int v = 0; v < V; ++v)
            if (row[v] > best) { best = row[v]; bi = v; }          /* equal values: the lower index */
        const int nxt = unfinished[b] ? bi : pad;
        seq[(size_t)b * max_len + step + 1] = nxt;
        tokens[b] = nxt;
        if (unfinished[b]) lengths[b] = step + 2;
        unfinished[b] = unfinished[b] && nxt != eos;
        left += unfinished[b];
    }
    return left;
}

static void row_stats(const float* x, int V, float* m_out, float* lse_out) {
    float m = -INFINITY, p[NT];
    for (int v = 0; v < V; ++v) m = fmaxf(m, x[v]);
    for (int t = 0; t < NT; ++t) {
        float s = 0.0f;
        for (int v = t; v < V; v += NT) s += rs_expf(x[v] - m);
        p[t] = s;
    }
    for (int stride = NT / 2; stride > 0; stride >>= 1)
        for (int t = 0; t < stride; ++t) p[t] += p[t + stride];
    *m_out = m;
    *lse_out = rs_logf(p[0]);
}

/* beam: logits [B][K][Vp]; run_seq / fin_seq [B][K][max_len], run_score / fin_score [B][K], fin_len / is_fin [B][K],
 * can_improve [B] in / out; tokens / src_rows [B][K], top_lp / top_idx [B][2K] out.
 * returns 1 if the search goes on after the step, 0 if it stops, < 0 on a bad argument */
int rs_avsr_checker_beam_step(const float* logits, int B, int K, int V, int Vp, int step, int max_len, int eos, float length_penalty,
                              int32_t* run_seq, float* run_score, int32_t* fin_seq, float* fin_score, int32_t* fin_len, int32_t* is_fin,
                              int32_t* can_improve, int32_t* tokens, int32_t* src_rows, float* top_lp_out, int32_t* top_idx_out) {
    if (K < 1 || K > MAXK || V < 2 || step < 0 || step + 1 >= max_len) return -1;
    const int cur = step + 1;
    const float den = (float)pow((double)cur, (double)length_penalty);
    int any_improve = 0, any_goes = 0;
    float* logp = (float*)malloc((size_t)K * V * sizeof(float));
    int32_t* old_run = (int32_t*)malloc((size_t)K * max_len * sizeof(int32_t));
    int32_t* old_fin = (int32_t*)malloc((size_t)K * max_len * sizeof(int32_t));
    if (!logp || !old_run || !old_fin) return -2;
    for (int b = 0; b < B; ++b) {
        const float* lg = logits + (size_t)b * K * Vp;
        int32_t* rs = run_seq + (size_t)b * K * max_len;
        int32_t* fs = fin_seq + (size_t)b * K * max_len;
        float* rsc = run_score + (size_t)b * K;
        float* fsc = fin_score + (size_t)b * K;
        for (int k = 0; k < K; ++k) {
            float m, lse;
            row_stats(lg + (size_t)k * Vp, V, &m, &lse);
            for (int v = 0; v < V; ++v) logp[(size_t)k * V + v] = ((lg[(size_t)k * Vp + v] - m) - lse) + rsc[k];
        }
        float top_lp[2 * MAXK], lp_run[2 * MAXK], m_score[3 * MAXK];
        int top_idx[2 * MAXK], parent[2 * MAXK], token[2 * MAXK], ends[2 * MAXK], just[2 * MAXK], keep[MAXK], best[MAXK], used[3 * MAXK];
        float prev_v = INFINITY;
        int prev_i = -1;
        for (int r = 0; r < 2 * K; ++r) {
            float bv = -INFINITY;
            int bi = 0x7fffffff;
            for (int i = 0; i < K * V; ++i) {
                const float val = logp[i];
                const int after = val < prev_v || (val == prev_v && i > prev_i);
                if (after && (val > bv || (val == bv && i < bi))) { bv = val; bi = i; }
            }
            top_lp[r] = bv; top_idx[r] = bi; prev_v = bv; prev_i = bi;
        }
        int all_end = 1;
        for (int j = 0; j < 2 * K; ++j) {
            int idx = top_idx[j];
            if (idx < 0 || idx >= K * V) idx = 0;
            parent[j] = idx / V; token[j] = idx % V;
            ends[j] = (token[j] == eos) || (cur + 1 >= max_len);
            all_end &= ends[j];
            lp_run[j] = top_lp[j] + (ends[j] ? 1.0f : 0.0f) * NEG;
            used[j] = 0;
            top_lp_out[(size_t)b * 2 * K + j] = top_lp[j];
            top_idx_out[(size_t)b * 2 * K + j] = top_idx[j];
        }
        for (int j = 0; j < K; ++j) {
            int w = -1;
            for (int c = 0; c < 2 * K; ++c)
                if (!used[c] && (w < 0 || lp_run[c] > lp_run[w])) w = c;
            used[w] = 1; keep[j] = w;
        }
        const int ci = can_improve[b];
        int old_len[MAXK], old_isfin[MAXK];
        for (int j = 0; j < K; ++j) { m_score[j] = fsc[j]; old_len[j] = fin_len[b * K + j]; old_isfin[j] = is_fin[b * K + j]; }
        for (int j = 0; j < 2 * K; ++j) {
            just[j] = ends[j] && j < K;
            float f = top_lp[j] / den;
            f = f + (ci ? 0.0f : 1.0f) * NEG;
            f = f + (just[j] ? 0.0f : 1.0f) * NEG;
            m_score[K + j] = f;
        }
        for (int c = 0; c < 3 * K; ++c) used[c] = 0;
        for (int j = 0; j < K; ++j) {
            int w = -1;
            for (int c = 0; c < 3 * K; ++c)
                if (!used[c] && (w < 0 || m_score[c] > m_score[w])) w = c;
            used[w] = 1; best[j] = w;
        }
        for (int i = 0; i < K * max_len; ++i) { old_run[i] = rs[i]; old_fin[i] = fs[i]; }
        float mn = INFINITY;
        for (int j = 0; j < K; ++j) mn = fminf(mn, m_score[best[j]]);
        const float best_running = lp_run[keep[0]] / den;
        int any = 0;
        for (int j = 0; j < K; ++j) {
            const int w = best[j], c = keep[j];
            const int nf = w < K ? old_isfin[w] : just[w - K];
            fsc[j] = m_score[w];
            fin_len[b * K + j] = w < K ? old_len[w] : cur + 1;
            is_fin[b * K + j] = nf;
            any |= best_running > (nf ? mn : NEG);
            for (int pos = 0; pos < max_len; ++pos) {
                if (w < K) fs[(size_t)j * max_len + pos] = old_fin[(size_t)w * max_len + pos];
                else fs[(size_t)j * max_len + pos] = pos == cur ? token[w - K] : old_run[(size_t)parent[w - K] * max_len + pos];
                rs[(size_t)j * max_len + pos] = pos == cur ? token[c] : old_run[(size_t)parent[c] * max_len + pos];
            }
            rsc[j] = lp_run[c];
            tokens[b * K + j] = token[c];
            src_rows[b * K + j] = b * K + parent[c];
        }
        can_improve[b] = ci && any;
        any_improve |= can_improve[b];
        any_goes |= !all_end;
    }
    free(logp); free(old_run); free(old_fin);
    return any_improve && any_goes;
}
