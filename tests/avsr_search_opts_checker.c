/*
 * avsr_search_opts_checker.c — TEST INFRASTRUCTURE.  tests/avsr_search_checker.c's two steps with the options of
 * rs_avsr_search_opts (csrc/k_avsr_search.hip's <true> kernels), restated for the CPU in the device's float32 order.  The plain
 * checker is included, not edited: row_stats, NT, MAXK and NEG are its.  Compile with -ffp-contract=off.
 *
 * Per hypothesis row and step, from the row's own prefix seq[0 .. step] (bos included), transformers' processors in
 * _get_logits_processor's order:
 *   repetition penalty p   every token of the prefix: s = s < 0 ? s * p : s / p
 *   no-repeat n-gram n     -inf for seq[i + n - 1] of every window i whose first n - 1 tokens equal the prefix's last n - 1
 *                          (nothing while the prefix has fewer than n tokens; n = 1: every token seen)
 *   min new tokens m       -inf for eos while step < m
 * greedy: on the raw logits before the argmax; beam: on (x[v] - m) - rs_logf(S) before the running score is added.
 * early_stopping 1: (top_lp / den) + (all K slots finished before ? 1 : 0) * NEG comes first in lp_fin, and the search also stops
 * once every clip's K slots are finished; 2 with length_penalty > 0: can_improve divides by pow(max_new_tokens, length_penalty).
 */
#include "avsr_search_checker.c"

/* s[0 .. V): the processed scores of one row, in place */
void rs_avsr_checker_opts_process(float* s, int V, const int32_t* seq, int step, int eos, float penalty, int ngram, int min_new) {
    unsigned char* mark = (unsigned char*)calloc((size_t)V, 1);
    for (int pos = 0; pos <= step; ++pos)
        if (seq[pos] >= 0 && seq[pos] < V) mark[seq[pos]] = 1;
    if (ngram > 0 && step + 1 >= ngram)
        for (int i = 0; i + ngram - 1 <= step; ++i) {
            int match = 1;
            for (int j = 0; j < ngram - 1; ++j) match &= seq[i + j] == seq[step + 2 - ngram + j];
            const int t = seq[i + ngram - 1];
            if (match && t >= 0 && t < V) mark[t] = 2;
        }
    if (step < min_new && eos >= 0 && eos < V) mark[eos] = 2;
    for (int v = 0; v < V; ++v) {
        if (mark[v] == 1) s[v] = s[v] < 0.0f ? s[v] * penalty : s[v] / penalty;
        if (mark[v] == 2) s[v] = -INFINITY;
    }
    free(mark);
}

/* (x[v] - m) - rs_logf(S) of one row in the device's summation order: what the beam processors act on */
void rs_avsr_checker_opts_logp(const float* x, int V, float* out) {
    float m, lse;
    row_stats(x, V, &m, &lse);
    for (int v = 0; v < V; ++v) out[v] = (x[v] - m) - lse;
}

int rs_avsr_checker_opts_greedy_step(const float* logits, int B, int V, int Vp, int step, int max_len, int eos, int pad, float penalty, int ngram,
                                     int min_new, int32_t* seq, int32_t* unfinished, int32_t* lengths, int32_t* tokens) {
    int left = 0;
    float* s = (float*)malloc((size_t)V * sizeof(float));
    for (int b = 0; b < B; ++b) {
        for (int v = 0; v < V; ++v) s[v] = logits[(size_t)b * Vp + v];
        rs_avsr_checker_opts_process(s, V, seq + (size_t)b * max_len, step, eos, penalty, ngram, min_new);
        int bi = 0;
        float best = -INFINITY;
        for (int v = 0; v < V; ++v)
            if (s[v] > best) { best = s[v]; bi = v; }
        const int nxt = unfinished[b] ? bi : pad;
        seq[(size_t)b * max_len + step + 1] = nxt;
        tokens[b] = nxt;
        if (unfinished[b]) lengths[b] = step + 2;
        unfinished[b] = unfinished[b] && nxt != eos;
        left += unfinished[b];
    }
    free(s);
    return left;
}

/* rs_avsr_checker_beam_step's arguments plus the options; early_stopping 0 / 1 / 2 */
int rs_avsr_checker_opts_beam_step(const float* logits, int B, int K, int V, int Vp, int step, int max_len, int eos, float length_penalty, float penalty,
                                   int ngram, int min_new, int early_stopping, int32_t* run_seq, float* run_score, int32_t* fin_seq, float* fin_score,
                                   int32_t* fin_len, int32_t* is_fin, int32_t* can_improve, int32_t* tokens, int32_t* src_rows, float* top_lp_out,
                                   int32_t* top_idx_out) {
    if (K < 1 || K > MAXK || V < 2 || step < 0 || step + 1 >= max_len) return -1;
    const int cur = step + 1;
    const float den = (float)pow((double)cur, (double)length_penalty);
    const float den_heur = early_stopping == 2 && length_penalty > 0.0f ? (float)pow((double)(max_len - 1), (double)length_penalty) : den;
    int any_improve = 0, any_goes = 0, all_full = 1;
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
            float* lp = logp + (size_t)k * V;
            rs_avsr_checker_opts_logp(lg + (size_t)k * Vp, V, lp);
            rs_avsr_checker_opts_process(lp, V, rs + (size_t)k * max_len, step, eos, penalty, ngram, min_new);
            for (int v = 0; v < V; ++v) lp[v] = lp[v] + rsc[k];
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
        int old_len[MAXK], old_isfin[MAXK], full = early_stopping == 1;
        for (int j = 0; j < K; ++j) {
            m_score[j] = fsc[j]; old_len[j] = fin_len[b * K + j]; old_isfin[j] = is_fin[b * K + j];
            full &= old_isfin[j] != 0;
        }
        for (int j = 0; j < 2 * K; ++j) {
            just[j] = ends[j] && j < K;
            float f = top_lp[j] / den;
            f = f + (full ? 1.0f : 0.0f) * NEG;
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
        const float best_running = lp_run[keep[0]] / den_heur;
        int any = 0, all_fin = 1;
        for (int j = 0; j < K; ++j) {
            const int w = best[j], c = keep[j];
            const int nf = w < K ? old_isfin[w] : just[w - K];
            all_fin &= nf != 0;
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
        all_full &= all_fin;
    }
    free(logp); free(old_run); free(old_fin);
    return any_improve && any_goes && !(early_stopping == 1 && all_full);
}
