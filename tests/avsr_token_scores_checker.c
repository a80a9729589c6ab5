/*
 * avsr_token_scores_checker.c — TEST INFRASTRUCTURE.  tests/avsr_search_opts_checker.c's two steps with the RECORDING of
 * csrc/k_avsr_search.hip's <.., true> kernels (the _scored entry points), restated for the CPU in the device's float32 order.  The
 * options checker is included, not edited: its processors, row_stats, NT, MAXK and NEG are used.  Compile with -ffp-contract=off.
 *
 * Per hypothesis row a history beside its prefix, indexed by sequence position pos = p + 1 (position 0 unused), re-parented and
 * copied into the finished slots with the prefixes:
 *   ts   the processed score s of the token chosen at pos: greedy, the logit after the processors; beam, (x[v] - m) - rs_logf(S)
 *        after the processors and before the running score is added
 *   tl   the log-sum-exp of the row's processed scores at that step: M = max_v s[v]; Z: "thread" t of 256 adds rs_expf(s[v] - M) over
 *        v = t, t + 256, ... in increasing v, a -inf column adding exactly 0.0f; the 256 partial sums are combined by the binary tree
 *        (stride 128 .. 1); lse = M + rs_logf(Z); a row whose every column is -inf has lse = -inf
 *   bi   beam: the flat row b K + parent the token was taken from
 * dump (may be null): [rows][Vp], the processed row of every hypothesis row in the order read; columns V .. Vp - 1 hold 0.
 */
#include "avsr_search_opts_checker.c"

static float row_plse(const float* s, int V) {
    float M = -INFINITY, p[NT];
    for (int v = 0; v < V; ++v) M = fmaxf(M, s[v]);
    for (int t = 0; t < NT; ++t) {
        float z = 0.0f;
        for (int v = t; v < V; v += NT) z += s[v] == -INFINITY ? 0.0f : rs_expf(s[v] - M);
        p[t] = z;
    }
    for (int stride = NT / 2; stride > 0; stride >>= 1)
        for (int t = 0; t < stride; ++t) p[t] += p[t + stride];
    return M == -INFINITY ? -INFINITY : M + rs_logf(p[0]);
}

static void dump_row(float* dump, size_t row, const float* s, int V, int Vp) {
    if (!dump) return;
    for (int v = 0; v < Vp; ++v) dump[row * Vp + v] = v < V ? s[v] : 0.0f;
}

/* rs_avsr_checker_opts_greedy_step's arguments; run_ts / run_tl [B][max_len] in / out */
int rs_avsr_checker_scored_greedy_step(const float* logits, int B, int V, int Vp, int step, int max_len, int eos, int pad, float penalty, int ngram,
                                       int min_new, int32_t* seq, int32_t* unfinished, int32_t* lengths, int32_t* tokens, float* run_ts, float* run_tl,
                                       float* dump) {
    int left = 0;
    float* s = (float*)malloc((size_t)V * sizeof(float));
    for (int b = 0; b < B; ++b) {
        for (int v = 0; v < V; ++v) s[v] = logits[(size_t)b * Vp + v];
        rs_avsr_checker_opts_process(s, V, seq + (size_t)b * max_len, step, eos, penalty, ngram, min_new);
        dump_row(dump, (size_t)b, s, V, Vp);
        int bi = 0;
        float best = -INFINITY;
        for (int v = 0; v < V; ++v)
            if (s[v] > best) { best = s[v]; bi = v; }
        if (unfinished[b]) {
            run_ts[(size_t)b * max_len + step + 1] = best;
            run_tl[(size_t)b * max_len + step + 1] = row_plse(s, V);
        }
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

/* rs_avsr_checker_opts_beam_step's arguments; run_ts / run_tl / run_bi / fin_ts / fin_tl / fin_bi [B][K][max_len] in / out */
int rs_avsr_checker_scored_beam_step(const float* logits, int B, int K, int V, int Vp, int step, int max_len, int eos, float length_penalty, float penalty,
                                     int ngram, int min_new, int early_stopping, int32_t* run_seq, float* run_score, int32_t* fin_seq, float* fin_score,
                                     int32_t* fin_len, int32_t* is_fin, int32_t* can_improve, int32_t* tokens, int32_t* src_rows, float* top_lp_out,
                                     int32_t* top_idx_out, float* run_ts, float* run_tl, int32_t* run_bi, float* fin_ts, float* fin_tl, int32_t* fin_bi,
                                     float* dump) {
    if (K < 1 || K > MAXK || V < 2 || step < 0 || step + 1 >= max_len) return -1;
    const int cur = step + 1;
    const float den = (float)pow((double)cur, (double)length_penalty);
    const float den_heur = early_stopping == 2 && length_penalty > 0.0f ? (float)pow((double)(max_len - 1), (double)length_penalty) : den;
    int any_improve = 0, any_goes = 0, all_full = 1;
    const size_t H = (size_t)K * max_len;
    float* proc = (float*)malloc((size_t)K * V * sizeof(float));
    float* logp = (float*)malloc((size_t)K * V * sizeof(float));
    int32_t* old_run = (int32_t*)malloc(H * sizeof(int32_t));
    int32_t* old_fin = (int32_t*)malloc(H * sizeof(int32_t));
    float* o_rts = (float*)malloc(H * sizeof(float));
    float* o_rtl = (float*)malloc(H * sizeof(float));
    int32_t* o_rbi = (int32_t*)malloc(H * sizeof(int32_t));
    float* o_fts = (float*)malloc(H * sizeof(float));
    float* o_ftl = (float*)malloc(H * sizeof(float));
    int32_t* o_fbi = (int32_t*)malloc(H * sizeof(int32_t));
    if (!proc || !logp || !old_run || !old_fin || !o_rts || !o_rtl || !o_rbi || !o_fts || !o_ftl || !o_fbi) return -2;
    for (int b = 0; b < B; ++b) {
        const float* lg = logits + (size_t)b * K * Vp;
        int32_t* rs = run_seq + (size_t)b * H;
        int32_t* fs = fin_seq + (size_t)b * H;
        float* rsc = run_score + (size_t)b * K;
        float* fsc = fin_score + (size_t)b * K;
        float plse[MAXK];
        for (int k = 0; k < K; ++k) {
            float* sp = proc + (size_t)k * V;
            rs_avsr_checker_opts_logp(lg + (size_t)k * Vp, V, sp);
            rs_avsr_checker_opts_process(sp, V, rs + (size_t)k * max_len, step, eos, penalty, ngram, min_new);
            dump_row(dump, (size_t)b * K + k, sp, V, Vp);
            plse[k] = row_plse(sp, V);
            for (int v = 0; v < V; ++v) logp[(size_t)k * V + v] = sp[v] + rsc[k];
        }
        float top_lp[2 * MAXK], lp_run[2 * MAXK], m_score[3 * MAXK], cand_ts[2 * MAXK], cand_tl[2 * MAXK];
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
            cand_ts[j] = proc[(size_t)parent[j] * V + token[j]];
            cand_tl[j] = plse[parent[j]];
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
        float *rts = run_ts + (size_t)b * H, *rtl = run_tl + (size_t)b * H, *fts = fin_ts + (size_t)b * H, *ftl = fin_tl + (size_t)b * H;
        int32_t *rbi = run_bi + (size_t)b * H, *fbi = fin_bi + (size_t)b * H;
        for (size_t i = 0; i < H; ++i) {
            old_run[i] = rs[i]; old_fin[i] = fs[i];
            o_rts[i] = rts[i]; o_rtl[i] = rtl[i]; o_rbi[i] = rbi[i]; o_fts[i] = fts[i]; o_ftl[i] = ftl[i]; o_fbi[i] = fbi[i];
        }
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
                const size_t d = (size_t)j * max_len + pos;
                if (w < K) fs[d] = old_fin[(size_t)w * max_len + pos];
                else fs[d] = pos == cur ? token[w - K] : old_run[(size_t)parent[w - K] * max_len + pos];
                rs[d] = pos == cur ? token[c] : old_run[(size_t)parent[c] * max_len + pos];
                if (pos < 1 || pos > cur) continue;                  /* the histories: the positions written so far */
                const size_t rp = (size_t)parent[c] * max_len + pos;
                rts[d] = pos == cur ? cand_ts[c] : o_rts[rp];
                rtl[d] = pos == cur ? cand_tl[c] : o_rtl[rp];
                rbi[d] = pos == cur ? b * K + parent[c] : o_rbi[rp];
                if (w < K) {
                    const size_t fp = (size_t)w * max_len + pos;
                    fts[d] = o_fts[fp]; ftl[d] = o_ftl[fp]; fbi[d] = o_fbi[fp];
                } else {
                    const size_t wp = (size_t)parent[w - K] * max_len + pos;
                    fts[d] = pos == cur ? cand_ts[w - K] : o_rts[wp];
                    ftl[d] = pos == cur ? cand_tl[w - K] : o_rtl[wp];
                    fbi[d] = pos == cur ? b * K + parent[w - K] : o_rbi[wp];
                }
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
    free(proc); free(logp); free(old_run); free(old_fin);
    free(o_rts); free(o_rtl); free(o_rbi); free(o_fts); free(o_ftl); free(o_fbi);
    return any_improve && any_goes && !(early_stopping == 1 && all_full);
}
