// k_avsr_search.hip — the two searches of AVHubertForConditionalGeneration.generate() on the device: what transformers'
// GenerationMixin._sample (do_sample False) and ._beam_search (v4.50+, early_stopping False, one eos token) do with the logits of
// every step (pkg/avsr/src/avhubert/modeling_avhubert.py:216,372-391; pkg/avsr/README.rst:41 `generate(**inputs, num_beams=5,
// max_new_tokens=256)`).  The same algorithm as reazonspeech_amd/avsr/generation.py (the host path) and oracle/avsr.py:158-227;
// restated for the CPU, operation for operation, in tests/avsr_search_checker.c.
//
// One launch per step and search (no kernel waits on another workgroup; the host loop is bounded by max_new_tokens):
//
//   avsr_greedy_step_kernel   one workgroup per row: argmax over v < V (equal values: the lower index), pad for rows that already
//                             emitted eos, the row's next decoder token, and the count of rows still unfinished
//   avsr_beam_step_kernel     one workgroup of 256 threads per clip, K <= 8 hypothesis rows:
//       1. log-softmax        per row k: m = max_v x[v]; S = sum_v rs_expf(x[v] - m); logp[v] = ((x[v] - m) - rs_logf(S)) + run_score[k]
//       2. top 2 K            of the K V values logp[k][v], by value descending, then flat index k V + v ascending: 2 K rounds, each
//                             the minimum in that order among the values after the previous pick (the rows are re-read from
//                             global memory / L2 every round: nothing of size K V is held in LDS or registers)
//       3. bookkeeping        thread 0 restates generation.py's float32 lines on the 2 K candidates (below); then all threads copy
//                             the token prefixes from the step's source buffers to its destination buffers
//
// SUMMATION ORDER of S (the only rounding-order choice in this file; max and the selection are exact in any order):
//   thread t of 256 owns the columns v = t, t + 256, t + 512, ... and adds their rs_expf terms to a zero in increasing v;
//   the 256 partial sums are then combined by a binary tree in LDS: for stride = 128, 64, ..., 1: p[t] += p[t + stride] for t < stride;
//   S = p[0].  rs_expf / rs_logf are k_rnnt_common.h's (oracle/rnnt_math.h on the host); the file is compiled with -ffp-contract=off.
//
// BOOKKEEPING, with cur = step + 1 (the position being written), den = (float)pow((double)cur, (double)length_penalty) computed on
// the host, NEG = -1e9f, candidates j = 0 .. 2K-1 in the order of (2.), parent = idx / V, token = idx % V:
//   ends[j]   = token == eos || cur + 1 >= max_len
//   lp_run[j] = top_lp[j] + (ends[j] ? 1.0f : 0.0f) * NEG;  the K largest, equal values in candidate order, run on
//   just[j]   = ends[j] && j < K                            (only one of the K best may finish)
//   lp_fin[j] = ((top_lp[j] / den) + (can_improve ? 0.0f : 1.0f) * NEG) + (just[j] ? 0.0f : 1.0f) * NEG
//   the K largest of [fin_score[0..K), lp_fin[0..2K)], equal values keeping the earlier position, are the new finished slots
//   can_improve &= any_j (run_score'[0] / den > (is_fin'[j] ? min_i fin_score'[i] : NEG))
//   the clip adds (can_improve ? 1 : 0) + (all_j ends[j] ? 0 : 0x10000) to the step's word go[step + 1]
// The search goes on after a step iff some clip can improve and some clip has a candidate that does not end: both halves of the
// word non-zero.  A step whose go[step] word says stop returns at once and leaves go[step + 1] zero, so every later step does too.
// A clip that cannot improve any more keeps extending its running beams until the global stop, as transformers does.
//
// State buffers ping-pong by step parity: step s reads run_seq / fin_seq [s & 1] and writes [(s + 1) & 1]; positions beyond the
// ones a step writes still hold pad_token_id from rs_avsr_search_begin.
#include <math.h>

#include "k_rnnt_common.h"

namespace {

constexpr int NT = 256;
constexpr int MAXK = 8;
constexpr int LAG = 2;          // rs_avsr_generate: the host runs at most this many steps ahead of the stop word it has read

struct SearchPtrs {
    int32_t *tok, *src, *run_seq, *fin_seq, *fin_len, *is_fin, *can, *last, *go;
    float *run_score, *fin_score;
};
struct SearchPlan {
    size_t off_tok, off_src, off_run_seq, off_fin_seq, off_fin_len, off_is_fin, off_can, off_last, off_go, off_run_score, off_fin_score, total;
};
SearchPlan search_plan(int B, int K, int max_len) {
    SearchPlan p{};
    const size_t R = (size_t)B * K;
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += rs_align(bytes); return at; };
    p.off_tok = take(R * 4); p.off_src = take(R * 4);
    p.off_run_seq = take(2 * R * max_len * 4); p.off_fin_seq = take(2 * R * max_len * 4);
    p.off_fin_len = take(R * 4); p.off_is_fin = take(R * 4);
    p.off_can = take((size_t)B * 4); p.off_last = take((size_t)B * 4);
    p.off_go = take((size_t)(max_len + 1) * 4);
    p.off_run_score = take(R * 4); p.off_fin_score = take(R * 4);
    p.total = o + 256;
    return p;
}
SearchPtrs search_ptrs(void* state, const SearchPlan& pl) {
    char* st = reinterpret_cast<char*>(state);
    auto ip = [&](size_t off) { return reinterpret_cast<int32_t*>(st + off); };
    SearchPtrs p;
    p.tok = ip(pl.off_tok); p.src = ip(pl.off_src); p.run_seq = ip(pl.off_run_seq); p.fin_seq = ip(pl.off_fin_seq);
    p.fin_len = ip(pl.off_fin_len); p.is_fin = ip(pl.off_is_fin); p.can = ip(pl.off_can); p.last = ip(pl.off_last); p.go = ip(pl.off_go);
    p.run_score = reinterpret_cast<float*>(st + pl.off_run_score); p.fin_score = reinterpret_cast<float*>(st + pl.off_fin_score);
    return p;
}

__host__ __device__ inline bool goes_on(bool greedy, uint32_t w) { return greedy ? w != 0 : ((w & 0xffffu) != 0 && (w >> 16) != 0); }

// grid B: the state before step 0
__global__ __launch_bounds__(NT) void avsr_search_init_kernel(SearchPtrs p, int B, int K, int max_len, int greedy, int bos, int pad) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const size_t R = (size_t)B * K;
    for (int i = tid; i < K * max_len; i += NT) {
        const int tokv = (i % max_len) == 0 ? bos : pad;
        for (int par = 0; par < 2; ++par) {
            p.run_seq[((size_t)par * R + (size_t)b * K) * max_len + i] = tokv;
            p.fin_seq[((size_t)par * R + (size_t)b * K) * max_len + i] = tokv;
        }
    }
    if (tid < K) {
        const int r = b * K + tid;
        p.tok[r] = bos;
        p.src[r] = r;
        p.run_score[r] = tid == 0 ? 0.0f : -1.0e9f;
        p.fin_score[r] = -1.0e9f;
        p.fin_len[r] = greedy ? 1 : 0;
        p.is_fin[r] = 0;
    }
    if (tid == 0) { p.can[b] = 1; p.last[b] = 0; }
    if (b == 0)
        for (int i = tid; i <= max_len; i += NT) p.go[i] = i == 0 ? (greedy ? B : 0x10001) : 0;
}

// (value, index) maximum, equal values: the lower index — over the 256 threads of a workgroup; every thread returns the result
__device__ __forceinline__ void block_argmax(float& v, int& i, float* sv, int* si) {
    for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_xor(v, off);
        const int oi = __shfl_xor(i, off);
        if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
    }
    const int w = threadIdx.x >> 6;
    __syncthreads();                                     // the previous use of sv / si has been read by everyone
    if ((threadIdx.x & 63) == 0) { sv[w] = v; si[w] = i; }
    __syncthreads();
    v = sv[0]; i = si[0];
    for (int k = 1; k < NT / 64; ++k)
        if (sv[k] > v || (sv[k] == v && si[k] < i)) { v = sv[k]; i = si[k]; }
}

// grid B (rows): transformers' _sample with do_sample False for one step
__global__ __launch_bounds__(NT) void avsr_greedy_step_kernel(const float* __restrict__ logits, int V, int Vp, int step, int max_len, int eos, int pad,
                                                              SearchPtrs p) {
    __shared__ float sv[NT / 64];
    __shared__ int si[NT / 64];
    if (p.go[step] == 0) return;
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* row = logits + (size_t)b * Vp;
    float best = -INFINITY;
    int bi = 0x7fffffff;
    for (int v = tid; v < V; v += NT) {
        const float x = row[v];
        if (x > best) { best = x; bi = v; }
    }
    block_argmax(best, bi, sv, si);
    if (tid == 0) {
        if (bi >= V) bi = 0;
        const int unfinished = p.can[b];
        const int nxt = unfinished ? bi : pad;
        p.run_seq[(size_t)b * max_len + step + 1] = nxt;
        p.tok[b] = nxt;
        if (unfinished) p.fin_len[b] = step + 2;
        const int still = unfinished && nxt != eos;
        p.can[b] = still;
        p.last[b] = step + 1;
        if (still) atomicAdd(&p.go[step + 1], 1);
    }
}

// grid B (clips): transformers' _beam_search for one step (the file's head comment)
__global__ __launch_bounds__(NT) void avsr_beam_step_kernel(const float* __restrict__ logits, int V, int Vp, int K, int step, int max_len, int eos, float den,
                                                            int B, SearchPtrs p) {
    __shared__ float red[MAXK][NT];
    __shared__ float row_max[MAXK], row_lse[MAXK], row_run[MAXK];
    __shared__ float top_lp[2 * MAXK], lp_run[2 * MAXK], m_score[3 * MAXK], new_score[MAXK];
    __shared__ int top_idx[2 * MAXK], parent[2 * MAXK], token[2 * MAXK], ends[2 * MAXK], just[2 * MAXK];
    __shared__ int keep[MAXK], best[MAXK], old_len[MAXK], old_fin[MAXK], used[3 * MAXK];
    __shared__ float sv[NT / 64];
    __shared__ int si[NT / 64];
    if (!goes_on(false, (uint32_t)p.go[step])) return;
    const int b = blockIdx.x, tid = threadIdx.x, cur = step + 1;
    const size_t R = (size_t)B * K;
    const float* lg = logits + (size_t)b * K * Vp;

    // 1. per-row maximum and sum of exponentials
    for (int k = 0; k < K; ++k) {
        float m = -INFINITY;
        for (int v = tid; v < V; v += NT) m = fmaxf(m, lg[(size_t)k * Vp + v]);
        red[k][tid] = m;
    }
    if (tid < K) row_run[tid] = p.run_score[b * K + tid];
    __syncthreads();
    for (int stride = NT / 2; stride > 0; stride >>= 1) {
        if (tid < stride)
            for (int k = 0; k < K; ++k) red[k][tid] = fmaxf(red[k][tid], red[k][tid + stride]);
        __syncthreads();
    }
    if (tid < K) row_max[tid] = red[tid][0];
    __syncthreads();
    for (int k = 0; k < K; ++k) {
        const float m = row_max[k];
        float s = 0.0f;
        for (int v = tid; v < V; v += NT) s += rs_expf(lg[(size_t)k * Vp + v] - m);
        red[k][tid] = s;
    }
    __syncthreads();
    for (int stride = NT / 2; stride > 0; stride >>= 1) {
        if (tid < stride)
            for (int k = 0; k < K; ++k) red[k][tid] += red[k][tid + stride];
        __syncthreads();
    }
    if (tid < K) row_lse[tid] = rs_logf(red[tid][0]);
    __syncthreads();

    // 2. the 2 K best (value descending, flat index ascending)
    float prev_v = INFINITY;
    int prev_i = -1;
    for (int r = 0; r < 2 * K; ++r) {
        float bv = -INFINITY;
        int bi = 0x7fffffff;
        for (int k = 0; k < K; ++k) {
            const float m = row_max[k], lse = row_lse[k], run = row_run[k];
            for (int v = tid; v < V; v += NT) {
                const float val = ((lg[(size_t)k * Vp + v] - m) - lse) + run;
                const int idx = k * V + v;
                const bool after = val < prev_v || (val == prev_v && idx > prev_i);
                if (after && (val > bv || (val == bv && idx < bi))) { bv = val; bi = idx; }
            }
        }
        block_argmax(bv, bi, sv, si);
        if (tid == 0) { top_lp[r] = bv; top_idx[r] = bi; }
        prev_v = bv; prev_i = bi;
    }
    __syncthreads();

    // 3. bookkeeping (generation.py's lines in float32, in its order)
    if (tid == 0) {
        const float NEG = -1.0e9f;
        const int ci = p.can[b];
        int all_end = 1;
        for (int j = 0; j < 2 * K; ++j) {
            int idx = top_idx[j];
            if (idx < 0 || idx >= K * V) idx = 0;        // only if a row held NaN: stay inside the buffers
            parent[j] = idx / V; token[j] = idx % V;
            ends[j] = (token[j] == eos) || (cur + 1 >= max_len);
            all_end &= ends[j];
            lp_run[j] = top_lp[j] + (ends[j] ? 1.0f : 0.0f) * NEG;
            used[j] = 0;
        }
        for (int j = 0; j < K; ++j) {                     // stable: the first of equal values
            int w = -1;
            for (int c = 0; c < 2 * K; ++c)
                if (!used[c] && (w < 0 || lp_run[c] > lp_run[w])) w = c;
            used[w] = 1; keep[j] = w;
        }
        for (int j = 0; j < K; ++j) {
            m_score[j] = p.fin_score[b * K + j];
            old_len[j] = p.fin_len[b * K + j];
            old_fin[j] = p.is_fin[b * K + j];
        }
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
        float mn = INFINITY;
        for (int j = 0; j < K; ++j) {
            const int w = best[j];
            new_score[j] = m_score[w];
            mn = fminf(mn, m_score[w]);
        }
        const float best_running = lp_run[keep[0]] / den;
        int any = 0;
        for (int j = 0; j < K; ++j) {
            const int w = best[j];
            const int nf = w < K ? old_fin[w] : just[w - K];
            p.fin_score[b * K + j] = new_score[j];
            p.fin_len[b * K + j] = w < K ? old_len[w] : cur + 1;
            p.is_fin[b * K + j] = nf;
            any |= best_running > (nf ? mn : NEG);
        }
        for (int j = 0; j < K; ++j) {
            p.run_score[b * K + j] = lp_run[keep[j]];
            p.tok[b * K + j] = token[keep[j]];
            p.src[b * K + j] = b * K + parent[keep[j]];
        }
        const int ci_new = ci && any;
        p.can[b] = ci_new;
        p.last[b] = cur;
        atomicAdd(&p.go[cur], (ci_new ? 1 : 0) + (all_end ? 0 : 0x10000));
    }
    __syncthreads();
    const int32_t* run_s = p.run_seq + ((size_t)(step & 1) * R + (size_t)b * K) * max_len;
    const int32_t* fin_s = p.fin_seq + ((size_t)(step & 1) * R + (size_t)b * K) * max_len;
    int32_t* run_d = p.run_seq + ((size_t)(cur & 1) * R + (size_t)b * K) * max_len;
    int32_t* fin_d = p.fin_seq + ((size_t)(cur & 1) * R + (size_t)b * K) * max_len;
    for (int j = 0; j < K; ++j) {
        const int c = keep[j], w = best[j];
        for (int pos = tid; pos <= cur && pos < max_len; pos += NT) {
            run_d[(size_t)j * max_len + pos] = pos == cur ? token[c] : run_s[(size_t)parent[c] * max_len + pos];
            int32_t f;
            if (w < K) f = fin_s[(size_t)w * max_len + pos];
            else f = pos == cur ? token[w - K] : run_s[(size_t)parent[w - K] * max_len + pos];
            fin_d[(size_t)j * max_len + pos] = f;
        }
    }
}

// grid B: the result of clip b: its best finished hypothesis (beam) or its row (greedy), from the buffers the last step wrote
__global__ __launch_bounds__(NT) void avsr_search_finish_kernel(SearchPtrs p, int B, int K, int max_len, int greedy, int32_t* sequences, int32_t* lengths,
                                                                float* scores) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const size_t R = (size_t)B * K;
    const int n = p.last[b];
    const int32_t* src = greedy ? p.run_seq + (size_t)b * max_len : p.fin_seq + ((size_t)(n & 1) * R + (size_t)b * K) * max_len;
    for (int i = tid; i < max_len; i += NT) sequences[(size_t)b * max_len + i] = src[i];
    if (tid == 0) {
        lengths[b] = p.fin_len[(size_t)b * K];
        if (scores) scores[b] = greedy ? 0.0f : p.fin_score[(size_t)b * K];
    }
}

int check_search(rs_ctx* ctx, const rs_avsr_search* sp, int B, int vocab, const void* state, size_t state_bytes, const char* what, SearchPlan* pl) {
    const rs_avsr_dims* d = rs_avsr_dims_of(ctx);
    if (!d) return rs_fail(ctx, RS_EINVAL, "%s: defined for an avsr context (rs_avsr_create) only", what);
    if (!sp || !state) return rs_fail(ctx, RS_EINVAL, "%s: null pointer", what);
    if (sp->beams < 1 || sp->beams > MAXK) return rs_fail(ctx, RS_EINVAL, "%s: beams must be 1..%d, got %d", what, MAXK, sp->beams);
    if (sp->greedy && sp->beams != 1) return rs_fail(ctx, RS_EINVAL, "%s: greedy search has one row per clip, got beams %d", what, sp->beams);
    if (sp->max_new_tokens < 1) return rs_fail(ctx, RS_EINVAL, "%s: max_new_tokens %d", what, sp->max_new_tokens);
    if (1 + (long long)sp->max_new_tokens > d->max_positions)
        return rs_fail(ctx, RS_EINVAL, "%s: 1 + max_new_tokens = %lld positions exceed max_target_positions %d", what, 1 + (long long)sp->max_new_tokens, d->max_positions);
    if (B <= 0 || B > 32767) return rs_fail(ctx, RS_EINVAL, "%s: %d clips (1 .. 32767)", what, B);
    if (vocab < 4 || (long long)vocab * sp->beams > 0x7fffffffLL) return rs_fail(ctx, RS_EINVAL, "%s: vocabulary %d (at least 4)", what, vocab);
    *pl = search_plan(B, sp->beams, 1 + sp->max_new_tokens);
    if (state_bytes < pl->total) return rs_fail(ctx, RS_EWORKSPACE, "%s: state %zu < %zu", what, state_bytes, pl->total);
    return RS_OK;
}

}  // namespace

extern "C" size_t rs_avsr_search_state_bytes(const rs_ctx* ctx, int B, int beams, int max_len) {
    if (!rs_avsr_dims_of(ctx) || B <= 0 || beams < 1 || beams > MAXK || max_len < 2) return 0;
    return search_plan(B, beams, max_len).total;
}

extern "C" int rs_avsr_search_begin(rs_ctx* ctx, const rs_avsr_search* search, int B, int vocab, void* state, size_t state_bytes, void* stream) {
    if (!ctx) return RS_EINVAL;
    SearchPlan pl;
    const int rc = check_search(ctx, search, B, vocab, state, state_bytes, "rs_avsr_search_begin", &pl);
    if (rc != RS_OK) return rc;
    hipLaunchKernelGGL(avsr_search_init_kernel, dim3(B), dim3(NT), 0, (hipStream_t)stream, search_ptrs(state, pl), B, search->beams, 1 + search->max_new_tokens,
                       search->greedy ? 1 : 0, search->bos_token_id, search->pad_token_id);
    RS_CHECK_LAUNCH(ctx, "avsr search begin");
    return RS_OK;
}

extern "C" int rs_avsr_search_step(rs_ctx* ctx, const float* logits, int step, const rs_avsr_search* search, int B, int vocab, void* state, size_t state_bytes,
                                   void* stream) {
    if (!ctx) return RS_EINVAL;
    SearchPlan pl;
    const int rc = check_search(ctx, search, B, vocab, state, state_bytes, "rs_avsr_search_step", &pl);
    if (rc != RS_OK) return rc;
    if (!logits || step < 0 || step >= search->max_new_tokens) return rs_fail(ctx, RS_EINVAL, "rs_avsr_search_step: bad argument (step %d of %d)", step, search->max_new_tokens);
    const int max_len = 1 + search->max_new_tokens, Vp = (vocab + 3) / 4 * 4;
    const SearchPtrs p = search_ptrs(state, pl);
    if (search->greedy) {
        hipLaunchKernelGGL(avsr_greedy_step_kernel, dim3(B), dim3(NT), 0, (hipStream_t)stream, logits, vocab, Vp, step, max_len, search->eos_token_id,
                           search->pad_token_id, p);
    } else {
        const float den = (float)pow((double)(step + 1), (double)search->length_penalty);
        hipLaunchKernelGGL(avsr_beam_step_kernel, dim3(B), dim3(NT), 0, (hipStream_t)stream, logits, vocab, Vp, search->beams, step, max_len, search->eos_token_id,
                           den, B, p);
    }
    RS_CHECK_LAUNCH(ctx, "avsr search step");
    return RS_OK;
}

extern "C" int rs_avsr_search_rows(rs_ctx* ctx, const rs_avsr_search* search, int B, void* state, size_t state_bytes, const int32_t** tokens,
                                   const int32_t** src_rows) {
    if (!ctx) return RS_EINVAL;
    SearchPlan pl;
    const int rc = check_search(ctx, search, B, 4, state, state_bytes, "rs_avsr_search_rows", &pl);
    if (rc != RS_OK) return rc;
    const SearchPtrs p = search_ptrs(state, pl);
    if (tokens) *tokens = p.tok;
    if (src_rows) *src_rows = p.src;
    return RS_OK;
}

extern "C" int rs_avsr_search_peek(rs_ctx* ctx, const rs_avsr_search* search, int B, void* state, size_t state_bytes, int step, int32_t* tokens, int32_t* src_rows,
                                   float* run_scores, float* fin_scores, int32_t* goes_on_out, void* stream) {
    if (!ctx) return RS_EINVAL;
    SearchPlan pl;
    const int rc = check_search(ctx, search, B, 4, state, state_bytes, "rs_avsr_search_peek", &pl);
    if (rc != RS_OK) return rc;
    if (step < 0 || step > search->max_new_tokens) return rs_fail(ctx, RS_EINVAL, "rs_avsr_search_peek: step %d of %d", step, search->max_new_tokens);
    const SearchPtrs p = search_ptrs(state, pl);
    const size_t R = (size_t)B * search->beams;
    hipStream_t s = (hipStream_t)stream;
    uint32_t w = 0;
    if (tokens) RS_HIP(ctx, hipMemcpyAsync(tokens, p.tok, R * 4, hipMemcpyDeviceToHost, s));
    if (src_rows) RS_HIP(ctx, hipMemcpyAsync(src_rows, p.src, R * 4, hipMemcpyDeviceToHost, s));
    if (run_scores) RS_HIP(ctx, hipMemcpyAsync(run_scores, p.run_score, R * 4, hipMemcpyDeviceToHost, s));
    if (fin_scores) RS_HIP(ctx, hipMemcpyAsync(fin_scores, p.fin_score, R * 4, hipMemcpyDeviceToHost, s));
    RS_HIP(ctx, hipMemcpyAsync(&w, p.go + step, 4, hipMemcpyDeviceToHost, s));
    RS_HIP(ctx, hipStreamSynchronize(s));
    if (goes_on_out) *goes_on_out = goes_on(search->greedy != 0, w) ? 1 : 0;
    return RS_OK;
}

extern "C" int rs_avsr_search_finish(rs_ctx* ctx, const rs_avsr_search* search, int B, void* state, size_t state_bytes, int32_t* sequences, int32_t* lengths,
                                     float* scores, void* stream) {
    if (!ctx) return RS_EINVAL;
    SearchPlan pl;
    const int rc = check_search(ctx, search, B, 4, state, state_bytes, "rs_avsr_search_finish", &pl);
    if (rc != RS_OK) return rc;
    if (!sequences || !lengths) return rs_fail(ctx, RS_EINVAL, "rs_avsr_search_finish: null pointer");
    hipLaunchKernelGGL(avsr_search_finish_kernel, dim3(B), dim3(NT), 0, (hipStream_t)stream, search_ptrs(state, pl), B, search->beams, 1 + search->max_new_tokens,
                       search->greedy ? 1 : 0, sequences, lengths, scores);
    RS_CHECK_LAUNCH(ctx, "avsr search finish");
    RS_HIP(ctx, hipStreamSynchronize((hipStream_t)stream));
    return RS_OK;
}

// ---- generate(): decoder step + search step per token, the stop word read LAG steps behind ------------------------------------------
namespace {
struct GenPlan { size_t off_dec, off_search, off_logits, total; };
GenPlan gen_plan(const rs_ctx* ctx, int B, int T, int beams, int max_len) {
    GenPlan g{};
    const rs_avsr_dims* d = rs_avsr_dims_of(ctx);
    const size_t dec = rs_avsr_decoder_state_bytes(ctx, B, T, beams, max_len);
    g.off_dec = 0;
    g.off_search = rs_align(dec);
    g.off_logits = g.off_search + rs_align(search_plan(B, beams, max_len).total);
    g.total = g.off_logits + rs_align((size_t)B * beams * ((d->vocab_size + 3) / 4 * 4) * 4) + 256;
    return g;
}
struct StopWatch {              // pinned words the go[] entries are copied to, and the events that say when they have arrived
    int32_t* words = nullptr;
    hipEvent_t ev[LAG + 1] = {};
    int n_ev = 0;
    ~StopWatch() {
        for (int i = 0; i < n_ev; ++i) (void)hipEventDestroy(ev[i]);
        if (words) (void)hipHostFree(words);
    }
};
}  // namespace

extern "C" size_t rs_avsr_generate_state_bytes(const rs_ctx* ctx, int B, int T, int beams, int max_len) {
    if (!rs_avsr_dims_of(ctx) || B <= 0 || T <= 0 || beams < 1 || beams > MAXK || max_len < 2) return 0;
    return gen_plan(ctx, B, T, beams, max_len).total;
}

extern "C" int rs_avsr_generate(rs_ctx* ctx, const float* enc, const float* padding_mask, int B, int T, const rs_avsr_search* search, int32_t* sequences,
                                int32_t* lengths, float* scores, void* state, size_t state_bytes, void* stream) {
    if (!ctx) return RS_EINVAL;
    const rs_avsr_dims* d = rs_avsr_dims_of(ctx);
    if (!d) return rs_fail(ctx, RS_EINVAL, "rs_avsr_generate: defined for an avsr context (rs_avsr_create) only");
    if (!ctx->finalized) return rs_fail(ctx, RS_ESTATE, "rs_finalize must precede rs_avsr_generate");
    if (!search || !enc || !padding_mask || !sequences || !lengths || !state || T <= 0) return rs_fail(ctx, RS_EINVAL, "rs_avsr_generate: bad argument");
    SearchPlan spl;
    int rc = check_search(ctx, search, B, d->vocab_size, state, (size_t)-1, "rs_avsr_generate", &spl);
    if (rc != RS_OK) return rc;
    const int K = search->beams, max_len = 1 + search->max_new_tokens;
    const bool greedy = search->greedy != 0;
    const GenPlan g = gen_plan(ctx, B, T, K, max_len);
    if (state_bytes < g.total) return rs_fail(ctx, RS_EWORKSPACE, "rs_avsr_generate: state %zu < %zu", state_bytes, g.total);
    char* st = reinterpret_cast<char*>(state);
    void* dec_state = st + g.off_dec;
    void* s_state = st + g.off_search;
    float* logits = reinterpret_cast<float*>(st + g.off_logits);
    const size_t dec_bytes = g.off_search, s_bytes = g.off_logits - g.off_search;
    hipStream_t s = (hipStream_t)stream;
    const SearchPtrs p = search_ptrs(s_state, spl);

    StopWatch sw;
    RS_HIP(ctx, hipHostMalloc(reinterpret_cast<void**>(&sw.words), (size_t)(max_len + 1) * 4, hipHostMallocDefault));
    for (; sw.n_ev < LAG + 1; ++sw.n_ev) RS_HIP(ctx, hipEventCreateWithFlags(&sw.ev[sw.n_ev], hipEventDisableTiming));

    rc = rs_avsr_decoder_begin(ctx, enc, B, T, K, max_len, dec_state, dec_bytes, stream);
    if (rc != RS_OK) return rc;
    rc = rs_avsr_search_begin(ctx, search, B, d->vocab_size, s_state, s_bytes, stream);
    if (rc != RS_OK) return rc;
    for (int step = 0; step < search->max_new_tokens; ++step) {
        // greedy rows keep their caches (no re-parenting); beam rows are re-parented by the rows the last selection wrote
        rc = rs_avsr_decoder_step(ctx, p.tok, greedy ? nullptr : p.src, step, padding_mask, B, T, K, max_len, logits, dec_state, dec_bytes, stream);
        if (rc != RS_OK) return rc;
        rc = rs_avsr_search_step(ctx, logits, step, search, B, d->vocab_size, s_state, s_bytes, stream);
        if (rc != RS_OK) return rc;
        RS_HIP(ctx, hipMemcpyAsync(sw.words + step + 1, p.go + step + 1, 4, hipMemcpyDeviceToHost, s));
        RS_HIP(ctx, hipEventRecord(sw.ev[step % (LAG + 1)], s));
        if (step >= LAG) {       // the word of step - LAG: steps issued past the stop return at once and change nothing
            const int e = step - LAG;
            RS_HIP(ctx, hipEventSynchronize(sw.ev[e % (LAG + 1)]));
            if (!goes_on(greedy, (uint32_t)sw.words[e + 1])) break;
        }
    }
    return rs_avsr_search_finish(ctx, search, B, s_state, s_bytes, sequences, lengths, scores, stream);
}
