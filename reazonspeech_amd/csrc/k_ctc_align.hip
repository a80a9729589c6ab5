// k_ctc_align.hip — CTC segmentation of a whole batch on the device (rs_ctc_align): a restatement, operation for operation, of
// espnet/asr/ctc_segmentation.py: ctc_segmentation() for the default CtcSegmentationParameters (blank_transition_cost_zero = False,
// preamble_transition_cost_zero = True, backtrack_from_max_t = False, max_prob = -1e10), which restates Kürzinger et al. (2020) §3.
//
//   ctc_align_kernel<NS>   one workgroup per utterance, 256 threads, a thread owns the symbols c = tid, tid + 256, ...
//     forward     table[t][c] = max(stay, switch) in float32 with only adds and maxima, in the host's order, so the values equal
//                 numpy's bit for bit.  table[t-1] and table[t] ping-pong in LDS: one barrier per frame.
//     gathers     p[t][gt[c][s]] does not depend on the recurrence.  NS > 0 (C <= NS * 256): a thread keeps the token ids of its NS
//                 symbols in registers and loads the posteriors of frame t + 1 while frame t is computed, so a frame's step waits
//                 only on loads issued a whole step earlier.  NS == 0 (more than 1024 symbols — above anything a 20 s window
//                 carries, kept so that C is not bounded): the same step, gathers issued in the step itself.
//     decisions   what the host's backtracking decides at (t, c) — stay, or switch with the token length whose probability explains
//                 table[t][c] - table[t-1][c-1-s] best, compared in double like Python's float() arithmetic — is a function of
//                 values the forward step holds, so the step stores ONE BYTE per (t, c) (0 = stay, 1 + s = switch) instead of the
//                 float32 table.  The owner of the last symbol keeps the running first maximum of table[:, C-1] (np.argmax).
//     backtrack   a short sequential walk over the decision bytes by one thread of the same workgroup after the last frame.
#include "rs_common.h"

namespace {

constexpr int ALIGN_THREADS = 256;
constexpr int ALIGN_MAX_S = 8;          // longest token of the character list (rs_ctc_align: S <= 8)
constexpr int ALIGN_MAX_T = 8000;       // CtcSegmentationParameters.min_window_size: longer inputs are windowed upstream, not here
constexpr float ALIGN_NEG = -1e10f;     // CtcSegmentationParameters.max_prob

// token ids of symbol c by token length; -1 = none (also: past the row's symbols, past S, or not a column of the posteriors)
__device__ __forceinline__ void load_gt(const int32_t* __restrict__ G, int c, int C, int S, int ld, int (&g)[ALIGN_MAX_S]) {
#pragma unroll
    for (int s = 0; s < ALIGN_MAX_S; ++s) {
        int v = -1;
        if (c < C && s < S) v = G[(size_t)c * S + s];
        g[s] = v < ld ? v : -1;
    }
}

// np.where(valid, lpz[t][idx], neg)
__device__ __forceinline__ void gather(const float* __restrict__ prow, const int (&g)[ALIGN_MAX_S], float (&v)[ALIGN_MAX_S]) {
#pragma unroll
    for (int s = 0; s < ALIGN_MAX_S; ++s) v[s] = g[s] >= 0 ? prow[g[s]] : ALIGN_NEG;
}

// one cell of the forward pass and the backtracking decision of that cell
__device__ __forceinline__ float align_step(int c, int C, int S, const float* prev, const int (&g)[ALIGN_MAX_S],
                                            const float (&v)[ALIGN_MAX_S], float pb, uint8_t* decision) {
    float best = v[0];
#pragma unroll
    for (int s = 1; s < ALIGN_MAX_S; ++s)
        if (s < S) best = fmaxf(best, v[s]);
    const float pc = prev[c];
    const float stay = c == 0 ? pc : pc + fmaxf(pb, best);
    float sw = ALIGN_NEG;
    float pr[ALIGN_MAX_S];
#pragma unroll
    for (int s = 0; s < ALIGN_MAX_S; ++s) {
        pr[s] = 0.0f;
        if (s < S && s + 1 <= C - 1 && c >= s + 1) {
            pr[s] = prev[c - 1 - s];
            sw = fmaxf(sw, pr[s] + v[s]);
        }
    }
    const float cur = fmaxf(stay, sw);
    int min_s = -1;
    double min_delta = INFINITY, max_lpz = -1e10;
#pragma unroll
    for (int s = 0; s < ALIGN_MAX_S; ++s)
        if (s < S && g[s] >= 0 && c - 1 - s >= 0) {
            const double sp = (double)v[s];
            const double dl = fabs(sp - ((double)cur - (double)pr[s]));
            if (dl < min_delta) { min_delta = dl; min_s = s; }
            if (sp > max_lpz) max_lpz = sp;
        }
    double stay_prob = (double)pb;
    if (max_lpz > stay_prob) stay_prob = max_lpz;
    if (c == 0) stay_prob = 0.0;
    const double est_stay = (double)cur - (double)pc;
    *decision = (min_s >= 0 && fabs(stay_prob - est_stay) > min_delta) ? (uint8_t)(1 + min_s) : (uint8_t)0;
    return cur;
}

template <int NS>
__global__ __launch_bounds__(ALIGN_THREADS) void ctc_align_kernel(const float* __restrict__ probs, int ld, const int32_t* __restrict__ enc_lens,
                                                                  int tp_max, const int32_t* __restrict__ gt, const int32_t* __restrict__ gt_lens,
                                                                  int c_max, int S, int blank, int cap, uint8_t* __restrict__ dec,
                                                                  int32_t* __restrict__ frames, int32_t* __restrict__ status) {
    extern __shared__ float tab[];      // [2][cap]
    __shared__ int s_start;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int T = enc_lens[b], C = gt_lens[b];
    int32_t* fr = frames + (size_t)b * c_max;
    for (int c = tid; c < c_max; c += ALIGN_THREADS) fr[c] = 0;
    int st = 0;
    if (C < 1 || C > c_max || T < 0 || T > tp_max) st = 3;      // lengths outside the buffers: nothing is read
    else if (C > T) st = 1;                                     // "Audio is shorter than text!"
    else if (T > ALIGN_MAX_T) st = 3;
    if (st != 0) {                                              // (uniform over the workgroup)
        if (tid == 0) status[b] = st;
        return;
    }
    float* t0 = tab;
    float* t1 = tab + cap;
    for (int c = tid; c < C; c += ALIGN_THREADS) t0[c] = c == 0 ? 0.0f : ALIGN_NEG;
    __syncthreads();
    const float* P = probs + (size_t)b * tp_max * ld;
    const int32_t* G = gt + (size_t)b * c_max * S;
    uint8_t* D = dec + (size_t)b * tp_max * c_max;
    const int c_last = C - 1;
    float best_v = c_last == 0 ? 0.0f : ALIGN_NEG;              // table[0][C-1]
    int best_t = 0;

    if constexpr (NS > 0) {
        int g[NS][ALIGN_MAX_S];
        float nv[NS][ALIGN_MAX_S];
        float nb = 0.0f;
#pragma unroll
        for (int k = 0; k < NS; ++k) load_gt(G, tid + k * ALIGN_THREADS, C, S, ld, g[k]);
        if (T > 1) {
            const float* prow = P + ld;
#pragma unroll
            for (int k = 0; k < NS; ++k) gather(prow, g[k], nv[k]);
            nb = prow[blank];
        }
        for (int t = 1; t < T; ++t) {
            float v[NS][ALIGN_MAX_S];
#pragma unroll
            for (int k = 0; k < NS; ++k)
#pragma unroll
                for (int s = 0; s < ALIGN_MAX_S; ++s) v[k][s] = nv[k][s];
            const float pb = nb;
            if (t + 1 < T) {                                    // the next frame's posteriors: in flight while this frame is computed
                const float* prow = P + (size_t)(t + 1) * ld;
#pragma unroll
                for (int k = 0; k < NS; ++k) gather(prow, g[k], nv[k]);
                nb = prow[blank];
            }
            const float* prev = (t & 1) ? t0 : t1;
            float* cur = (t & 1) ? t1 : t0;
#pragma unroll
            for (int k = 0; k < NS; ++k) {
                const int c = tid + k * ALIGN_THREADS;
                if (c < C) {
                    uint8_t d;
                    const float x = align_step(c, C, S, prev, g[k], v[k], pb, &d);
                    cur[c] = x;
                    D[(size_t)t * c_max + c] = d;
                    if (c == c_last && x > best_v) { best_v = x; best_t = t; }
                }
            }
            __syncthreads();
        }
    } else {
        for (int t = 1; t < T; ++t) {
            const float* prow = P + (size_t)t * ld;
            const float pb = prow[blank];
            const float* prev = (t & 1) ? t0 : t1;
            float* cur = (t & 1) ? t1 : t0;
            for (int c = tid; c < C; c += ALIGN_THREADS) {
                int g[ALIGN_MAX_S];
                float v[ALIGN_MAX_S];
                load_gt(G, c, C, S, ld, g);
                gather(prow, g, v);
                uint8_t d;
                const float x = align_step(c, C, S, prev, g, v, pb, &d);
                cur[c] = x;
                D[(size_t)t * c_max + c] = d;
                if (c == c_last && x > best_v) { best_v = x; best_t = t; }
            }
            __syncthreads();
        }
    }
    if (tid == c_last % ALIGN_THREADS) s_start = best_t;
    __threadfence_block();
    __syncthreads();
    if (tid == 0) {
        int c = c_last, t = s_start;
        while (t != 0 || c != 0) {
            if (t == 0) { st = 2; break; }                      // the host's IndexError
            const int d = D[(size_t)t * c_max + c];
            if (d) {
                for (int s = 0; s < d; ++s) fr[c - s] = t;
                c -= d;
            }
            t -= 1;
        }
        status[b] = st;
    }
}

}  // namespace

// the layout: one back-pointer byte per (utterance, frame, symbol)
static uint8_t* align_layout(int B, int tp_max, int c_max, rs_arena& a) { return a.take<uint8_t>((size_t)B * (size_t)tp_max * (size_t)c_max); }

size_t rs_ctc_align_workspace_bytes_impl(int B, int tp_max, int c_max) {
    rs_arena a;
    align_layout(B, tp_max, c_max, a);
    return a.bytes();
}

int rs_ctc_align_impl(rs_ctx* ctx, const float* probs, int ld, const int32_t* enc_lens, int B, int tp_max, const int32_t* gt,
                      const int32_t* gt_lens, int c_max, int S, int blank, int32_t* frames, int32_t* status, void* ws, hipStream_t s) {
    const int cap = c_max < ALIGN_MAX_T ? c_max : ALIGN_MAX_T;           // a row with more symbols than frames is never computed
    const size_t lds = (size_t)2 * cap * sizeof(float);
    rs_arena arena(ws);                                                  // (rs_ctc_align compared the size with the query's)
    uint8_t* dec = align_layout(B, tp_max, c_max, arena);
    rs_prof_scope prof(ctx, RS_PROF_DECODE, s, (double)B * tp_max * c_max * (3.0 * S + 2.0), (double)B * tp_max * c_max * (4.0 * S + 1.0));
#define RS_ALIGN_ARGS probs, ld, enc_lens, tp_max, gt, gt_lens, c_max, S, blank, cap, dec, frames, status
    if (c_max <= ALIGN_THREADS) hipLaunchKernelGGL(ctc_align_kernel<1>, dim3(B), dim3(ALIGN_THREADS), lds, s, RS_ALIGN_ARGS);
    else if (c_max <= 2 * ALIGN_THREADS) hipLaunchKernelGGL(ctc_align_kernel<2>, dim3(B), dim3(ALIGN_THREADS), lds, s, RS_ALIGN_ARGS);
    else if (c_max <= 4 * ALIGN_THREADS) hipLaunchKernelGGL(ctc_align_kernel<4>, dim3(B), dim3(ALIGN_THREADS), lds, s, RS_ALIGN_ARGS);
    else hipLaunchKernelGGL(ctc_align_kernel<0>, dim3(B), dim3(ALIGN_THREADS), lds, s, RS_ALIGN_ARGS);
#undef RS_ALIGN_ARGS
    prof.end();
    RS_CHECK_LAUNCH(ctx, "ctc_align");
    return RS_OK;
}
